// deep_fold4_host_test.cpp -- the host arithmetic of "Out-of-domain sampling over coset leaves" (include/stark_mi.h) as a
// stand-alone program for the sanitizers: the opening sections written by the kernel's lane-cooperative writer
// (mg_coset_open_write) into buffers of exactly the layout's length and read back by the verifier's parser
// (deep_coset_parse), every refusal of that parser, and the four-point comparison of Q (deep_coset_q_matches) against the
// DEEP codeword computed by the lane bodies of the two codeword kernels.  CPU only:
//   g++ -O1 -g -std=c++17 -DSMI_EMU_CHECKS -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-unknown-pragmas
//       tests/cpp/deep_fold4_host_test.cpp -o deep_fold4_host_test; ./deep_fold4_host_test
#include <cstdio>
#include <vector>

#include "../../stark_rs_amd/csrc/tables.h"
#include "../../stark_rs_amd/csrc/xargs_core.h"
#include "../../stark_rs_amd/csrc/mgpu_core.h"

static int failures = 0;
#define EXPECT(cond)                                                                                     \
    do {                                                                                                 \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; }          \
    } while (0)

static uint64_t state = 0x434f5345;
static uint64_t next64() {   // splitmix64
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the sections of G groups over random columns and node bytes, written lane by lane, parsed, and spoiled
static void section_case(uint32_t W, uint32_t A, uint32_t D, uint32_t log_N, uint32_t t, uint64_t p) {
    const DeepGroups gr = deep_groups(W, A, D);
    const uint64_t N = 1ull << log_N, q = N / 4;
    std::vector<std::vector<uint32_t>> cols(gr.G);
    std::vector<std::vector<uint8_t>> nodes(gr.G);
    MgCosetTable tab{};
    size_t total = 0;
    for (uint32_t k = 0; k < gr.G; k++) {
        cols[k].resize((size_t)gr.V[k] * N);   // stride == N: the last read is the buffer's last word
        for (auto &v : cols[k]) v = (uint32_t)(next64() % p);
        nodes[k].resize((2 * q - 1) * 32);
        for (auto &b : nodes[k]) b = (uint8_t)next64();
        tab.g[k] = MgCosetGroup{cols[k].data(), N, nodes[k].data(), total, gr.V[k], 0};
        total += (size_t)mg_coset_open_bytes(gr.V[k], t, log_N);
    }
    EXPECT(total == deep_coset_sections_len(gr, t, log_N));
    std::vector<uint64_t> top(t);
    for (uint32_t s = 0; s < t; s++) top[s] = s == 0 ? N - 1 : (s == 1 ? 0 : next64() % N);   // the last leaf, the first, random ones
    std::vector<uint8_t> out(total, 0xEE);
    for (uint32_t s = 0; s < t; s++)
        for (uint32_t k = 0; k < gr.G; k++)
            for (uint32_t lane = 0; lane < 64; lane++) mg_coset_open_write(tab.g[k], log_N, top[s], s, t, out.data() + tab.g[k].out_at, lane, 64);
    std::vector<uint64_t> vals[3];
    size_t at[3] = {0, 0, 0};
    EXPECT(deep_coset_parse(out.data(), out.size(), gr, t, log_N, vals, at) == DEEP_COSET_OK);
    for (uint32_t k = 0; k < gr.G; k++) {
        EXPECT(at[k] == tab.g[k].out_at && vals[k].size() == (size_t)t * 4 * gr.V[k]);
        for (uint32_t s = 0; s < t; s++) {
            const uint64_t a = top[s] % q;
            for (uint32_t c = 0; c < gr.V[k]; c++)
                for (uint32_t j = 0; j < 4; j++) EXPECT(vals[k][(size_t)s * 4 * gr.V[k] + 4 * c + j] == cols[k][(size_t)c * N + a + j * q]);
            // the path: the sibling of a's ancestor on every level
            const uint8_t *path = out.data() + at[k] + (size_t)t * (9 + 32 * gr.V[k]) + (size_t)s * (9 + 32 * (log_N - 2)) + 9;
            for (uint32_t l = 0; l + 2 < log_N; l++) {
                const uint64_t sib = (a >> l) ^ 1, start = 2 * q - ((2 * q) >> l);
                EXPECT(memcmp(path + 32 * l, &nodes[k][(start + sib) * 32], 32) == 0);
            }
        }
    }
    // every refusal, on exact-size copies so that a read past a shortened buffer is the sanitizer's to find
    for (size_t cut : {(size_t)1, total / 2, total}) {
        std::vector<uint8_t> shorter(out.begin(), out.end() - cut);
        EXPECT(deep_coset_parse(shorter.data(), shorter.size(), gr, t, log_N, vals, at) == DEEP_COSET_LENGTH);
    }
    std::vector<uint8_t> longer(out);
    longer.push_back(0);
    EXPECT(deep_coset_parse(longer.data(), longer.size(), gr, t, log_N, vals, at) == DEEP_COSET_LENGTH);
    for (uint32_t k = 0; k < gr.G; k++) {
        const size_t rec = tab.g[k].out_at + (size_t)(t - 1) * (9 + 32 * gr.V[k]), path = tab.g[k].out_at + (size_t)t * (9 + 32 * gr.V[k]);
        std::vector<uint8_t> m(out);
        m[rec] = 3;
        EXPECT(deep_coset_parse(m.data(), m.size(), gr, t, log_N, vals, at) == DEEP_COSET_RECORD);
        m = out, m[rec + 1] ^= 1;
        EXPECT(deep_coset_parse(m.data(), m.size(), gr, t, log_N, vals, at) == DEEP_COSET_RECORD);
        m = out, m[rec + 8] = 0x80;   // a count whose low bytes are right
        EXPECT(deep_coset_parse(m.data(), m.size(), gr, t, log_N, vals, at) == DEEP_COSET_RECORD);
        m = out, m[path] = 2;
        EXPECT(deep_coset_parse(m.data(), m.size(), gr, t, log_N, vals, at) == DEEP_COSET_PATH);
        m = out, m[path + 1] ^= 1;
        EXPECT(deep_coset_parse(m.data(), m.size(), gr, t, log_N, vals, at) == DEEP_COSET_PATH);
    }
}

// Q over a whole domain by the codeword kernels' lane bodies, then every coset against deep_coset_q_matches
static void quotient_case(uint64_t p, uint64_t g, uint32_t W, uint32_t A, uint32_t D, uint32_t log_n, uint32_t lb, bool extreme) {
    FieldSetup fs;
    EXPECT(field_setup(p, g, &fs));
    const Fp F = fs.F;
    const uint32_t log_N = log_n + lb;
    const uint64_t N = 1ull << log_N, q = N / 4;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - log_n), F.p), omega = host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), F.p);
    const size_t cnt = deep_args_record(W, A, D);
    std::vector<uint64_t> ood(cnt), ch(cnt);
    for (size_t i = 0; i < cnt; i++) ood[i] = extreme ? p - 1 : next64() % p, ch[i] = extreme ? ~0ull : next64();
    std::vector<uint32_t> lde(W * N), cl(4 * A * N), seg(4 * D * N);
    for (auto *v : {&lde, &cl, &seg})
        for (auto &x : *v) x = extreme ? (uint32_t)p - 1 - (uint32_t)(next64() % 2) : (uint32_t)(next64() % p);
    const FqH z{{(uint32_t)(next64() % p), 1 + (uint32_t)(next64() % (p - 1)), (uint32_t)(next64() % p), (uint32_t)(next64() % p)}};
    std::vector<uint32_t> tab;
    if (A) deep_compose_args_build(F, (uint32_t)g, W, A, D, w_n, z, ood.data(), ch.data(), &tab);
    else deep_compose_build(F, (uint32_t)g, W, D, w_n, z, ood.data(), ch.data(), &tab);
    const uint32_t g_m = air_to_m((uint32_t)g, F.p), h_m = air_to_m((uint32_t)g, F.p), omega_m = air_to_m(omega, F.p);
    std::vector<uint32_t> Q(4 * N);
    for (uint64_t i0 = 0; i0 < N; i0 += DEEP_ROWS) {
        uint32_t o[4][DEEP_ROWS];
        const uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, i0, F), F);
        auto load = [&](const std::vector<uint32_t> &src) {
            return [&src, i0, N](uint32_t c, uint32_t v[4]) {
                for (int k = 0; k < 4; k++) v[k] = src[(size_t)c * N + i0 + k];
            };
        };
        if (A) deep_compose_args_points(tab.data(), W, A, D, g_m, F, x_m, omega_m, load(lde), load(cl), load(seg), o);
        else deep_compose_points(tab.data(), W, D, g_m, F, x_m, omega_m, load(lde), load(seg), o);
        for (int k = 0; k < DEEP_ROWS; k++)
            for (int e = 0; e < 4; e++) Q[(size_t)e * N + i0 + k] = o[e][k];
    }
    const DeepGroups gr = deep_groups(W, A, D);
    const std::vector<uint32_t> *src[3] = {&lde, A ? &cl : &seg, &seg};
    const uint32_t iota = host_powmod(omega, q, F.p);
    for (uint64_t a = 0; a < q; a++) {
        std::vector<uint64_t> rec[3];
        uint64_t coset[16];
        for (uint32_t k = 0; k < gr.G; k++)
            for (uint32_t c = 0; c < gr.V[k]; c++)
                for (uint32_t j = 0; j < 4; j++) rec[k].push_back((*src[k])[(size_t)c * N + a + j * q]);
        for (uint32_t e = 0; e < 4; e++)
            for (uint32_t j = 0; j < 4; j++) coset[4 * e + j] = Q[(size_t)e * N + a + j * q];
        const uint64_t *r[3] = {rec[0].data(), gr.G > 1 ? rec[1].data() : nullptr, gr.G > 2 ? rec[2].data() : nullptr};
        const uint32_t x_a = host_mulmod((uint32_t)g, host_powmod(omega, a, F.p), F.p);
        EXPECT(deep_coset_q_matches(F.p, (uint32_t)g, W, A, D, w_n, x_a, iota, z, ood.data(), ch.data(), r, coset));
        if (a % 3) continue;   // the spoiled records on a third of the cosets
        for (uint32_t k = 0; k < gr.G; k++) {   // a value swapped between two coset points of one column
            const uint32_t c = (uint32_t)(next64() % gr.V[k]), j = (uint32_t)(next64() % 3);
            if (rec[k][4 * c + j] == rec[k][4 * c + j + 1] || ch[0] == ~0ull) continue;
            std::swap(rec[k][4 * c + j], rec[k][4 * c + j + 1]);
            EXPECT(!deep_coset_q_matches(F.p, (uint32_t)g, W, A, D, w_n, x_a, iota, z, ood.data(), ch.data(), r, coset));
            std::swap(rec[k][4 * c + j], rec[k][4 * c + j + 1]);
        }
        for (int k = 0; k < 16; k += 5) {   // a coordinate of the coset record moved
            coset[k] = (coset[k] + 1) % p;
            EXPECT(!deep_coset_q_matches(F.p, (uint32_t)g, W, A, D, w_n, x_a, iota, z, ood.data(), ch.data(), r, coset));
            coset[k] = (coset[k] + p - 1) % p;
        }
        EXPECT(!deep_coset_q_matches(F.p, (uint32_t)g, W, A, D, w_n, host_mulmod(x_a, omega, F.p), iota, z, ood.data(), ch.data(), r, coset));
    }
}

int main() {
    for (uint64_t p : {998244353ull, 469762049ull}) {
        section_case(1, 0, 1, 3, 1, p);    // q = 2: a path of one digest
        section_case(4, 0, 2, 5, 4, p);
        section_case(9, 3, 2, 6, 5, p);
        section_case(64, 8, 16, 4, 3, p);  // 256 values a record in every group
    }
    for (int extreme = 0; extreme < 2; extreme++) {
        quotient_case(998244353, 3, 1, 0, 1, 1, 2, extreme);
        quotient_case(998244353, 3, 3, 0, 2, 3, 2, extreme);
        quotient_case(469762049, 3, 3, 2, 2, 3, 2, extreme);
        quotient_case(469762049, 3, 9, 8, 4, 2, 3, extreme);
        quotient_case(998244353, 3, 64, 8, 16, 1, 4, extreme);
    }
    std::printf(failures ? "deep_fold4_host_test: %d FAILURES\n" : "deep_fold4_host_test: ok\n", failures);
    return failures ? 1 : 0;
}
