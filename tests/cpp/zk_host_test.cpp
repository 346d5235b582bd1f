// zk_host_test.cpp -- the host-runnable code of "Zero-knowledge DEEP proofs" (include/stark_mi.h) as a
// stand-alone program for the sanitizers: the generator's lane body against Hash::from_bytes of the 48-byte message, the masked
// split read from and written into buffers of exactly the documented sizes (the kernel's two aligned loads included) and
// recombined coefficient by coefficient, and the derived AIR with the plan's numbers and refusals.  CPU only:
//   g++ -O1 -g -std=c++17 -DSMI_EMU_CHECKS -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-unknown-pragmas
//       tests/cpp/zk_host_test.cpp -o zk_host_test; ./zk_host_test
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../stark_rs_amd/csrc/tables.h"
#include "../../stark_rs_amd/csrc/zk_core.h"

static int failures = 0;
#define EXPECT(cond)                                                                                     \
    do {                                                                                                 \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; }          \
    } while (0)

static uint64_t state = 0x5a4b;
static uint64_t next64() {   // splitmix64
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static void random_case(uint32_t p, uint64_t stream, uint64_t first_lane, uint64_t lanes) {
    const Fp F = fp_make(p);
    uint8_t seed[32];
    for (auto &b : seed) b = (uint8_t)next64();
    const ZkRandSeed S = zk_rand_seed(seed, stream);
    for (uint64_t lane = first_lane; lane < first_lane + lanes; lane++) {
        uint32_t v[ZK_RAND_PER_LANE];
        zk_rand_lane(S.mid, lane, F, v);
        for (int h = 0; h < 2; h++) {
            uint8_t msg[48];
            memcpy(msg, seed, 32);
            for (int i = 0; i < 8; i++) msg[32 + i] = (uint8_t)(stream >> (8 * i)), msg[40 + i] = (uint8_t)((2 * lane + h) >> (8 * i));
            uint32_t d[8];
            hashc::hash_bytes(msg, 48, d);
            for (int k = 0; k < 4; k++) EXPECT(v[4 * h + k] == (uint32_t)((((uint64_t)d[2 * k + 1] << 32) | d[2 * k]) % p));
        }
    }
}

// the kernel's lane over exact-size buffers: h_stride == h_len, so the last aligned load is cut by h_len
static void split_case(uint32_t p, uint32_t log_n, uint32_t ks, uint64_t h_len) {
    const uint64_t n = 1ull << log_n, L = n - ks;
    const uint32_t Dp = (uint32_t)((h_len + L - 1) / L);
    std::vector<uint32_t> hc(4 * h_len), rho((size_t)4 * (Dp - 1) * ks), out((size_t)4 * Dp * n, 0xffffffffu);
    for (auto &v : hc) v = (uint32_t)(next64() % p);
    for (auto &v : rho) v = (uint32_t)(next64() % p);
    const ZkSegShape S{n, L, h_len, ks, Dp};
    auto load4 = [](const uint32_t *src, uint64_t at, uint64_t len, uint32_t v[4]) {
        for (int q = 0; q < 4; q++) v[q] = at + q < len ? src[at + q] : 0u;
    };
    auto store4 = [](uint32_t *dst, uint64_t at, uint64_t len, const uint32_t v[4]) {
        for (int q = 0; q < 4; q++)
            if (at + q < len) dst[at + q] = v[q];
    };
    for (uint32_t col = 0; col < 4 * Dp; col++)
        for (uint64_t m0 = 0; m0 < n; m0 += 4) zk_seg_group(S, col, m0, hc.data(), h_len, rho.data(), out.data(), n, p, load4, store4);
    // sum_j x^(j L) H~_j = H coefficient by coefficient: position i collects column j at m = i - j L for every j with 0 <= m < n
    for (uint32_t e = 0; e < 4; e++)
        for (uint64_t i = 0; i < (uint64_t)Dp * L + ks; i++) {
            uint32_t acc = 0;
            for (uint32_t j = 0; j < Dp; j++)
                if (i >= j * L && i - j * L < n) acc = fp_add(acc, out[(size_t)(4 * j + e) * n + (i - j * L)], p);
            EXPECT(acc == (i < h_len ? hc[e * h_len + i] : 0u));
        }
}

static void air_case(uint32_t p, uint32_t g) {
    FieldSetup fs;
    EXPECT(field_setup(p, g, &fs));
    // fib with a periodic column: a' = b + pi, b' = a + b
    const uint32_t cft[3] = {0, 3, 6}, tff[7] = {0, 1, 2, 3, 4, 5, 6}, var[6] = {2, 1, 4, 3, 0, 1}, ex[6] = {1, 1, 1, 1, 1, 1}, bcol[2] = {0, 1}, plog[1] = {2};
    const uint64_t coeff[6] = {1, p - 1, p - 1, 1, p - 1, p - 1}, brow[2] = {0, 47}, bval[2] = {1, 5}, pval[4] = {3, p - 1, 0, 7};
    smi_air air{2, 6, 6, 2, cft, coeff, tff, var, ex, bcol, brow, bval, 1, 0, plog, pval};
    smi_stark_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.log_n = 6, cfg.log_blowup = 2, cfg.n_cols = 2, cfg.row_leaves = 1, cfg.trace_offset = 5, cfg.lde_offset = g, cfg.num_colinearity_tests = 1;
    std::string why;
    uint32_t d = 0, Dp = 0, kt = 0, ks = 0;
    EXPECT(zk_plan(p, &cfg, &air, &d, &Dp, &kt, &ks, &why) == SMI_OK);
    EXPECT(d == 2 && Dp == 2 && kt == 16 && ks == 5);
    ZkAir Z;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg.log_n), p);
    EXPECT(zk_derive_air(p, w_n, &cfg, &air, &Z, &why) == SMI_OK);
    EXPECT(Z.air.n_periodic == 2 && Z.air.n_factors == 12 && Z.pval.size() == 4 + 64 && Z.plog[1] == 6);
    EXPECT(Z.var[0] == 2 && Z.var[1] == 2 * 2 + 1 && Z.var[4] == 4 && Z.var[5] == 5);   // next b; E; pi (this row) stays; E
    for (uint64_t r = 0; r < 64; r++) EXPECT((Z.pval[4 + r] == 0) == (r >= 47 && r <= 62));
    std::string why2;
    EXPECT(air_validate(p, &cfg, &Z.air, nullptr, nullptr, &why2, false, true) == SMI_OK);
    const uint64_t late[2] = {0, 48};
    smi_air bad = air;
    bad.boundary_row = late;
    EXPECT(zk_plan(p, &cfg, &bad, nullptr, nullptr, nullptr, nullptr, &why) == SMI_ERR_BAD_ARG && why.find("zk deep: boundary point 1 lies on row 48") == 0);
    cfg.num_colinearity_tests = 3;
    EXPECT(zk_plan(p, &cfg, &air, nullptr, nullptr, nullptr, nullptr, &why) == SMI_ERR_BAD_ARG && why.find("zk deep: k_t = 8 t + 8 = 32 >= n / 2") == 0);
}

int main() {
    for (uint32_t p : {998244353u, 1073692673u, 12289u}) {
        random_case(p, 0, 0, 40);
        random_case(p, ~0ull, (1ull << 40) - 3, 6);
    }
    for (uint32_t p : {998244353u, 536813569u}) {
        split_case(p, 6, 5, 64);
        split_case(p, 6, 5, 128);
        split_case(p, 7, 9, 256);
        split_case(p, 7, 5, 2 * 123);
        split_case(p, 6, 9, 57);
        split_case(p, 5, 3, 29 * 4);
    }
    air_case(998244353u, 3);
    std::printf(failures ? "%d failures\n" : "zk host test ok\n", failures);
    return failures ? 1 : 0;
}
