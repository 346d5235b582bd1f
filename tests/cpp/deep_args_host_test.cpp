// deep_args_host_test.cpp -- the host arithmetic of "Out-of-domain sampling with an argument list" (include/stark_mi.h) as a
// stand-alone program for the sanitizers: the table builder (deep_compose_args_build), the lane body over that table
// (deep_compose_args_points) against Q at a point from three rows (deep_args_q_at), and the extended consistency check
// (deep_xargs_ood_sides) over a list with a permutation, a selected lookup and a periodic table member.  CPU only:
//   g++ -O1 -g -std=c++17 -DSMI_EMU_CHECKS -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-unknown-pragmas
//       tests/cpp/deep_args_host_test.cpp -o deep_args_host_test; ./deep_args_host_test
#include <cstdio>
#include <vector>

#include "../../stark_rs_amd/csrc/tables.h"
#include "../../stark_rs_amd/csrc/xargs_core.h"

static int failures = 0;
#define EXPECT(cond)                                                                                     \
    do {                                                                                                 \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; }          \
    } while (0)

static uint64_t state = 0x5354524b;
static uint64_t next64() {   // splitmix64
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static void compose_case(uint64_t p, uint64_t g, uint32_t W, uint32_t A, uint32_t D, uint32_t log_n, uint32_t lb, bool extreme) {
    FieldSetup fs;
    EXPECT(field_setup(p, g, &fs));
    const Fp F = fs.F;
    const uint32_t log_N = log_n + lb;
    const uint64_t N = 1ull << log_N;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - log_n), F.p), omega = host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), F.p);
    const size_t cnt = deep_args_record(W, A, D);
    std::vector<uint64_t> ood(cnt), ch(cnt);
    for (size_t i = 0; i < cnt; i++) ood[i] = extreme ? p - 1 : next64() % p, ch[i] = extreme ? ~0ull : next64();
    std::vector<uint32_t> lde(W * N), cl(4 * A * N), seg(4 * D * N);
    for (auto *v : {&lde, &cl, &seg})
        for (auto &x : *v) x = extreme ? (uint32_t)p - 1 : (uint32_t)(next64() % p);
    const FqH z{{(uint32_t)(next64() % p), 1 + (uint32_t)(next64() % (p - 1)), (uint32_t)(next64() % p), (uint32_t)(next64() % p)}};
    std::vector<uint32_t> tab;
    deep_compose_args_build(F, (uint32_t)g, W, A, D, w_n, z, ood.data(), ch.data(), &tab);
    EXPECT(tab.size() == deep_args_tab_words(W, A, D));
    const uint32_t g_m = air_to_m((uint32_t)g, F.p), h_m = air_to_m((uint32_t)g, F.p), omega_m = air_to_m(omega, F.p);
    for (uint64_t i0 = 0; i0 < N; i0 += DEEP_ROWS) {
        uint32_t o[4][DEEP_ROWS];
        const uint32_t x_m = mont_mul(h_m, mont_pow(omega_m, i0, F), F);
        auto load = [&](const std::vector<uint32_t> &src) {
            return [&src, i0, N](uint32_t c, uint32_t v[4]) {
                for (int q = 0; q < 4; q++) v[q] = src[(size_t)c * N + i0 + q];
            };
        };
        deep_compose_args_points(tab.data(), W, A, D, g_m, F, x_m, omega_m, load(lde), load(cl), load(seg), o);
        for (int q = 0; q < DEEP_ROWS; q++) {
            const uint64_t i = i0 + q;
            std::vector<uint64_t> tr(W), cr(4 * A), sr(4 * D);
            for (uint32_t c = 0; c < W; c++) tr[c] = lde[(size_t)c * N + i];
            for (uint32_t c = 0; c < 4 * A; c++) cr[c] = cl[(size_t)c * N + i];
            for (uint32_t c = 0; c < 4 * D; c++) sr[c] = seg[(size_t)c * N + i];
            const uint32_t x = host_mulmod((uint32_t)g, host_powmod(omega, i, F.p), F.p);
            const FqH want = deep_args_q_at(F.p, (uint32_t)g, W, A, D, w_n, x, z, ood.data(), ch.data(), tr.data(), cr.data(), sr.data());
            for (int e = 0; e < 4; e++) EXPECT(o[e][q] == want.c[e]);
        }
    }
}

static void consistency_case(uint64_t p, uint64_t g) {
    FieldSetup fs;
    EXPECT(field_setup(p, g, &fs));
    const uint32_t log_n = 4, W = 5;
    smi_stark_cfg cfg{};
    cfg.log_n = log_n, cfg.log_blowup = 2, cfg.n_cols = W, cfg.row_leaves = 1, cfg.trace_offset = 1, cfg.lde_offset = g, cfg.num_colinearity_tests = 2;
    const uint32_t plog[1] = {2};
    const uint64_t pval[4] = {7, 11, 13, p - 1};
    smi_air air{};
    air.n_periodic = 1, air.periodic_log_period = plog, air.periodic_value = pval;
    const uint32_t first_term[1] = {0}, none32[1] = {0};   // no constraint, no boundary point: every table present and empty
    const uint64_t none64[1] = {0};
    air.constraint_first_term = first_term, air.term_first_factor = first_term;
    air.term_coeff = none64, air.factor_var = none32, air.factor_exp = none32;
    air.boundary_col = none32, air.boundary_row = none64, air.boundary_value = none64;
    const uint32_t pa[1] = {0}, pb[1] = {1}, la[1] = {2}, lbv[1] = {2 * W};   // a lookup of column 2 in periodic column 0
    smi_air_xarg arg[2] = {};
    arg[0].kind = SMI_ARG_PERM, arg[0].width = 1, arg[0].a_var = pa, arg[0].b_var = pb, arg[0].a_sel = 4, arg[0].b_sel = SMI_ARG_NO_SELECTOR;
    arg[1].kind = SMI_ARG_LOOKUP, arg[1].width = 1, arg[1].mult_col = 3, arg[1].a_var = la, arg[1].b_var = lbv, arg[1].a_sel = 4, arg[1].b_sel = SMI_ARG_NO_SELECTOR;
    smi_air_xargs xargs{};
    xargs.count = 2, xargs.arg = arg;
    uint32_t d = 0, D = 0;
    std::string why;
    EXPECT(deep_xargs_plan(p, &cfg, &air, &xargs, &d, &D, &why) == SMI_OK);
    if (!why.empty()) std::printf("plan: %s\n", why.c_str());
    EXPECT(d == 3 && D == 2);
    EXPECT(deep_args_proof_len(&cfg, 2, D) > 9 + 32 * (2 * W + 4 + D));
    smi_stark_cfg small = cfg;
    small.log_blowup = 1;
    EXPECT(deep_xargs_plan(p, &small, &air, &xargs, nullptr, nullptr, &why) == SMI_ERR_EXPANSION_TOO_SMALL);
    const uint32_t K = 0, A = 2, NW = W + K + 2 * A;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - log_n), fs.F.p);
    std::vector<uint64_t> ch(8), weights(4 * NW), ood(deep_args_record(W, A, D));
    for (int round = 0; round < 3; round++) {
        for (auto &v : ch) v = round == 2 ? ~0ull : next64();
        for (auto &v : weights) v = round == 2 ? ~0ull : next64();
        for (auto &v : ood) v = round == 1 ? p - 1 : next64() % p;
        const FqH z{{(uint32_t)(next64() % p), 1, (uint32_t)(next64() % p), (uint32_t)(p - 1)}};
        FqH l1, r1, l2, r2;
        deep_xargs_ood_sides((uint32_t)p, (uint32_t)g, &cfg, &air, &xargs, D, w_n, ch.data(), weights.data(), z, ood.data(), &l1, &r1);
        deep_xargs_ood_sides((uint32_t)p, (uint32_t)g, &cfg, &air, &xargs, D, w_n, ch.data(), weights.data(), z, ood.data(), &l2, &r2);
        EXPECT(fqh_eq(l1, l2) && fqh_eq(r1, r2));
        for (int e = 0; e < 4; e++) EXPECT(l1.c[e] < p && r1.c[e] < p);
        ood[4 * (2 * W + 1)] = (ood[4 * (2 * W + 1)] + 1) % p;   // a_1 changed: the left side moves, the right does not
        deep_xargs_ood_sides((uint32_t)p, (uint32_t)g, &cfg, &air, &xargs, D, w_n, ch.data(), weights.data(), z, ood.data(), &l2, &r2);
        EXPECT(!fqh_eq(l1, l2) && fqh_eq(r1, r2));
        // the transcript's two new steps leave 32 bytes a counter behind them
        Transcript tr;
        uint8_t root[32] = {1, 2, 3};
        uint64_t zr[4];
        std::vector<uint64_t> gammas;
        deep_args_transcript_z(tr, root, NW, zr);
        deep_args_transcript_gammas(tr, ood.data(), NW, ood.size(), &gammas);
        EXPECT(gammas.size() == ood.size() && tr.bytes.size() == 32 + 8 * 4 + 16 * ood.size());
    }
}

int main() {
    for (int extreme = 0; extreme < 2; extreme++) {
        compose_case(998244353, 3, 1, 1, 1, 1, 2, extreme);
        compose_case(998244353, 3, 3, 2, 2, 3, 2, extreme);
        compose_case(469762049, 3, 9, 8, 4, 2, 3, extreme);
        compose_case(469762049, 3, 64, 8, 16, 1, 4, extreme);
    }
    consistency_case(998244353, 3);
    consistency_case(469762049, 3);
    std::printf(failures ? "deep_args_host_test: %d FAILURES\n" : "deep_args_host_test: ok\n", failures);
    return failures ? 1 : 0;
}
