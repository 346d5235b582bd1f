// emu_zkargs.cpp -- CPU emulator of the kernels of zero-knowledge DEEP proofs with an argument list (TEST INFRASTRUCTURE).
//
// emu_zk_args_tail runs zk_args_tail_kernel's grid over zk_tail_group, with `aligned` standing for the kernel's VEC (a 16-byte
// store is four word stores here, and the emulator checks that it is aligned and inside the column);
// emu_air_compose_zk_xargs runs emu_air_compose_ext over the derived AIR and then air_zk_xargs_compose_kernel's grid-stride loop
// over zkx_compose_points; emu_zkx_derived_air hands out the derived AIR with both exemption columns; emu_zkx_ood_lhs the left
// side of the verifier's consistency check.  Same arguments and statuses as the C ABI, with (p, g) in place of a context.
#include <string.h>

#include <string>
#include <vector>

#include "emu_host.h"
#include "tables.h"
#include "zkargs_core.h"

extern "C" int emu_air_compose_ext(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const uint32_t *lde, uint64_t stride,
                                   const uint64_t *weights, uint32_t *out, uint64_t out_stride, int force_direct);
extern "C" int emu_ntt(uint64_t p, uint64_t g, const uint32_t *in, uint32_t *out, uint32_t L, uint32_t n_in, uint32_t batch, uint64_t in_stride,
                       uint64_t out_stride, int inverse, uint64_t offset, uint64_t post_scale);

using emu_host::HostAtomics;
using emu_host::load4;
using emu_host::periodic_tables;
using emu_host::store4;


// c: 4 A coordinate columns c_stride apart; rnd: 4 A (k_t - 1) words; closing: 4 A words.  aligned: c counts as 16-byte aligned.
// *bad counts 16-byte stores that are misaligned or leave their column's tail (must stay 0).
extern "C" int emu_zk_args_tail(uint32_t *c, uint64_t c_stride, uint32_t log_n, uint32_t k_t, uint32_t n_args, const uint32_t *rnd, int aligned,
                                uint64_t *closing, uint32_t *bad) {
    if (log_n < 2 || log_n > 27) return SMI_ERR_BAD_ARG;
    const uint64_t n = 1ull << log_n;
    if (k_t < 2 || k_t >= n / 2 || (k_t & 7) || !n_args || n_args > SMI_ARGS_MAX || c_stride < n) return SMI_ERR_BAD_ARG;
    const ZkTailShape S{n, n - k_t, k_t, n_args};
    uint32_t wrong = 0;
    const uint64_t groups = zk_tail_groups(S), lanes = (groups + ZK_BLOCK - 1) / ZK_BLOCK * ZK_BLOCK;
    for (uint32_t col = 0; col < 4 * n_args; col++)
        for (uint64_t grp = 0; grp < lanes; grp++) {
            if (!grp) closing[col] = zk_tail_closing(S, col, c, c_stride);
            if (grp >= groups) continue;
            zk_tail_group(
                S, col, grp, aligned != 0, rnd, c, c_stride,
                [&](uint32_t *dst, const uint32_t v[4]) {
                    const uint64_t at = (uint64_t)(dst - c);
                    if ((at & 3) || at < col * c_stride + S.na + 1 || at + 4 > col * c_stride + n) wrong++;
                    for (int q = 0; q < 4; q++) dst[q] = v[q];
                },
                [&](uint32_t *dst, uint32_t v) { *dst = v; });
        }
    if (bad) *bad = wrong;
    return SMI_OK;
}

// grid: workgroups of the streaming launch (0: as the library sizes it for 256 compute units); weights: 4 (W + K + 3 A)
extern "C" int emu_air_compose_zk_xargs(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air0, const smi_air_xargs *xargs,
                                        const uint32_t *lde, uint64_t stride, const uint32_t *cl, uint64_t c_stride, const uint64_t *challenges,
                                        const uint64_t *weights, uint32_t *out, uint64_t out_stride, int force_direct, uint32_t grid) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr)) return SMI_ERR_BAD_ARG;
    std::string why;
    uint32_t kt = 0;
    int rc = zkx_plan(p, cfg, air0, xargs, nullptr, nullptr, &kt, nullptr, &why);
    if (rc != SMI_OK) return rc;
    const uint32_t log_N = cfg->log_n + cfg->log_blowup;
    const Fp F = fs.F;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg->log_n), F.p);
    ZkAir Z;
    rc = zk_derive_air(p, w_n, cfg, air0, &Z, &why, true);
    if (rc != SMI_OK) return rc;
    rc = emu_air_compose_ext(p, g, cfg, &Z.air, lde, stride, weights, out, out_stride, force_direct);
    if (rc != SMI_OK) return rc;
    AirHost H;
    air_build(F, host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), F.p), cfg, &Z.air, &H);
    std::vector<uint32_t> tab;
    if (!periodic_tables(p, g, H.per, &tab)) return SMI_ERR_BAD_ARG;
    H.dev.ptab = tab.data();
    const AirDev &A = H.dev;
    if (c_stride < A.N) return SMI_ERR_BAD_ARG;
    XArgsDev XD;
    xargs_build(F, (uint32_t)g, xargs, cfg->n_cols, &Z.air, H.per, challenges, &XD);
    XSharedDev SH;
    const bool shared = xshared_build(xargs, cfg->n_cols, &SH);
    const uint64_t *w = weights + 4 * (uint64_t)(A.W + A.K);
    const uint64_t groups = A.N / PERM_ROWS, want = (groups + PERM_BLOCK - 1) / PERM_BLOCK, n = 1ull << cfg->log_n;
    if (!grid) grid = (uint32_t)(want < 2048 ? want : 2048);
    const uint64_t gstep = (uint64_t)grid * PERM_BLOCK;
    const uint32_t B = 1u << A.log_B, tau = (uint32_t)cfg->trace_offset, tau_m = air_to_m(tau, F.p);
    const uint32_t tna_m = air_to_m(host_mulmod(tau % F.p, host_powmod(w_n, n - kt, F.p), F.p), F.p), ea_op = XOP_PER | (A.Q - 1);
    const uint32_t xstep_m = mont_pow(A.omega_m, gstep * PERM_ROWS, F);
    for (uint64_t gid = 0; gid < gstep && gid < groups; gid++) {
        uint32_t x_m = mont_mul(A.h_m, mont_pow(A.omega_m, gid * PERM_ROWS, F), F);
        for (uint64_t gq = gid; gq < groups; gq += gstep) {
            const uint64_t i0 = gq * PERM_ROWS, i1 = (i0 + B) & (A.N - 1);
            uint32_t acc[4][PERM_ROWS];
            for (int e = 0; e < 4; e++) load4(out + e * out_stride, i0, A.N, acc[e]);
            auto ld = [&](uint32_t op, uint32_t v[4]) {
                if (xop_periodic(op)) {
                    uint64_t L, at;
                    const uint32_t *table = xargs_table_at(A.plog, A.pofs, A.ptab, op & 0xffu, i0, &L, &at);
                    load4(table, at, L, v);
                } else {
                    load4(lde + (uint64_t)op * stride, i0, A.N, v);
                }
            };
            auto ldc = [&](uint32_t col, bool next, uint32_t v[4]) { load4(cl + (uint64_t)col * c_stride, next ? i1 : i0, A.N, v); };
            if (shared) zkx_compose_points(XD, SH, F, w, tau_m, tna_m, ea_op, A.izt_m, B, i0, x_m, A.omega_m, ld, ldc, acc);
            else zkx_compose_points(XD, XNoShared{}, F, w, tau_m, tna_m, ea_op, A.izt_m, B, i0, x_m, A.omega_m, ld, ldc, acc);
            for (int e = 0; e < 4; e++) store4(out + e * out_stride, i0, A.N, acc[e]);
            x_m = mont_mul(x_m, xstep_m, F);
        }
    }
    return SMI_OK;
}

// emu_zk_derived_air (emu_zk.cpp) for the list form: both exemption columns filled
extern "C" int emu_zkx_derived_air(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, uint64_t *head, uint32_t *cft, uint64_t *coeff,
                                   uint32_t *tff, uint32_t *var, uint32_t *exp, uint32_t *plog, uint64_t *pval) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs) || !cfg || cfg->log_n > fs.K) return SMI_ERR_UNSUPPORTED_PRIME;
    ZkAir Z;
    std::string why;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg->log_n), fs.F.p);
    const int rc = zk_derive_air(p, w_n, cfg, air, &Z, &why, true);
    if (rc != SMI_OK) return rc;
    const uint64_t h[6] = {Z.air.n_constraints, Z.air.n_terms, Z.air.n_factors, Z.air.n_boundary, Z.air.n_periodic, Z.pval.size()};
    memcpy(head, h, sizeof h);
    if (!cft) return SMI_OK;
    memcpy(cft, Z.cft.data(), Z.cft.size() * 4);
    memcpy(coeff, Z.coeff.data(), Z.coeff.size() * 8);
    memcpy(tff, Z.tff.data(), Z.tff.size() * 4);
    memcpy(var, Z.var.data(), Z.var.size() * 4);
    memcpy(exp, Z.exp.data(), Z.exp.size() * 4);
    memcpy(plog, Z.plog.data(), Z.plog.size() * 4);
    memcpy(pval, Z.pval.data(), Z.pval.size() * 8);
    return SMI_OK;
}

// the multiplicity helper with a row bound, lane by lane (xargs_core.h); order as emu_xargs_multiplicities.  Kept apart from
// emu_xargs_multiplicities on purpose: tests/test_zk_args_emu.py compares the two at rows = n, as the GPU test compares the
// two entry points.
extern "C" int emu_xargs_multiplicities_rows(uint64_t p, uint64_t g, const smi_air *air, const smi_air_xargs *xargs, uint32_t a, const uint32_t *trace,
                                             uint32_t n_cols, uint32_t log_n, uint64_t rows, uint32_t *mult, int order, uint64_t *missing) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30) || !n_cols || n_cols > 64 || log_n < 1 || log_n > 27) return SMI_ERR_BAD_ARG;
    int rc = xargs_periodic_check(p, air, log_n, nullptr);
    if (rc != SMI_OK) return rc;
    rc = xargs_validate(xargs, n_cols, air->n_periodic, nullptr);
    if (rc != SMI_OK) return rc;
    if (xargs_any_next(xargs)) return SMI_ERR_BAD_ARG;   // smi_dev_xargs_multiplicities_rows: this-row operands only
    rc = xargs_shared_rows(p, xargs, log_n, nullptr);
    if (rc != SMI_OK) return rc;
    if (a >= xargs->count || (xargs->arg[a].kind & 0xffu) != SMI_ARG_LOOKUP) return SMI_ERR_BAD_ARG;
    const uint64_t n = 1ull << log_n, cap = lookup_table_slots(n);
    if (!rows || rows > n) return SMI_ERR_BAD_ARG;
    AirPeriodic per;
    xargs_periodic_plan((uint32_t)p, air, log_n, &per);
    XArgsDev XD;
    const uint64_t no_challenges[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    xargs_build(fs.F, (uint32_t)g, xargs, n_cols, air, per, no_challenges, &XD);
    XD.pvals = per.vals.data();
    XSharedDev SH;
    xshared_build(xargs, n_cols, &SH);
    std::vector<uint32_t> tab(cap, LOOKUP_EMPTY);
    memset(mult, 0, n * 4);
    uint64_t first = ~0ull;
    bool exhausted = false;
    for (uint64_t k = 0; k < rows; k++) {
        const uint32_t t = (uint32_t)(order ? rows - 1 - k : k);
        if (!xlookup_insert_lane(XD, a, trace, n, tab.data(), (uint32_t)cap, t, HostAtomics{})) exhausted = true;
    }
    for (uint64_t k = 0; k < rows; k++) {
        const uint32_t r = (uint32_t)(order ? rows - 1 - k : k);
        if (SH.J[a] > 1) {   // xargs_count_shared_kernel: *missing is 4 row + tuple
            uint32_t miss = 0;
            const int got = xshared_count_lane(XD, SH, a, trace, n, tab.data(), (uint32_t)cap, r, mult, HostAtomics{}, &miss);
            if ((got & 1) && 4 * (uint64_t)r + miss < first) first = 4 * (uint64_t)r + miss;
            if (got & 2) exhausted = true;
            continue;
        }
        const int got = xlookup_count_lane(XD, a, trace, n, tab.data(), (uint32_t)cap, r, mult, HostAtomics{});
        if (got == 1 && r < first) first = r;
        if (got == 2) exhausted = true;
    }
    if (missing) *missing = first;
    if (exhausted) return SMI_ERR_BAD_ARG;
    return first != ~0ull ? SMI_ERR_LOOKUP_MISSING : SMI_OK;
}

// the left side of the verifier's consistency check; challenges = alpha, gamma; weights: 4 (W + K + 3 A); ood: 4 (2 W + 2 A + D')
extern "C" int emu_zkx_ood_lhs(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air0, const smi_air_xargs *xargs, const uint64_t *challenges,
                               const uint64_t *weights, const uint64_t *z, const uint64_t *ood, uint64_t *lhs) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    std::string why;
    int rc = zkx_plan(p, cfg, air0, xargs, nullptr, nullptr, nullptr, nullptr, &why);
    if (rc != SMI_OK) return rc;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg->log_n), fs.F.p);
    ZkAir Z;
    rc = zk_derive_air(p, w_n, cfg, air0, &Z, &why, true);
    if (rc != SMI_OK) return rc;
    FqH zq;
    for (int e = 0; e < 4; e++) zq.c[e] = (uint32_t)(z[e] % p);
    const FqH l = zkx_ood_lhs((uint32_t)p, (uint32_t)g, cfg, &Z.air, xargs, w_n, challenges, weights, zq, ood);
    for (int e = 0; e < 4; e++) lhs[e] = l.c[e];
    return SMI_OK;
}
