// emu_xargs.cpp -- CPU emulator of the kernels of the argument list with selectors and periodic members (TEST INFRASTRUCTURE).
//
// emu_xargs_columns runs the three launches of smi_dev_xargs_columns over xargs_core.h's lane code for every lane, workgroup
// and argument, with the kernels' own lane batching and block split; emu_air_compose_xargs runs emu_air_compose_ext and then
// air_xargs_compose_kernel's grid-stride loop over xargs_compose_points; emu_xargs_multiplicities runs the helper's two
// launches lane by lane.  emu_args_columns and emu_air_compose_args, the plain list's, are their own checks in front of the
// same code, as in the library.  Same arguments and statuses as the C ABI, with (p, g) in place of a context.
#include <string.h>

#include <string>
#include <vector>

#include "emu_host.h"
#include "tables.h"
#include "xargs_core.h"

extern "C" int emu_air_compose_ext(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const uint32_t *lde, uint64_t stride,
                                   const uint64_t *weights, uint32_t *out, uint64_t out_stride, int force_direct);
extern "C" int emu_ntt(uint64_t p, uint64_t g, const uint32_t *in, uint32_t *out, uint32_t L, uint32_t n_in, uint32_t batch, uint64_t in_stride,
                       uint64_t out_stride, int inverse, uint64_t offset, uint64_t post_scale);

using emu_host::HostAtomics;
using emu_host::load4;
using emu_host::periodic_tables;
using emu_host::store4;

namespace {
// args_wg_scan of args_dev.h: v[tid] -> excl[tid] and the aggregate
Fq wg_scan(bool perm, const Fq *v, Fq *excl, uint32_t g_m, const Fp &F) {
    static thread_local uint32_t sc[2][4][PERM_BLOCK];
    for (uint32_t tid = 0; tid < PERM_BLOCK; tid++)
        for (int e = 0; e < 4; e++) sc[0][e][tid] = v[tid].c[e];
    int cur = 0;
    for (uint32_t off = 1; off < PERM_BLOCK; off <<= 1) {
        for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) args_scan_step(perm, sc[cur], sc[cur ^ 1], tid, off, g_m, F);
        cur ^= 1;
    }
    for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) excl[tid] = tid ? perm_scan_at(sc[cur], tid - 1) : args_identity(perm, F);
    return perm_scan_at(sc[cur], PERM_BLOCK - 1);
}
int checks(uint64_t p, uint64_t g, const smi_air *air, const smi_air_xargs *xargs, uint32_t n_cols, uint32_t log_n, FieldSetup *fs) {
    if (!field_setup(p, g, fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30)) return SMI_ERR_BAD_ARG;
    if (!n_cols || n_cols > 64 || log_n < 1 || log_n > 27) return SMI_ERR_BAD_ARG;
    const int prc = xargs_periodic_check(p, air, log_n, nullptr);
    if (prc != SMI_OK) return prc;
    const int vrc = xargs_validate(xargs, n_cols, air->n_periodic, nullptr);
    return vrc != SMI_OK ? vrc : xargs_shared_rows(p, xargs, log_n, nullptr);
}
// the three launches of a column build behind the entry points' checks.  air: nullptr for a plain list
int columns_run(const FieldSetup &fs, uint64_t g, const smi_air *air, const smi_air_xargs *xargs, const uint32_t *trace, uint32_t n_cols, uint32_t log_n,
                const uint64_t *challenges, uint32_t *c, uint64_t c_stride, uint32_t *closes, uint64_t *key) {
    const Fp F = fs.F;
    const uint64_t n = 1ull << log_n, nb = (n + PERM_TILE - 1) / PERM_TILE;
    if (c_stride < n) return SMI_ERR_BAD_ARG;
    AirPeriodic per;
    if (air) xargs_periodic_plan(F.p, air, log_n, &per);
    XArgsDev XD;
    xargs_build(F, (uint32_t)g, xargs, n_cols, air, per, challenges, &XD);
    XD.pvals = per.vals.data();
    const uint32_t A = XD.A;
    XSharedDev SH;   // a list with a shared lookup runs xargs_block_shared_kernel: *key is 64 row + 8 a + side
    const bool shared = xshared_build(xargs, n_cols, &SH);
    std::vector<Fq> agg_all((size_t)A * nb), total(A);
    uint64_t first = ~0ull;
    std::vector<Fq> agg(PERM_BLOCK), pre(PERM_BLOCK), pls((size_t)PERM_BLOCK * PERM_ROWS);
    // xargs_block_kernel: grid (nb, A)
    for (uint32_t a = 0; a < A; a++) {
        const bool perm = XD.kind[a] == SMI_ARG_PERM;
        uint32_t *ca = c + 4 * (uint64_t)a * c_stride;
        for (uint64_t b = 0; b < nb; b++) {
            for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
                const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
                uint64_t k;
                auto ld = [&](uint32_t op, uint32_t v[4]) {
                    if (row0 >= n) {
                        v[0] = v[1] = v[2] = v[3] = 0u;
                    } else if (xop_next(op)) {   // xargs_block_body's NEXT branch, the 16-byte form where a column has four words
                        const bool per = xop_periodic(op);
                        const uint32_t j = op & 0xffu;
                        const uint64_t len = per ? 1ull << XD.plog[j] : n, at = row0 & (len - 1);
                        const uint32_t *col = per ? XD.pvals + XD.pfirst[j] : trace + (uint64_t)j * n;
                        if (len >= 4) {
                            uint32_t own[4];
                            load4(col, at, len, own);
                            xargs_next4(col, at, len, own, v);
                        } else {
                            xargs_next4_words(col, row0, len, n, v);
                        }
                    } else if (xop_periodic(op)) xargs_periodic_rows(XD, op & 0xffu, row0, v);
                    else load4(trace + (uint64_t)op * n, row0, n, v);
                };
                if (shared) xargs_lane_column(XD, SH, a, F, row0, n, ld, &pls[(size_t)tid * PERM_ROWS], &agg[tid], &k);
                else xargs_lane_column(XD, a, F, row0, n, ld, &pls[(size_t)tid * PERM_ROWS], &agg[tid], &k);
                if (k < first) first = k;
            }
            agg_all[(size_t)a * nb + b] = wg_scan(perm, agg.data(), pre.data(), XD.g_m, F);
            for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
                const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
                if (row0 >= n) break;
                uint32_t o[4][PERM_ROWS];
                for (int q = 0; q < PERM_ROWS; q++) {
                    const Fq w = args_combine(perm, pls[(size_t)tid * PERM_ROWS + q], pre[tid], XD.g_m, F);
                    for (int e = 0; e < 4; e++) o[e][q] = w.c[e];
                }
                for (int e = 0; e < 4; e++) store4(ca + e * c_stride, row0, n, o[e]);
            }
        }
    }
    // args_scan_kernel: workgroup a, PERM_BLOCK aggregates at a time
    for (uint32_t a = 0; a < A; a++) {
        const bool perm = XD.kind[a] == SMI_ARG_PERM;
        Fq *bs = &agg_all[(size_t)a * nb];
        Fq carry = args_identity(perm, F);
        for (uint64_t base = 0; base < nb; base += PERM_BLOCK) {
            for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) agg[tid] = base + tid < nb ? bs[base + tid] : args_identity(perm, F);
            const Fq tile = wg_scan(perm, agg.data(), pre.data(), XD.g_m, F);
            for (uint32_t tid = 0; tid < PERM_BLOCK && base + tid < nb; tid++)
                bs[base + tid] = args_scan_out(perm, args_combine(perm, carry, pre[tid], XD.g_m, F), F);
            carry = args_combine(perm, carry, tile, XD.g_m, F);
        }
        total[a] = args_scan_out(perm, carry, F);
    }
    // args_propagate_kernel: grid (nb, A)
    for (uint32_t a = 0; a < A; a++) {
        uint32_t *ca = c + 4 * (uint64_t)a * c_stride;
        for (uint64_t b = 0; b < nb; b++)
            for (uint32_t tid = 0; tid < PERM_BLOCK; tid++) {
                const uint64_t row0 = (b * PERM_BLOCK + tid) * PERM_ROWS;
                if (row0 >= n) break;
                uint32_t v[4][PERM_ROWS];
                for (int e = 0; e < 4; e++) load4(ca + e * c_stride, row0, n, v[e]);
                args_propagate_rows(XD.kind[a] == SMI_ARG_PERM, agg_all[(size_t)a * nb + b].c, v, XD.g_m, F);
                for (int e = 0; e < 4; e++) store4(ca + e * c_stride, row0, n, v[e]);
            }
    }
    if (key) *key = first;
    if (first != ~0ull) return SMI_ERR_NO_INVERSE;
    uint32_t mask = 0;
    for (uint32_t a = 0; a < A; a++) {
        const uint32_t *t = total[a].c;
        if (t[0] == (XD.kind[a] == SMI_ARG_PERM ? 1u : 0u) && !(t[1] | t[2] | t[3])) mask |= 1u << a;
    }
    if (closes) *closes = mask;
    return SMI_OK;
}
}  // namespace

// order: the order in which the lanes of each launch run (0: ascending, 1: descending) -- the result must not depend on it.
// *missing: the smallest selected row whose tuple is in no selected table row, or ~0
extern "C" int emu_xargs_multiplicities(uint64_t p, uint64_t g, const smi_air *air, const smi_air_xargs *xargs, uint32_t a, const uint32_t *trace,
                                        uint32_t n_cols, uint32_t log_n, uint32_t *mult, int order, uint64_t *missing) {
    FieldSetup fs;
    const int rc = checks(p, g, air, xargs, n_cols, log_n, &fs);
    if (rc != SMI_OK) return rc;
    if (a >= xargs->count || (xargs->arg[a].kind & 0xffu) != SMI_ARG_LOOKUP) return SMI_ERR_BAD_ARG;
    const uint64_t n = 1ull << log_n, cap = lookup_table_slots(n);
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
    const bool next = xargs_dev_any_next(XD, &SH);   // the NEXT instantiations of the two launches
    for (uint64_t k = 0; k < n; k++) {
        const uint32_t t = (uint32_t)(order ? n - 1 - k : k);
        const bool ok = next ? xlookup_insert_lane<true>(XD, a, trace, n, tab.data(), (uint32_t)cap, t, HostAtomics{})
                             : xlookup_insert_lane<false>(XD, a, trace, n, tab.data(), (uint32_t)cap, t, HostAtomics{});
        if (!ok) exhausted = true;
    }
    for (uint64_t k = 0; k < n; k++) {
        const uint32_t r = (uint32_t)(order ? n - 1 - k : k);
        if (SH.J[a] > 1) {   // xargs_count_shared_kernel: *missing is 4 row + tuple
            uint32_t miss = 0;
            const int got = next ? xshared_count_lane<true>(XD, SH, a, trace, n, tab.data(), (uint32_t)cap, r, mult, HostAtomics{}, &miss)
                                 : xshared_count_lane<false>(XD, SH, a, trace, n, tab.data(), (uint32_t)cap, r, mult, HostAtomics{}, &miss);
            if ((got & 1) && 4 * (uint64_t)r + miss < first) first = 4 * (uint64_t)r + miss;
            if (got & 2) exhausted = true;
            continue;
        }
        const int got = next ? xlookup_count_lane<true>(XD, a, trace, n, tab.data(), (uint32_t)cap, r, mult, HostAtomics{})
                             : xlookup_count_lane<false>(XD, a, trace, n, tab.data(), (uint32_t)cap, r, mult, HostAtomics{});
        if (got == 1 && r < first) first = r;
        if (got == 2) exhausted = true;
    }
    if (missing) *missing = first;
    if (exhausted) return SMI_ERR_BAD_ARG;
    return first != ~0ull ? SMI_ERR_LOOKUP_MISSING : SMI_OK;
}

// c: 4 A coordinate columns c_stride apart.  *closes: the mask; *key: the smallest 16 row + 2 a + side with a zero
// denominator, or ~0 -- for a list with a shared lookup 64 row + 8 a + side, side = j for f_j and J for f_T
extern "C" int emu_xargs_columns(uint64_t p, uint64_t g, const smi_air *air, const smi_air_xargs *xargs, const uint32_t *trace, uint32_t n_cols,
                                 uint32_t log_n, const uint64_t *challenges, uint32_t *c, uint64_t c_stride, uint32_t *closes, uint64_t *key) {
    FieldSetup fs;
    const int rc = checks(p, g, air, xargs, n_cols, log_n, &fs);
    if (rc != SMI_OK) return rc;
    return columns_run(fs, g, air, xargs, trace, n_cols, log_n, challenges, c, c_stride, closes, key);
}
// the plain list (emu_args_columns of old): its own checks, then the same list in the operand form -- no AIR, no periodic column
extern "C" int emu_args_columns(uint64_t p, uint64_t g, const smi_air_args *args, const uint32_t *trace, uint32_t n_cols, uint32_t log_n,
                                const uint64_t *challenges, uint32_t *c, uint64_t c_stride, uint32_t *closes, uint64_t *key) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr) || p >= (1ull << 30)) return SMI_ERR_BAD_ARG;
    if (!n_cols || n_cols > 64 || log_n < 1 || log_n > 27) return SMI_ERR_BAD_ARG;
    const int rc = args_validate(args, n_cols, nullptr);
    if (rc != SMI_OK) return rc;
    const XArgsOfPlain x(args);
    return columns_run(fs, g, nullptr, &x.list, trace, n_cols, log_n, challenges, c, c_stride, closes, key);
}

// the main composition and the streaming launch behind the entry points' checks.  pair: the AIR whose periodic columns the
// operands may name (air itself), nullptr for a plain list
static int compose_run(const FieldSetup &fs, uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const smi_air *pair,
                       const smi_air_xargs *xargs, const uint32_t *lde, uint64_t stride, const uint32_t *cl, uint64_t c_stride, const uint64_t *challenges,
                       const uint64_t *weights, uint32_t *out, uint64_t out_stride, int force_direct, uint32_t grid) {
    const int rc = emu_air_compose_ext(p, g, cfg, air, lde, stride, weights, out, out_stride, force_direct);
    if (rc != SMI_OK) return rc;
    const uint32_t log_N = cfg->log_n + cfg->log_blowup;
    const Fp F = fs.F;
    AirHost H;
    air_build(F, host_powmod(fs.wmax[0], 1ull << (fs.K - log_N), F.p), cfg, air, &H);
    std::vector<uint32_t> tab;
    if (pair && !periodic_tables(p, g, H.per, &tab)) return SMI_ERR_BAD_ARG;
    H.dev.ptab = tab.data();
    const AirDev &A = H.dev;
    if (c_stride < A.N) return SMI_ERR_BAD_ARG;
    XArgsDev XD;
    xargs_build(F, (uint32_t)g, xargs, cfg->n_cols, pair, pair ? H.per : AirPeriodic{}, challenges, &XD);
    XSharedDev SH;
    const bool shared = xshared_build(xargs, cfg->n_cols, &SH);
    const uint64_t *w = weights + 4 * (uint64_t)(A.W + A.K);
    const uint64_t groups = A.N / PERM_ROWS, want = (groups + PERM_BLOCK - 1) / PERM_BLOCK;
    if (!grid) grid = (uint32_t)(want < 2048 ? want : 2048);
    const uint64_t gstep = (uint64_t)grid * PERM_BLOCK;
    const uint32_t B = 1u << A.log_B, tau_m = air_to_m((uint32_t)cfg->trace_offset, F.p);
    const uint32_t xstep_m = mont_pow(A.omega_m, gstep * PERM_ROWS, F);
    for (uint64_t gid = 0; gid < gstep && gid < groups; gid++) {
        uint32_t x_m = mont_mul(A.h_m, mont_pow(A.omega_m, gid * PERM_ROWS, F), F);
        for (uint64_t gq = gid; gq < groups; gq += gstep) {
            const uint64_t i0 = gq * PERM_ROWS, i1 = (i0 + B) & (A.N - 1);
            uint32_t acc[4][PERM_ROWS];
            for (int e = 0; e < 4; e++) load4(out + e * out_stride, i0, A.N, acc[e]);
            auto ld = [&](uint32_t op, uint32_t v[4]) {
                const uint64_t ia = xop_next(op) ? i1 : i0;   // air_xargs_compose_body's NEXT loader
                if (xop_periodic(op)) {
                    uint64_t L, at;
                    const uint32_t *table = xargs_table_at(A.plog, A.pofs, A.ptab, op & 0xffu, ia, &L, &at);
                    load4(table, at, L, v);
                } else {
                    load4(lde + (uint64_t)(op & 0xffu) * stride, ia, A.N, v);
                }
            };
            auto ldc = [&](uint32_t col, bool next, uint32_t v[4]) { load4(cl + (uint64_t)col * c_stride, next ? i1 : i0, A.N, v); };
            if (shared) xargs_compose_points(XD, SH, F, w, tau_m, A.izt_m, B, i0, x_m, A.omega_m, ld, ldc, acc);
            else xargs_compose_points(XD, XNoShared{}, F, w, tau_m, A.izt_m, B, i0, x_m, A.omega_m, ld, ldc, acc);
            for (int e = 0; e < 4; e++) store4(out + e * out_stride, i0, A.N, acc[e]);
            x_m = mont_mul(x_m, xstep_m, F);
        }
    }
    return SMI_OK;
}

// grid: workgroups of the streaming launch (0: as the library sizes it for 256 compute units)
extern "C" int emu_air_compose_xargs(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_xargs *xargs, const uint32_t *lde,
                                     uint64_t stride, const uint32_t *cl, uint64_t c_stride, const uint64_t *challenges, const uint64_t *weights,
                                     uint32_t *out, uint64_t out_stride, int force_direct, uint32_t grid) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr)) return SMI_ERR_BAD_ARG;
    std::string why;
    // the launch itself has no bound on E: the DEEP provers run it at every blowup a composition of D segments fits
    const int prc = xargs_plan(p, cfg, air, xargs, nullptr, nullptr, &why);
    if (prc != SMI_OK && prc != SMI_ERR_EXPANSION_TOO_SMALL) return prc;
    return compose_run(fs, p, g, cfg, air, air, xargs, lde, stride, cl, c_stride, challenges, weights, out, out_stride, force_direct, grid);
}
// the plain list: its own plan, then the same list in the operand form
extern "C" int emu_air_compose_args(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_args *args, const uint32_t *lde,
                                    uint64_t stride, const uint32_t *cl, uint64_t c_stride, const uint64_t *challenges, const uint64_t *weights,
                                    uint32_t *out, uint64_t out_stride, int force_direct, uint32_t grid) {
    FieldSetup fs;
    if (!field_setup(p, g, &fs)) return SMI_ERR_UNSUPPORTED_PRIME;
    if (!ext_field_ok(p, g, nullptr)) return SMI_ERR_BAD_ARG;
    std::string why;
    const int prc = args_plan(p, cfg, air, args, nullptr, nullptr, &why);
    if (prc != SMI_OK) return prc;
    const XArgsOfPlain x(args);
    return compose_run(fs, p, g, cfg, air, nullptr, &x.list, lde, stride, cl, c_stride, challenges, weights, out, out_stride, force_direct, grid);
}

// both sides of the verifier's extended out-of-domain consistency check (include/stark_mi.h, "Out-of-domain sampling with an
// argument list"; four canonical coordinates each): challenges = alpha, gamma; weights = the 4 (W + K + 2 A) challenges
extern "C" int emu_deep_xargs_ood_sides(uint64_t p, uint64_t g, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_xargs *xargs,
                                        const uint64_t *challenges, const uint64_t *weights, const uint64_t *z, const uint64_t *ood, uint64_t *lhs,
                                        uint64_t *rhs) {
    FieldSetup fs;
    int rc = checks(p, g, air, xargs, cfg->n_cols, cfg->log_n, &fs);
    if (rc != SMI_OK) return rc;
    uint32_t D = 0;
    rc = deep_xargs_plan(p, cfg, air, xargs, nullptr, &D, nullptr);
    if (rc != SMI_OK) return rc;
    FqH zq, l, r;
    for (int e = 0; e < 4; e++) {
        if (z[e] >= p) return SMI_ERR_NON_CANONICAL;
        zq.c[e] = (uint32_t)z[e];
    }
    if (fqh_in_base(zq)) return SMI_ERR_BAD_ARG;
    for (size_t i = 0; i < deep_args_record(cfg->n_cols, xargs->count, D); i++)
        if (ood[i] >= p) return SMI_ERR_NON_CANONICAL;
    const uint32_t w_n = host_powmod(fs.wmax[0], 1ull << (fs.K - cfg->log_n), fs.F.p);
    deep_xargs_ood_sides((uint32_t)p, (uint32_t)g, cfg, air, xargs, D, w_n, challenges, weights, zq, ood, &l, &r);
    for (int e = 0; e < 4; e++) lhs[e] = l.c[e], rhs[e] = r.c[e];
    return SMI_OK;
}
