// args_core.h -- several permutation and lookup arguments in one proof (include/stark_mi.h, "Argument list"): the layer that
// runs A arguments through the lane bodies of perm_core.h and lookup_core.h at once.  The A auxiliary columns are built by
// one trio of launches (the argument is the second grid dimension), the 2 A auxiliary quotients are added by one streaming
// launch that reads and writes the codeword once.  Shared by the HIP kernels (args.hip), the verifier (verify.hip, host) and
// the CPU emulator (emu_args.cpp), which runs the same lane batching and block split.
//
// Number forms are those of the argument's own section: a permutation's column is in Montgomery form until the propagation
// launch, a lookup's column is plain throughout.  All arguments share alpha and gamma, so alpha's powers and gamma are kept
// once; the column lists are per argument.  ArgsDev travels as a kernel argument and is indexed with the argument number and
// the tuple member only, both wave-uniform: every table read stays a scalar load.
#pragma once
#include <string>
#include <vector>

#include "lookup_core.h"

static_assert(SMI_ARG_PERM == 0 && SMI_ARG_LOOKUP == 1, "ArgsDev::kind holds the ABI's values");

struct ArgsDev {   // passed to the kernels by value: 760 bytes at A = 8, m = 8
    uint32_t A, g_m;                             // arguments; g in Montgomery form
    uint32_t apow_mm[SMI_PERM_MAX_WIDTH][4];     // alpha^j * R^2, once for every argument
    uint32_t gamma_m[4];                         // gamma * R
    uint32_t kind[SMI_ARGS_MAX], m[SMI_ARGS_MAX], mcol[SMI_ARGS_MAX];
    uint32_t lcol[SMI_ARGS_MAX][SMI_PERM_MAX_WIDTH], rcol[SMI_ARGS_MAX][SMI_PERM_MAX_WIDTH];
};
static_assert(sizeof(ArgsDev) <= 1024, "the kernel arguments stay well inside 4 KB");

// ------------------------------------------------------------------------------------------------ the columns
// One lane of the block launch for argument a: perm_lane_column or lookup_lane_column behind tuples read through the shared
// tables.  pl[q]: the lane's prefix before row q, *agg: the lane's product or sum.  *key: ~0, or for the smallest row of
// the lane with a zero denominator 16 row + 2 a + side (side 0: f_L, side 1: f_R or f_T).
template <class Load4>
SMI_HD void args_lane_column(const ArgsDev &AD, uint32_t a, const Fp &F, uint64_t row0, uint64_t n, Load4 load4, Fq pl[PERM_ROWS], Fq *agg, uint64_t *key) {
    Fq fl[PERM_ROWS], fr[PERM_ROWS];
    tuples_of(AD.apow_mm, AD.gamma_m, AD.m[a], F, AD.lcol[a], load4, fl);
    tuples_of(AD.apow_mm, AD.gamma_m, AD.m[a], F, AD.rcol[a], load4, fr);
    uint64_t z;
    if (AD.kind[a] == SMI_ARG_PERM) {
        perm_lane_ratios(AD.g_m, F, row0, n, fl, fr, pl, agg, &z);           // z: the row
        *key = z == ~0ull ? z : 16 * z + 2 * a + 1;
    } else {
        uint32_t mult[PERM_ROWS];
        load4(AD.mcol[a], mult);
        lookup_lane_deltas(AD.g_m, F, row0, n, fl, fr, mult, pl, agg, &z);   // z: 2 row + side
        *key = z == ~0ull ? z : 16 * (z >> 1) + 2 * a + (z & 1);
    }
}
// The scan's monoid by kind: a product of Montgomery elements from one, or a sum of plain elements from zero.
SMI_HD Fq args_identity(bool perm, const Fp &F) { return perm ? fq_one(F) : Fq{{0, 0, 0, 0}}; }
SMI_HD Fq args_combine(bool perm, const Fq &a, const Fq &b, uint32_t g_m, const Fp &F) { return perm ? fq_mul(a, b, g_m, F) : fq_add(a, b, F.p); }
SMI_HD void args_scan_step(bool perm, const uint32_t (*in)[PERM_BLOCK], uint32_t (*out)[PERM_BLOCK], uint32_t tid, uint32_t off, uint32_t g_m, const Fp &F) {
    if (perm) perm_scan_step(in, out, tid, off, g_m, F);
    else lookup_scan_step(in, out, tid, off, F.p);
}
// what the scan launch stores: plain either way (a permutation's prefixes leave Montgomery form here, as in perm_scan_kernel)
SMI_HD Fq args_scan_out(bool perm, const Fq &w, const Fp &F) {
    return perm ? Fq{{from_mont(w.c[0], F), from_mont(w.c[1], F), from_mont(w.c[2], F), from_mont(w.c[3], F)}} : w;
}
// The propagation launch's lane: v[e][q] = coordinate e of the stored row q, pre = the plain prefix of the row's workgroup.
SMI_HD void args_propagate_rows(bool perm, const uint32_t pre[4], uint32_t v[4][PERM_ROWS], uint32_t g_m, const Fp &F) {
    if (perm) {
        const ExtMul M = ext_mul_prepare(pre, g_m, F);   // plain: (stored Montgomery value) * M is plain
#pragma unroll
        for (int q = 0; q < PERM_ROWS; q++) {
            const uint32_t a[4] = {v[0][q], v[1][q], v[2][q], v[3][q]};
            uint32_t o[4];
            ext_mul_prepared(a, M, F, o);
#pragma unroll
            for (int e = 0; e < 4; e++) v[e][q] = o[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int q = 0; q < PERM_ROWS; q++) v[e][q] = fp_add(v[e][q], pre[e], F.p);
    }
}

// ------------------------------------------------------------------------------------------------ the auxiliary quotients
// One point of a permutation's two quotients, the body of perm_compose_points' loop with Q a template argument (see
// lookup_compose_point: every index into the lane's arrays is a constant).
template <int Q>
SMI_HD void args_perm_point(uint32_t g_m, const Fp &F, const ExtMul &wb, const ExtMul &wt, uint32_t di_m, uint32_t izt, const Fq &fl, const Fq &fr,
                            uint32_t zc[4][PERM_ROWS], uint32_t zx[4][PERM_ROWS], uint32_t acc[4][PERM_ROWS]) {
    const uint32_t p = F.p;
    const ExtMul ML = ext_mul_prepare(fl.c, g_m, F), MR = ext_mul_prepare(fr.c, g_m, F);
    uint32_t zq[4], zn[4], a[4], b[4], tq[4], bq[4], u[4], v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) zq[e] = zc[e][Q], zn[e] = zx[e][Q];
    ext_mul_prepared(zn, MR, F, a);   // z(w x) f_R(x), plain
    ext_mul_prepared(zq, ML, F, b);   // z(x) f_L(x)
#pragma unroll
    for (int e = 0; e < 4; e++) {
        tq[e] = mont_mul(fp_sub(a[e], b[e], p), izt, F);
        bq[e] = mont_mul(e ? zq[e] : fp_sub(zq[0], 1u, p), di_m, F);
    }
    ext_mul_prepared(bq, wb, F, u);
    ext_mul_prepared(tq, wt, F, v);
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e][Q] = fp_add(acc[e][Q], fp_add(u[e], v[e], p), p);
}

// One lane and trip of the streaming launch: PERM_ROWS consecutive points i0 .. i0 + PERM_ROWS - 1 and all A arguments.
//   w: 8 A unreduced weight coordinates (argument a's boundary weight at 8 a, its transition weight at 8 a + 4), read with
//   uniform addresses; load4(col, v): extended trace column col at the four points; loadc(col, next, v): coordinate column
//   col < 4 A of the extended auxiliary columns at the four points, or one row further; acc[e][q]: the composition so far,
//   kept in registers across the arguments.  1 / (x_i - tau) (one Fermat power per lane) and the four entries of the
//   1 / (x^n - tau^n) table are fetched once, not once per argument.
template <class Load4, class LoadC>
SMI_HD void args_compose_points(const ArgsDev &AD, const Fp &F, const uint64_t *w, uint32_t tau_m, const uint32_t *izt_m, uint32_t B, uint64_t i0,
                                uint32_t x0_m, uint32_t omega_m, Load4 load4, LoadC loadc, uint32_t acc[4][PERM_ROWS]) {
    static_assert(PERM_ROWS == 4, "the four points are written out");
    const uint32_t p = F.p;
    uint32_t d[PERM_ROWS], pre[PERM_ROWS], di[PERM_ROWS];
    uint32_t x = x0_m;
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) {
        d[q] = fp_sub(x, tau_m, p);   // never 0: the coset does not meet the trace domain
        x = mont_mul(x, omega_m, F);
    }
    pre[0] = d[0];
#pragma unroll
    for (int q = 1; q < PERM_ROWS; q++) pre[q] = mont_mul(pre[q - 1], d[q], F);
    uint32_t inv = mont_pow(pre[PERM_ROWS - 1], p - 2, F);
#pragma unroll
    for (int q = PERM_ROWS - 1; q >= 0; q--) {
        di[q] = q ? mont_mul(inv, pre[q - 1], F) : inv;   // 1 / (x_q - tau), Montgomery
        if (q) inv = mont_mul(inv, d[q], F);
    }
    const uint32_t ib = (uint32_t)(i0 & (B - 1));   // i0 and B are multiples of 4: the four table entries are consecutive
    const uint32_t z0 = izt_m[ib], z1 = izt_m[ib + 1], z2 = izt_m[ib + 2], z3 = izt_m[ib + 3];
    for (uint32_t a = 0; a < AD.A; a++) {   // wave-uniform
        uint32_t cc[4][PERM_ROWS], cx[4][PERM_ROWS], wm[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            loadc(4 * a + e, false, cc[e]);
            loadc(4 * a + e, true, cx[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[8 * a + e], F);
        const ExtMul wb = ext_mul_prepare(wm, AD.g_m, F);
#pragma unroll
        for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[8 * a + 4 + e], F);
        const ExtMul wt = ext_mul_prepare(wm, AD.g_m, F);
        Fq fl[PERM_ROWS], fr[PERM_ROWS];
        tuples_of(AD.apow_mm, AD.gamma_m, AD.m[a], F, AD.lcol[a], load4, fl);
        tuples_of(AD.apow_mm, AD.gamma_m, AD.m[a], F, AD.rcol[a], load4, fr);
        if (AD.kind[a] == SMI_ARG_PERM) {
            args_perm_point<0>(AD.g_m, F, wb, wt, di[0], z0, fl[0], fr[0], cc, cx, acc);
            args_perm_point<1>(AD.g_m, F, wb, wt, di[1], z1, fl[1], fr[1], cc, cx, acc);
            args_perm_point<2>(AD.g_m, F, wb, wt, di[2], z2, fl[2], fr[2], cc, cx, acc);
            args_perm_point<3>(AD.g_m, F, wb, wt, di[3], z3, fl[3], fr[3], cc, cx, acc);
        } else {
            uint32_t mult[PERM_ROWS];
            load4(AD.mcol[a], mult);
            lookup_compose_point<0>(AD.g_m, F, wb, wt, di[0], z0, fl[0], fr[0], mult[0], cc, cx, acc);
            lookup_compose_point<1>(AD.g_m, F, wb, wt, di[1], z1, fl[1], fr[1], mult[1], cc, cx, acc);
            lookup_compose_point<2>(AD.g_m, F, wb, wt, di[2], z2, fl[2], fr[2], mult[2], cc, cx, acc);
            lookup_compose_point<3>(AD.g_m, F, wb, wt, di[3], z3, fl[3], fr[3], mult[3], cc, cx, acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// the sentences of the argument-list verifier's opening checks, in the order of verify.hip's OpeningWords: length, row,
// path, authentication, canonical, composition.  tests/test_gpu_args.py reaches each of them.
static const char *const ARGS_SENTENCES[6] = {"argument openings: wrong length",
                                              "argument openings: malformed row",
                                              "argument openings: malformed path",
                                              "argument openings: authentication path does not verify",
                                              "argument openings: an opened value is not canonical",
                                              "argument openings: the composition of the opened rows is not the codeword value"};

inline smi_air_perm args_as_perm(const smi_air_arg &a) { return smi_air_perm{a.width, 0, a.a_col, a.b_col}; }
inline smi_air_lookup args_as_lookup(const smi_air_arg &a) { return smi_air_lookup{a.width, a.mult_col, a.a_col, a.b_col}; }

// every argument by its own section's rules; the reason names the argument
inline int args_validate(const smi_air_args *args, uint32_t n_cols, std::string *why) {
    auto fail = [&](const std::string &s) {
        if (why) *why = s;
        return SMI_ERR_BAD_ARG;
    };
    if (!args) return fail("args: null argument list");
    if (args->count < 1 || args->count > SMI_ARGS_MAX) return fail("args: count must be in 1 .. SMI_ARGS_MAX (" + std::to_string(SMI_ARGS_MAX) + ")");
    if (!args->arg) return fail("args: null argument array");
    for (uint32_t a = 0; a < args->count; a++) {
        const smi_air_arg &g = args->arg[a];
        std::string inner;
        int rc = SMI_OK;
        if (g.kind == SMI_ARG_PERM) {
            const smi_air_perm pm = args_as_perm(g);
            rc = perm_validate(&pm, n_cols, &inner);
        } else if (g.kind == SMI_ARG_LOOKUP) {
            const smi_air_lookup lk = args_as_lookup(g);
            rc = lookup_validate(&lk, n_cols, &inner);
        } else {
            rc = SMI_ERR_BAD_ARG;
            inner = "kind must be SMI_ARG_PERM (0) or SMI_ARG_LOOKUP (1)";
        }
        if (rc != SMI_OK) return fail("args: argument " + std::to_string(a) + ": " + inner);
    }
    return SMI_OK;
}

// smi_air_plan_args: the AIR's own plan with d = max(d_air, 2 if any permutation, 3 if any lookup)
inline int args_plan(uint64_t p, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_args *args, uint32_t *degree, uint64_t *fri_expansion,
                     std::string *why) {
    uint32_t d = 0;
    const int rc = air_validate(p, cfg, air, &d, nullptr, why);
    if (rc != SMI_OK) return rc;
    const int arc = args_validate(args, cfg->n_cols, why);
    if (arc != SMI_OK) return arc;
    if ((p & 3) != 1) {
        if (why) *why = "args: p = 3 (mod 4): the quartic extension does not exist";
        return SMI_ERR_BAD_ARG;
    }
    for (uint32_t a = 0; a < args->count; a++) {
        const uint32_t da = args->arg[a].kind == SMI_ARG_LOOKUP ? 3 : 2;
        if (d < da) d = da;
    }
    const uint64_t B = 1ull << cfg->log_blowup;
    uint64_t D = 1;
    while (D < d - 1) D <<= 1;
    const uint64_t E = D > B ? 0 : B / D;
    if (E < 4) {
        if (why) *why = "args: 2^log_blowup / D < 4";
        return SMI_ERR_EXPANSION_TOO_SMALL;
    }
    if (degree) *degree = d;
    if (fri_expansion) *fri_expansion = E;
    return SMI_OK;
}

// the kernels' tables of a validated list under alpha = ch[0..3], gamma = ch[4..7]
inline void args_build(const Fp &F, uint32_t g, const smi_air_args *args, const uint64_t ch[8], ArgsDev *AD) {
    static const uint32_t none[SMI_PERM_MAX_WIDTH] = {0, 0, 0, 0, 0, 0, 0, 0};
    const smi_air_perm widest = {SMI_PERM_MAX_WIDTH, 0, none, none};
    PermDev PD;
    perm_build(F, g, &widest, ch, &PD);   // alpha's powers and gamma as every argument reads them
    *AD = ArgsDev{};
    AD->A = args->count;
    AD->g_m = PD.g_m;
    for (uint32_t j = 0; j < SMI_PERM_MAX_WIDTH; j++)
        for (int e = 0; e < 4; e++) AD->apow_mm[j][e] = PD.apow_mm[j][e];
    for (int e = 0; e < 4; e++) AD->gamma_m[e] = PD.gamma_m[e];
    for (uint32_t a = 0; a < args->count; a++) {
        const smi_air_arg &s = args->arg[a];
        AD->kind[a] = s.kind;
        AD->m[a] = s.width;
        AD->mcol[a] = s.kind == SMI_ARG_LOOKUP ? s.mult_col : 0;
        for (uint32_t j = 0; j < s.width; j++) AD->lcol[a][j] = s.a_col[j], AD->rcol[a][j] = s.b_col[j];
    }
}
