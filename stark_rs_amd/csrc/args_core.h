// args_core.h -- several permutation and lookup arguments in one proof (include/stark_mi.h, "Argument list"): what the
// argument lists share.  The A auxiliary columns are built by one trio of launches (the argument is the second grid
// dimension), the 2 A auxiliary quotients are added by one streaming launch that reads and writes the codeword once.  Here
// are the scan's monoid by kind, the propagation's lane, a permutation's quotients at a point, and the host side of the
// plain list: its checks, its plan and the verifier's sentences.  The lane bodies that read tuples are xargs_core.h's, for
// the plain list too: it is an operand list without selectors or periodic members (xargs_of_plain there).  Shared by the HIP
// kernels (args.hip, xargs.hip), the verifier (verify.hip, host) and the CPU emulator (emu_xargs.cpp).
//
// Number forms are those of the argument's own section: a permutation's column is in Montgomery form until the propagation
// launch, a lookup's column is plain throughout.
#pragma once
#include <string>
#include <vector>

#include "lookup_core.h"

static_assert(SMI_ARG_PERM == 0 && SMI_ARG_LOOKUP == 1, "the kernels' kind[] holds the ABI's values");

// ------------------------------------------------------------------------------------------------ the columns
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
