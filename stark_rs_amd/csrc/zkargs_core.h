// zkargs_core.h -- what zero-knowledge DEEP proofs add for an argument list (include/stark_mi.h, "Zero-knowledge DEEP proofs
// with an argument list"), shared by the kernels of zkargs.hip, the prover (deep.hip), the verifier (verify.hip) and the CPU
// emulator (emu_zkargs.cpp): the lane body of the tail step, the lane body of the three auxiliary quotients, and on the host
// the plan, the layout and the auxiliary quotients at z.  The derived AIR with both exemption columns is zk_core.h's
// zk_derive_air(list = true).
#pragma once
#include "xargs_core.h"
#include "zk_core.h"

// ------------------------------------------------------------------------------------------------ the tail step
// Coordinate column col = 4 a + e of the auxiliary columns (c_stride apart) keeps rows 0 .. n_a, and its rows n_a + 1 .. n - 1
// take elements col (k_t - 1) .. of rnd.  The lanes of a column work on groups of four words that are aligned in memory when
// c is (vec): the column's tail starts at word col c_stride + n_a + 1, which is odd, so the first group holds one to three
// words of the tail and the last group may end early; both store word by word, every group in between with one 16-byte store.
// Without vec the groups start at the tail's first word and every word is stored alone.  The random words are read one by
// one: they sit at col (k_t - 1) + i, which shares no alignment with the column.
struct ZkTailShape {
    uint64_t n, na;
    uint32_t kt, A;
};
SMI_HD uint64_t zk_tail_groups(const ZkTailShape &S) { return (S.kt - 1 + 3) / 4 + 1; }   // enough for any alignment of the first word
template <class Store4, class Store1>
SMI_HD void zk_tail_group(const ZkTailShape &S, uint32_t col, uint64_t grp, bool vec, const uint32_t *__restrict__ rnd, uint32_t *c, size_t c_stride,
                          Store4 &&store4, Store1 &&store1) {
    const uint64_t first = (uint64_t)col * c_stride + S.na + 1, last = (uint64_t)col * c_stride + S.n;
    const uint64_t w0 = (vec ? first & ~(uint64_t)3 : first) + 4 * grp;
    if (w0 >= last) return;
    const uint32_t *src = rnd + (size_t)col * (S.kt - 1);
    uint32_t v[4];
    bool whole = vec;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const bool in = w0 + q >= first && w0 + q < last;
        v[q] = in ? src[w0 + q - first] : 0u;
        whole = whole && in;
    }
    if (whole) {
        store4(c + w0, v);
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (w0 + q >= first && w0 + q < last) store1(c + w0 + q, v[q]);
    }
}
// the closing value's coordinate e of argument a: row n_a of column 4 a + e, as the column build left it
SMI_HD uint32_t zk_tail_closing(const ZkTailShape &S, uint32_t col, const uint32_t *c, size_t c_stride) { return c[(uint64_t)col * c_stride + S.na]; }

// ------------------------------------------------------------------------------------------------ the auxiliary quotients
// cq_a at point Q of the lane: (c_a(x) - init_a) / (x - tau w^n_a) under the weight wc, added to acc.  dci_m: the inverse of the
// denominator, Montgomery; cc: the column's coordinates at the lane's points (plain).
template <int Q>
SMI_HD void zkx_close_point(bool perm, const Fp &F, const ExtMul &wc, uint32_t dci_m, uint32_t cc[4][PERM_ROWS], uint32_t acc[4][PERM_ROWS]) {
    uint32_t cq[4], u[4];
#pragma unroll
    for (int e = 0; e < 4; e++) cq[e] = mont_mul(e || !perm ? cc[e][Q] : fp_sub(cc[0][Q], 1u, F.p), dci_m, F);
    ext_mul_prepared(cq, wc, F, u);
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e][Q] = fp_add(acc[e][Q], u[e], F.p);
}

// One lane and trip of the streaming launch: xargs_compose_points (xargs_core.h) with the three quotients of this variant.
//   w: 12 A unreduced weight coordinates -- bq_a at 12 a, wq_a at 12 a + 4, cq_a at 12 a + 8;
//   tna_m = tau w^n_a (Montgomery); ea_op: the operand code of the periodic column that holds E_A.
// The eight denominators x_q - tau and x_q - tau w^n_a of the lane's four points share one inversion, whatever A is.  E_A(x_q)
// goes into 1 / (x_q^n - tau^n) once per trip, so wq_a is the xargs section's transition quotient computed by that section's
// point functions, and bq_a comes with it; cq_a is one more product per point and argument.
// SH as in xargs_compose_points: a shared lookup goes through xshared_compose and takes its closing quotient like any lookup.
template <class SHT, class Load4, class LoadC>
SMI_HD void zkx_compose_points(const XArgsDev &XD, const SHT &SH, const Fp &F, const uint64_t *w, uint32_t tau_m, uint32_t tna_m, uint32_t ea_op, const uint32_t *izt_m,
                               uint32_t B, uint64_t i0, uint32_t x0_m, uint32_t omega_m, Load4 load4, LoadC loadc, uint32_t acc[4][PERM_ROWS]) {
    static_assert(PERM_ROWS == 4, "the four points are written out");
    const uint32_t p = F.p;
    uint32_t d[2 * PERM_ROWS], pre[2 * PERM_ROWS], di[2 * PERM_ROWS];
    uint32_t x = x0_m;
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) {
        d[q] = fp_sub(x, tau_m, p);               // never 0: the coset does not meet the trace domain
        d[PERM_ROWS + q] = fp_sub(x, tna_m, p);
        x = mont_mul(x, omega_m, F);
    }
    pre[0] = d[0];
#pragma unroll
    for (int q = 1; q < 2 * PERM_ROWS; q++) pre[q] = mont_mul(pre[q - 1], d[q], F);
    uint32_t inv = mont_pow(pre[2 * PERM_ROWS - 1], p - 2, F);
#pragma unroll
    for (int q = 2 * PERM_ROWS - 1; q >= 0; q--) {
        di[q] = q ? mont_mul(inv, pre[q - 1], F) : inv;   // Montgomery
        if (q) inv = mont_mul(inv, d[q], F);
    }
    const uint32_t ib = (uint32_t)(i0 & (B - 1));   // i0 and B are multiples of 4: the four table entries are consecutive
    uint32_t ea[PERM_ROWS], zt[PERM_ROWS];
    load4(ea_op, ea);
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) zt[q] = mont_mul(izt_m[ib + q], to_mont(ea[q], F), F);   // E_A(x) / (x^n - tau^n), Montgomery
    for (uint32_t a = 0; a < XD.A; a++) {   // wave-uniform
        uint32_t cc[4][PERM_ROWS], cx[4][PERM_ROWS], wm[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            loadc(4 * a + e, false, cc[e]);
            loadc(4 * a + e, true, cx[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[12 * a + e], F);
        const ExtMul wb = ext_mul_prepare(wm, XD.g_m, F);
#pragma unroll
        for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[12 * a + 4 + e], F);
        const ExtMul wt = ext_mul_prepare(wm, XD.g_m, F);
#pragma unroll
        for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[12 * a + 8 + e], F);
        const ExtMul wc = ext_mul_prepare(wm, XD.g_m, F);
        const bool perm = XD.kind[a] == SMI_ARG_PERM;
        if (xshared_tuples(SH, a) >= 2) {
            xshared_compose(XD, SH, a, F, wb, wt, di, zt, load4, cc, cx, acc);
        } else if (perm) {
            Fq fl[PERM_ROWS], fr[PERM_ROWS];
            tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, XD.aop[a], load4, fl);
            tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, XD.bop[a], load4, fr);
            uint32_t s[PERM_ROWS];
            if (XD.asel[a] != SMI_ARG_NO_SELECTOR) {
                load4(XD.asel[a], s);
                xargs_select(F, s, fl);
            }
            if (XD.bsel[a] != SMI_ARG_NO_SELECTOR) {
                load4(XD.bsel[a], s);
                xargs_select(F, s, fr);
            }
            args_perm_point<0>(XD.g_m, F, wb, wt, di[0], zt[0], fl[0], fr[0], cc, cx, acc);
            args_perm_point<1>(XD.g_m, F, wb, wt, di[1], zt[1], fl[1], fr[1], cc, cx, acc);
            args_perm_point<2>(XD.g_m, F, wb, wt, di[2], zt[2], fl[2], fr[2], cc, cx, acc);
            args_perm_point<3>(XD.g_m, F, wb, wt, di[3], zt[3], fl[3], fr[3], cc, cx, acc);
        } else {
            Fq fl[PERM_ROWS], fr[PERM_ROWS];
            tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, XD.aop[a], load4, fl);
            tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, XD.bop[a], load4, fr);
            uint32_t sa[PERM_ROWS], mult[PERM_ROWS];
            xlookup_weights(XD, a, F, load4, sa, mult);
            xlookup_compose_point<0>(XD.g_m, F, wb, wt, di[0], zt[0], fl[0], fr[0], sa[0], mult[0], cc, cx, acc);
            xlookup_compose_point<1>(XD.g_m, F, wb, wt, di[1], zt[1], fl[1], fr[1], sa[1], mult[1], cc, cx, acc);
            xlookup_compose_point<2>(XD.g_m, F, wb, wt, di[2], zt[2], fl[2], fr[2], sa[2], mult[2], cc, cx, acc);
            xlookup_compose_point<3>(XD.g_m, F, wb, wt, di[3], zt[3], fl[3], fr[3], sa[3], mult[3], cc, cx, acc);
        }
        zkx_close_point<0>(perm, F, wc, di[4], cc, acc);
        zkx_close_point<1>(perm, F, wc, di[5], cc, acc);
        zkx_close_point<2>(perm, F, wc, di[6], cc, acc);
        zkx_close_point<3>(perm, F, wc, di[7], cc, acc);
    }
}

// ------------------------------------------------------------------------------------------------ host side
// Streams of smi_dev_random_fill this variant adds to zk_core.h's: the tails of the auxiliary columns, the salt of tree 2.
// Tree 3 (segments, R, salt) keeps ZK_STREAM_SALT2 = 5.
enum : uint64_t { ZK_STREAM_ARGS_TAIL = 6, ZK_STREAM_SALT_ARGS = 7 };

#define ZKX_BAD_RECORD "zk deep argument: the out-of-domain record is missing or has the wrong count"
#define ZKX_RECORD_CANONICAL "zk deep argument: an out-of-domain coordinate is not canonical"
#define ZKX_Z_IN_BASE_FIELD "zk deep argument: the out-of-domain point z lies in the base field"
#define ZKX_INCONSISTENT \
    "zk deep argument: out-of-domain consistency check fails: the derived AIR's constraints and the auxiliary quotients at z do not give the masked " \
    "segments' value"
#define ZKX_NO_LAYER "zk deep argument: FRI has no fold at this shape (F = 0), so there is no layer-0 coset to compare the masked DEEP quotient with"
static const char *const ZKX_SENTENCES[6] = {"zk deep argument coset openings: wrong length",
                                             "zk deep argument coset openings: malformed record",
                                             "zk deep argument coset openings: malformed path",
                                             "zk deep argument coset openings: authentication path does not verify",
                                             "zk deep argument coset openings: an opened value is not canonical",
                                             "zk deep argument coset openings: the masked DEEP quotient of the opened cosets is not the codeword value"};

inline uint32_t zkx_kt(uint64_t t) { return (uint32_t)(8 * t + 16); }

// smi_air_plan_deep_zk_xargs: the list's own checks, the refusals of the derived AIR, d = max(d_air + 1, 3 per permutation
// without a selector, 4 per permutation with one and per lookup), D, D' = ceil(D n / (n - k_s)) and the bounds of zk_plan
inline int zkx_plan(uint64_t p, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_xargs *xargs, uint32_t *degree, uint32_t *segments,
                    uint32_t *kt_out, uint32_t *ks_out, std::string *why, uint32_t *D_out = nullptr) {
    auto fail = [&](int code, const std::string &s) {
        if (why) *why = s;
        return code;
    };
    if (!cfg || !air) return fail(SMI_ERR_BAD_ARG, "air: null argument");
    ZkAir Z;
    int rc = zk_derive_air(p, 0, cfg, air, &Z, why, true);
    if (rc != SMI_OK) return rc;
    rc = xargs_validate(xargs, cfg->n_cols, air->n_periodic, why);
    if (rc != SMI_OK) return rc;
    // "Argument list: next-row operands": the row after the last active row is random under zero knowledge
    rc = xargs_refuse_next(xargs, "zk deep argument", "the zero-knowledge proofs take this-row operands only (the row after the last active row is random)", why);
    if (rc != SMI_OK) return rc;
    if ((p & 3) != 1) return fail(SMI_ERR_BAD_ARG, "xargs: p = 3 (mod 4): the quartic extension does not exist");
    uint32_t d = 0;
    rc = air_validate(p, cfg, &Z.air, &d, nullptr, why, false, true);
    if (rc != SMI_OK) return rc;
    rc = xargs_shared_rows(p, xargs, cfg->log_n, why);
    if (rc != SMI_OK) return rc;
    for (uint32_t a = 0; a < xargs->count; a++) d = std::max(d, xarg_degree(xargs->arg[a], true));
    const uint64_t B = 1ull << cfg->log_blowup;
    uint64_t D = 1;
    while (D < (uint64_t)d - 1 && D < (1ull << 32)) D <<= 1;
    if (D > B)
        return fail(SMI_ERR_BAD_ARG, "zk deep argument: D > 2^log_blowup: the composition of a degree-" + std::to_string(d) +
                                         " constraint has degree >= N and does not fit the evaluation domain");
    if (B < 4) return fail(SMI_ERR_EXPANSION_TOO_SMALL, "zk deep argument: 2^log_blowup < 4 (Fri::new's assert on the expansion factor)");
    const uint64_t n = 1ull << cfg->log_n, ks = zk_ks(cfg->num_colinearity_tests), L = n - ks;   // k_s < k_t < n / 2
    const uint64_t Dp = (D * n + L - 1) / L;
    if (4 * Dp + 5 > ZK_MAX_RECORD)
        return fail(SMI_ERR_BAD_ARG,
                    "zk deep argument: 4 D' + 5 = " + std::to_string(4 * Dp + 5) + " > 64: a leaf of the segment tree is wider than the leaf hash takes");
    if (cfg->n_cols + 1 > ZK_MAX_RECORD) return fail(SMI_ERR_BAD_ARG, "zk deep argument: W + 1 > 64: the trace tree has no room for the salt column");
    if (degree) *degree = d;
    if (segments) *segments = (uint32_t)Dp;
    if (D_out) *D_out = (uint32_t)D;
    if (kt_out) *kt_out = zkx_kt(cfg->num_colinearity_tests);
    if (ks_out) *ks_out = (uint32_t)ks;
    return SMI_OK;
}

// the groups of a proof: the trace and its salt; the auxiliary coordinates and their salt; the segments, R and their salt
inline DeepGroups zkx_groups(uint32_t W, uint32_t A, uint32_t Dp) {
    DeepGroups gr;
    gr.G = 3;
    gr.V[0] = W + 1;
    gr.V[1] = 4 * A + 1;
    gr.V[2] = 4 * Dp + 5;
    return gr;
}
// 9 + 32 (2 W + 2 A + D') + len_FRI4(N, B, t) + the three sections
inline size_t zkx_proof_len(const smi_stark_cfg *cfg, uint32_t A, uint32_t Dp, uint64_t *folds) {
    const uint32_t W = cfg->n_cols, log_N = cfg->log_n + cfg->log_blowup;
    const FriFold4Layout lay = fri_layout_fold4(deep_fri_cfg(cfg, 1));
    if (folds) *folds = lay.F;
    return 9 + 32 * (2 * (size_t)W + 2 * (size_t)A + Dp) + lay.proof_len + deep_coset_sections_len(zkx_groups(W, A, Dp), cfg->num_colinearity_tests, log_N);
}

// The left side of the consistency check: deep_ood_sides's over the DERIVED AIR (dair) plus the 3 A auxiliary quotients at z
// under the weights W + K + 3 a .. + 2.  xargs_aux_at_z gives bq_a and the wrapping transition quotient; wq_a carries
// E_A(z) = prod_{r = n_a}^{n - 1} (z - tau w^r), cq_a = (a_a - init_a) / (z - tau w^n_a).  ood: 4 (2 W + 2 A + D') values.
inline FqH zkx_ood_lhs(uint32_t p, uint32_t g, const smi_stark_cfg *cfg, const smi_air *dair, const smi_air_xargs *xargs, uint32_t w_n, const uint64_t ch[8],
                       const uint64_t *weights, const FqH &z, const uint64_t *ood) {
    const uint32_t W = cfg->n_cols, K = dair->n_constraints, Q = dair->n_periodic, A = xargs->count, tau = (uint32_t)cfg->trace_offset;
    const uint64_t n = 1ull << cfg->log_n, kt = zkx_kt(cfg->num_colinearity_tests), na = n - kt;
    FqH acc, unused;
    deep_ood_sides(p, g, cfg, dair, 0, w_n, weights, z, ood, &acc, &unused);
    std::vector<FqH> u(W), per(Q);
    for (uint32_t c = 0; c < W; c++) u[c] = fqh_of(ood + 4 * (size_t)c, p);
    for (uint32_t j = 0, at = 0; j < Q; at += 1u << dair->periodic_log_period[j], j++)
        per[j] = deep_periodic_at(dair, j, dair->periodic_value + at, cfg->log_n, tau, w_n, z, p, g);
    uint32_t al[4], ga[4];
    perm_challenges(p, ch, al, ga);
    const FqH alpha{{al[0], al[1], al[2], al[3]}}, gamma{{ga[0], ga[1], ga[2], ga[3]}};
    const FqH ixt = fqh_inv(fqh_sub(z, fqh(tau % p), p), p, g);
    const FqH izt = fqh_inv(fqh_sub(fqh_pow(z, n, p, g), fqh(host_powmod(tau, n, p)), p), p, g);
    uint32_t pt = host_mulmod(tau % p, host_powmod(w_n, na, p), p);   // tau w^n_a
    const FqH ict = fqh_inv(fqh_sub(z, fqh(pt), p), p, g);
    FqH ea = fqh(1 % p);
    for (uint64_t r = na; r < n; r++) {
        ea = fqh_mul(ea, fqh_sub(z, fqh(pt), p), p, g);
        pt = host_mulmod(pt, w_n, p);
    }
    for (uint32_t a = 0; a < A; a++) {
        const FqH ca = fqh_of(ood + 4 * (2 * (size_t)W + a), p), cb = fqh_of(ood + 4 * (2 * (size_t)W + A + a), p);
        FqH bq, wq;
        xargs_aux_at_z(p, g, W, xargs->arg[a], alpha, gamma, u.data(), per.data(), nullptr, nullptr, ca, cb, ixt, izt, &bq, &wq);   // no next-row operand: zkx_plan
        wq = fqh_mul(wq, ea, p, g);
        const FqH init = fqh((xargs->arg[a].kind & 0xffu) == SMI_ARG_PERM ? 1 % p : 0);
        const FqH cq = fqh_mul(fqh_sub(ca, init, p), ict, p, g);
        const uint64_t *wa = weights + 4 * ((size_t)W + K + 3 * (size_t)a);
        acc = fqh_add(acc, fqh_mul(fqh_of(wa, p), bq, p, g), p);
        acc = fqh_add(acc, fqh_mul(fqh_of(wa + 4, p), wq, p, g), p);
        acc = fqh_add(acc, fqh_mul(fqh_of(wa + 8, p), cq, p, g), p);
    }
    return acc;
}
