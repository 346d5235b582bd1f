// deep_core.h -- out-of-domain sampling (include/stark_mi.h, "Out-of-domain sampling"): the plan and the proof length, the
// lane bodies of the two kernels of deep.hip -- coefficient columns evaluated at points of F_q (deep_eval_kernel,
// deep_eval_combine_kernel) and the DEEP codeword (deep_compose_kernel) -- with the host tables they read, and the
// verifier's side in plain host arithmetic: the transcript, the out-of-domain consistency check with the constraint
// evaluator over F_q operands, and Q at one point from two opened rows.  Shared by the HIP kernels (deep.hip), the verifier
// (verify.hip, host) and the CPU emulator (emu_deep.cpp), which runs the same lane bodies and block split.
//
// Number forms.  Coefficients and extended cells are plain residues.  The powers of a point come from the host in
// Montgomery form coordinate by coordinate, so mont_mul(plain coefficient, .) is a plain coordinate of the product: a
// coefficient times a power is four base-field multiplies.  In the compose lane x, z, z w and the inverted denominators are
// Montgomery, the gammas Montgomery (the segment ones prepared, fri_core.h ExtMul), the accumulated numerators plain.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/stark_mi.h"
#include "air_core.h"
#include "fri_core.h"
#include "fri_plan.h"
#include "perm_core.h"
#include "transcript_core.h"

#define DEEP_ROWS 4                               // consecutive coefficients / points per lane: one 16-byte access per column
#define DEEP_BLOCK 256                            // lanes per workgroup
#define DEEP_TILE (DEEP_ROWS * DEEP_BLOCK)        // coefficients of one column a workgroup reduces
#define DEEP_MAX_SEGMENTS 16                      // 4 D <= 64: the widest row the leaf hash takes
#define DEEP_MAX_POINTS 2                         // smi_dev_poly_eval_ext: any one or two points
#define DEEP_MAX_SHIFTS SMI_AIR_MAX_WINDOW        // smi_dev_poly_eval_ext_shifts: z, z w, .. z w^(S-1), a table per point

// the sentences of the prover's refusal and of the verifier's own rejections (verify.hip; tests match on them)
#define DEEP_Z_IN_BASE_FIELD "deep: the out-of-domain point z lies in the base field"
#define DEEP_BAD_RECORD "deep: the out-of-domain record is missing or has the wrong count"
#define DEEP_RECORD_CANONICAL "deep: an out-of-domain coordinate is not canonical"
#define DEEP_INCONSISTENT "deep: out-of-domain consistency check fails: the constraints at z do not give the segments' value"
#define DEEP_NO_LAYER "deep: FRI has no fold at this shape, so there is no layer-0 triple to compare the DEEP quotient with"
static const char *const DEEP_SENTENCES[6] = {"deep openings: wrong length",
                                              "deep openings: malformed row",
                                              "deep openings: malformed path",
                                              "deep openings: authentication path does not verify",
                                              "deep openings: an opened value is not canonical",
                                              "deep openings: the DEEP quotient of the opened rows is not the codeword value"};

// ------------------------------------------------------------------------------------------------ evaluation
// Table of one launch, u32 words, P = n_points:
//   pw[k][e][j], j < DEEP_TILE  : coordinate e of z_k^j                      at (k * 4 + e) * DEEP_TILE + j
//   tp[k][j][e], j < DEEP_BLOCK : coordinate e of (z_k^DEEP_TILE)^j          at 4 P DEEP_TILE + (k * DEEP_BLOCK + j) * 4 + e
//   st[k][e]                    : coordinate e of (z_k^DEEP_TILE)^DEEP_BLOCK at 4 P (DEEP_TILE + DEEP_BLOCK) + 4 k + e
// all Montgomery.
inline size_t deep_eval_tab_words(uint32_t P) { return (size_t)P * (4 * DEEP_TILE + 4 * DEEP_BLOCK + 4); }
SMI_HD size_t deep_eval_tp_at(uint32_t P) { return (size_t)4 * P * DEEP_TILE; }
SMI_HD size_t deep_eval_st_at(uint32_t P) { return (size_t)4 * P * (DEEP_TILE + DEEP_BLOCK); }
inline uint64_t deep_eval_blocks(uint64_t n_coeffs) { return (n_coeffs + DEEP_TILE - 1) / DEEP_TILE; }

// one lane of deep_eval_kernel: its DEEP_ROWS coefficients a[q] against coordinate e of the powers, tw[e][q] -> the lane's
// share of the workgroup's partial sum, plain
SMI_HD void deep_eval_lane(const uint32_t a[DEEP_ROWS], const uint32_t tw[4][DEEP_ROWS], const Fp &F, uint32_t acc[4]) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
        uint32_t s = 0;
#pragma unroll
        for (int q = 0; q < DEEP_ROWS; q++) s = fp_add(s, mont_mul(a[q], tw[e][q], F), F.p);
        acc[e] = s;
    }
}
// one lane of deep_eval_combine_kernel: the partial sums tid, tid + DEEP_BLOCK, .. of one column and point (element b at
// part[b * pitch .. + 3], plain) by Horner in (z^DEEP_TILE)^DEEP_BLOCK from the top, then times (z^DEEP_TILE)^tid
SMI_HD void deep_eval_combine_lane(const uint32_t *part, uint32_t pitch, uint32_t nb, uint32_t tid, const uint32_t tp_m[4], const uint32_t st_m[4],
                                   uint32_t g_m, const Fp &F, uint32_t acc[4]) {
    acc[0] = acc[1] = acc[2] = acc[3] = 0;
    if (tid >= nb) return;
    const ExtMul S = ext_mul_prepare(st_m, g_m, F);
    uint32_t t[4];
    for (uint32_t m = (nb - 1 - tid) / DEEP_BLOCK;; m--) {
        const uint32_t *v = part + (size_t)(tid + m * DEEP_BLOCK) * pitch;
        ext_mul_prepared(acc, S, F, t);
#pragma unroll
        for (int e = 0; e < 4; e++) acc[e] = fp_add(t[e], v[e], F.p);
        if (!m) break;
    }
    const ExtMul T = ext_mul_prepare(tp_m, g_m, F);
    ext_mul_prepared(acc, T, F, t);
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e] = t[e];
}

// ------------------------------------------------------------------------------------------------ the DEEP codeword
// Table of one launch, u32 words:
//   gamma_c    (Montgomery)            at 4 c + e
//   gamma'_c   (Montgomery)            at 4 W + 4 c + e
//   gamma''_j  (prepared: b_m | gb_m)  at 8 W + 8 j + e, 8 W + 8 j + 4 + e
//   -C1 = -(sum_c gamma_c u_c + sum_j gamma''_j s_j), -C2 = -sum_c gamma'_c v_c (plain), z, z w (Montgomery): the last 16
inline size_t deep_tab_words(uint32_t W, uint32_t D) { return (size_t)8 * W + 8 * D + 16; }

// One lane: the DEEP_ROWS consecutive points x0, x0 omega, ..  load_t(c, v): extended trace column c at the four points;
// load_s(col, v): segment column col (4 j + e: coordinate e of H_j); out[e][q]: coordinate e of Q at point q, plain.
// The 2 DEEP_ROWS denominators x - z and x - z w share one F_q inversion; none is zero, since z and z w lie outside F_p.
template <class LoadT, class LoadS>
SMI_HD void deep_compose_points(const uint32_t *tab, uint32_t W, uint32_t D, uint32_t g_m, const Fp &F, uint32_t x0_m, uint32_t omega_m, LoadT load_t,
                                LoadS load_s, uint32_t out[4][DEEP_ROWS]) {
    const uint32_t p = F.p;
    const uint32_t *cst = tab + 8 * (size_t)W + 8 * (size_t)D;
    Fq dinv[2 * DEEP_ROWS];
    {
        Fq den[2 * DEEP_ROWS], pre[2 * DEEP_ROWS];
        uint32_t x = x0_m;
#pragma unroll
        for (int q = 0; q < DEEP_ROWS; q++) {
            den[q] = Fq{{fp_sub(x, cst[8], p), fp_neg(cst[9], p), fp_neg(cst[10], p), fp_neg(cst[11], p)}};
            den[DEEP_ROWS + q] = Fq{{fp_sub(x, cst[12], p), fp_neg(cst[13], p), fp_neg(cst[14], p), fp_neg(cst[15], p)}};
            x = mont_mul(x, omega_m, F);
        }
        pre[0] = den[0];
#pragma unroll
        for (int i = 1; i < 2 * DEEP_ROWS; i++) pre[i] = fq_mul(pre[i - 1], den[i], g_m, F);
        Fq inv = fq_inv(pre[2 * DEEP_ROWS - 1], g_m, F);
#pragma unroll
        for (int i = 2 * DEEP_ROWS - 1; i >= 0; i--) {
            dinv[i] = i ? fq_mul(inv, pre[i - 1], g_m, F) : inv;
            if (i) inv = fq_mul(inv, den[i], g_m, F);
        }
    }
    uint32_t a1[DEEP_ROWS][4], a2[DEEP_ROWS][4];
#pragma unroll
    for (int q = 0; q < DEEP_ROWS; q++)
#pragma unroll
        for (int e = 0; e < 4; e++) a1[q][e] = cst[e], a2[q][e] = cst[4 + e];
    for (uint32_t c = 0; c < W; c++) {
        uint32_t v[DEEP_ROWS];
        load_t(c, v);
        const uint32_t *g1 = tab + 4 * (size_t)c, *g2 = tab + 4 * (size_t)(W + c);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t b1 = g1[e], b2 = g2[e];
#pragma unroll
            for (int q = 0; q < DEEP_ROWS; q++) {
                a1[q][e] = fp_add(a1[q][e], mont_mul(v[q], b1, F), p);
                a2[q][e] = fp_add(a2[q][e], mont_mul(v[q], b2, F), p);
            }
        }
    }
    for (uint32_t j = 0; j < D; j++) {
        uint32_t h[4][DEEP_ROWS];
#pragma unroll
        for (int e = 0; e < 4; e++) load_s(4 * j + e, h[e]);
        ExtMul M;
#pragma unroll
        for (int e = 0; e < 4; e++) M.b_m[e] = tab[8 * (size_t)W + 8 * j + e], M.gb_m[e] = tab[8 * (size_t)W + 8 * j + 4 + e];
#pragma unroll
        for (int q = 0; q < DEEP_ROWS; q++) {
            const uint32_t hv[4] = {h[0][q], h[1][q], h[2][q], h[3][q]};
            uint32_t o[4];
            ext_mul_prepared(hv, M, F, o);
#pragma unroll
            for (int e = 0; e < 4; e++) a1[q][e] = fp_add(a1[q][e], o[e], p);
        }
    }
#pragma unroll
    for (int q = 0; q < DEEP_ROWS; q++) {
        const Fq n1{{a1[q][0], a1[q][1], a1[q][2], a1[q][3]}}, n2{{a2[q][0], a2[q][1], a2[q][2], a2[q][3]}};
        const Fq r1 = fq_mul(n1, dinv[q], g_m, F), r2 = fq_mul(n2, dinv[DEEP_ROWS + q], g_m, F);
#pragma unroll
        for (int e = 0; e < 4; e++) out[e][q] = fp_add(r1.c[e], r2.c[e], p);
    }
}

// ------------------------------------------------------------------------------------------------ ... under a transition window
// include/stark_mi.h, "AIR: transition windows": the trace is opened at z w^s for s < S (S = 3 or 4), so Q has S quotient
// groups.  Table of one launch, u32 words -- for S = 2 it is the table above:
//   gamma_{s,c} (Montgomery)            at 4 (s W + c) + e
//   gamma''_j   (prepared: b_m | gb_m)  at 4 S W + 8 j + e, 4 S W + 8 j + 4 + e
//   -C_s (plain; C_0 with the segments' sum) at 4 S W + 8 D + 4 s + e, then z w^s (Montgomery) at 4 S W + 8 D + 4 S + 4 s + e
inline size_t deep_window_tab_words(uint32_t W, uint32_t D, uint32_t S) { return (size_t)4 * S * W + 8 * D + 8 * S; }

// One lane of deep_compose_window_kernel: deep_compose_points with S accumulators a point.  The S DEEP_ROWS denominators
// x - z w^s share one F_q inversion, taken after the column loop; an inverse is used as soon as it is peeled off, so no
// array of inverses is kept, but the accumulators (16 S words) and the prefix products (16 S words) are live together.
template <int I, class Body>
SMI_HD void deep_steps_down(Body &body) {   // body(I), body(I - 1), .. body(0) with the index a compile-time constant
    body(std::integral_constant<int, I>{});
    if constexpr (I > 0) deep_steps_down<I - 1>(body);
}
template <int S, class LoadT, class LoadS>
SMI_HD void deep_compose_window_points(const uint32_t *tab, uint32_t W, uint32_t D, uint32_t g_m, const Fp &F, uint32_t x0_m, uint32_t omega_m, LoadT load_t,
                                       LoadS load_s, uint32_t out[4][DEEP_ROWS]) {
    const uint32_t p = F.p;
    const uint32_t *sg = tab + 4 * (size_t)S * W, *cst = sg + 8 * (size_t)D, *zs = cst + 4 * S;
    uint32_t a[S][DEEP_ROWS][4];
#pragma unroll
    for (int s = 0; s < S; s++)
#pragma unroll
        for (int q = 0; q < DEEP_ROWS; q++)
#pragma unroll
            for (int e = 0; e < 4; e++) a[s][q][e] = cst[4 * s + e];
    for (uint32_t c = 0; c < W; c++) {
        uint32_t v[DEEP_ROWS];
        load_t(c, v);
#pragma unroll
        for (int s = 0; s < S; s++) {
            const uint32_t *gs = tab + 4 * ((size_t)s * W + c);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t b = gs[e];
#pragma unroll
                for (int q = 0; q < DEEP_ROWS; q++) a[s][q][e] = fp_add(a[s][q][e], mont_mul(v[q], b, F), p);
            }
        }
    }
    for (uint32_t j = 0; j < D; j++) {
        uint32_t h[4][DEEP_ROWS];
#pragma unroll
        for (int e = 0; e < 4; e++) load_s(4 * j + e, h[e]);
        ExtMul M;
#pragma unroll
        for (int e = 0; e < 4; e++) M.b_m[e] = sg[8 * (size_t)j + e], M.gb_m[e] = sg[8 * (size_t)j + 4 + e];
#pragma unroll
        for (int q = 0; q < DEEP_ROWS; q++) {
            const uint32_t hv[4] = {h[0][q], h[1][q], h[2][q], h[3][q]};
            uint32_t o[4];
            ext_mul_prepared(hv, M, F, o);
#pragma unroll
            for (int e = 0; e < 4; e++) a[0][q][e] = fp_add(a[0][q][e], o[e], p);
        }
    }
    // den[s * DEEP_ROWS + q] = x_q - z w^s, recomputed where it is needed: one subtraction in coordinate 0
    uint32_t xq[DEEP_ROWS];
    xq[0] = x0_m;
#pragma unroll
    for (int q = 1; q < DEEP_ROWS; q++) xq[q] = mont_mul(xq[q - 1], omega_m, F);
    auto den = [&](int i) {
        const uint32_t *zw = zs + 4 * (i / DEEP_ROWS);
        return Fq{{fp_sub(xq[i % DEEP_ROWS], zw[0], p), fp_neg(zw[1], p), fp_neg(zw[2], p), fp_neg(zw[3], p)}};
    };
    Fq pre[S * DEEP_ROWS];
    pre[0] = den(0);
#pragma unroll
    for (int i = 1; i < S * DEEP_ROWS; i++) pre[i] = fq_mul(pre[i - 1], den(i), g_m, F);
    Fq inv = fq_inv(pre[S * DEEP_ROWS - 1], g_m, F);
    uint32_t r[DEEP_ROWS][4];
#pragma unroll
    for (int q = 0; q < DEEP_ROWS; q++)
#pragma unroll
        for (int e = 0; e < 4; e++) r[q][e] = 0;
    // 4 S steps of three F_q products each: more than an unroll pragma takes, so the steps are instantiated one by one
    auto step = [&](auto I) {
        constexpr int i = decltype(I)::value, s = i / DEEP_ROWS, q = i % DEEP_ROWS;
        const Fq di = i ? fq_mul(inv, pre[i ? i - 1 : 0], g_m, F) : inv;
        if (i) inv = fq_mul(inv, den(i), g_m, F);
        const Fq t = fq_mul(Fq{{a[s][q][0], a[s][q][1], a[s][q][2], a[s][q][3]}}, di, g_m, F);
#pragma unroll
        for (int e = 0; e < 4; e++) r[q][e] = fp_add(r[q][e], t.c[e], p);
    };
    deep_steps_down<S * DEEP_ROWS - 1>(step);
#pragma unroll
    for (int q = 0; q < DEEP_ROWS; q++)
#pragma unroll
        for (int e = 0; e < 4; e++) out[e][q] = r[q][e];
}

// ------------------------------------------------------------------------------------------------ ... with auxiliary columns
// include/stark_mi.h, "Out-of-domain sampling with an argument list": A committed F_q columns c_a, stored as 4 A extended
// coordinate columns, are opened at z and z w like the trace.  Table of one launch, u32 words:
//   gamma_c    (Montgomery)            at 4 c + e
//   gamma'_c   (Montgomery)            at 4 W + 4 c + e
//   delta_a    (prepared: b_m | gb_m)  at 8 W + 16 a + e,      8 W + 16 a + 4 + e
//   delta'_a   (prepared)              at 8 W + 16 a + 8 + e,  8 W + 16 a + 12 + e
//   gamma''_j  (prepared)              at 8 W + 16 A + 8 j + e, 8 W + 16 A + 8 j + 4 + e
//   -C1 = -(sum_c gamma_c u_c + sum_a delta_a a_a + sum_j gamma''_j s_j), -C2 = -(sum_c gamma'_c v_c + sum_a delta'_a b_a)
//   (plain), z, z w (Montgomery): the last 16
inline size_t deep_args_tab_words(uint32_t W, uint32_t A, uint32_t D) { return (size_t)8 * W + 16 * (size_t)A + 8 * D + 16; }

// the 2 DEEP_ROWS inverted denominators 1 / (x - z), 1 / (x - z w) of a lane under one F_q inversion (cst: the table's last
// 16 words); none is zero, since z and z w lie outside F_p
SMI_HD void deep_lane_inverses(const uint32_t *cst, uint32_t g_m, const Fp &F, uint32_t x0_m, uint32_t omega_m, Fq dinv[2 * DEEP_ROWS]) {
    const uint32_t p = F.p;
    Fq den[2 * DEEP_ROWS], pre[2 * DEEP_ROWS];
    uint32_t x = x0_m;
#pragma unroll
    for (int q = 0; q < DEEP_ROWS; q++) {
        den[q] = Fq{{fp_sub(x, cst[8], p), fp_neg(cst[9], p), fp_neg(cst[10], p), fp_neg(cst[11], p)}};
        den[DEEP_ROWS + q] = Fq{{fp_sub(x, cst[12], p), fp_neg(cst[13], p), fp_neg(cst[14], p), fp_neg(cst[15], p)}};
        x = mont_mul(x, omega_m, F);
    }
    pre[0] = den[0];
#pragma unroll
    for (int i = 1; i < 2 * DEEP_ROWS; i++) pre[i] = fq_mul(pre[i - 1], den[i], g_m, F);
    Fq inv = fq_inv(pre[2 * DEEP_ROWS - 1], g_m, F);
#pragma unroll
    for (int i = 2 * DEEP_ROWS - 1; i >= 0; i--) {
        dinv[i] = i ? fq_mul(inv, pre[i - 1], g_m, F) : inv;
        if (i) inv = fq_mul(inv, den[i], g_m, F);
    }
}

// One lane of deep_compose_args_kernel: deep_compose_points with load_c(col, v): auxiliary coordinate column col (4 a + e:
// coordinate e of c_a) at the four points.  One column stream is live at a time -- a trace column's four words, or the
// sixteen of one F_q column -- next to the 2 x 4 x 4 accumulator words and the 8 inverses; the gammas are wave-uniform
// table reads.
template <class LoadT, class LoadC, class LoadS>
SMI_HD void deep_compose_args_points(const uint32_t *tab, uint32_t W, uint32_t A, uint32_t D, uint32_t g_m, const Fp &F, uint32_t x0_m, uint32_t omega_m,
                                     LoadT load_t, LoadC load_c, LoadS load_s, uint32_t out[4][DEEP_ROWS]) {
    const uint32_t p = F.p;
    const uint32_t *aux = tab + 8 * (size_t)W, *sg = aux + 16 * (size_t)A, *cst = sg + 8 * (size_t)D;
    Fq dinv[2 * DEEP_ROWS];
    deep_lane_inverses(cst, g_m, F, x0_m, omega_m, dinv);
    uint32_t a1[DEEP_ROWS][4], a2[DEEP_ROWS][4];
#pragma unroll
    for (int q = 0; q < DEEP_ROWS; q++)
#pragma unroll
        for (int e = 0; e < 4; e++) a1[q][e] = cst[e], a2[q][e] = cst[4 + e];
    for (uint32_t c = 0; c < W; c++) {
        uint32_t v[DEEP_ROWS];
        load_t(c, v);
        const uint32_t *g1 = tab + 4 * (size_t)c, *g2 = tab + 4 * (size_t)(W + c);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t b1 = g1[e], b2 = g2[e];
#pragma unroll
            for (int q = 0; q < DEEP_ROWS; q++) {
                a1[q][e] = fp_add(a1[q][e], mont_mul(v[q], b1, F), p);
                a2[q][e] = fp_add(a2[q][e], mont_mul(v[q], b2, F), p);
            }
        }
    }
    // Range: ext_mul_prepared (fri_core.h) sums four 32 x 32 products of a plain coordinate with a Montgomery word, and wants
    // every plain coordinate below p so that the sum stays below p 2^32.  The first factor here is always a loaded cell as it
    // stands -- a canonical residue of the extended column, never a partial sum --, each product comes back reduced, and the
    // accumulators a1, a2 only ever see fp_add of two residues: they stay below p for the fq_mul at the end, whatever A and D.
    for (uint32_t a = 0; a < A; a++) {
        uint32_t h[4][DEEP_ROWS];
#pragma unroll
        for (int e = 0; e < 4; e++) load_c(4 * a + e, h[e]);
        ExtMul M1, M2;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            M1.b_m[e] = aux[16 * (size_t)a + e], M1.gb_m[e] = aux[16 * (size_t)a + 4 + e];
            M2.b_m[e] = aux[16 * (size_t)a + 8 + e], M2.gb_m[e] = aux[16 * (size_t)a + 12 + e];
        }
#pragma unroll
        for (int q = 0; q < DEEP_ROWS; q++) {
            const uint32_t hv[4] = {h[0][q], h[1][q], h[2][q], h[3][q]};
            uint32_t o1[4], o2[4];
            ext_mul_prepared(hv, M1, F, o1);
            ext_mul_prepared(hv, M2, F, o2);
#pragma unroll
            for (int e = 0; e < 4; e++) a1[q][e] = fp_add(a1[q][e], o1[e], p), a2[q][e] = fp_add(a2[q][e], o2[e], p);
        }
    }
    for (uint32_t j = 0; j < D; j++) {
        uint32_t h[4][DEEP_ROWS];
#pragma unroll
        for (int e = 0; e < 4; e++) load_s(4 * j + e, h[e]);
        ExtMul M;
#pragma unroll
        for (int e = 0; e < 4; e++) M.b_m[e] = sg[8 * (size_t)j + e], M.gb_m[e] = sg[8 * (size_t)j + 4 + e];
#pragma unroll
        for (int q = 0; q < DEEP_ROWS; q++) {
            const uint32_t hv[4] = {h[0][q], h[1][q], h[2][q], h[3][q]};
            uint32_t o[4];
            ext_mul_prepared(hv, M, F, o);
#pragma unroll
            for (int e = 0; e < 4; e++) a1[q][e] = fp_add(a1[q][e], o[e], p);
        }
    }
#pragma unroll
    for (int q = 0; q < DEEP_ROWS; q++) {
        const Fq n1{{a1[q][0], a1[q][1], a1[q][2], a1[q][3]}}, n2{{a2[q][0], a2[q][1], a2[q][2], a2[q][3]}};
        const Fq r1 = fq_mul(n1, dinv[q], g_m, F), r2 = fq_mul(n2, dinv[DEEP_ROWS + q], g_m, F);
#pragma unroll
        for (int e = 0; e < 4; e++) out[e][q] = fp_add(r1.c[e], r2.c[e], p);
    }
}

// ------------------------------------------------------------------------------------------------ host side: F_q, plain
struct FqH {
    uint32_t c[4];
};
inline FqH fqh(uint32_t v) { return FqH{{v, 0, 0, 0}}; }
inline FqH fqh_of(const uint64_t *v, uint32_t p) { return FqH{{(uint32_t)(v[0] % p), (uint32_t)(v[1] % p), (uint32_t)(v[2] % p), (uint32_t)(v[3] % p)}}; }
inline FqH fqh_add(const FqH &a, const FqH &b, uint32_t p) { return FqH{{fp_add(a.c[0], b.c[0], p), fp_add(a.c[1], b.c[1], p), fp_add(a.c[2], b.c[2], p), fp_add(a.c[3], b.c[3], p)}}; }
inline FqH fqh_sub(const FqH &a, const FqH &b, uint32_t p) { return FqH{{fp_sub(a.c[0], b.c[0], p), fp_sub(a.c[1], b.c[1], p), fp_sub(a.c[2], b.c[2], p), fp_sub(a.c[3], b.c[3], p)}}; }
inline FqH fqh_mul(const FqH &a, const FqH &b, uint32_t p, uint32_t g) {
    FqH o;
    ext_mul_host(p, g, a.c, b.c, o.c);
    return o;
}
inline FqH fqh_scale(const FqH &a, uint32_t k, uint32_t p) { return FqH{{host_mulmod(a.c[0], k, p), host_mulmod(a.c[1], k, p), host_mulmod(a.c[2], k, p), host_mulmod(a.c[3], k, p)}}; }
inline FqH fqh_inv(const FqH &a, uint32_t p, uint32_t g) {   // a != 0
    FqH o{{0, 0, 0, 0}};
    (void)ext_inv_host(p, g, a.c, o.c);
    return o;
}
inline FqH fqh_pow(FqH b, uint64_t e, uint32_t p, uint32_t g) {
    FqH r = fqh(1 % p);
    while (e) {
        if (e & 1) r = fqh_mul(r, b, p, g);
        b = fqh_mul(b, b, p, g);
        e >>= 1;
    }
    return r;
}
inline bool fqh_eq(const FqH &a, const FqH &b) { return a.c[0] == b.c[0] && a.c[1] == b.c[1] && a.c[2] == b.c[2] && a.c[3] == b.c[3]; }
inline bool fqh_in_base(const FqH &a) { return !(a.c[1] | a.c[2] | a.c[3]); }

// the table of deep_eval_kernel / deep_eval_combine_kernel for the P points z[k] (plain coordinates)
inline void deep_eval_build(const Fp &F, uint32_t g, uint32_t P, const FqH *z, std::vector<uint32_t> *tab) {
    const uint32_t p = F.p;
    tab->assign(deep_eval_tab_words(P), 0);
    uint32_t *t = tab->data();
    for (uint32_t k = 0; k < P; k++) {
        FqH pw = fqh(1 % p);
        for (uint32_t j = 0; j < DEEP_TILE; j++) {
            for (int e = 0; e < 4; e++) t[(size_t)(k * 4 + e) * DEEP_TILE + j] = air_to_m(pw.c[e], p);
            pw = fqh_mul(pw, z[k], p, g);
        }
        const FqH zt = pw;   // z^DEEP_TILE
        pw = fqh(1 % p);
        for (uint32_t j = 0; j < DEEP_BLOCK; j++) {
            for (int e = 0; e < 4; e++) t[deep_eval_tp_at(P) + (size_t)(k * DEEP_BLOCK + j) * 4 + e] = air_to_m(pw.c[e], p);
            pw = fqh_mul(pw, zt, p, g);
        }
        for (int e = 0; e < 4; e++) t[deep_eval_st_at(P) + 4 * k + e] = air_to_m(pw.c[e], p);
    }
}

// the table of deep_compose_kernel (S = 2) and deep_compose_window_kernel.  ood: the record's 4 (S W + D) canonical values
// (u_{s,c} s-major, then s_j); ch: as many unreduced challenges in that order; w_n = omega_n
inline void deep_compose_build(const Fp &F, uint32_t g, uint32_t W, uint32_t D, uint32_t w_n, const FqH &z, const uint64_t *ood, const uint64_t *ch,
                               std::vector<uint32_t> *tab, uint32_t S = 2) {
    const uint32_t p = F.p;
    tab->assign(deep_window_tab_words(W, D, S), 0);   // S = 2: deep_tab_words(W, D)
    uint32_t *t = tab->data();
    FqH cs[SMI_AIR_MAX_WINDOW] = {fqh(0), fqh(0), fqh(0), fqh(0)};
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t c = 0; c < W; c++) {
            const size_t i = (size_t)s * W + c;
            const FqH gs = fqh_of(ch + 4 * i, p);
            for (int e = 0; e < 4; e++) t[4 * i + e] = air_to_m(gs.c[e], p);
            cs[s] = fqh_add(cs[s], fqh_mul(gs, fqh_of(ood + 4 * i, p), p, g), p);
        }
    uint32_t *sg = t + 4 * (size_t)S * W;
    for (uint32_t j = 0; j < D; j++) {
        const FqH g3 = fqh_of(ch + 4 * ((size_t)S * W + j), p);
        for (int e = 0; e < 4; e++) {
            sg[8 * j + e] = air_to_m(g3.c[e], p);
            sg[8 * j + 4 + e] = air_to_m(host_mulmod(g3.c[e], g, p), p);
        }
        cs[0] = fqh_add(cs[0], fqh_mul(g3, fqh_of(ood + 4 * ((size_t)S * W + j), p), p, g), p);
    }
    uint32_t *cst = sg + 8 * (size_t)D;
    FqH zw = z;
    for (uint32_t s = 0; s < S; s++) {
        for (int e = 0; e < 4; e++) {
            cst[4 * s + e] = fp_neg(cs[s].c[e], p);
            cst[4 * S + 4 * s + e] = air_to_m(zw.c[e], p);
        }
        zw = fqh_scale(zw, w_n, p);
    }
}

// ------------------------------------------------------------------------------------------------ plan, layout, transcript
// smi_air_plan_deep: smi_air_plan's checks without its bound on E, then D <= B, B >= 4, 4 D <= 64
// max_window: 2 for the callers that prove a list or a derived AIR; the plain entry points pass SMI_AIR_MAX_WINDOW
inline int deep_plan(uint64_t p, const smi_stark_cfg *cfg, const smi_air *air, uint32_t *degree, uint32_t *segments, std::string *why,
                     uint32_t max_window = 2) {
    auto fail = [&](int code, const std::string &s) {
        if (why) *why = s;
        return code;
    };
    uint32_t d = 0;
    const int rc = air_validate(p, cfg, air, &d, nullptr, why, false, true, max_window);
    if (rc != SMI_OK) return rc;
    if ((p & 3) != 1) return fail(SMI_ERR_BAD_ARG, "deep: p = 3 (mod 4): the quartic extension does not exist");
    const uint64_t B = 1ull << cfg->log_blowup;
    const uint64_t D = air_segments(d, air_window(air), 1ull << cfg->log_n);
    if (D > B)
        return fail(SMI_ERR_BAD_ARG, "deep: D > 2^log_blowup: the composition of a degree-" + std::to_string(d) + " constraint has degree >= N and does not fit the evaluation domain");
    if (B < 4) return fail(SMI_ERR_EXPANSION_TOO_SMALL, "deep: 2^log_blowup < 4 (Fri::new's assert on the expansion factor)");
    if (4 * D > 64) return fail(SMI_ERR_BAD_ARG, "deep: 4 D > 64: a row of the segment tree is wider than the leaf hash takes");
    if (degree) *degree = d;
    if (segments) *segments = (uint32_t)D;
    return SMI_OK;
}
inline smi_fri_cfg deep_fri_cfg(const smi_stark_cfg *cfg, uint64_t omega_N) {
    smi_fri_cfg fc;
    fc.omega = omega_N;
    fc.offset = cfg->lde_offset;
    fc.domain_length = 1ull << (cfg->log_n + cfg->log_blowup);
    fc.expansion_factor = 1ull << cfg->log_blowup;
    fc.num_colinearity_tests = cfg->num_colinearity_tests;
    return fc;
}
// 9 + 32 (S W + D) + len_FRI(N, B, t) + the two opening sections of two rows per test
inline size_t deep_proof_len(const smi_stark_cfg *cfg, uint32_t D, uint32_t S = 2) {
    const uint64_t W = cfg->n_cols, t = cfg->num_colinearity_tests, log_N = cfg->log_n + cfg->log_blowup;
    const smi_fri_cfg fc = deep_fri_cfg(cfg, 1);
    return (size_t)(9 + 32 * (S * W + D) + fri_layout_ext(fc, true).proof_len + 2 * t * (9 + 8 * W) + 2 * t * (9 + 32 * log_N) + 2 * t * (9 + 32ull * D) +
                    2 * t * (9 + 32 * log_N));
}

// The transcript in its three steps (prover and verifier): root_1 and the weights; root_2 and z; the record and the gammas.
inline void deep_transcript_weights(Transcript &T, const uint8_t root1[32], uint32_t W, uint32_t K, std::vector<uint64_t> *weights) {
    transcript_ext(T, root1, W, K, weights);
}
inline void deep_transcript_z(Transcript &T, const uint8_t root2[32], uint32_t W, uint32_t K, uint64_t z[4]) {
    std::vector<uint64_t> ch;
    transcript_indexed(T, root2, 4 * ((uint64_t)W + K), 4, &ch);
    for (int e = 0; e < 4; e++) z[e] = ch[e];
}
inline void deep_transcript_gammas(Transcript &T, const uint64_t *ood, uint32_t W, uint32_t K, uint32_t D, std::vector<uint64_t> *gammas, uint32_t S = 2) {
    const uint64_t cnt = 4 * (S * (uint64_t)W + D);
    for (uint64_t i = 0; i < cnt; i++) T.absorb_index(ood[i]);   // the payload: every value as 8 little-endian bytes
    for (uint64_t m = 0; m < cnt; m++) {
        T.absorb_index(4 * ((uint64_t)W + K) + 4 + m);
        gammas->push_back(T.challenge());
    }
}

// ------------------------------------------------------------------------------------------------ the verifier's side
// C_k over F_q operands in smi_air's numbering: X[v], v < S (W + Q)
inline FqH deep_constraint(const smi_air *air, uint32_t k, const FqH *X, uint32_t p, uint32_t g) {
    FqH ck = fqh(0);
    for (uint32_t t = air->constraint_first_term[k]; t < air->constraint_first_term[k + 1]; t++) {
        FqH m = fqh((uint32_t)(air->term_coeff[t] % p));
        for (uint32_t f = air->term_first_factor[t]; f < air->term_first_factor[t + 1]; f++)
            m = fqh_mul(m, fqh_pow(X[air->factor_var[f]], air->factor_exp[f], p, g), p, g);
        ck = fqh_add(ck, m, p);
    }
    return ck;
}
// pi_j(x) = q_j(y), y = (x / tau)^(n / P_j), by the barycentric form over the P_j-th roots of unity:
// q(y) = (y^P - 1) / P * sum_r v_r w_P^r / (y - w_P^r); for x outside F_p no y is such a root (an n-th root of unity of
// F_q lies in F_p).  One F_q inversion per column and point (Montgomery's trick over the P denominators).
inline FqH deep_periodic_at(const smi_air *air, uint32_t j, const uint64_t *vals, uint32_t log_n, uint32_t tau, uint32_t w_n, const FqH &x, uint32_t p,
                            uint32_t g) {
    const uint32_t l = air->periodic_log_period[j];
    const uint64_t P = 1ull << l, n = 1ull << log_n;
    const FqH y = fqh_pow(fqh_scale(x, host_powmod(tau, p - 2, p), p), n / P, p, g);
    const uint32_t wP = host_powmod(w_n, n / P, p);
    std::vector<FqH> den(P), pre(P);
    uint32_t wr = 1 % p;
    for (uint64_t r = 0; r < P; r++) {
        den[r] = fqh_sub(y, fqh(wr), p);
        pre[r] = r ? fqh_mul(pre[r - 1], den[r], p, g) : den[r];
        wr = host_mulmod(wr, wP, p);
    }
    FqH inv = fqh_inv(pre[P - 1], p, g), acc = fqh(0);
    const uint32_t wP_inv = host_powmod(wP, p - 2, p);
    wr = host_powmod(wP, P - 1, p);
    for (uint64_t r = P; r-- > 0;) {
        const FqH di = r ? fqh_mul(inv, pre[r - 1], p, g) : inv;
        if (r) inv = fqh_mul(inv, den[r], p, g);
        acc = fqh_add(acc, fqh_scale(di, host_mulmod((uint32_t)(vals[r] % p), wr, p), p), p);
        wr = host_mulmod(wr, wP_inv, p);
    }
    const FqH zp = fqh_sub(fqh_pow(y, P, p, g), fqh(1 % p), p);
    return fqh_scale(fqh_mul(acc, zp, p, g), host_powmod((uint32_t)(P % p), p - 2, p), p);
}
// Both sides of the out-of-domain consistency check for a z outside F_p:
//   lhs = sum_c w_c term_c(z) + sum_k w_{W+k} tq_k(z) from u = f(z), v = f(z w);   rhs = sum_j z^(j n) s_j.
// weights: the 4 (W + K) unreduced challenges; ood: the record's 4 (2 W + D) canonical values; w_n = omega_n.
// Under a window of S = air_window(air) rows the record holds u_{s,c} = f_c(z w^s) s-major, 4 (S W + D) values, the
// operands are X[s W + c] = u_{s,c} and X[S W + s Q + j] = pi_j(z w^s), and the numerator carries the S - 1 exemption roots.
inline void deep_ood_sides(uint32_t p, uint32_t g, const smi_stark_cfg *cfg, const smi_air *air, uint32_t D, uint32_t w_n, const uint64_t *weights, const FqH &z,
                           const uint64_t *ood, FqH *lhs, FqH *rhs) {
    const uint32_t W = cfg->n_cols, K = air->n_constraints, Q = air->n_periodic, tau = (uint32_t)cfg->trace_offset, S = air_window(air);
    const uint64_t n = 1ull << cfg->log_n;
    FqH acc = fqh(0);
    for (uint32_t c = 0; c < W; c++) {
        FqH term = fqh_of(ood + 4 * (size_t)c, p);
        std::vector<uint32_t> r, val;
        for (uint32_t b = 0; b < air->n_boundary; b++)
            if (air->boundary_col[b] == c) {
                r.push_back(host_mulmod(tau, host_powmod(w_n, air->boundary_row[b], p), p));
                val.push_back((uint32_t)(air->boundary_value[b] % p));
            }
        if (!r.empty()) {   // I_c(z) in Lagrange form, Z_c(z) = prod (z - r_j)
            FqH ix = fqh(0), zc = fqh(1 % p);
            for (size_t j = 0; j < r.size(); j++) {
                FqH num = fqh(1 % p);
                uint32_t den = 1 % p;
                for (size_t i = 0; i < r.size(); i++) {
                    if (i == j) continue;
                    num = fqh_mul(num, fqh_sub(z, fqh(r[i]), p), p, g);
                    den = host_mulmod(den, fp_sub(r[j], r[i], p), p);
                }
                ix = fqh_add(ix, fqh_scale(num, host_mulmod(val[j], host_powmod(den, p - 2, p), p), p), p);
                zc = fqh_mul(zc, fqh_sub(z, fqh(r[j]), p), p, g);
            }
            term = fqh_mul(fqh_sub(term, ix, p), fqh_inv(zc, p, g), p, g);
        }
        acc = fqh_add(acc, fqh_mul(fqh_of(weights + 4 * (size_t)c, p), term, p, g), p);
    }
    if (K) {
        std::vector<FqH> X((size_t)S * (W + Q));
        for (size_t i = 0; i < (size_t)S * W; i++) X[i] = fqh_of(ood + 4 * i, p);
        FqH zw = z;
        for (uint32_t s = 0; s < S; s++) {
            for (uint32_t j = 0, at = 0; j < Q; at += 1u << air->periodic_log_period[j], j++)
                X[(size_t)S * W + (size_t)s * Q + j] = deep_periodic_at(air, j, air->periodic_value + at, cfg->log_n, tau, w_n, zw, p, g);
            zw = fqh_scale(zw, w_n, p);
        }
        FqH ex = fqh(1 % p);   // prod_{s = 1 .. S-1} (z - tau w^(n-s))
        for (uint32_t s = 1; s < S; s++) ex = fqh_mul(ex, fqh_sub(z, fqh(host_mulmod(tau, host_powmod(w_n, n - s, p), p)), p), p, g);
        const FqH zt = fqh_mul(ex, fqh_inv(fqh_sub(fqh_pow(z, n, p, g), fqh(host_powmod(tau, n, p)), p), p, g), p, g);
        for (uint32_t k = 0; k < K; k++)
            acc = fqh_add(acc, fqh_mul(fqh_of(weights + 4 * (size_t)(W + k), p), fqh_mul(deep_constraint(air, k, X.data(), p, g), zt, p, g), p, g), p);
    }
    *lhs = acc;
    const FqH zn = fqh_pow(z, n, p, g);
    FqH r = fqh(0), pw = fqh(1 % p);
    for (uint32_t j = 0; j < D; j++) {
        r = fqh_add(r, fqh_mul(pw, fqh_of(ood + 4 * ((size_t)S * W + j), p), p, g), p);
        pw = fqh_mul(pw, zn, p, g);
    }
    *rhs = r;
}
// Q(x) from the opened rows at x: trow = the W trace values, srow = the 4 D segment values (canonical)
// S: the window; the record and the gammas hold S W + D elements, group s over the denominator x - z w^s
inline FqH deep_q_at(uint32_t p, uint32_t g, uint32_t W, uint32_t D, uint32_t w_n, uint32_t x, const FqH &z, const uint64_t *ood, const uint64_t *gammas,
                     const uint64_t *trow, const uint64_t *srow, uint32_t S = 2) {
    FqH q = fqh(0), zw = z;
    for (uint32_t s = 0; s < S; s++) {
        FqH num = fqh(0);
        for (uint32_t c = 0; c < W; c++) {
            const size_t i = (size_t)s * W + c;
            num = fqh_add(num, fqh_mul(fqh_of(gammas + 4 * i, p), fqh_sub(fqh((uint32_t)trow[c]), fqh_of(ood + 4 * i, p), p), p, g), p);
        }
        for (uint32_t j = 0; j < D && !s; j++) {
            const size_t i = (size_t)S * W + j;
            num = fqh_add(num, fqh_mul(fqh_of(gammas + 4 * i, p), fqh_sub(fqh_of(srow + 4 * (size_t)j, p), fqh_of(ood + 4 * i, p), p), p, g), p);
        }
        q = fqh_add(q, fqh_mul(num, fqh_inv(fqh_sub(fqh(x), zw, p), p, g), p, g), p);
        zw = fqh_scale(zw, w_n, p);
    }
    return q;
}

// ------------------------------------------------------------------------------------------------ ... with an argument list
// include/stark_mi.h, "Out-of-domain sampling with an argument list".  The record holds 4 (2 W + 2 A + D) values in the
// order u, v, a, b, s; the challenges follow it: gamma, gamma', delta, delta', gamma''.  The plan, the auxiliary quotients at
// z and the consistency check need the list and live in xargs_core.h.
static const char *const DEEP_ARGS_SENTENCES[6] = {"deep argument openings: wrong length",
                                                   "deep argument openings: malformed row",
                                                   "deep argument openings: malformed path",
                                                   "deep argument openings: authentication path does not verify",
                                                   "deep argument openings: an opened value is not canonical",
                                                   "deep argument openings: the DEEP quotient of the opened rows is not the codeword value"};
#define DEEP_ARGS_INCONSISTENT \
    "deep arguments: out-of-domain consistency check fails: the constraints and the auxiliary quotients at z do not give the segments' value"

inline size_t deep_args_record(uint32_t W, uint32_t A, uint32_t D) { return 4 * (2 * (size_t)W + 2 * (size_t)A + D); }

// the table of deep_compose_args_kernel.  ood: the record's canonical values; ch: as many unreduced challenges; w_n = omega_n
inline void deep_compose_args_build(const Fp &F, uint32_t g, uint32_t W, uint32_t A, uint32_t D, uint32_t w_n, const FqH &z, const uint64_t *ood,
                                    const uint64_t *ch, std::vector<uint32_t> *tab) {
    const uint32_t p = F.p;
    tab->assign(deep_args_tab_words(W, A, D), 0);
    uint32_t *t = tab->data();
    FqH c1 = fqh(0), c2 = fqh(0);
    auto prepared = [&](const FqH &v, uint32_t *at) {
        for (int e = 0; e < 4; e++) at[e] = air_to_m(v.c[e], p), at[4 + e] = air_to_m(host_mulmod(v.c[e], g, p), p);
    };
    for (uint32_t c = 0; c < W; c++) {
        const FqH g1 = fqh_of(ch + 4 * (size_t)c, p), g2 = fqh_of(ch + 4 * (size_t)(W + c), p);
        for (int e = 0; e < 4; e++) t[4 * c + e] = air_to_m(g1.c[e], p), t[4 * (W + c) + e] = air_to_m(g2.c[e], p);
        c1 = fqh_add(c1, fqh_mul(g1, fqh_of(ood + 4 * (size_t)c, p), p, g), p);
        c2 = fqh_add(c2, fqh_mul(g2, fqh_of(ood + 4 * (size_t)(W + c), p), p, g), p);
    }
    for (uint32_t a = 0; a < A; a++) {
        const size_t ia = 2 * (size_t)W + a, ib = 2 * (size_t)W + A + a;
        const FqH d1 = fqh_of(ch + 4 * ia, p), d2 = fqh_of(ch + 4 * ib, p);
        prepared(d1, t + 8 * (size_t)W + 16 * (size_t)a);
        prepared(d2, t + 8 * (size_t)W + 16 * (size_t)a + 8);
        c1 = fqh_add(c1, fqh_mul(d1, fqh_of(ood + 4 * ia, p), p, g), p);
        c2 = fqh_add(c2, fqh_mul(d2, fqh_of(ood + 4 * ib, p), p, g), p);
    }
    for (uint32_t j = 0; j < D; j++) {
        const size_t is = 2 * (size_t)W + 2 * (size_t)A + j;
        const FqH g3 = fqh_of(ch + 4 * is, p);
        prepared(g3, t + 8 * (size_t)W + 16 * (size_t)A + 8 * (size_t)j);
        c1 = fqh_add(c1, fqh_mul(g3, fqh_of(ood + 4 * is, p), p, g), p);
    }
    uint32_t *cst = t + 8 * (size_t)W + 16 * (size_t)A + 8 * (size_t)D;
    const FqH zw = fqh_scale(z, w_n, p);
    for (int e = 0; e < 4; e++) {
        cst[e] = fp_neg(c1.c[e], p);
        cst[4 + e] = fp_neg(c2.c[e], p);
        cst[8 + e] = air_to_m(z.c[e], p);
        cst[12 + e] = air_to_m(zw.c[e], p);
    }
}

// 9 + 32 (2W + 2A + D) + len_FRI(N, B, t) + the three opening sections of two rows per test
inline size_t deep_args_proof_len(const smi_stark_cfg *cfg, uint32_t A, uint32_t D) {
    const uint64_t W = cfg->n_cols, t = cfg->num_colinearity_tests, log_N = cfg->log_n + cfg->log_blowup;
    const smi_fri_cfg fc = deep_fri_cfg(cfg, 1);
    const uint64_t path = 2 * t * (9 + 32 * log_N);
    return (size_t)(9 + 32 * (2 * W + 2 * (uint64_t)A + D) + fri_layout_ext(fc, true).proof_len + 2 * t * (9 + 8 * W) + path + 2 * t * (9 + 32ull * A) + path +
                    2 * t * (9 + 32ull * D) + path);
}

// The transcript's last two steps (the first two are transcript_perm_challenges and transcript_args_weights): root_3 and z
// under the counters 8 + 4 NW + e, then the record and the gammas under the counters after those; NW = W + K + 2 A
inline void deep_args_transcript_z(Transcript &T, const uint8_t root3[32], uint64_t NW, uint64_t z[4]) {
    std::vector<uint64_t> ch;
    transcript_indexed(T, root3, 8 + 4 * NW, 4, &ch);
    for (int e = 0; e < 4; e++) z[e] = ch[e];
}
inline void deep_args_transcript_gammas(Transcript &T, const uint64_t *ood, uint64_t NW, size_t n_ood, std::vector<uint64_t> *gammas) {
    for (size_t i = 0; i < n_ood; i++) T.absorb_index(ood[i]);   // the payload: every value as 8 little-endian bytes
    for (size_t m = 0; m < n_ood; m++) {
        T.absorb_index(8 + 4 * NW + 4 + m);
        gammas->push_back(T.challenge());
    }
}

// Q(x) from the three opened rows at x: trow = the W trace values, crow = the 4 A coordinates of the auxiliary columns, srow =
// the 4 D segment values (canonical)
inline FqH deep_args_q_at(uint32_t p, uint32_t g, uint32_t W, uint32_t A, uint32_t D, uint32_t w_n, uint32_t x, const FqH &z, const uint64_t *ood,
                          const uint64_t *gammas, const uint64_t *trow, const uint64_t *crow, const uint64_t *srow) {
    FqH n1 = fqh(0), n2 = fqh(0);
    auto term = [&](const FqH &f, size_t i) { return fqh_mul(fqh_of(gammas + 4 * i, p), fqh_sub(f, fqh_of(ood + 4 * i, p), p), p, g); };
    for (uint32_t c = 0; c < W; c++) {
        const FqH f = fqh((uint32_t)trow[c]);
        n1 = fqh_add(n1, term(f, c), p);
        n2 = fqh_add(n2, term(f, (size_t)W + c), p);
    }
    for (uint32_t a = 0; a < A; a++) {
        const FqH f = fqh_of(crow + 4 * (size_t)a, p);
        n1 = fqh_add(n1, term(f, 2 * (size_t)W + a), p);
        n2 = fqh_add(n2, term(f, 2 * (size_t)W + A + a), p);
    }
    for (uint32_t j = 0; j < D; j++) n1 = fqh_add(n1, term(fqh_of(srow + 4 * (size_t)j, p), 2 * (size_t)W + 2 * (size_t)A + j), p);
    const FqH d1 = fqh_sub(fqh(x), z, p), d2 = fqh_sub(fqh(x), fqh_scale(z, w_n, p), p);
    return fqh_add(fqh_mul(n1, fqh_inv(d1, p, g), p, g), fqh_mul(n2, fqh_inv(d2, p, g), p, g), p);
}

// ------------------------------------------------------------------------------------------------ ... over coset leaves
// include/stark_mi.h, "Out-of-domain sampling over coset leaves": every committed group of columns -- the trace (V = W), the
// auxiliary coordinates (V = 4 A, argument lists only) and the segments (V = 4 D) -- is a tree of N / 4 coset leaves
// (smi_dev_merkle_build_cosets), FRI folds by 4, and a test opens one leaf and one path per group.  What the two variants
// share is written once over a list of groups: the section lengths, the parsing, and Q at the four points of a coset.
#define DEEP_FOLD4_NO_LAYER \
    "deep fold4: FRI has no fold at this shape (F = 0), so there is no layer-0 coset to compare the DEEP quotient with"
static const char *const DEEP_FOLD4_SENTENCES[6] = {"deep coset openings: wrong length",
                                                    "deep coset openings: malformed record",
                                                    "deep coset openings: malformed path",
                                                    "deep coset openings: authentication path does not verify",
                                                    "deep coset openings: an opened value is not canonical",
                                                    "deep coset openings: the DEEP quotient of the opened cosets is not the codeword value"};
static const char *const DEEP_ARGS_FOLD4_SENTENCES[6] = {"deep argument coset openings: wrong length",
                                                         "deep argument coset openings: malformed record",
                                                         "deep argument coset openings: malformed path",
                                                         "deep argument coset openings: authentication path does not verify",
                                                         "deep argument coset openings: an opened value is not canonical",
                                                         "deep argument coset openings: the DEEP quotient of the opened cosets is not the codeword value"};

// the groups of one proof in section order: W, 4 D (A == 0) or W, 4 A, 4 D
struct DeepGroups {
    uint32_t G, V[3];
};
inline DeepGroups deep_groups(uint32_t W, uint32_t A, uint32_t D) {
    DeepGroups gr;
    gr.G = A ? 3 : 2;
    gr.V[0] = W;
    gr.V[1] = A ? 4 * A : 4 * D;
    gr.V[2] = A ? 4 * D : 0;
    return gr;
}
// one group's section: t records of 4 V values, then t paths of log2 N - 2 digests
inline size_t deep_coset_section_len(uint32_t V, uint64_t t, uint32_t log_N) { return (size_t)(t * (9 + 32ull * V) + t * (9 + 32ull * (log_N - 2))); }
inline size_t deep_coset_sections_len(const DeepGroups &gr, uint64_t t, uint32_t log_N) {
    size_t s = 0;
    for (uint32_t k = 0; k < gr.G; k++) s += deep_coset_section_len(gr.V[k], t, log_N);
    return s;
}
// 9 + 32 (2 W + 2 A + D) + len_FRI4(N, B, t) + the sections; A == 0: the plain-AIR variant
inline size_t deep_fold4_proof_len(const smi_stark_cfg *cfg, uint32_t A, uint32_t D, uint64_t *folds, uint32_t S = 2) {
    const uint32_t W = cfg->n_cols, log_N = cfg->log_n + cfg->log_blowup;
    const FriFold4Layout lay = fri_layout_fold4(deep_fri_cfg(cfg, 1));
    if (folds) *folds = lay.F;
    return 9 + 32 * ((size_t)S * W + 2 * (size_t)A + D) + lay.proof_len + deep_coset_sections_len(deep_groups(W, A, D), cfg->num_colinearity_tests, log_N);
}

enum { DEEP_COSET_OK = 0, DEEP_COSET_LENGTH = 1, DEEP_COSET_RECORD = 2, DEEP_COSET_PATH = 3 };
// The opening sections as they stand in a proof (`len` bytes at `sec`): the exact length, then group by group the tag and
// count of every record and of every path.  -> DEEP_COSET_OK with vals[k] = the t x 4 V_k values of group k and at[k] = the
// offset of its section, or the first check that fails.
inline int deep_coset_parse(const uint8_t *sec, size_t len, const DeepGroups &gr, uint64_t t, uint32_t log_N, std::vector<uint64_t> vals[3], size_t at[3]) {
    if (len != deep_coset_sections_len(gr, t, log_N)) return DEEP_COSET_LENGTH;
    auto u64_at = [](const uint8_t *b) {
        uint64_t v = 0;
        for (int i = 7; i >= 0; i--) v = (v << 8) | b[i];
        return v;
    };
    const uint64_t depth = log_N - 2;
    size_t off = 0;
    for (uint32_t k = 0; k < gr.G; k++) {
        const size_t cnt = 4 * (size_t)gr.V[k], rec = 9 + 8 * cnt, prec = 9 + 32 * (size_t)depth;
        at[k] = off;
        vals[k].resize((size_t)t * cnt);
        for (uint64_t s = 0; s < t; s++) {
            const uint8_t *r = sec + off + s * rec;
            if (r[0] != 2 || u64_at(r + 1) != cnt) return DEEP_COSET_RECORD;
            for (size_t i = 0; i < cnt; i++) vals[k][s * cnt + i] = u64_at(r + 9 + 8 * i);
        }
        for (uint64_t s = 0; s < t; s++) {
            const uint8_t *r = sec + off + t * rec + s * prec;
            if (r[0] != 3 || u64_at(r + 1) != depth) return DEEP_COSET_PATH;
        }
        off += (size_t)t * (rec + prec);
    }
    return DEEP_COSET_OK;
}
// Q at the four points x_a iota^j of one test's coset from its opened leaves (rec[k]: the 4 V_k canonical values of group k,
// column c at point j = value 4 c + j) against the layer-0 coset record of FRI (coordinate e at point j = value 4 e + j).
// Point by point through deep_q_at / deep_args_q_at.
inline bool deep_coset_q_matches(uint32_t p, uint32_t g, uint32_t W, uint32_t A, uint32_t D, uint32_t w_n, uint32_t x_a, uint32_t iota, const FqH &z,
                                 const uint64_t *ood, const uint64_t *gammas, const uint64_t *const rec[3], const uint64_t coset[16], uint32_t S = 2) {
    const DeepGroups gr = deep_groups(W, A, D);
    std::vector<uint64_t> row[3];
    uint32_t x = x_a;
    for (uint32_t j = 0; j < 4; j++) {
        for (uint32_t k = 0; k < gr.G; k++) {
            row[k].resize(gr.V[k]);
            for (uint32_t c = 0; c < gr.V[k]; c++) row[k][c] = rec[k][4 * (size_t)c + j];
        }
        const FqH q = A ? deep_args_q_at(p, g, W, A, D, w_n, x, z, ood, gammas, row[0].data(), row[1].data(), row[2].data())
                        : deep_q_at(p, g, W, D, w_n, x, z, ood, gammas, row[0].data(), row[1].data(), S);
        for (uint32_t e = 0; e < 4; e++)
            if (q.c[e] != coset[4 * e + j]) return false;
        x = host_mulmod(x, iota, p);
    }
    return true;
}
