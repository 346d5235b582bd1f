// perm_core.h -- the permutation argument over a committed extension column (include/stark_mi.h, "Permutation argument"):
// F_q arithmetic with both factors variable, the lane bodies of the column build (perm_block_kernel) and of the two
// auxiliary quotients (air_perm_compose_kernel), and the host-side tables.  Shared by the HIP kernels (perm.hip), the
// verifier (verify.hip, host) and the CPU emulator (emu_perm.cpp), which runs the same lane batching and block split.
//
// Number forms.  Trace and extended cells are plain residues.  Inside the column build every F_q element is in Montgomery
// form coordinate by coordinate: the powers of alpha come from the host as alpha^j R^2, so that mont_mul(plain cell, .) is
// the Montgomery form of the product, and gamma as gamma R.  A product of two Montgomery elements is Montgomery; a product
// of a plain and a Montgomery element is plain (ext_mul_prepared reduces once per coordinate either way).
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/stark_mi.h"
#include "air_core.h"
#include "fri_core.h"

#define PERM_ROWS 4       // consecutive rows (column build) or points (composition) per lane: one 16-byte access per column
#define PERM_BLOCK 256    // lanes per workgroup; a workgroup covers PERM_ROWS * PERM_BLOCK rows
#define PERM_TILE (PERM_ROWS * PERM_BLOCK)

struct Fq {
    uint32_t c[4];
};

struct PermDev {   // passed to the kernels by value
    uint32_t m, g_m;                            // tuple width; g in Montgomery form
    uint32_t lcol[SMI_PERM_MAX_WIDTH], rcol[SMI_PERM_MAX_WIDTH];
    uint32_t apow_mm[SMI_PERM_MAX_WIDTH][4];    // alpha^j * R^2, coordinate by coordinate
    uint32_t gamma_m[4];                        // gamma * R
};

SMI_HD Fq fq_one(const Fp &F) { return Fq{{F.r1, 0, 0, 0}}; }
SMI_HD bool fq_is_zero(const Fq &a) { return !(a.c[0] | a.c[1] | a.c[2] | a.c[3]); }
// a * b: 20 multiplies and 8 reductions (b is prepared on the spot: its coordinates and g times them)
SMI_HD Fq fq_mul(const Fq &a, const Fq &b, uint32_t g_m, const Fp &F) {
    const ExtMul M = ext_mul_prepare(b.c, g_m, F);
    Fq o;
    ext_mul_prepared(a.c, M, F, o.c);
    return o;
}
// a^-1 for a != 0 in Montgomery form, by the tower route of ext_inv_host (fri_core.h): F_p < F_p[Y] / (Y^2 - g) < F_q with
// Y = X^2, one Fermat power in F_p.
SMI_HD Fq fq_inv(const Fq &a, uint32_t g_m, const Fp &F) {
    const uint32_t p = F.p;
    // (u + v Y)(u' + v' Y) = u u' + g v v' + (u v' + v u') Y
    const uint32_t Au = a.c[0], Av = a.c[2], Bu = a.c[1], Bv = a.c[3];
    const uint32_t A2u = fp_add(mont_mul(Au, Au, F), mont_mul(g_m, mont_mul(Av, Av, F), F), p), A2v = fp_add(mont_mul(Au, Av, F), mont_mul(Au, Av, F), p);
    const uint32_t B2u = fp_add(mont_mul(Bu, Bu, F), mont_mul(g_m, mont_mul(Bv, Bv, F), F), p), B2v = fp_add(mont_mul(Bu, Bv, F), mont_mul(Bu, Bv, F), p);
    const uint32_t Du = fp_sub(A2u, mont_mul(g_m, B2v, F), p), Dv = fp_sub(A2v, B2u, p);   // A^2 - Y B^2
    const uint32_t norm = fp_sub(mont_mul(Du, Du, F), mont_mul(g_m, mont_mul(Dv, Dv, F), F), p);
    const uint32_t ni = mont_pow(norm, p - 2, F);
    const uint32_t Iu = mont_mul(Du, ni, F), Iv = mont_mul(fp_neg(Dv, p), ni, F);           // D^-1
    Fq o;
    o.c[0] = fp_add(mont_mul(Au, Iu, F), mont_mul(g_m, mont_mul(Av, Iv, F), F), p);
    o.c[2] = fp_add(mont_mul(Au, Iv, F), mont_mul(Av, Iu, F), p);
    o.c[1] = fp_neg(fp_add(mont_mul(Bu, Iu, F), mont_mul(g_m, mont_mul(Bv, Iv, F), F), p), p);
    o.c[3] = fp_neg(fp_add(mont_mul(Bu, Iv, F), mont_mul(Bv, Iu, F), p), p);
    return o;
}

// f[q] = gamma + sum_j alpha^j * T[cols[j]][row q] for the lane's PERM_ROWS rows, Montgomery form.  load4(col, v) fetches the
// four plain cells of column col (one 16-byte access where the layout allows); the members are the outer loop, so a column is
// fetched once for the four rows and nothing is indexed by a runtime value but the kernel's own argument.  A product of an
// F_q element by a base-field cell is four multiplies.
// tuples_of takes the tables by pointer (the argument list of args_core.h keeps alpha's powers once for all its arguments).
template <class Load4>
SMI_HD void tuples_of(const uint32_t (*apow_mm)[4], const uint32_t *gamma_m, uint32_t m, const Fp &F, const uint32_t *cols, Load4 load4, Fq f[PERM_ROWS]) {
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) f[q] = Fq{{gamma_m[0], gamma_m[1], gamma_m[2], gamma_m[3]}};
    for (uint32_t j = 0; j < m; j++) {
        uint32_t v[PERM_ROWS];
        load4(cols[j], v);
        const uint32_t a0 = apow_mm[j][0], a1 = apow_mm[j][1], a2 = apow_mm[j][2], a3 = apow_mm[j][3];
#pragma unroll
        for (int q = 0; q < PERM_ROWS; q++) {
            f[q].c[0] = fp_add(f[q].c[0], mont_mul(v[q], a0, F), F.p);
            f[q].c[1] = fp_add(f[q].c[1], mont_mul(v[q], a1, F), F.p);
            f[q].c[2] = fp_add(f[q].c[2], mont_mul(v[q], a2, F), F.p);
            f[q].c[3] = fp_add(f[q].c[3], mont_mul(v[q], a3, F), F.p);
        }
    }
}
template <class Load4>
SMI_HD void perm_tuples(const PermDev &PD, const Fp &F, const uint32_t *cols, Load4 load4, Fq f[PERM_ROWS]) {
    tuples_of(PD.apow_mm, PD.gamma_m, PD.m, F, cols, load4, f);
}

// One lane of the column build: rows row0 .. row0 + PERM_ROWS - 1 (those below n; the others count as rho = 1 and load4 may
// return anything for them).  zl[q]: the product of the lane's rho before row q (zl[0] = 1), *prod the product of all of
// them, both Montgomery.  One F_q inversion serves the lane's denominators (Montgomery's trick); a zero denominator would
// spoil the whole batch, so it is replaced by one first and its row is reported: *zero_row is the smallest such row, or ~0.
// perm_lane_ratios is the part behind the tuples: num = f_L and den = f_R of the lane's rows on entry (both are overwritten).
SMI_HD void perm_lane_ratios(uint32_t g_m, const Fp &F, uint64_t row0, uint64_t n, Fq num[PERM_ROWS], Fq den[PERM_ROWS], Fq zl[PERM_ROWS], Fq *prod,
                             uint64_t *zero_row) {
    Fq pre[PERM_ROWS];
    const Fq one = fq_one(F);
    uint64_t zr = ~0ull;
#pragma unroll
    for (int q = PERM_ROWS - 1; q >= 0; q--) {
        if (row0 + q >= n) {
            num[q] = one;
            den[q] = one;
        } else if (fq_is_zero(den[q])) {
            den[q] = one;
            zr = row0 + q;
        }
    }
    pre[0] = den[0];
#pragma unroll
    for (int q = 1; q < PERM_ROWS; q++) pre[q] = fq_mul(pre[q - 1], den[q], g_m, F);
    Fq inv = fq_inv(pre[PERM_ROWS - 1], g_m, F);
#pragma unroll
    for (int q = PERM_ROWS - 1; q >= 0; q--) {
        const Fq di = q ? fq_mul(inv, pre[q - 1], g_m, F) : inv;   // 1 / den[q]
        if (q) inv = fq_mul(inv, den[q], g_m, F);
        num[q] = fq_mul(num[q], di, g_m, F);                        // rho
    }
    zl[0] = one;
#pragma unroll
    for (int q = 1; q < PERM_ROWS; q++) zl[q] = fq_mul(zl[q - 1], num[q - 1], g_m, F);
    *prod = fq_mul(zl[PERM_ROWS - 1], num[PERM_ROWS - 1], g_m, F);
    *zero_row = zr;
}
template <class Load4>
SMI_HD void perm_lane_column(const PermDev &PD, const Fp &F, uint64_t row0, uint64_t n, Load4 load4, Fq zl[PERM_ROWS], Fq *prod, uint64_t *zero_row) {
    Fq num[PERM_ROWS], den[PERM_ROWS];
    perm_tuples(PD, F, PD.lcol, load4, num);
    perm_tuples(PD, F, PD.rcol, load4, den);
    perm_lane_ratios(PD.g_m, F, row0, n, num, den, zl, prod, zero_row);
}

// One lane of the auxiliary quotients: PERM_ROWS consecutive points i0 .. i0 + PERM_ROWS - 1.
//   x0_m: x_{i0}, Montgomery; omega_m: omega_N; tau_m: the trace offset; izt_m: the B-entry table 1 / (x^n - tau^n) of the
//   AIR blob; wb / wt: the weights of the boundary and of the transition quotient, Montgomery, prepared;
//   load4(col, v): extended trace column col at the four points; zc[e][q] / zx[e][q]: coordinate e of the extended column z
//   at point q and one row further ((i + B) mod N), plain; acc[e][q]: the composition so far, updated in place.
// 1 / (x_i - tau) is batched over the lane's points in the base field: one Fermat power per lane.
template <class Load4>
SMI_HD void perm_compose_points(const PermDev &PD, const Fp &F, const ExtMul &wb, const ExtMul &wt, uint32_t tau_m, const uint32_t *izt_m, uint32_t B,
                                uint64_t i0, uint32_t x0_m, uint32_t omega_m, Load4 load4, uint32_t zc[4][PERM_ROWS],
                                uint32_t zx[4][PERM_ROWS], uint32_t acc[4][PERM_ROWS]) {
    const uint32_t p = F.p;
    uint32_t d[PERM_ROWS], pre[PERM_ROWS];
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
    Fq fl[PERM_ROWS], fr[PERM_ROWS];
    perm_tuples(PD, F, PD.lcol, load4, fl);
    perm_tuples(PD, F, PD.rcol, load4, fr);
#pragma unroll
    for (int q = PERM_ROWS - 1; q >= 0; q--) {
        const uint32_t di = q ? mont_mul(inv, pre[q - 1], F) : inv;   // 1 / (x_q - tau), Montgomery
        if (q) inv = mont_mul(inv, d[q], F);
        const ExtMul ML = ext_mul_prepare(fl[q].c, PD.g_m, F), MR = ext_mul_prepare(fr[q].c, PD.g_m, F);
        uint32_t zq[4], zn[4], a[4], b[4], tq[4], bq[4], u[4], v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) zq[e] = zc[e][q], zn[e] = zx[e][q];
        ext_mul_prepared(zn, MR, F, a);   // z(w x) f_R(x), plain
        ext_mul_prepared(zq, ML, F, b);   // z(x) f_L(x)
        const uint32_t s = izt_m[(uint32_t)((i0 + q) & (B - 1))];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            tq[e] = mont_mul(fp_sub(a[e], b[e], p), s, F);
            bq[e] = mont_mul(e ? zq[e] : fp_sub(zq[0], 1u, p), di, F);
        }
        ext_mul_prepared(bq, wb, F, u);
        ext_mul_prepared(tq, wt, F, v);
#pragma unroll
        for (int e = 0; e < 4; e++) acc[e][q] = fp_add(acc[e][q], fp_add(u[e], v[e], p), p);
    }
}

// The workgroup's scan of one F_q element per lane (Montgomery form), Hillis-Steele over two buffers of 4 x PERM_BLOCK words:
// step `off` of lane tid reads in[.][tid] and in[.][tid - off] and writes out[.][tid]; a barrier separates the steps (the
// kernels' __syncthreads, the emulator's loop over the lanes).  After the last step (off = PERM_BLOCK / 2) lane tid's
// exclusive prefix is element tid - 1 of the buffer written last (one for lane 0) and the product is element PERM_BLOCK - 1.
SMI_HD void perm_scan_step(const uint32_t (*in)[PERM_BLOCK], uint32_t (*out)[PERM_BLOCK], uint32_t tid, uint32_t off, uint32_t g_m, const Fp &F) {
    Fq x{{in[0][tid], in[1][tid], in[2][tid], in[3][tid]}};
    if (tid >= off) {
        const Fq y{{in[0][tid - off], in[1][tid - off], in[2][tid - off], in[3][tid - off]}};
        x = fq_mul(y, x, g_m, F);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) out[e][tid] = x.c[e];
}
SMI_HD Fq perm_scan_at(const uint32_t (*buf)[PERM_BLOCK], uint32_t i) { return Fq{{buf[0][i], buf[1][i], buf[2][i], buf[3][i]}}; }

// ------------------------------------------------------------------------------------------------ host side
inline int perm_validate(const smi_air_perm *perm, uint32_t n_cols, std::string *why) {
    auto fail = [&](const std::string &s) {
        if (why) *why = s;
        return SMI_ERR_BAD_ARG;
    };
    if (!perm) return fail("perm: null argument");
    if (perm->width < 1 || perm->width > SMI_PERM_MAX_WIDTH) return fail("perm: width must be in 1 .. SMI_PERM_MAX_WIDTH (" + std::to_string(SMI_PERM_MAX_WIDTH) + ")");
    if (!perm->left_col || !perm->right_col) return fail("perm: null column list");
    for (uint32_t j = 0; j < perm->width; j++) {
        if (perm->left_col[j] >= n_cols) return fail("perm: left_col must be < n_cols");
        if (perm->right_col[j] >= n_cols) return fail("perm: right_col must be < n_cols");
    }
    return SMI_OK;
}

// smi_air_plan_perm: the AIR's own plan with the two auxiliary constraints of degree 2 counted in
inline int perm_plan(uint64_t p, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_perm *perm, uint32_t *degree, uint64_t *fri_expansion,
                     std::string *why) {
    uint32_t d = 0;
    const int rc = air_validate(p, cfg, air, &d, nullptr, why);
    if (rc != SMI_OK) return rc;
    const int prc = perm_validate(perm, cfg->n_cols, why);
    if (prc != SMI_OK) return prc;
    if ((p & 3) != 1) {
        if (why) *why = "perm: p = 3 (mod 4): the quartic extension does not exist";
        return SMI_ERR_BAD_ARG;
    }
    if (d < 2) d = 2;
    const uint64_t B = 1ull << cfg->log_blowup;
    uint64_t D = 1;
    while (D < d - 1) D <<= 1;
    const uint64_t E = D > B ? 0 : B / D;
    if (E < 4) {
        if (why) *why = "perm: 2^log_blowup / D < 4";
        return SMI_ERR_EXPANSION_TOO_SMALL;
    }
    if (degree) *degree = d;
    if (fri_expansion) *fri_expansion = E;
    return SMI_OK;
}

// alpha = challenges[0..3] mod p, gamma = challenges[4..7] mod p (host, plain) and the kernels' tables
inline void perm_challenges(uint32_t p, const uint64_t ch[8], uint32_t alpha[4], uint32_t gamma[4]) {
    for (int e = 0; e < 4; e++) alpha[e] = (uint32_t)(ch[e] % p), gamma[e] = (uint32_t)(ch[4 + e] % p);
}
inline void perm_build(const Fp &F, uint32_t g, const smi_air_perm *perm, const uint64_t ch[8], PermDev *PD) {
    const uint32_t p = F.p;
    uint32_t alpha[4], gamma[4], pw[4] = {1 % p, 0, 0, 0};
    perm_challenges(p, ch, alpha, gamma);
    PD->m = perm->width;
    PD->g_m = air_to_m(g, p);
    for (uint32_t j = 0; j < SMI_PERM_MAX_WIDTH; j++) {
        PD->lcol[j] = j < perm->width ? perm->left_col[j] : 0;
        PD->rcol[j] = j < perm->width ? perm->right_col[j] : 0;
        for (int e = 0; e < 4; e++) PD->apow_mm[j][e] = air_to_m(air_to_m(pw[e], p), p);
        ext_mul_host(p, g, pw, alpha, pw);
    }
    for (int e = 0; e < 4; e++) PD->gamma_m[e] = air_to_m(gamma[e], p);
}
