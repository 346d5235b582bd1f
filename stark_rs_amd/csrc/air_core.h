// air_core.h -- the AIR composition shared by the HIP kernels (air.hip), the verifier (verify.hip, host) and the CPU
// emulator of the non-GPU tests (emu_air.cpp): validation of an smi_air, the flat tables a kernel reads, and the
// per-thread evaluator of the composition codeword
//   cw[i] = sum_c w_c * term_c(x_i) + sum_k w_{W+k} * C_k(row i, row i+B) * (x_i - tau*w^(n-1)) / (x_i^n - tau^n)
// (include/stark_mi.h, "AIR").  The reference has no counterpart (its Trace has no consumer).
//
// Transition windows (include/stark_mi.h, "AIR: transition windows").  An AIR with a window of S = 3 or 4 rows reads row
// i + s B for s < S: the tile's halo is (S - 1) B points, the operands are numbered s R + row, and the quotient's numerator
// carries the S - 1 exemption roots tau w^(n-s).  That code is the WIN = true instantiation of the templates below; WIN =
// false is the two-row code as it was, so the kernels of a two-row AIR do not change with the window's existence.
//
// Periodic columns.  Column j (period P_j) is a table of L_j = P_j * B values tbl_j[i] = pi_j(x_i), i < L_j, that is read
// modulo its length: pi_j(x_i) = tbl_j[i mod L_j], pi_j(w x_i) = tbl_j[(i + B) mod L_j] (stark_mi.h has the identity).
// The tables lie back to back in one buffer (AirDev::ptab), longest period first, so that every table starts at a
// multiple of its own length; air_periodic_plan lays them out and names the transforms that fill them.  On the trace
// itself (the checker) B = 1 and the tables are the values themselves.
//
// Number forms.  Column values are plain residues, as smi_dev_lde leaves them.  x_i, the boundary roots, the inverse
// tables and the weights are in Montgomery form (suffix _m), so mont_mul(plain, mont) stays plain.  A term's
// coefficient is stored as coeff * R^e (e = the term's total exponent): after its e products with plain operands the
// value is plain again, with no conversion per point.  The interpolants' coefficients are plain: Horner with a
// Montgomery x keeps the running value plain.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/stark_mi.h"
#include "field.h"

#define AIR_MAX_WEIGHTS (64 + SMI_AIR_MAX_CONSTRAINTS)
#define AIR_INV_BATCH 16     // values per field inversion (Montgomery's trick), held in registers
#define AIR_BLOCK 256        // threads per workgroup when the tile has at least that many points
#define AIR_LDS_BYTES 65536  // tile + halo of all columns must fit in this

struct AirDev {   // pointers into one blob of u32 (device memory for the kernels, host memory for the emulator / verifier)
    uint32_t W, K, n_bcols;
    uint32_t log_B;            // next row = index + B
    uint64_t N;
    const uint32_t *cft;       // K + 1: first term of constraint k
    const uint32_t *tcoef;     // n_terms: coeff * R^(total exponent) mod p
    const uint32_t *tff;       // n_terms + 1: first factor of term t
    const uint32_t *fac;       // n_factors: operand | exp << 16; the operands are numbered by tile row, R = W + Q rows:
                               // row (trace column c: c, periodic column j: W + j) at this row, s R + row at row + s
    const uint32_t *free_col;  // W - n_bcols: the columns without a boundary point, ascending
    const uint32_t *bcol;      // n_bcols: the columns with boundary points, ascending
    const uint32_t *bfirst;    // n_bcols + 1: first point of boundary column j
    const uint32_t *broot_m;   // tau * w^row of every boundary point, Montgomery form
    const uint32_t *bicoef;    // interpolant of boundary column j, bfirst[j+1]-bfirst[j] plain coefficients, low first
    const uint32_t *izt_m;     // B entries: 1 / (h^n * zeta^b - tau^n), Montgomery form
    const uint32_t *lane_pow_m;  // AIR_BLOCK entries: omega_N^t, Montgomery form
    uint32_t last_m;           // tau * w^(n-1), Montgomery form
    uint32_t h_m, omega_m;     // lde_offset and omega_N, Montgomery form
    uint32_t Q;                // periodic columns
    const uint32_t *plog;      // Q: log2 of the length L_j of table j
    const uint32_t *pofs;      // Q: first element of table j in ptab, a multiple of L_j
    const uint32_t *ptab;      // the tables, plain residues; not part of the blob
    uint32_t S;                // the window, 2 .. SMI_AIR_MAX_WINDOW; behind the two-row fields, whose offsets stay
    uint32_t lastx_m[2];       // tau * w^(n-2), tau * w^(n-3), Montgomery form: the further exemption roots of S = 3, 4
};

// periodic column j at the point with index i, s rows further, from memory: table j read at i + s B modulo its length
SMI_HD uint32_t air_periodic_operand(const AirDev &A, uint32_t j, uint32_t s, uint64_t i) {
    const uint64_t at = i + ((uint64_t)s << A.log_B);
    return A.ptab[A.pofs[j] + (uint32_t)(at & ((1ull << A.plog[j]) - 1))];
}
// operand `var` of a point without a tile: cur(c) / nxt(c) the trace column c at this row / the next, i the point's index
template <class Cur, class Nxt>
SMI_HD uint32_t air_mem_operand(const AirDev &A, uint32_t var, uint64_t i, Cur cur, Nxt nxt) {
    const uint32_t R = A.W + A.Q;
    const bool next = var >= R;
    const uint32_t c = next ? var - R : var;
    if (c >= A.W) return air_periodic_operand(A, c - A.W, next ? 1u : 0u, i);
    return next ? nxt(c) : cur(c);
}
// the shift s < S <= 4 of operand `var` = s R + row: three compares of wave-uniform values, no division
SMI_HD uint32_t air_var_shift(uint32_t var, uint32_t R) { return (uint32_t)(var >= R) + (uint32_t)(var >= 2 * R) + (uint32_t)(var >= 3 * R); }
// air_mem_operand under a window: at(c, s) the trace column c at row + s
template <class At>
SMI_HD uint32_t air_mem_operand_win(const AirDev &A, uint32_t var, uint64_t i, At at) {
    const uint32_t R = A.W + A.Q, s = air_var_shift(var, R), c = var - s * R;
    if (c >= A.W) return air_periodic_operand(A, c - A.W, s, i);
    return at(c, s);
}
// (x - last) and, WIN, the further exemption roots: the numerator of 1 / Z_T
template <bool WIN>
SMI_HD uint32_t air_exempt(const AirDev &A, const Fp &F, uint32_t x_m) {
    uint32_t e = fp_sub(x_m, A.last_m, F.p);
    if (WIN)
        for (uint32_t s = 2; s < A.S; s++) e = mont_mul(e, fp_sub(x_m, A.lastx_m[s - 2], F.p), F);
    return e;
}

// ------------------------------------------------------------------------------------------------ evaluator
// C_k at one point; fetch(var) returns the plain operand of AirDev::fac's numbering
template <class Fetch>
SMI_HD uint32_t air_constraint(const AirDev &A, const Fp &F, uint32_t k, Fetch fetch) {
    uint32_t ck = 0;
    for (uint32_t t = A.cft[k]; t < A.cft[k + 1]; t++) {
        uint32_t m = A.tcoef[t];
        for (uint32_t f = A.tff[t]; f < A.tff[t + 1]; f++) {
            const uint32_t fe = A.fac[f], v = fetch(fe & 0xffffu);
            for (uint32_t e = fe >> 16; e; e--) m = mont_mul(m, v, F);
        }
        ck = fp_add(ck, m, F.p);
    }
    return ck;
}

// P points of one thread.  x_m[q]: the point, Montgomery form; ib[q] = (index of point q) mod B; w_m: the W + K weights
// reduced mod p, Montgomery form; fetch(q, var) the operands of point q.  One field inversion per AIR_INV_BATCH
// boundary quotients: the P points of up to AIR_INV_BATCH / P boundary columns share it.
template <int P, bool WIN = false, class Fetch>
SMI_HD void air_compose_points(const AirDev &A, const Fp &F, const uint32_t *w_m, const uint32_t *x_m, const uint32_t *ib, Fetch fetch,
                               uint32_t *out) {
    uint32_t acc[P];
    for (int q = 0; q < P; q++) acc[q] = 0;
    // columns without a boundary point: the plain weighted sum of smi_dev_combine_columns
    const uint32_t n_free = A.W - A.n_bcols;
    for (uint32_t j = 0; j < n_free; j++) {
        const uint32_t c = A.free_col[j], w = w_m[c];
        for (int q = 0; q < P; q++) acc[q] = fp_add(acc[q], mont_mul(fetch(q, c), w, F), F.p);
    }
    // boundary quotients (f_c - I_c) / Z_c
    constexpr int G = AIR_INV_BATCH / P;   // columns per inversion
    for (uint32_t j0 = 0; j0 < A.n_bcols; j0 += G) {   // table entries outside, the P points inside, as below
        uint32_t z[AIR_INV_BATCH], pre[AIR_INV_BATCH];
        for (int g = 0; g < G; g++) {
            for (int q = 0; q < P; q++) z[g * P + q] = F.r1;
            if (j0 + g < A.n_bcols)
                for (uint32_t b = A.bfirst[j0 + g]; b < A.bfirst[j0 + g + 1]; b++) {
                    const uint32_t r = A.broot_m[b];
                    for (int q = 0; q < P; q++) z[g * P + q] = mont_mul(z[g * P + q], fp_sub(x_m[q], r, F.p), F);
                }
        }
        pre[0] = z[0];
        for (int i = 1; i < AIR_INV_BATCH; i++) pre[i] = mont_mul(pre[i - 1], z[i], F);
        uint32_t inv = mont_pow(pre[AIR_INV_BATCH - 1], F.p - 2, F);   // never 0: the coset does not meet the trace domain
        for (int g = G - 1; g >= 0; g--) {
            uint32_t zi[P];   // 1 / z[g * P + q]
            for (int q = P - 1; q >= 0; q--) {
                const int i = g * P + q;
                zi[q] = i ? mont_mul(inv, pre[i - 1], F) : inv;
                inv = mont_mul(inv, z[i], F);
            }
            if (j0 + g >= A.n_bcols) continue;
            const uint32_t c = A.bcol[j0 + g], b0 = A.bfirst[j0 + g], b1 = A.bfirst[j0 + g + 1], wc = w_m[c];
            uint32_t ix[P];   // I_c(x), Horner from the top coefficient
            for (int q = 0; q < P; q++) ix[q] = 0;
            for (uint32_t b = b1; b > b0; b--) {
                const uint32_t coef = A.bicoef[b - 1];
                for (int q = 0; q < P; q++) ix[q] = fp_add(mont_mul(ix[q], x_m[q], F), coef, F.p);
            }
            for (int q = 0; q < P; q++) {
                const uint32_t u = mont_mul(wc, zi[q], F);   // weight / Z, Montgomery form
                acc[q] = fp_add(acc[q], mont_mul(fp_sub(fetch(q, c), ix[q], F.p), u, F), F.p);
            }
        }
    }
    // transition quotients: (sum_k w_k C_k) * (x - last) / (x^n - tau^n) (WIN: the S - 1 exemption roots, air_exempt).
    // Terms outside, the P points inside: a table entry is fetched once for the P points, and their P product chains are
    // independent
    if (A.K) {
        uint32_t s[P];
        for (int q = 0; q < P; q++) s[q] = 0;
        for (uint32_t k = 0; k < A.K; k++) {
            uint32_t ck[P];
            for (int q = 0; q < P; q++) ck[q] = 0;
            for (uint32_t t = A.cft[k]; t < A.cft[k + 1]; t++) {
                uint32_t m[P];
                const uint32_t coef = A.tcoef[t];
                for (int q = 0; q < P; q++) m[q] = coef;
                for (uint32_t f = A.tff[t]; f < A.tff[t + 1]; f++) {
                    const uint32_t fe = A.fac[f], var = fe & 0xffffu;
                    uint32_t v[P];
                    for (int q = 0; q < P; q++) v[q] = fetch(q, var);
                    for (uint32_t e = fe >> 16; e; e--)
                        for (int q = 0; q < P; q++) m[q] = mont_mul(m[q], v[q], F);
                }
                for (int q = 0; q < P; q++) ck[q] = fp_add(ck[q], m[q], F.p);
            }
            const uint32_t wk = w_m[A.W + k];
            for (int q = 0; q < P; q++) s[q] = fp_add(s[q], mont_mul(ck[q], wk, F), F.p);
        }
        for (int q = 0; q < P; q++) {
            const uint32_t zt = mont_mul(air_exempt<WIN>(A, F, x_m[q]), A.izt_m[ib[q]], F);
            acc[q] = fp_add(acc[q], mont_mul(s[q], zt, F), F.p);
        }
    }
    for (int q = 0; q < P; q++) out[q] = acc[q];
}

// The same P points under weights from the quartic extension (stark_mi.h, "AIR with extension weights"): weight j has
// four coordinates, w_m[e * AIR_MAX_WEIGHTS + j] the e-th (reduced, Montgomery form), and out[e * P + q] is coordinate e of
// point q.  The quotients do not depend on the weights: every term_c and every C_k is evaluated once per point -- the
// Horner chains, the batched inversion, the table walk are the ones above -- and enters four accumulators, so coordinate
// e is exactly what air_compose_points returns for the weight vector (w_{.,e}).
template <int P, bool WIN = false, class Fetch>
SMI_HD void air_compose_points_ext(const AirDev &A, const Fp &F, const uint32_t *w_m, const uint32_t *x_m, const uint32_t *ib, Fetch fetch,
                                   uint32_t *out) {
    uint32_t acc[4][P];
    for (int e = 0; e < 4; e++)
        for (int q = 0; q < P; q++) acc[e][q] = 0;
    const uint32_t n_free = A.W - A.n_bcols;
    for (uint32_t j = 0; j < n_free; j++) {
        const uint32_t c = A.free_col[j];
        uint32_t v[P];
        for (int q = 0; q < P; q++) v[q] = fetch(q, c);
        for (int e = 0; e < 4; e++) {
            const uint32_t w = w_m[e * AIR_MAX_WEIGHTS + c];
            for (int q = 0; q < P; q++) acc[e][q] = fp_add(acc[e][q], mont_mul(v[q], w, F), F.p);
        }
    }
    constexpr int G = AIR_INV_BATCH / P;   // columns per inversion
    for (uint32_t j0 = 0; j0 < A.n_bcols; j0 += G) {
        uint32_t z[AIR_INV_BATCH], pre[AIR_INV_BATCH];
        for (int g = 0; g < G; g++) {
            for (int q = 0; q < P; q++) z[g * P + q] = F.r1;
            if (j0 + g < A.n_bcols)
                for (uint32_t b = A.bfirst[j0 + g]; b < A.bfirst[j0 + g + 1]; b++) {
                    const uint32_t r = A.broot_m[b];
                    for (int q = 0; q < P; q++) z[g * P + q] = mont_mul(z[g * P + q], fp_sub(x_m[q], r, F.p), F);
                }
        }
        pre[0] = z[0];
        for (int i = 1; i < AIR_INV_BATCH; i++) pre[i] = mont_mul(pre[i - 1], z[i], F);
        uint32_t inv = mont_pow(pre[AIR_INV_BATCH - 1], F.p - 2, F);   // never 0: the coset does not meet the trace domain
        for (int g = G - 1; g >= 0; g--) {
            uint32_t zi[P];   // 1 / z[g * P + q]
            for (int q = P - 1; q >= 0; q--) {
                const int i = g * P + q;
                zi[q] = i ? mont_mul(inv, pre[i - 1], F) : inv;
                inv = mont_mul(inv, z[i], F);
            }
            if (j0 + g >= A.n_bcols) continue;
            const uint32_t c = A.bcol[j0 + g], b0 = A.bfirst[j0 + g], b1 = A.bfirst[j0 + g + 1];
            uint32_t ix[P];   // I_c(x), Horner from the top coefficient
            for (int q = 0; q < P; q++) ix[q] = 0;
            for (uint32_t b = b1; b > b0; b--) {
                const uint32_t coef = A.bicoef[b - 1];
                for (int q = 0; q < P; q++) ix[q] = fp_add(mont_mul(ix[q], x_m[q], F), coef, F.p);
            }
            uint32_t bq[P];   // the boundary quotient (f_c - I_c) / Z_c, plain
            for (int q = 0; q < P; q++) bq[q] = mont_mul(fp_sub(fetch(q, c), ix[q], F.p), zi[q], F);
            for (int e = 0; e < 4; e++) {
                const uint32_t w = w_m[e * AIR_MAX_WEIGHTS + c];
                for (int q = 0; q < P; q++) acc[e][q] = fp_add(acc[e][q], mont_mul(bq[q], w, F), F.p);
            }
        }
    }
    if (A.K) {
        uint32_t zt[P];   // (x - last) / (x^n - tau^n), Montgomery form
        for (int q = 0; q < P; q++) zt[q] = mont_mul(air_exempt<WIN>(A, F, x_m[q]), A.izt_m[ib[q]], F);
        for (uint32_t k = 0; k < A.K; k++) {
            uint32_t ck[P];
            for (int q = 0; q < P; q++) ck[q] = 0;
            for (uint32_t t = A.cft[k]; t < A.cft[k + 1]; t++) {
                uint32_t m[P];
                const uint32_t coef = A.tcoef[t];
                for (int q = 0; q < P; q++) m[q] = coef;
                for (uint32_t f = A.tff[t]; f < A.tff[t + 1]; f++) {
                    const uint32_t fe = A.fac[f], var = fe & 0xffffu;
                    uint32_t v[P];
                    for (int q = 0; q < P; q++) v[q] = fetch(q, var);
                    for (uint32_t e = fe >> 16; e; e--)
                        for (int q = 0; q < P; q++) m[q] = mont_mul(m[q], v[q], F);
                }
                for (int q = 0; q < P; q++) ck[q] = fp_add(ck[q], m[q], F.p);
            }
            for (int q = 0; q < P; q++) ck[q] = mont_mul(ck[q], zt[q], F);   // tq_k, plain
            for (int e = 0; e < 4; e++) {
                const uint32_t wk = w_m[e * AIR_MAX_WEIGHTS + A.W + k];
                for (int q = 0; q < P; q++) acc[e][q] = fp_add(acc[e][q], mont_mul(ck[q], wk, F), F.p);
            }
        }
    }
    for (int e = 0; e < 4; e++)
        for (int q = 0; q < P; q++) out[e * P + q] = acc[e][q];
}

// The tile of T points a workgroup stages per column: T points and a halo of (S - 1) B (B for two rows), wrapping at N.
// Tile element e of column c sits at tile[c * (T + halo) + e] and comes from column index (base + e) mod N.  Periodic
// column j is tile row W + j, staged the same way from table index (base + e) mod L_j: air_tile is asked for W + Q rows.
struct AirTile {
    uint32_t T, threads, P;   // points per tile, threads per workgroup, points per thread (T = threads * P)
};
// W: tile rows; weight_vecs: 4 for the ext kernel; window: the AIR's S
inline AirTile air_tile(uint32_t W, uint64_t B, uint64_t N, uint32_t weight_vecs = 1, uint32_t window = 2) {
    AirTile t{0, 0, 0};
    const uint64_t halo = (uint64_t)(window - 1) * B;
    for (uint32_t T = 1024; T >= 64; T >>= 1) {
        if (T > N || (uint64_t)W * (T + halo) * 4 + (uint64_t)weight_vecs * AIR_MAX_WEIGHTS * 4 > AIR_LDS_BYTES) continue;
        t.T = T;
        t.threads = T >= AIR_BLOCK ? AIR_BLOCK : T;
        t.P = T / t.threads;
        return t;
    }
    return t;   // T == 0: no tile fits (many columns at a large blowup, or N < 64): operands come straight from memory
}

// ------------------------------------------------------------------------------------------------ host side
inline uint32_t air_inv(uint32_t a, uint32_t p) { return host_powmod(a, p - 2, p); }
inline uint32_t air_to_m(uint32_t a, uint32_t p) { return (uint32_t)(((uint64_t)a << 32) % p); }

// Everything smi_air_plan promises.  *why names the limit that was broken.
// tables_only: the AIR's own tables against n_cols and log_n (smi_dev_air_check: no extension, no offsets).
// any_expansion: E < 4 is not refused (out-of-domain sampling runs FRI at the blowup: deep_core.h deep_plan has its own bounds).
// max_window: the widest transition window the caller takes.  The plan, the composition, the checker and the plain DEEP
// provers and verifiers pass SMI_AIR_MAX_WINDOW; everybody else keeps 2 and so refuses a wider AIR here, before any work.
inline uint32_t air_window(const smi_air *air) { return air->window ? air->window : 2u; }
// D: the smallest power of two >= max(1, d - 1), doubled while D n <= d (n - 1) + (S - 1) - n, the quotient's degree bound.
// It doubles (once) for (d, S) in {(2, 3), (2, 4), (3, 4)} alone, and never for S = 2.
inline uint64_t air_segments(uint64_t d, uint32_t S, uint64_t n) {
    uint64_t D = 1;
    while (D < d - 1 && D < (1ull << 32)) D <<= 1;
    while (D * n + n <= d * (n - 1) + (S - 1) && D < (1ull << 32)) D <<= 1;
    return D;
}
inline int air_validate(uint64_t p64, const smi_stark_cfg *cfg, const smi_air *air, uint32_t *degree, uint64_t *fri_expansion,
                        std::string *why, bool tables_only = false, bool any_expansion = false, uint32_t max_window = 2) {
    auto fail = [&](int code, const std::string &s) {
        if (why) *why = s;
        return code;
    };
    if (!cfg || !air) return fail(SMI_ERR_BAD_ARG, "air: null argument");
    if (p64 < 3 || p64 >= (1ull << 30) || !(p64 & 1)) return fail(SMI_ERR_UNSUPPORTED_PRIME, "air: modulus must be an odd prime < 2^30");
    const uint32_t p = (uint32_t)p64, W = cfg->n_cols;
    if (!W || W > 64) return fail(SMI_ERR_BAD_ARG, "air: 1..64 columns");
    if (cfg->log_n < 1 || cfg->log_n > 27) return fail(SMI_ERR_BAD_ARG, "air: log_n must be in 1 .. 27");
    if (!tables_only && (cfg->log_n + cfg->log_blowup > 27 || ((p64 - 1) >> (cfg->log_n + cfg->log_blowup)) << (cfg->log_n + cfg->log_blowup) != p64 - 1))
        return fail(p == 998244353u ? SMI_ERR_ROOT_TOO_LARGE : SMI_ERR_UNSUPPORTED_PRIME, "air: LDE domain too large for this modulus");
    if (air->n_constraints > SMI_AIR_MAX_CONSTRAINTS)
        return fail(SMI_ERR_BAD_ARG, "air: more than SMI_AIR_MAX_CONSTRAINTS (" + std::to_string(SMI_AIR_MAX_CONSTRAINTS) + ") constraints");
    if (air->n_terms > SMI_AIR_MAX_TERMS) return fail(SMI_ERR_BAD_ARG, "air: more than SMI_AIR_MAX_TERMS (" + std::to_string(SMI_AIR_MAX_TERMS) + ") terms");
    if (air->n_boundary > (uint64_t)SMI_AIR_MAX_BOUNDARY_PER_COL * W)
        return fail(SMI_ERR_BAD_ARG, "air: more than SMI_AIR_MAX_BOUNDARY_PER_COL (" + std::to_string(SMI_AIR_MAX_BOUNDARY_PER_COL) + ") boundary points per column");
    if ((uint64_t)air->n_factors > (uint64_t)SMI_AIR_MAX_TERM_FACTORS * air->n_terms)
        return fail(SMI_ERR_BAD_ARG, "air: more than SMI_AIR_MAX_TERM_FACTORS (" + std::to_string(SMI_AIR_MAX_TERM_FACTORS) + ") factors in a term");
    if (air->n_periodic > SMI_AIR_MAX_PERIODIC)
        return fail(SMI_ERR_BAD_ARG, "air: more than SMI_AIR_MAX_PERIODIC (" + std::to_string(SMI_AIR_MAX_PERIODIC) + ") periodic columns");
    const uint32_t K = air->n_constraints, nt = air->n_terms, nf = air->n_factors, nb = air->n_boundary, Q = air->n_periodic;
    if (air->window == 1 || air->window > SMI_AIR_MAX_WINDOW)
        return fail(SMI_ERR_BAD_ARG, "air: window must be 0 or 2 (two rows) or 3 .. SMI_AIR_MAX_WINDOW (" + std::to_string(SMI_AIR_MAX_WINDOW) + ")");
    const uint32_t S = air_window(air);
    if (S > max_window)
        return fail(SMI_ERR_BAD_ARG, "air: a transition window of " + std::to_string(S) +
                                         " rows is taken by smi_air_plan, the composition, the checker and the plain DEEP provers and verifiers only");
    if (S > 2 && (1ull << cfg->log_n) < S) return fail(SMI_ERR_BAD_ARG, "air: window " + std::to_string(S) + " needs a trace of at least as many rows");
    if ((!air->constraint_first_term) || (!air->term_first_factor) || (nt && !air->term_coeff) || (nf && (!air->factor_var || !air->factor_exp)) ||
        (nb && (!air->boundary_col || !air->boundary_row || !air->boundary_value)) || (Q && (!air->periodic_log_period || !air->periodic_value)))
        return fail(SMI_ERR_BAD_ARG, "air: null table");
    for (uint64_t j = 0, at = 0; j < Q; j++) {
        if (air->periodic_log_period[j] > cfg->log_n) return fail(SMI_ERR_BAD_ARG, "air: periodic_log_period must be <= log_n (a period divides the trace length)");
        for (uint64_t i = 0, P = 1ull << air->periodic_log_period[j]; i < P; i++)
            if (air->periodic_value[at + i] >= p) return fail(SMI_ERR_NON_CANONICAL, "air: periodic value >= p");
        at += 1ull << air->periodic_log_period[j];
    }
    if (air->constraint_first_term[0] != 0 || air->constraint_first_term[K] != nt) return fail(SMI_ERR_BAD_ARG, "air: constraint_first_term must run from 0 to n_terms");
    for (uint32_t k = 0; k < K; k++)
        if (air->constraint_first_term[k] > air->constraint_first_term[k + 1]) return fail(SMI_ERR_BAD_ARG, "air: constraint_first_term must ascend");
    if (air->term_first_factor[0] != 0 || air->term_first_factor[nt] != nf) return fail(SMI_ERR_BAD_ARG, "air: term_first_factor must run from 0 to n_factors");
    uint64_t d = 1;
    for (uint32_t t = 0; t < nt; t++) {
        const uint32_t f0 = air->term_first_factor[t], f1 = air->term_first_factor[t + 1];
        if (f0 > f1 || f1 > nf) return fail(SMI_ERR_BAD_ARG, "air: term_first_factor must ascend");
        if (f1 - f0 > SMI_AIR_MAX_TERM_FACTORS)
            return fail(SMI_ERR_BAD_ARG, "air: more than SMI_AIR_MAX_TERM_FACTORS (" + std::to_string(SMI_AIR_MAX_TERM_FACTORS) + ") factors in a term");
        if (air->term_coeff[t] >= p) return fail(SMI_ERR_NON_CANONICAL, "air: term coefficient >= p");
        uint64_t deg = 0;
        for (uint32_t f = f0; f < f1; f++) {
            if (air->factor_var[f] >= S * (W + Q))   // two rows: the sentence they always had
                return fail(SMI_ERR_BAD_ARG, S == 2 ? "air: factor_var must be < 2 * n_cols + 2 * n_periodic (row shifts 0 and 1 only)"
                                                    : "air: factor_var must be < window * (n_cols + n_periodic) (row shifts 0 .. window - 1)");
            if (air->factor_exp[f] < 1 || air->factor_exp[f] > SMI_AIR_MAX_EXP)
                return fail(SMI_ERR_BAD_ARG, "air: factor_exp must be in 1 .. SMI_AIR_MAX_EXP (" + std::to_string(SMI_AIR_MAX_EXP) + ")");
            deg += air->factor_exp[f];
        }
        if (deg > d) d = deg;
    }
    const uint64_t n = 1ull << cfg->log_n;
    std::vector<uint32_t> per_col(W, 0);
    for (uint32_t j = 0; j < nb; j++) {
        if (air->boundary_col[j] >= W) return fail(SMI_ERR_BAD_ARG, "air: boundary_col must be < n_cols");
        if (air->boundary_row[j] >= n) return fail(SMI_ERR_BAD_ARG, "air: boundary_row must be < n");
        if (air->boundary_value[j] >= p) return fail(SMI_ERR_NON_CANONICAL, "air: boundary value >= p");
        if (++per_col[air->boundary_col[j]] > SMI_AIR_MAX_BOUNDARY_PER_COL)
            return fail(SMI_ERR_BAD_ARG, "air: more than SMI_AIR_MAX_BOUNDARY_PER_COL (" + std::to_string(SMI_AIR_MAX_BOUNDARY_PER_COL) + ") boundary points per column");
        for (uint32_t i = 0; i < j; i++)
            if (air->boundary_col[i] == air->boundary_col[j] && air->boundary_row[i] == air->boundary_row[j])
                return fail(SMI_ERR_BAD_ARG, "air: a (column, row) boundary point is given twice");
    }
    if (degree) *degree = (uint32_t)d;
    if (tables_only) return SMI_OK;
    const uint64_t B = 1ull << cfg->log_blowup;
    const uint64_t D = air_segments(d, S, 1ull << cfg->log_n);   // d >= 1
    const uint64_t E = D > B ? 0 : B / D;
    if (E < 4 && !any_expansion) return fail(SMI_ERR_EXPANSION_TOO_SMALL, "air: 2^log_blowup / D < 4: the quotients of a degree-" + std::to_string(d) + " constraint do not fit under the FRI degree bound");
    const uint64_t tau = cfg->trace_offset, h = cfg->lde_offset;
    if (!tau || tau >= p || !h || h >= p) return fail(SMI_ERR_BAD_ARG, "air: offsets must be in 1 .. p-1");
    const uint64_t N = n * B;
    if (host_powmod((uint32_t)h, N, p) == 1)
        return fail(SMI_ERR_BAD_ARG, "air: lde_offset^N == 1: the evaluation coset meets the trace domain and a zerofier vanishes on it");
    if (host_powmod(host_mulmod((uint32_t)h, air_inv((uint32_t)tau, p), p), N, p) == 1)
        return fail(SMI_ERR_BAD_ARG, "air: (lde_offset / trace_offset)^N == 1: the evaluation coset meets the trace domain");
    if (degree) *degree = (uint32_t)d;
    if (fri_expansion) *fri_expansion = E;
    return SMI_OK;
}

// The tables of a validated AIR as one blob of u32.  omega_N: the primitive N-th root the LDE uses.
// The periodic tables of one AIR: the columns grouped by period, longest first (a group is one batched extension of
// `count` columns from 2^log_period values to 2^log_len), the values in that order as u32, and every column's place.
struct AirPeriodGroup {
    uint32_t log_period, log_len, count;
    size_t in_off, out_off;   // first value / first table element of the group
    uint32_t lde_offset;      // (h / tau)^(n / P): the coset the group's extension evaluates on
};
struct AirPeriodic {
    std::vector<AirPeriodGroup> groups;
    std::vector<uint32_t> vals;             // the values, grouped; the tables themselves when log_B = 0 (the checker)
    std::vector<uint32_t> log_len, ofs;     // per column j as the AIR numbers them
    size_t table_words = 0;
};
// tables_only: no extension (B = 1, the offsets unused)
inline void air_periodic_plan(uint32_t p, const smi_stark_cfg *cfg, const smi_air *air, bool tables_only, AirPeriodic *out) {
    const uint32_t Q = air->n_periodic, lb = tables_only ? 0 : cfg->log_blowup;
    out->groups.clear();
    out->vals.clear();
    out->log_len.assign(Q, 0);
    out->ofs.assign(Q, 0);
    out->table_words = 0;
    if (!Q) return;
    std::vector<size_t> first(Q);
    size_t at = 0;
    for (uint32_t j = 0; j < Q; j++) first[j] = at, at += (size_t)1 << air->periodic_log_period[j];
    out->vals.reserve(at);
    const uint32_t ratio = tables_only ? 1 : host_mulmod((uint32_t)cfg->lde_offset, host_powmod((uint32_t)cfg->trace_offset, p - 2, p), p);
    for (int l = (int)cfg->log_n; l >= 0; l--) {
        AirPeriodGroup g{(uint32_t)l, (uint32_t)l + lb, 0, out->vals.size(), out->table_words, 0};
        for (uint32_t j = 0; j < Q; j++) {
            if (air->periodic_log_period[j] != (uint32_t)l) continue;
            out->log_len[j] = g.log_len;
            out->ofs[j] = (uint32_t)(g.out_off + ((size_t)g.count << g.log_len));
            for (size_t i = 0; i < (size_t)1 << l; i++) out->vals.push_back((uint32_t)air->periodic_value[first[j] + i]);
            g.count++;
        }
        if (!g.count) continue;
        g.lde_offset = host_powmod(ratio, 1ull << (cfg->log_n - l), p);
        out->table_words += (size_t)g.count << g.log_len;
        out->groups.push_back(g);
    }
}

struct AirHost {
    std::vector<uint32_t> blob;
    size_t off[13];
    AirDev dev;   // pointers unset until air_bind; ptab is the caller's to set
    AirPeriodic per;
};
inline void air_bind(AirHost &H, const uint32_t *base) {
    const uint32_t **slot[13] = {&H.dev.cft,    &H.dev.tcoef,   &H.dev.tff,    &H.dev.fac,   &H.dev.free_col,   &H.dev.bcol, &H.dev.bfirst,
                                 &H.dev.broot_m, &H.dev.bicoef, &H.dev.izt_m,  &H.dev.lane_pow_m, &H.dev.plog, &H.dev.pofs};
    for (int i = 0; i < 13; i++) *slot[i] = base + H.off[i];
}
// tables_only: the constraint tables alone (smi_dev_air_check); every other pointer then names the blob's end.
inline void air_build(const Fp &F, uint32_t omega_N, const smi_stark_cfg *cfg, const smi_air *air, AirHost *H, bool tables_only = false) {
    const uint32_t p = F.p, W = cfg->n_cols, K = air->n_constraints, nt = air->n_terms, nf = air->n_factors;
    const uint64_t n = 1ull << cfg->log_n, B = 1ull << cfg->log_blowup, N = n * B;
    const uint32_t tau = (uint32_t)cfg->trace_offset, h = (uint32_t)cfg->lde_offset;
    const uint32_t w = host_powmod(omega_N, B, p);   // omega_n
    std::vector<uint32_t> &b = H->blob;
    b.clear();
    auto mark = [&](int i) { H->off[i] = b.size(); };
    auto periodic = [&]() {   // sections 11 and 12
        air_periodic_plan(p, cfg, air, tables_only, &H->per);
        mark(11);
        for (uint32_t v : H->per.log_len) b.push_back(v);
        mark(12);
        for (uint32_t v : H->per.ofs) b.push_back(v);
        H->dev.Q = air->n_periodic;
        H->dev.ptab = nullptr;
    };
    mark(0);
    for (uint32_t k = 0; k <= K; k++) b.push_back(air->constraint_first_term[k]);
    mark(1);
    for (uint32_t t = 0; t < nt; t++) {
        uint64_t e = 0;
        for (uint32_t f = air->term_first_factor[t]; f < air->term_first_factor[t + 1]; f++) e += air->factor_exp[f];
        b.push_back(host_mulmod((uint32_t)air->term_coeff[t], host_powmod(F.r1, e, p), p));
    }
    mark(2);
    for (uint32_t t = 0; t <= nt; t++) b.push_back(air->term_first_factor[t]);
    mark(3);
    const uint32_t S = air_window(air);
    // smi_air's variables s W + c, S W + s Q + j to tile rows s R + c, s R + W + j; with Q = 0 the two numberings are one
    for (uint32_t f = 0; f < nf; f++) {
        const uint32_t Q = air->n_periodic, v = air->factor_var[f], R = W + Q;
        const uint32_t row = v < S * W ? (v / W) * R + v % W : ((v - S * W) / Q) * R + W + (v - S * W) % Q;   // < S (W + Q) <= 320
        b.push_back(row | (air->factor_exp[f] << 16));   // exponent <= SMI_AIR_MAX_EXP < 2^16
    }
    if (tables_only) {
        for (int i = 4; i < 11; i++) mark(i);
        H->dev.W = W;
        H->dev.K = K;
        H->dev.n_bcols = 0;
        H->dev.log_B = 0;
        H->dev.N = n;
        H->dev.last_m = H->dev.h_m = H->dev.omega_m = 0;
        H->dev.S = S;
        H->dev.lastx_m[0] = H->dev.lastx_m[1] = 0;
        periodic();
        b.push_back(0);
        air_bind(*H, b.data());
        return;
    }
    std::vector<std::vector<uint32_t>> pts(W);   // boundary point indices per column, in the order given
    for (uint32_t j = 0; j < air->n_boundary; j++) pts[air->boundary_col[j]].push_back(j);
    mark(4);
    for (uint32_t c = 0; c < W; c++)
        if (pts[c].empty()) b.push_back(c);
    mark(5);
    uint32_t nbc = 0;
    for (uint32_t c = 0; c < W; c++)
        if (!pts[c].empty()) b.push_back(c), nbc++;
    mark(6);
    uint32_t run = 0;
    b.push_back(0);
    for (uint32_t c = 0; c < W; c++)
        if (!pts[c].empty()) b.push_back(run += (uint32_t)pts[c].size());
    mark(7);
    for (uint32_t c = 0; c < W; c++)
        for (uint32_t j : pts[c]) b.push_back(air_to_m(host_mulmod(tau, host_powmod(w, air->boundary_row[j], p), p), p));
    mark(8);
    for (uint32_t c = 0; c < W; c++) {   // Lagrange: I(x) = sum_j v_j * prod_{i != j} (x - r_i) / (r_j - r_i)
        const size_t m = pts[c].size();
        if (!m) continue;
        std::vector<uint32_t> r(m), I(m, 0);
        for (size_t j = 0; j < m; j++) r[j] = host_mulmod(tau, host_powmod(w, air->boundary_row[pts[c][j]], p), p);
        for (size_t j = 0; j < m; j++) {
            std::vector<uint32_t> num(1, 1);
            uint32_t den = 1;
            for (size_t i = 0; i < m; i++) {
                if (i == j) continue;
                num.push_back(0);
                for (size_t k = num.size() - 1; k > 0; k--) num[k] = fp_sub(num[k - 1], host_mulmod(num[k], r[i], p), p);
                num[0] = fp_neg(host_mulmod(num[0], r[i], p), p);
                den = host_mulmod(den, fp_sub(r[j], r[i], p), p);
            }
            const uint32_t s = host_mulmod((uint32_t)air->boundary_value[pts[c][j]], air_inv(den, p), p);
            for (size_t k = 0; k < num.size(); k++) I[k] = fp_add(I[k], host_mulmod(num[k], s, p), p);
        }
        for (size_t k = 0; k < m; k++) b.push_back(I[k]);
    }
    mark(9);
    const uint32_t hn = host_powmod(h, n, p), taun = host_powmod(tau, n, p), zeta = host_powmod(omega_N, n, p);
    uint32_t zb = hn;
    for (uint64_t i = 0; i < B; i++) {
        b.push_back(air_to_m(air_inv(fp_sub(zb, taun, p), p), p));
        zb = host_mulmod(zb, zeta, p);
    }
    mark(10);
    uint32_t lp = 1;
    for (uint32_t t = 0; t < AIR_BLOCK; t++) {
        b.push_back(air_to_m(lp, p));
        lp = host_mulmod(lp, omega_N, p);
    }
    periodic();
    while (b.size() & 3) b.push_back(0);
    AirDev &d = H->dev;
    d.W = W;
    d.K = K;
    d.n_bcols = nbc;
    d.log_B = cfg->log_blowup;
    d.N = N;
    d.last_m = air_to_m(host_mulmod(tau, host_powmod(w, n - 1, p), p), p);
    d.S = S;
    for (uint32_t s = 2; s < 4; s++) d.lastx_m[s - 2] = s < S ? air_to_m(host_mulmod(tau, host_powmod(w, n - s, p), p), p) : 0;
    d.h_m = air_to_m(h, p);
    d.omega_m = air_to_m(omega_N, p);
    air_bind(*H, b.data());
}

// One workgroup's tile, one "thread" at a time: what air_compose_kernel runs between its barriers, over `tile`
// ((W + Q) x (T + B) staged elements).  Shared so that the emulator executes the kernel's own indexing.
template <int P, bool WIN = false>
SMI_HD void air_tile_thread(const AirDev &A, const Fp &F, const uint32_t *w_m, const uint32_t *tile, uint32_t T, uint32_t threads,
                            uint64_t base, uint32_t xbase_m, uint32_t step_m, uint32_t tid, uint32_t *out) {
    const uint32_t B = 1u << A.log_B, pitch = T + (WIN ? (A.S - 1) << A.log_B : B), R = A.W + A.Q;
    uint32_t x_m[P], ib[P], res[P];
    uint32_t x = mont_mul(xbase_m, A.lane_pow_m[tid], F);
    for (int q = 0; q < P; q++) {
        x_m[q] = x;
        ib[q] = (uint32_t)((base + tid + (uint64_t)q * threads) & (B - 1));
        x = mont_mul(x, step_m, F);
    }
    air_compose_points<P, WIN>(
        A, F, w_m, x_m, ib,
        [&](int q, uint32_t var) {   // rows 0 .. W-1 the trace columns, W .. R-1 the periodic ones; the next row is B further
            if (WIN) {               // row + s is s B further
                const uint32_t s = air_var_shift(var, R);
                return tile[(var - s * R) * pitch + tid + q * threads + (s << A.log_B)];
            }
            const uint32_t c = var < R ? var : var - R;
            return tile[c * pitch + tid + q * threads + (var < R ? 0 : B)];
        },
        res);
    for (int q = 0; q < P; q++) out[base + tid + (uint64_t)q * threads] = res[q];
}

// The same point without a tile (no tile fits, or the columns are not 16-byte aligned): operands straight from memory,
// one power per point.  The rare path: many columns at a large blowup, or a domain of fewer than 64 points.
template <bool WIN = false>
SMI_HD void air_direct_point(const AirDev &A, const Fp &F, const uint32_t *w_m, const uint32_t *cols, uint64_t stride, uint64_t i,
                             uint32_t *out) {
    const uint64_t B = 1ull << A.log_B, nx = (i + B) & (A.N - 1);
    const uint32_t x_m = mont_mul(A.h_m, mont_pow(A.omega_m, i, F), F), ib = (uint32_t)(i & (B - 1));
    uint32_t res;
    air_compose_points<1, WIN>(
        A, F, w_m, &x_m, &ib,
        [&](int, uint32_t var) {
            if (WIN) return air_mem_operand_win(A, var, i, [&](uint32_t c, uint32_t s) { return cols[c * stride + ((i + ((uint64_t)s << A.log_B)) & (A.N - 1))]; });
            return air_mem_operand(A, var, i, [&](uint32_t c) { return cols[c * stride + i]; }, [&](uint32_t c) { return cols[c * stride + nx]; });
        },
        &res);
    out[i] = res;
}

// air_tile_thread / air_direct_point under extension weights: the same tile, the same x, four output columns out_stride
// apart (w_m: 4 * AIR_MAX_WEIGHTS words, air_compose_points_ext)
template <int P, bool WIN = false>
SMI_HD void air_tile_thread_ext(const AirDev &A, const Fp &F, const uint32_t *w_m, const uint32_t *tile, uint32_t T, uint32_t threads,
                                uint64_t base, uint32_t xbase_m, uint32_t step_m, uint32_t tid, uint32_t *out, uint64_t out_stride) {
    const uint32_t B = 1u << A.log_B, pitch = T + (WIN ? (A.S - 1) << A.log_B : B), R = A.W + A.Q;
    uint32_t x_m[P], ib[P], res[4 * P];
    uint32_t x = mont_mul(xbase_m, A.lane_pow_m[tid], F);
    for (int q = 0; q < P; q++) {
        x_m[q] = x;
        ib[q] = (uint32_t)((base + tid + (uint64_t)q * threads) & (B - 1));
        x = mont_mul(x, step_m, F);
    }
    air_compose_points_ext<P, WIN>(
        A, F, w_m, x_m, ib,
        [&](int q, uint32_t var) {
            if (WIN) {
                const uint32_t s = air_var_shift(var, R);
                return tile[(var - s * R) * pitch + tid + q * threads + (s << A.log_B)];
            }
            const uint32_t c = var < R ? var : var - R;
            return tile[c * pitch + tid + q * threads + (var < R ? 0 : B)];
        },
        res);
    for (int e = 0; e < 4; e++)
        for (int q = 0; q < P; q++) out[e * out_stride + base + tid + (uint64_t)q * threads] = res[e * P + q];
}
template <bool WIN = false>
SMI_HD void air_direct_point_ext(const AirDev &A, const Fp &F, const uint32_t *w_m, const uint32_t *cols, uint64_t stride, uint64_t i,
                                 uint32_t *out, uint64_t out_stride) {
    const uint64_t B = 1ull << A.log_B, nx = (i + B) & (A.N - 1);
    const uint32_t x_m = mont_mul(A.h_m, mont_pow(A.omega_m, i, F), F), ib = (uint32_t)(i & (B - 1));
    uint32_t res[4];
    air_compose_points_ext<1, WIN>(
        A, F, w_m, &x_m, &ib,
        [&](int, uint32_t var) {
            if (WIN) return air_mem_operand_win(A, var, i, [&](uint32_t c, uint32_t s) { return cols[c * stride + ((i + ((uint64_t)s << A.log_B)) & (A.N - 1))]; });
            return air_mem_operand(A, var, i, [&](uint32_t c) { return cols[c * stride + i]; }, [&](uint32_t c) { return cols[c * stride + nx]; });
        },
        res);
    for (int e = 0; e < 4; e++) out[e * out_stride + i] = res[e];
}
