// lookup_core.h -- the LogUp lookup argument over a committed extension column (include/stark_mi.h, "Lookup argument"):
// the lane bodies of the multiplicity helper (two launches over an open-addressing table of row indices), of the column
// build (lookup_block_kernel) and of the two auxiliary quotients (air_lookup_compose_kernel), and the host-side tables.
// Shared by the HIP kernels (lookup.hip), the verifier (verify.hip, host) and the CPU emulator (emu_lookup.cpp), which runs
// the same lane batching and block split.  F_q arithmetic, the tuple values and the lane geometry are perm_core.h's.
//
// Number forms.  Trace and extended cells, the multiplicities and the column s are plain residues.  f_L and f_T are in
// Montgomery form coordinate by coordinate (perm_tuples); a product of a plain and a Montgomery element is plain, so
// delta = (f_T - M f_L) * (f_L f_T)^-1 with a plain numerator comes out plain and the additive scan needs no conversion.
#pragma once
#include "perm_core.h"

static_assert(SMI_LOOKUP_MAX_WIDTH == SMI_PERM_MAX_WIDTH, "LookupDev carries its tuple tables in a PermDev");

struct LookupDev {   // passed to the kernels by value
    PermDev P;       // lcol: the lookup columns, rcol: the table columns; alpha's powers and gamma
    uint32_t mcol;   // the multiplicity column
};

#define LOOKUP_EMPTY 0xffffffffu   // a free slot of the helper's table (row indices are < 2^27)

// ------------------------------------------------------------------------------------------------ the multiplicity helper
// The hash of a tuple is a function of its values alone, so that a lookup tuple and an equal table tuple start at the same
// slot; any such function gives the same multiplicities.
SMI_HD uint32_t lookup_hash(const uint32_t *trace, uint64_t n, const uint32_t *cols, uint32_t m, uint64_t row) {
    uint32_t h = 0x9e3779b9u;
    for (uint32_t j = 0; j < m; j++) {
        h ^= trace[(uint64_t)cols[j] * n + row];
        h *= 0x85ebca6bu;
        h ^= h >> 15;
    }
    return h;
}
SMI_HD bool lookup_same(const uint32_t *trace, uint64_t n, const uint32_t *acols, uint64_t arow, const uint32_t *bcols, uint64_t brow, uint32_t m) {
    for (uint32_t j = 0; j < m; j++)
        if (trace[(uint64_t)acols[j] * n + arow] != trace[(uint64_t)bcols[j] * n + brow]) return false;
    return true;
}
// Insert launch, lane t: after it every distinct table tuple owns one slot, which holds the lowest row with that tuple.
// at.cas(slot, expect, value) -> the old word; at.min(slot, value).  false: the probe ran through the whole table.
template <class Atomics>
SMI_HD bool lookup_insert_lane(const LookupDev &LD, const uint32_t *trace, uint64_t n, uint32_t *tab, uint32_t cap, uint32_t t, Atomics at) {
    uint32_t slot = lookup_hash(trace, n, LD.P.rcol, LD.P.m, t) & (cap - 1);
    for (uint32_t i = 0; i < cap; i++) {
        const uint32_t old = at.cas(tab + slot, LOOKUP_EMPTY, t);
        if (old == LOOKUP_EMPTY) return true;
        if (lookup_same(trace, n, LD.P.rcol, old, LD.P.rcol, t, LD.P.m)) {   // a slot keeps its tuple: any occupant it ever had serves
            at.min(tab + slot, t);
            return true;
        }
        slot = (slot + 1) & (cap - 1);
    }
    return false;
}
// Count launch, lane r: 0 counted, 1 the tuple is in no table row, 2 the probe ran through the whole table.
template <class Atomics>
SMI_HD int lookup_count_lane(const LookupDev &LD, const uint32_t *trace, uint64_t n, const uint32_t *tab, uint32_t cap, uint32_t r, uint32_t *mult, Atomics at) {
    uint32_t slot = lookup_hash(trace, n, LD.P.lcol, LD.P.m, r) & (cap - 1);
    for (uint32_t i = 0; i < cap; i++) {
        const uint32_t t = tab[slot];
        if (t == LOOKUP_EMPTY) return 1;
        if (lookup_same(trace, n, LD.P.rcol, t, LD.P.lcol, r, LD.P.m)) {
            at.add(mult + t, 1u);
            return 0;
        }
        slot = (slot + 1) & (cap - 1);
    }
    return 2;
}
inline uint64_t lookup_table_slots(uint64_t n) { return 2 * n; }   // a power of two >= 2 n: n is one

// ------------------------------------------------------------------------------------------------ the column
SMI_HD Fq fq_add(const Fq &a, const Fq &b, uint32_t p) {
    return Fq{{fp_add(a.c[0], b.c[0], p), fp_add(a.c[1], b.c[1], p), fp_add(a.c[2], b.c[2], p), fp_add(a.c[3], b.c[3], p)}};
}
// One lane of the column build: rows row0 .. row0 + PERM_ROWS - 1 (those at or above n count as delta = 0 and load4 may
// return anything for them).  sl[q]: the sum of the lane's delta before row q (sl[0] = 0), *sum the sum of all of them, plain.
// delta[r] = 1 / f_L(r) - M[r] / f_T(r) = (f_T - M f_L) / (f_L f_T): one F_q inversion serves the lane's four products.  A
// zero f_L or f_T is replaced by one and reported: *zero_at is the smallest 2 * row + (0: f_L, 1: f_T), or ~0.
// lookup_lane_deltas is the part behind the tuples: fl = f_L, ft = f_T and mult = M of the lane's rows on entry (fl and ft
// are overwritten).
SMI_HD void lookup_lane_deltas(uint32_t g_m, const Fp &F, uint64_t row0, uint64_t n, Fq fl[PERM_ROWS], Fq ft[PERM_ROWS], const uint32_t mult[PERM_ROWS],
                               Fq sl[PERM_ROWS], Fq *sum, uint64_t *zero_at) {
    const uint32_t p = F.p;
    Fq den[PERM_ROWS], pre[PERM_ROWS];
    const Fq one = fq_one(F);
    uint64_t za = ~0ull;
#pragma unroll
    for (int q = PERM_ROWS - 1; q >= 0; q--) {
        if (row0 + q >= n) {
            fl[q] = one;
            ft[q] = one;
        } else {
            if (fq_is_zero(ft[q])) {
                ft[q] = one;
                za = 2 * (row0 + q) + 1;
            }
            if (fq_is_zero(fl[q])) {
                fl[q] = one;
                za = 2 * (row0 + q);
            }
        }
        den[q] = fq_mul(fl[q], ft[q], g_m, F);
    }
    pre[0] = den[0];
#pragma unroll
    for (int q = 1; q < PERM_ROWS; q++) pre[q] = fq_mul(pre[q - 1], den[q], g_m, F);
    Fq inv = fq_inv(pre[PERM_ROWS - 1], g_m, F);
    Fq delta[PERM_ROWS];
#pragma unroll
    for (int q = PERM_ROWS - 1; q >= 0; q--) {
        const Fq di = q ? fq_mul(inv, pre[q - 1], g_m, F) : inv;   // 1 / den[q], Montgomery
        if (q) inv = fq_mul(inv, den[q], g_m, F);
        Fq num;                                                        // f_T - M f_L, plain
#pragma unroll
        for (int e = 0; e < 4; e++) num.c[e] = fp_sub(from_mont(ft[q].c[e], F), mont_mul(mult[q], fl[q].c[e], F), p);
        delta[q] = fq_mul(num, di, g_m, F);                         // plain
        if (row0 + q >= n) delta[q] = Fq{{0, 0, 0, 0}};
    }
    sl[0] = Fq{{0, 0, 0, 0}};
#pragma unroll
    for (int q = 1; q < PERM_ROWS; q++) sl[q] = fq_add(sl[q - 1], delta[q - 1], p);
    *sum = fq_add(sl[PERM_ROWS - 1], delta[PERM_ROWS - 1], p);
    *zero_at = za;
}
template <class Load4>
SMI_HD void lookup_lane_column(const LookupDev &LD, const Fp &F, uint64_t row0, uint64_t n, Load4 load4, Fq sl[PERM_ROWS], Fq *sum, uint64_t *zero_at) {
    const PermDev &PD = LD.P;
    Fq fl[PERM_ROWS], ft[PERM_ROWS];
    uint32_t mult[PERM_ROWS];
    perm_tuples(PD, F, PD.lcol, load4, fl);
    perm_tuples(PD, F, PD.rcol, load4, ft);
    load4(LD.mcol, mult);
    lookup_lane_deltas(PD.g_m, F, row0, n, fl, ft, mult, sl, sum, zero_at);
}

// The workgroup's additive scan of one F_q element per lane, Hillis-Steele over two buffers of 4 x PERM_BLOCK words, with the
// step structure of perm_scan_step: four base-field additions where the product scan has an F_q product.
SMI_HD void lookup_scan_step(const uint32_t (*in)[PERM_BLOCK], uint32_t (*out)[PERM_BLOCK], uint32_t tid, uint32_t off, uint32_t p) {
#pragma unroll
    for (int e = 0; e < 4; e++) out[e][tid] = tid >= off ? fp_add(in[e][tid - off], in[e][tid], p) : in[e][tid];
}

// One point of the auxiliary quotients (the arguments of lookup_compose_points, point Q of the lane's four; di_m = 1 / (x -
// tau) and izt = 1 / (x^n - tau^n), Montgomery).  Q is a template argument and the four points are instantiated one after
// the other: every index into the lane's arrays is a constant, whatever the unroller makes of a body of this size.
template <int Q>
SMI_HD void lookup_compose_point(uint32_t g_m, const Fp &F, const ExtMul &wb, const ExtMul &wt, uint32_t di_m, uint32_t izt, const Fq &fl, const Fq &ft,
                                 uint32_t mult, uint32_t sc[4][PERM_ROWS], uint32_t sx[4][PERM_ROWS], uint32_t acc[4][PERM_ROWS]) {
    const uint32_t p = F.p;
    const Fq lt = fq_mul(fl, ft, g_m, F);                   // f_L f_T, Montgomery
    const ExtMul MP = ext_mul_prepare(lt.c, g_m, F);
    uint32_t ds[4], a[4], tq[4], bq[4], u[4], v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) ds[e] = fp_sub(sx[e][Q], sc[e][Q], p);
    ext_mul_prepared(ds, MP, F, a);                         // (s(w x) - s(x)) f_L f_T, plain
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const uint32_t t = fp_add(fp_sub(a[e], from_mont(ft.c[e], F), p), mont_mul(mult, fl.c[e], F), p);
        tq[e] = mont_mul(t, izt, F);
        bq[e] = mont_mul(sc[e][Q], di_m, F);
    }
    ext_mul_prepared(bq, wb, F, u);
    ext_mul_prepared(tq, wt, F, v);
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e][Q] = fp_add(acc[e][Q], fp_add(u[e], v[e], p), p);
}

// One lane of the auxiliary quotients: PERM_ROWS consecutive points i0 .. i0 + PERM_ROWS - 1; the arguments are those of
// perm_compose_points with s in place of z (sc: this row, sx: one row further, plain).  Per point
//   w_b s / (x - tau)  +  w_t ((s' - s) f_L f_T - f_T + M f_L) / (x^n - tau^n).
// 1 / (x_i - tau) is batched over the lane's points in the base field: one Fermat power per lane.
template <class Load4>
SMI_HD void lookup_compose_points(const LookupDev &LD, const Fp &F, const ExtMul &wb, const ExtMul &wt, uint32_t tau_m, const uint32_t *izt_m, uint32_t B,
                                  uint64_t i0, uint32_t x0_m, uint32_t omega_m, Load4 load4, uint32_t sc[4][PERM_ROWS],
                                  uint32_t sx[4][PERM_ROWS], uint32_t acc[4][PERM_ROWS]) {
    static_assert(PERM_ROWS == 4, "the four points are written out");
    const PermDev &PD = LD.P;
    const uint32_t p = F.p;
    uint32_t d[PERM_ROWS], pre[PERM_ROWS], di[PERM_ROWS], mult[PERM_ROWS];
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
    Fq fl[PERM_ROWS], ft[PERM_ROWS];
    perm_tuples(PD, F, PD.lcol, load4, fl);
    perm_tuples(PD, F, PD.rcol, load4, ft);
    load4(LD.mcol, mult);
    const uint32_t ib = (uint32_t)(i0 & (B - 1));   // i0 and B are multiples of 4: the four table entries are consecutive
    lookup_compose_point<0>(PD.g_m, F, wb, wt, di[0], izt_m[ib], fl[0], ft[0], mult[0], sc, sx, acc);
    lookup_compose_point<1>(PD.g_m, F, wb, wt, di[1], izt_m[ib + 1], fl[1], ft[1], mult[1], sc, sx, acc);
    lookup_compose_point<2>(PD.g_m, F, wb, wt, di[2], izt_m[ib + 2], fl[2], ft[2], mult[2], sc, sx, acc);
    lookup_compose_point<3>(PD.g_m, F, wb, wt, di[3], izt_m[ib + 3], fl[3], ft[3], mult[3], sc, sx, acc);
}

// ------------------------------------------------------------------------------------------------ host side
// the sentences of the lookup verifier's opening checks, in the order of verify.hip's OpeningWords: length, row, path,
// authentication, canonical, composition.  tests/test_gpu_lookup.py reaches each of them.
static const char *const LOOKUP_SENTENCES[6] = {"lookup openings: wrong length",
                                                "lookup openings: malformed row",
                                                "lookup openings: malformed path",
                                                "lookup openings: authentication path does not verify",
                                                "lookup openings: an opened value is not canonical",
                                                "lookup openings: the composition of the opened rows is not the codeword value"};

inline int lookup_validate(const smi_air_lookup *lk, uint32_t n_cols, std::string *why) {
    auto fail = [&](const std::string &s) {
        if (why) *why = s;
        return SMI_ERR_BAD_ARG;
    };
    if (!lk) return fail("lookup: null argument");
    if (lk->width < 1 || lk->width > SMI_LOOKUP_MAX_WIDTH)
        return fail("lookup: width must be in 1 .. SMI_LOOKUP_MAX_WIDTH (" + std::to_string(SMI_LOOKUP_MAX_WIDTH) + ")");
    if (!lk->lookup_col || !lk->table_col) return fail("lookup: null column list");
    if (lk->mult_col >= n_cols) return fail("lookup: mult_col must be < n_cols");
    for (uint32_t j = 0; j < lk->width; j++) {
        if (lk->lookup_col[j] >= n_cols) return fail("lookup: lookup_col must be < n_cols");
        if (lk->table_col[j] >= n_cols) return fail("lookup: table_col must be < n_cols");
        if (lk->lookup_col[j] == lk->mult_col || lk->table_col[j] == lk->mult_col) return fail("lookup: mult_col must be none of the tuple columns");
    }
    return SMI_OK;
}

// smi_air_plan_lookup: the AIR's own plan with the auxiliary transition of degree 3 counted in
inline int lookup_plan(uint64_t p, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_lookup *lk, uint32_t *degree, uint64_t *fri_expansion,
                       std::string *why) {
    uint32_t d = 0;
    const int rc = air_validate(p, cfg, air, &d, nullptr, why);
    if (rc != SMI_OK) return rc;
    const int lrc = lookup_validate(lk, cfg->n_cols, why);
    if (lrc != SMI_OK) return lrc;
    if ((p & 3) != 1) {
        if (why) *why = "lookup: p = 3 (mod 4): the quartic extension does not exist";
        return SMI_ERR_BAD_ARG;
    }
    if (d < 3) d = 3;
    const uint64_t B = 1ull << cfg->log_blowup;
    uint64_t D = 1;
    while (D < d - 1) D <<= 1;
    const uint64_t E = D > B ? 0 : B / D;
    if (E < 4) {
        if (why) *why = "lookup: 2^log_blowup / D < 4";
        return SMI_ERR_EXPANSION_TOO_SMALL;
    }
    if (degree) *degree = d;
    if (fri_expansion) *fri_expansion = E;
    return SMI_OK;
}

inline void lookup_build(const Fp &F, uint32_t g, const smi_air_lookup *lk, const uint64_t ch[8], LookupDev *LD) {
    const smi_air_perm as_perm = {lk->width, 0, lk->lookup_col, lk->table_col};
    perm_build(F, g, &as_perm, ch, &LD->P);
    LD->mcol = lk->mult_col;
}
