// xargs_core.h -- the argument list with selectors and periodic members (include/stark_mi.h, "Argument list with selectors
// and periodic members"): args_core.h's layer with operands in place of columns.  An operand is a trace column or a periodic
// column of the AIR, either of them at this row or one row later ("Argument list: next-row operands", XOP_NEXT); every
// argument has two optional selectors.  Shared by the HIP kernels (xargs.hip), the verifier
// (verify.hip, host) and the CPU emulator (emu_xargs.cpp), which runs the same lane batching and block split.
//
// Number forms are args_core.h's.  A selector cell is a plain residue S: g = 1 + S (f - 1) is formed in Montgomery form
// (S goes through to_mont once per row), S f_T and M S_b are plain products.  XArgsDev travels as a kernel argument and is
// indexed with the argument number and the tuple member only, both wave-uniform, and so is the kind of an operand: every
// table read stays a scalar load and every branch on it is taken by the whole wave.
#pragma once
#include <algorithm>

#include "args_core.h"
#include "deep_core.h"

#define XOP_PER 0x100u   // operand code: trace column c is c (< 64), periodic column j is XOP_PER | j
#define XOP_NEXT 0x200u  // ... read one row later, cyclically ("Argument list: next-row operands"): SMI_ARG_NEXT_ROW on the device

struct XArgsDev {   // passed to the kernels by value: 960 bytes
    uint32_t A, g_m;
    uint32_t apow_mm[SMI_PERM_MAX_WIDTH][4];   // alpha^j * R^2
    uint32_t gamma_m[4];                       // gamma * R
    uint32_t kind[SMI_ARGS_MAX], m[SMI_ARGS_MAX], mcol[SMI_ARGS_MAX];
    uint32_t asel[SMI_ARGS_MAX], bsel[SMI_ARGS_MAX];   // operand codes, or SMI_ARG_NO_SELECTOR
    uint32_t aop[SMI_ARGS_MAX][SMI_PERM_MAX_WIDTH], bop[SMI_ARGS_MAX][SMI_PERM_MAX_WIDTH];
    // the raw periodic values as air_periodic_plan groups them (AirPeriodic::vals): column j has 2^plog[j] values from
    // pvals + pfirst[j], and pfirst[j] is a multiple of its period.  The column build and the helper read these; the
    // compose launch reads the extended tables of the AIR blob instead.
    uint32_t plog[SMI_AIR_MAX_PERIODIC], pfirst[SMI_AIR_MAX_PERIODIC];
    const uint32_t *pvals;
};
static_assert(sizeof(XArgsDev) <= 1024, "the kernel arguments stay well inside 4 KB");
static_assert(SMI_AIR_MAX_PERIODIC <= XOP_PER && 64 <= XOP_PER, "an operand code holds a column of either kind");

// Shared-table lookups (include/stark_mi.h, "Shared-table lookups"): the J looked-up tuples of every argument and their
// selectors.  It travels by value NEXT TO XArgsDev and only to the kernels' shared instantiations, which a list with some
// J >= 2 takes; XArgsDev and the instantiations of every other list stay what they were.  For a shared lookup XD.aop[a] is
// tuple 0 and XD.asel[a] is SMI_ARG_NO_SELECTOR; XD.kind[a] is the kind alone (the low byte).  Indexed like XArgsDev with
// wave-uniform numbers only.
struct XSharedDev {   // 1184 bytes
    uint32_t J[SMI_ARGS_MAX];                           // tuples of argument a; 1 for a permutation and for a single lookup
    uint32_t sel[SMI_ARGS_MAX][SMI_ARG_MAX_TUPLES];     // operand codes, or SMI_ARG_NO_SELECTOR
    uint32_t op[SMI_ARGS_MAX][SMI_ARG_MAX_TUPLES][SMI_PERM_MAX_WIDTH];
};
struct XNoShared {};   // in the place of XSharedDev for a list without a shared lookup: every use of it folds away
static_assert(sizeof(XArgsDev) + sizeof(XSharedDev) + 192 <= 4096, "the kernel arguments of the shared instantiations stay inside 4 KB");
SMI_HD uint32_t xshared_tuples(const XNoShared &, uint32_t) { return 1u; }
SMI_HD uint32_t xshared_tuples(const XSharedDev &SH, uint32_t a) { return SH.J[a]; }

SMI_HD bool xop_periodic(uint32_t op) { return (op & XOP_PER) != 0; }
SMI_HD bool xop_next(uint32_t op) { return (op & XOP_NEXT) != 0; }
// the operand code of a validated operand v (W = n_cols): SMI_ARG_NO_SELECTOR stays what it is
inline uint32_t xop_code(uint32_t v, uint32_t W) {
    if (v == SMI_ARG_NO_SELECTOR) return v;
    const uint32_t t = v & ~SMI_ARG_NEXT_ROW, c = t < W ? t : (XOP_PER | (t - 2 * W));
    return (v & SMI_ARG_NEXT_ROW) ? (c | XOP_NEXT) : c;
}
// A next-row operand at the lane's four rows at .. at + 3 of a cyclic column of len words (a power of two): the words at + 1 ..
// at + 4 modulo len.  xargs_next4: len >= 4 and `at` a multiple of 4 below len -- three of the lane's own four words (own)
// serve, the fourth is one word further and wraps only to word 0.  xargs_next4_words: any len, word by word; a row at or above
// `rows` gives zero.
SMI_HD void xargs_next4(const uint32_t *col, uint64_t at, uint64_t len, const uint32_t own[PERM_ROWS], uint32_t v[PERM_ROWS]) {
    v[0] = own[1], v[1] = own[2], v[2] = own[3];
    v[3] = col[(at + 4) & (len - 1)];
}
SMI_HD void xargs_next4_words(const uint32_t *col, uint64_t at, uint64_t len, uint64_t rows, uint32_t v[PERM_ROWS]) {
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) v[q] = at + q < rows ? col[(at + q + 1) & (len - 1)] : 0u;
}
// the four values of periodic column j at the rows row0 .. row0 + 3 of the trace: v_j[(row0 + q) mod P_j], word by word --
// with P_j = 1 or 2 the wrap falls inside the lane
SMI_HD void xargs_periodic_rows(const XArgsDev &XD, uint32_t j, uint64_t row0, uint32_t v[PERM_ROWS]) {
    const uint32_t mask = (1u << XD.plog[j]) - 1u;
    const uint32_t *src = XD.pvals + XD.pfirst[j];
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) v[q] = src[(uint32_t)(row0 + q) & mask];
}
// one cell of an operand on the trace (the multiplicity helper).  NEXT: the list has a next-row operand, which reads row
// (row + 1) mod n; without it the codes are bare and nothing here looks at the flag
template <bool NEXT = false>
SMI_HD uint32_t xargs_cell(const XArgsDev &XD, const uint32_t *trace, uint64_t n, uint32_t op, uint64_t row) {
    if (NEXT) {
        if (xop_next(op)) row = (row + 1) & (n - 1);
        if (!xop_periodic(op)) op &= 0xffu;
    }
    if (xop_periodic(op)) return XD.pvals[XD.pfirst[op & 0xffu] + ((uint32_t)row & ((1u << XD.plog[op & 0xffu]) - 1u))];
    return trace[(uint64_t)op * n + row];
}

// On the evaluation coset periodic column j is its extended table of L_j = P_j B entries read modulo its length, exactly as
// air_periodic_operand reads it.  -> the table and where the entries of the points i0 .. i0 + 3 start in it; *L = L_j.  B >= 4 and
// i0 is a multiple of 4, so the four entries are consecutive and end inside the table.
SMI_HD const uint32_t *xargs_table_at(const uint32_t *plog, const uint32_t *pofs, const uint32_t *ptab, uint32_t j, uint64_t i0, uint64_t *L,
                                      uint64_t *at) {
    *L = 1ull << plog[j];
    *at = i0 & (*L - 1);
    return ptab + pofs[j];
}

// ------------------------------------------------------------------------------------------------ the columns
// f <- g = 1 + S (f - 1) for the lane's rows (f Montgomery, S plain)
SMI_HD void xargs_select(const Fp &F, const uint32_t s[PERM_ROWS], Fq f[PERM_ROWS]) {
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) {
        const uint32_t s_m = to_mont(s[q], F);
        f[q].c[0] = fp_add(F.r1, mont_mul(s_m, fp_sub(f[q].c[0], F.r1, F.p), F), F.p);
#pragma unroll
        for (int e = 1; e < 4; e++) f[q].c[e] = mont_mul(s_m, f[q].c[e], F);
    }
}
// lookup_lane_deltas (lookup_core.h) with a selector on the lookup side: delta = S_a / f_L - M / f_T = (S_a f_T - M f_L) /
// (f_L f_T), sa = S_a of the lane's rows (plain), mult = M S_b.  With sa = 1 every value is lookup_lane_deltas's
// (mont_mul(1, x) is from_mont(x)).  A zero f_L or f_T is reported whatever the selectors hold.
SMI_HD void xlookup_lane_deltas(uint32_t g_m, const Fp &F, uint64_t row0, uint64_t n, Fq fl[PERM_ROWS], Fq ft[PERM_ROWS], const uint32_t sa[PERM_ROWS],
                                const uint32_t mult[PERM_ROWS], Fq sl[PERM_ROWS], Fq *sum, uint64_t *zero_at) {
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
        Fq num;                                                        // S_a f_T - M f_L, plain
#pragma unroll
        for (int e = 0; e < 4; e++) num.c[e] = fp_sub(mont_mul(sa[q], ft[q].c[e], F), mont_mul(mult[q], fl[q].c[e], F), p);
        delta[q] = fq_mul(num, di, g_m, F);                         // plain
        if (row0 + q >= n) delta[q] = Fq{{0, 0, 0, 0}};
    }
    sl[0] = Fq{{0, 0, 0, 0}};
#pragma unroll
    for (int q = 1; q < PERM_ROWS; q++) sl[q] = fq_add(sl[q - 1], delta[q - 1], p);
    *sum = fq_add(sl[PERM_ROWS - 1], delta[PERM_ROWS - 1], p);
    *zero_at = za;
}
// S_a and M S_b of a lookup's four rows or points (plain); load4(op, v) the operand loader
template <class Load4>
SMI_HD void xlookup_weights(const XArgsDev &XD, uint32_t a, const Fp &F, Load4 load4, uint32_t sa[PERM_ROWS], uint32_t mult[PERM_ROWS]) {
    load4(XD.mcol[a], mult);
    if (XD.asel[a] != SMI_ARG_NO_SELECTOR) load4(XD.asel[a], sa);
    else sa[0] = sa[1] = sa[2] = sa[3] = 1u;
    if (XD.bsel[a] != SMI_ARG_NO_SELECTOR) {
        uint32_t sb[PERM_ROWS];
        load4(XD.bsel[a], sb);
#pragma unroll
        for (int q = 0; q < PERM_ROWS; q++) mult[q] = mont_mul(to_mont(mult[q], F), sb[q], F);
    }
}
// One lane of the block launch for argument a: perm_lane_column or lookup_lane_column behind tuples of operands, with the
// selectors.  load4(op, v): the four cells of operand op at the lane's rows (anything for rows at or above n).  A
// permutation goes through perm_lane_ratios with g_L and g_R in place of f_L and f_R; a lookup through xlookup_lane_deltas.
// pl[q]: the lane's prefix before row q, *agg: the lane's product or sum.  *key: ~0, or for the smallest row of the lane
// with a zero denominator 16 row + 2 a + side (side 0: f_L, side 1: g_R or f_T).
template <class Load4>
SMI_HD void xargs_lane_column(const XArgsDev &XD, uint32_t a, const Fp &F, uint64_t row0, uint64_t n, Load4 load4, Fq pl[PERM_ROWS], Fq *agg, uint64_t *key) {
    Fq fl[PERM_ROWS], fr[PERM_ROWS];
    tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, XD.aop[a], load4, fl);
    tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, XD.bop[a], load4, fr);
    uint64_t z;
    if (XD.kind[a] == SMI_ARG_PERM) {
        uint32_t s[PERM_ROWS];
        if (XD.asel[a] != SMI_ARG_NO_SELECTOR) {
            load4(XD.asel[a], s);
            xargs_select(F, s, fl);
        }
        if (XD.bsel[a] != SMI_ARG_NO_SELECTOR) {
            load4(XD.bsel[a], s);
            xargs_select(F, s, fr);
        }
        perm_lane_ratios(XD.g_m, F, row0, n, fl, fr, pl, agg, &z);            // z: the row
        *key = z == ~0ull ? z : 16 * z + 2 * a + 1;
    } else {
        uint32_t sa[PERM_ROWS], mult[PERM_ROWS];
        xlookup_weights(XD, a, F, load4, sa, mult);
        xlookup_lane_deltas(XD.g_m, F, row0, n, fl, fr, sa, mult, pl, agg, &z);   // z: 2 row + side
        *key = z == ~0ull ? z : 16 * (z >> 1) + 2 * a + (z & 1);
    }
}

// ---- shared-table lookups: the fold.  (Nn, P) <- (Nn f_j + S_j P, P f_j) over the tuples j < J from (0, 1), so that
// sum_j S_j / f_j = Nn / P: after it a row has ONE denominator P f_T and one numerator Nn f_T - (M S_b) P, and the lane's
// batched inversion is the single lookup's.  P is Montgomery, Nn plain (plain times Montgomery is plain; S_j is a plain cell);
// the first tuple sets (S_0, f_0) without a product.  Two F_q values a row are live across the tuples, whatever J is.
// DETECT (the column build): a zero f_j of a row below n is replaced by one and zj[q] keeps the smallest such j of row q
// (zj comes in as ~0).
template <bool DETECT, class Load4>
SMI_HD void xshared_fold(const XArgsDev &XD, const XSharedDev &SH, uint32_t a, const Fp &F, uint64_t row0, uint64_t n, Load4 load4, Fq P[PERM_ROWS],
                         Fq Nn[PERM_ROWS], uint32_t zj[PERM_ROWS]) {
    const uint32_t p = F.p;
    for (uint32_t j = 0; j < SH.J[a]; j++) {   // wave-uniform
        Fq f[PERM_ROWS];
        uint32_t s[PERM_ROWS];
        tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, SH.op[a][j], load4, f);
        if (SH.sel[a][j] != SMI_ARG_NO_SELECTOR) load4(SH.sel[a][j], s);
        else s[0] = s[1] = s[2] = s[3] = 1u;
#pragma unroll
        for (int q = 0; q < PERM_ROWS; q++) {
            if (DETECT && row0 + q < n && fq_is_zero(f[q])) {
                f[q] = fq_one(F);
                if (zj[q] == ~0u) zj[q] = j;
            }
            if (!j) {
                P[q] = f[q];
                Nn[q] = Fq{{s[q], 0, 0, 0}};
            } else {
                const Fq t = fq_mul(Nn[q], f[q], XD.g_m, F);   // plain
#pragma unroll
                for (int e = 0; e < 4; e++) Nn[q].c[e] = fp_add(t.c[e], mont_mul(s[q], P[q].c[e], F), p);
                P[q] = fq_mul(P[q], f[q], XD.g_m, F);
            }
        }
    }
}
// xlookup_lane_deltas behind the fold: delta = Nn / P - M S_b / f_T = (Nn f_T - (M S_b) P) / (P f_T).  *zero_at: the smallest
// 8 row + side, side = j for f_j and J for f_T, or ~0.
SMI_HD void xshared_lane_deltas(uint32_t g_m, const Fp &F, uint64_t row0, uint64_t n, uint32_t J, Fq P[PERM_ROWS], Fq Nn[PERM_ROWS], Fq ft[PERM_ROWS],
                                const uint32_t zj[PERM_ROWS], const uint32_t mult[PERM_ROWS], Fq sl[PERM_ROWS], Fq *sum, uint64_t *zero_at) {
    const uint32_t p = F.p;
    Fq den[PERM_ROWS], pre[PERM_ROWS];
    const Fq one = fq_one(F);
    uint64_t za = ~0ull;
#pragma unroll
    for (int q = PERM_ROWS - 1; q >= 0; q--) {
        if (row0 + q >= n) {
            P[q] = one;
            ft[q] = one;
        } else {
            if (fq_is_zero(ft[q])) {
                ft[q] = one;
                za = 8 * (row0 + q) + J;
            }
            if (zj[q] != ~0u) za = 8 * (row0 + q) + zj[q];
        }
        den[q] = fq_mul(P[q], ft[q], g_m, F);
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
        Fq num = fq_mul(Nn[q], ft[q], g_m, F);                         // Nn f_T - (M S_b) P, plain
#pragma unroll
        for (int e = 0; e < 4; e++) num.c[e] = fp_sub(num.c[e], mont_mul(mult[q], P[q].c[e], F), p);
        delta[q] = fq_mul(num, di, g_m, F);                         // plain
        if (row0 + q >= n) delta[q] = Fq{{0, 0, 0, 0}};
    }
    sl[0] = Fq{{0, 0, 0, 0}};
#pragma unroll
    for (int q = 1; q < PERM_ROWS; q++) sl[q] = fq_add(sl[q - 1], delta[q - 1], p);
    *sum = fq_add(sl[PERM_ROWS - 1], delta[PERM_ROWS - 1], p);
    *zero_at = za;
}
// xargs_lane_column of a list with a shared lookup.  *key: the smallest 64 row + 8 a + side with a zero denominator, or ~0:
// side = j for f_j and J for f_T, so a single lookup keeps 0 for f_L and 1 for f_T and a permutation 1 for g_R, and the
// order is (row, argument, side).  A list without a shared lookup keeps the key of the function above.
template <class Load4>
SMI_HD void xargs_lane_column(const XArgsDev &XD, const XSharedDev &SH, uint32_t a, const Fp &F, uint64_t row0, uint64_t n, Load4 load4, Fq pl[PERM_ROWS],
                              Fq *agg, uint64_t *key) {
    if (SH.J[a] < 2) {
        xargs_lane_column(XD, a, F, row0, n, load4, pl, agg, key);
        if (*key != ~0ull) *key = 64 * (*key >> 4) + 8 * a + (*key & 1);
        return;
    }
    Fq P[PERM_ROWS], Nn[PERM_ROWS], ft[PERM_ROWS];
    uint32_t zj[PERM_ROWS] = {~0u, ~0u, ~0u, ~0u}, sa[PERM_ROWS], mult[PERM_ROWS];
    xshared_fold<true>(XD, SH, a, F, row0, n, load4, P, Nn, zj);
    tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, XD.bop[a], load4, ft);
    xlookup_weights(XD, a, F, load4, sa, mult);   // XD.asel[a] is unset: sa is all ones and is not read
    uint64_t z;
    xshared_lane_deltas(XD.g_m, F, row0, n, SH.J[a], P, Nn, ft, zj, mult, pl, agg, &z);
    *key = z == ~0ull ? z : 64 * (z >> 3) + 8 * a + (z & 7);
}
template <class Load4>
SMI_HD void xargs_lane_column(const XArgsDev &XD, const XNoShared &, uint32_t a, const Fp &F, uint64_t row0, uint64_t n, Load4 load4, Fq pl[PERM_ROWS],
                              Fq *agg, uint64_t *key) {
    xargs_lane_column(XD, a, F, row0, n, load4, pl, agg, key);
}

// ------------------------------------------------------------------------------------------------ the multiplicity helper
// lookup_core.h's helper over operands: the hash and the comparison read cells through xargs_cell, an unselected row takes
// no part.  The hash is lookup_hash's function of the values.
template <bool NEXT = false>
SMI_HD uint32_t xlookup_hash(const XArgsDev &XD, const uint32_t *trace, uint64_t n, const uint32_t *ops, uint32_t m, uint64_t row) {
    uint32_t h = 0x9e3779b9u;
    for (uint32_t j = 0; j < m; j++) {
        h ^= xargs_cell<NEXT>(XD, trace, n, ops[j], row);
        h *= 0x85ebca6bu;
        h ^= h >> 15;
    }
    return h;
}
template <bool NEXT = false>
SMI_HD bool xlookup_same(const XArgsDev &XD, const uint32_t *trace, uint64_t n, const uint32_t *aops, uint64_t arow, const uint32_t *bops, uint64_t brow,
                         uint32_t m) {
    for (uint32_t j = 0; j < m; j++)
        if (xargs_cell<NEXT>(XD, trace, n, aops[j], arow) != xargs_cell<NEXT>(XD, trace, n, bops[j], brow)) return false;
    return true;
}
template <bool NEXT = false>
SMI_HD bool xargs_selected(const XArgsDev &XD, const uint32_t *trace, uint64_t n, uint32_t sel, uint64_t row) {
    return sel == SMI_ARG_NO_SELECTOR || xargs_cell<NEXT>(XD, trace, n, sel, row) != 0;
}
// Insert launch, lane t (lookup_insert_lane): a table row with S_b = 0 is not inserted.
template <bool NEXT = false, class Atomics>
SMI_HD bool xlookup_insert_lane(const XArgsDev &XD, uint32_t a, const uint32_t *trace, uint64_t n, uint32_t *tab, uint32_t cap, uint32_t t, Atomics at) {
    if (!xargs_selected<NEXT>(XD, trace, n, XD.bsel[a], t)) return true;
    const uint32_t *bops = XD.bop[a], m = XD.m[a];
    uint32_t slot = xlookup_hash<NEXT>(XD, trace, n, bops, m, t) & (cap - 1);
    for (uint32_t i = 0; i < cap; i++) {
        const uint32_t old = at.cas(tab + slot, LOOKUP_EMPTY, t);
        if (old == LOOKUP_EMPTY) return true;
        if (xlookup_same<NEXT>(XD, trace, n, bops, old, bops, t, m)) {   // a slot keeps its tuple: any occupant it ever had serves
            at.min(tab + slot, t);
            return true;
        }
        slot = (slot + 1) & (cap - 1);
    }
    return false;
}
// Count launch: the probe of one looked-up tuple (operands aops, selector sel) of row r.  0 counted or not selected, 1 the
// tuple is in no selected table row, 2 the probe ran through the whole table.
template <bool NEXT = false, class Atomics>
SMI_HD int xlookup_count_tuple(const XArgsDev &XD, uint32_t a, const uint32_t *trace, uint64_t n, const uint32_t *aops, uint32_t sel, const uint32_t *tab,
                               uint32_t cap, uint32_t r, uint32_t *mult, Atomics at) {
    if (!xargs_selected<NEXT>(XD, trace, n, sel, r)) return 0;
    const uint32_t *bops = XD.bop[a], m = XD.m[a];
    uint32_t slot = xlookup_hash<NEXT>(XD, trace, n, aops, m, r) & (cap - 1);
    for (uint32_t i = 0; i < cap; i++) {
        const uint32_t t = tab[slot];
        if (t == LOOKUP_EMPTY) return 1;
        if (xlookup_same<NEXT>(XD, trace, n, bops, t, aops, r, m)) {
            at.add(mult + t, 1u);
            return 0;
        }
        slot = (slot + 1) & (cap - 1);
    }
    return 2;
}
// Count launch, lane r (lookup_count_lane): the statuses of xlookup_count_tuple for the argument's one tuple.
template <bool NEXT = false, class Atomics>
SMI_HD int xlookup_count_lane(const XArgsDev &XD, uint32_t a, const uint32_t *trace, uint64_t n, const uint32_t *tab, uint32_t cap, uint32_t r,
                              uint32_t *mult, Atomics at) {
    return xlookup_count_tuple<NEXT>(XD, a, trace, n, XD.aop[a], XD.asel[a], tab, cap, r, mult, at);
}
// Count launch of a shared lookup, lane r: one probe per selected tuple of the row, so M[t] counts the (row, tuple) pairs
// that hit table row t.  -> bit 0: some tuple is missing, *miss = the smallest such j; bit 1: a probe ran through the table.
template <bool NEXT = false, class Atomics>
SMI_HD int xshared_count_lane(const XArgsDev &XD, const XSharedDev &SH, uint32_t a, const uint32_t *trace, uint64_t n, const uint32_t *tab, uint32_t cap,
                              uint32_t r, uint32_t *mult, Atomics at, uint32_t *miss) {
    int out = 0;
    for (uint32_t j = 0; j < SH.J[a]; j++) {
        const int got = xlookup_count_tuple<NEXT>(XD, a, trace, n, SH.op[a][j], SH.sel[a][j], tab, cap, r, mult, at);
        if (got == 1 && !(out & 1)) *miss = j, out |= 1;
        if (got == 2) out |= 2;
    }
    return out;
}

// ------------------------------------------------------------------------------------------------ the auxiliary quotients
// lookup_compose_point (lookup_core.h) with the selectors: the transition's numerator is (s' - s) f_L f_T - S_a f_T +
// (M S_b) f_L; sa = S_a and mult = M S_b at the point, plain.
template <int Q>
SMI_HD void xlookup_compose_point(uint32_t g_m, const Fp &F, const ExtMul &wb, const ExtMul &wt, uint32_t di_m, uint32_t izt, const Fq &fl, const Fq &ft,
                                  uint32_t sa, uint32_t mult, uint32_t sc[4][PERM_ROWS], uint32_t sx[4][PERM_ROWS], uint32_t acc[4][PERM_ROWS]) {
    const uint32_t p = F.p;
    const Fq lt = fq_mul(fl, ft, g_m, F);                   // f_L f_T, Montgomery
    const ExtMul MP = ext_mul_prepare(lt.c, g_m, F);
    uint32_t ds[4], a[4], tq[4], bq[4], u[4], v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) ds[e] = fp_sub(sx[e][Q], sc[e][Q], p);
    ext_mul_prepared(ds, MP, F, a);                         // (s(w x) - s(x)) f_L f_T, plain
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const uint32_t t = fp_add(fp_sub(a[e], mont_mul(sa, ft.c[e], F), p), mont_mul(mult, fl.c[e], F), p);
        tq[e] = mont_mul(t, izt, F);
        bq[e] = mont_mul(sc[e][Q], di_m, F);
    }
    ext_mul_prepared(bq, wb, F, u);
    ext_mul_prepared(tq, wt, F, v);
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e][Q] = fp_add(acc[e][Q], fp_add(u[e], v[e], p), p);
}

// xlookup_compose_point behind the fold: S_a f_T becomes Nn f_T and f_L becomes P, so the transition's numerator is
// (s' - s) P f_T - Nn f_T + (M S_b) P; P, ft Montgomery, Nn and mult plain.
template <int Q>
SMI_HD void xshared_compose_point(uint32_t g_m, const Fp &F, const ExtMul &wb, const ExtMul &wt, uint32_t di_m, uint32_t izt, const Fq &P, const Fq &ft,
                                  const Fq &Nn, uint32_t mult, uint32_t sc[4][PERM_ROWS], uint32_t sx[4][PERM_ROWS], uint32_t acc[4][PERM_ROWS]) {
    const uint32_t p = F.p;
    const ExtMul MT = ext_mul_prepare(ft.c, g_m, F);
    uint32_t lt[4], nf[4], ds[4], a[4], tq[4], bq[4], u[4], v[4];
    ext_mul_prepared(P.c, MT, F, lt);                       // P f_T, Montgomery
    ext_mul_prepared(Nn.c, MT, F, nf);                      // Nn f_T, plain
    const ExtMul MP = ext_mul_prepare(lt, g_m, F);
#pragma unroll
    for (int e = 0; e < 4; e++) ds[e] = fp_sub(sx[e][Q], sc[e][Q], p);
    ext_mul_prepared(ds, MP, F, a);                         // (s(w x) - s(x)) P f_T, plain
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const uint32_t t = fp_add(fp_sub(a[e], nf[e], p), mont_mul(mult, P.c[e], F), p);
        tq[e] = mont_mul(t, izt, F);
        bq[e] = mont_mul(sc[e][Q], di_m, F);
    }
    ext_mul_prepared(bq, wb, F, u);
    ext_mul_prepared(tq, wt, F, v);
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e][Q] = fp_add(acc[e][Q], fp_add(u[e], v[e], p), p);
}
// the two quotients of shared lookup a at the lane's four points: the fold, then the point function above.  di: 1 / (x_q -
// tau), zt: what multiplies the transition's numerator (Montgomery both).  The overload for XNoShared is never reached.
template <class Load4>
SMI_HD void xshared_compose(const XArgsDev &XD, const XSharedDev &SH, uint32_t a, const Fp &F, const ExtMul &wb, const ExtMul &wt, const uint32_t di[PERM_ROWS],
                            const uint32_t zt[PERM_ROWS], Load4 load4, uint32_t cc[4][PERM_ROWS], uint32_t cx[4][PERM_ROWS], uint32_t acc[4][PERM_ROWS]) {
    Fq P[PERM_ROWS], Nn[PERM_ROWS], ft[PERM_ROWS];
    uint32_t sa[PERM_ROWS], mult[PERM_ROWS];
    xshared_fold<false>(XD, SH, a, F, 0, 0, load4, P, Nn, sa);
    tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, XD.bop[a], load4, ft);
    xlookup_weights(XD, a, F, load4, sa, mult);   // sa: all ones, not read
    xshared_compose_point<0>(XD.g_m, F, wb, wt, di[0], zt[0], P[0], ft[0], Nn[0], mult[0], cc, cx, acc);
    xshared_compose_point<1>(XD.g_m, F, wb, wt, di[1], zt[1], P[1], ft[1], Nn[1], mult[1], cc, cx, acc);
    xshared_compose_point<2>(XD.g_m, F, wb, wt, di[2], zt[2], P[2], ft[2], Nn[2], mult[2], cc, cx, acc);
    xshared_compose_point<3>(XD.g_m, F, wb, wt, di[3], zt[3], P[3], ft[3], Nn[3], mult[3], cc, cx, acc);
}
template <class Load4>
SMI_HD void xshared_compose(const XArgsDev &, const XNoShared &, uint32_t, const Fp &, const ExtMul &, const ExtMul &, const uint32_t *, const uint32_t *, Load4,
                            uint32_t (*)[PERM_ROWS], uint32_t (*)[PERM_ROWS], uint32_t (*)[PERM_ROWS]) {}

// One lane and trip of the streaming launch: PERM_ROWS consecutive points i0 .. i0 + PERM_ROWS - 1 and all A arguments.
//   w: 8 A unreduced weight coordinates (argument a's boundary weight at 8 a, its transition weight at 8 a + 4), read with
//   uniform addresses; load4(op, v): operand op at the four points -- an extended trace column, or the extended periodic
//   table read modulo its length; loadc(col, next, v): coordinate column col < 4 A of the extended auxiliary columns at the
//   four points, or one row further; acc[e][q]: the composition so far, kept in registers across the arguments.
//   1 / (x_i - tau) (one Fermat power per lane) and the four entries of the 1 / (x^n - tau^n) table are fetched once, not
//   once per argument.
// SH: XSharedDev for a list with a shared lookup (its arguments with J >= 2 go through xshared_compose), XNoShared otherwise.
template <class SHT, class Load4, class LoadC>
SMI_HD void xargs_compose_points(const XArgsDev &XD, const SHT &SH, const Fp &F, const uint64_t *w, uint32_t tau_m, const uint32_t *izt_m, uint32_t B, uint64_t i0,
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
    for (uint32_t a = 0; a < XD.A; a++) {   // wave-uniform
        uint32_t cc[4][PERM_ROWS], cx[4][PERM_ROWS], wm[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            loadc(4 * a + e, false, cc[e]);
            loadc(4 * a + e, true, cx[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[8 * a + e], F);
        const ExtMul wb = ext_mul_prepare(wm, XD.g_m, F);
#pragma unroll
        for (int e = 0; e < 4; e++) wm[e] = to_mont_u64(w[8 * a + 4 + e], F);
        const ExtMul wt = ext_mul_prepare(wm, XD.g_m, F);
        if (xshared_tuples(SH, a) >= 2) {
            const uint32_t zt[PERM_ROWS] = {z0, z1, z2, z3};
            xshared_compose(XD, SH, a, F, wb, wt, di, zt, load4, cc, cx, acc);
            continue;
        }
        Fq fl[PERM_ROWS], fr[PERM_ROWS];
        tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, XD.aop[a], load4, fl);
        tuples_of(XD.apow_mm, XD.gamma_m, XD.m[a], F, XD.bop[a], load4, fr);
        if (XD.kind[a] == SMI_ARG_PERM) {
            uint32_t s[PERM_ROWS];
            if (XD.asel[a] != SMI_ARG_NO_SELECTOR) {
                load4(XD.asel[a], s);
                xargs_select(F, s, fl);
            }
            if (XD.bsel[a] != SMI_ARG_NO_SELECTOR) {
                load4(XD.bsel[a], s);
                xargs_select(F, s, fr);
            }
            args_perm_point<0>(XD.g_m, F, wb, wt, di[0], z0, fl[0], fr[0], cc, cx, acc);
            args_perm_point<1>(XD.g_m, F, wb, wt, di[1], z1, fl[1], fr[1], cc, cx, acc);
            args_perm_point<2>(XD.g_m, F, wb, wt, di[2], z2, fl[2], fr[2], cc, cx, acc);
            args_perm_point<3>(XD.g_m, F, wb, wt, di[3], z3, fl[3], fr[3], cc, cx, acc);
        } else {
            uint32_t sa[PERM_ROWS], mult[PERM_ROWS];
            xlookup_weights(XD, a, F, load4, sa, mult);
            xlookup_compose_point<0>(XD.g_m, F, wb, wt, di[0], z0, fl[0], fr[0], sa[0], mult[0], cc, cx, acc);
            xlookup_compose_point<1>(XD.g_m, F, wb, wt, di[1], z1, fl[1], fr[1], sa[1], mult[1], cc, cx, acc);
            xlookup_compose_point<2>(XD.g_m, F, wb, wt, di[2], z2, fl[2], fr[2], sa[2], mult[2], cc, cx, acc);
            xlookup_compose_point<3>(XD.g_m, F, wb, wt, di[3], z3, fl[3], fr[3], sa[3], mult[3], cc, cx, acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// The reject sentences of the verifier are the argument list's (ARGS_SENTENCES, args_core.h): the checks and their order
// are the same.

// J of an argument: bits 8 .. 15 of kind hold J - 1
inline uint32_t xarg_tuples(const smi_air_xarg &g) { return ((g.kind >> SMI_ARG_TUPLES_SHIFT) & 0xffu) + 1; }
// every argument by the section's rules; W = n_cols, Q = the AIR's periodic columns; the reason names the argument
inline int xargs_validate(const smi_air_xargs *xargs, uint32_t W, uint32_t Q, std::string *why) {
    auto fail = [&](const std::string &s) {
        if (why) *why = s;
        return SMI_ERR_BAD_ARG;
    };
    if (!xargs) return fail("xargs: null argument list");
    if (xargs->count < 1 || xargs->count > SMI_ARGS_MAX) return fail("xargs: count must be in 1 .. SMI_ARGS_MAX (" + std::to_string(SMI_ARGS_MAX) + ")");
    if (!xargs->arg) return fail("xargs: null argument array");
    for (uint32_t a = 0; a < xargs->count; a++) {
        const smi_air_xarg &g = xargs->arg[a];
        const std::string who = "xargs: argument " + std::to_string(a) + ": ";
        auto operand = [&](uint32_t v, const char *what) -> std::string {
            v &= ~SMI_ARG_NEXT_ROW;   // "Argument list: next-row operands": the flag on a this-row variable; nothing else gains from it
            if (v < W || (v >= 2 * W && v < 2 * W + Q)) return "";
            if (v < 2 * W || v < 2 * W + 2 * Q) return std::string(what) + " is a next-row variable: only this-row operands (c < n_cols, or 2 n_cols + j)";
            return std::string(what) + " must be a variable of the AIR (< 2 n_cols + 2 n_periodic)";
        };
        const uint32_t kind = g.kind & 0xffu, J = xarg_tuples(g);   // bits 8 .. 15: J - 1 ("Shared-table lookups")
        if ((g.kind >> 16) || (kind != SMI_ARG_PERM && kind != SMI_ARG_LOOKUP)) return fail(who + "kind must be SMI_ARG_PERM (0) or SMI_ARG_LOOKUP (1)");
        if (kind == SMI_ARG_PERM && J > 1) return fail(who + "a permutation takes no tuple count (bits 8 .. 15 of kind must be 0)");
        if (J > SMI_ARG_MAX_TUPLES) return fail(who + "a shared lookup has at most SMI_ARG_MAX_TUPLES (" + std::to_string(SMI_ARG_MAX_TUPLES) + ") tuples");
        if (g.width < 1 || g.width > SMI_PERM_MAX_WIDTH) return fail(who + "width must be in 1 .. 8");
        if (!g.a_var || !g.b_var) return fail(who + "null operand list");
        if (J > 1 && g.a_sel != SMI_ARG_NO_SELECTOR) return fail(who + "a shared lookup keeps its selectors behind the tuples in a_var: a_sel must be SMI_ARG_NO_SELECTOR");
        for (uint32_t j = 0; j < J * g.width; j++) {
            const std::string e = operand(g.a_var[j], "a_var");
            if (!e.empty()) return fail(who + (J > 1 ? "tuple " + std::to_string(j / g.width) + ": " : "") + e);
        }
        for (uint32_t j = 0; j < g.width; j++) {
            const std::string e = operand(g.b_var[j], "b_var");
            if (!e.empty()) return fail(who + e);
        }
        for (uint32_t j = 0; J > 1 && j < J; j++)
            if (g.a_var[J * g.width + j] != SMI_ARG_NO_SELECTOR) {
                const std::string e = operand(g.a_var[J * g.width + j], "selector");
                if (!e.empty()) return fail(who + "tuple " + std::to_string(j) + ": " + e);
            }
        const uint32_t sel[2] = {g.a_sel, g.b_sel};
        for (int k = 0; k < 2; k++)
            if (sel[k] != SMI_ARG_NO_SELECTOR) {
                const std::string e = operand(sel[k], k ? "b_sel" : "a_sel");
                if (!e.empty()) return fail(who + e);
            }
        if (kind == SMI_ARG_LOOKUP) {
            auto bare = [](uint32_t v) { return v == SMI_ARG_NO_SELECTOR ? v : v & ~SMI_ARG_NEXT_ROW; };   // next(mult_col) is mult_col here
            if (g.mult_col >= W) return fail(who + "mult_col must be < n_cols");
            for (uint32_t j = 0; j < J * g.width; j++)
                if (bare(g.a_var[j]) == g.mult_col) return fail(who + "mult_col must be none of the tuple operands");
            for (uint32_t j = 0; j < g.width; j++)
                if (bare(g.b_var[j]) == g.mult_col) return fail(who + "mult_col must be none of the tuple operands");
            if (bare(g.a_sel) == g.mult_col || bare(g.b_sel) == g.mult_col) return fail(who + "mult_col must be none of the selectors");
            for (uint32_t j = 0; J > 1 && j < J; j++)
                if (bare(g.a_var[J * g.width + j]) == g.mult_col) return fail(who + "mult_col must be none of the selectors");
        }
    }
    return SMI_OK;
}
// "Argument list: next-row operands".  The first next-row operand of the list as "argument a: what", or "" -- who takes no
// such list (the zero-knowledge variants, the helper over a row bound) refuses with xargs_refuse_next's sentence.
inline std::string xargs_first_next(const smi_air_xargs *xargs) {
    for (uint32_t a = 0; a < xargs->count; a++) {
        const smi_air_xarg &g = xargs->arg[a];
        const uint32_t J = xarg_tuples(g);
        auto next = [](uint32_t v) { return v != SMI_ARG_NO_SELECTOR && (v & SMI_ARG_NEXT_ROW); };
        const char *what = nullptr;
        for (uint32_t j = 0; j < J * g.width && !what; j++)
            if (next(g.a_var[j])) what = "a_var";
        for (uint32_t j = 0; j < g.width && !what; j++)
            if (next(g.b_var[j])) what = "b_var";
        for (uint32_t j = 0; J > 1 && j < J && !what; j++)
            if (next(g.a_var[J * g.width + j])) what = "a tuple selector";
        if (!what && next(g.a_sel)) what = "a_sel";
        if (!what && next(g.b_sel)) what = "b_sel";
        if (what) return "argument " + std::to_string(a) + ": " + what;
    }
    return "";
}
inline bool xargs_any_next(const smi_air_xargs *xargs) { return !xargs_first_next(xargs).empty(); }
// a validated list: SMI_OK, or SMI_ERR_BAD_ARG with "<who>: argument a: <what> is a next-row operand: <reason>"
inline int xargs_refuse_next(const smi_air_xargs *xargs, const char *who, const char *reason, std::string *why) {
    const std::string at = xargs_first_next(xargs);
    if (at.empty()) return SMI_OK;
    if (why) *why = std::string(who) + ": " + at + " is a next-row operand: " + reason;
    return SMI_ERR_BAD_ARG;
}
// the same question of the kernels' tables: which instantiation a launch takes
inline bool xargs_dev_any_next(const XArgsDev &XD, const XSharedDev *SH) {
    auto next = [](uint32_t op) { return op != SMI_ARG_NO_SELECTOR && xop_next(op); };
    for (uint32_t a = 0; a < XD.A; a++) {
        bool any = next(XD.asel[a]) || next(XD.bsel[a]);
        for (uint32_t j = 0; j < XD.m[a]; j++) any = any || next(XD.aop[a][j]) || next(XD.bop[a][j]);
        for (uint32_t t = 0; SH && t < SH->J[a]; t++) {
            any = any || next(SH->sel[a][t]);
            for (uint32_t j = 0; j < XD.m[a]; j++) any = any || next(SH->op[a][t][j]);
        }
        if (any) return true;
    }
    return false;
}

// the bound of a shared lookup that needs the trace length: M counts (row, tuple) pairs, up to J n of them in one cell, and
// must stay below p.  (J = 1: n divides p - 1.)
inline int xargs_shared_rows(uint64_t p, const smi_air_xargs *xargs, uint32_t log_n, std::string *why) {
    for (uint32_t a = 0; a < xargs->count; a++) {
        const uint64_t J = xarg_tuples(xargs->arg[a]);
        if (J > 1 && (J << log_n) >= p) {
            if (why) *why = "xargs: argument " + std::to_string(a) + ": J n >= p: the multiplicities of a shared lookup could wrap";
            return SMI_ERR_BAD_ARG;
        }
    }
    return SMI_OK;
}
// the degree argument g contributes: 2 for a permutation without a selector, 3 with one, J + 2 for a lookup; one more under zk
inline uint32_t xarg_degree(const smi_air_xarg &g, bool zk) {
    const bool sel = g.a_sel != SMI_ARG_NO_SELECTOR || g.b_sel != SMI_ARG_NO_SELECTOR;
    return ((g.kind & 0xffu) == SMI_ARG_LOOKUP ? xarg_tuples(g) + 2 : sel ? 3 : 2) + (zk ? 1 : 0);
}

// the periodic columns of air as the column build and the helper read them (no cfg at hand): counts, periods <= n, values
// canonical
inline int xargs_periodic_check(uint64_t p, const smi_air *air, uint32_t log_n, std::string *why) {
    auto fail = [&](int rc, const std::string &s) {
        if (why) *why = s;
        return rc;
    };
    if (!air) return fail(SMI_ERR_BAD_ARG, "xargs: null air");
    if (air->n_periodic > SMI_AIR_MAX_PERIODIC) return fail(SMI_ERR_BAD_ARG, "xargs: n_periodic > SMI_AIR_MAX_PERIODIC");
    if (air->n_periodic && (!air->periodic_log_period || !air->periodic_value)) return fail(SMI_ERR_BAD_ARG, "xargs: null periodic tables");
    size_t at = 0;
    for (uint32_t j = 0; j < air->n_periodic; j++) {
        if (air->periodic_log_period[j] > log_n) return fail(SMI_ERR_BAD_ARG, "xargs: periodic_log_period must be <= log_n");
        for (size_t i = 0; i < (size_t)1 << air->periodic_log_period[j]; i++)
            if (air->periodic_value[at + i] >= p) return fail(SMI_ERR_NON_CANONICAL, "xargs: periodic value >= p");
        at += (size_t)1 << air->periodic_log_period[j];
    }
    return SMI_OK;
}

// smi_air_plan_xargs: the AIR's own plan with d = max(d_air, 2 per permutation without a selector, 3 per permutation with
// one and per lookup)
inline int xargs_plan(uint64_t p, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_xargs *xargs, uint32_t *degree, uint64_t *fri_expansion,
                      std::string *why) {
    uint32_t d = 0;
    const int rc = air_validate(p, cfg, air, &d, nullptr, why);
    if (rc != SMI_OK) return rc;
    const int arc = xargs_validate(xargs, cfg->n_cols, air->n_periodic, why);
    if (arc != SMI_OK) return arc;
    if ((p & 3) != 1) {
        if (why) *why = "xargs: p = 3 (mod 4): the quartic extension does not exist";
        return SMI_ERR_BAD_ARG;
    }
    const int src = xargs_shared_rows(p, xargs, cfg->log_n, why);
    if (src != SMI_OK) return src;
    for (uint32_t a = 0; a < xargs->count; a++) d = std::max(d, xarg_degree(xargs->arg[a], false));
    const uint64_t B = 1ull << cfg->log_blowup;
    uint64_t D = 1;
    while (D < d - 1) D <<= 1;
    const uint64_t E = D > B ? 0 : B / D;
    if (E < 4) {
        if (why) *why = "xargs: 2^log_blowup / D < 4";
        return SMI_ERR_EXPANSION_TOO_SMALL;
    }
    if (degree) *degree = d;
    if (fri_expansion) *fri_expansion = E;
    return SMI_OK;
}

// the kernels' tables of a validated list under alpha = ch[0..3], gamma = ch[4..7].  per: the AIR's periodic plan (its vals
// are what pvals will point at); W = n_cols.  pvals is the caller's to set.
inline void xargs_build(const Fp &F, uint32_t g, const smi_air_xargs *xargs, uint32_t W, const smi_air *air, const AirPeriodic &per, const uint64_t ch[8],
                        XArgsDev *XD) {
    static const uint32_t none[SMI_PERM_MAX_WIDTH] = {0, 0, 0, 0, 0, 0, 0, 0};
    const smi_air_perm widest = {SMI_PERM_MAX_WIDTH, 0, none, none};
    PermDev PD;
    perm_build(F, g, &widest, ch, &PD);   // alpha's powers and gamma as every argument reads them
    *XD = XArgsDev{};
    XD->A = xargs->count;
    XD->g_m = PD.g_m;
    for (uint32_t j = 0; j < SMI_PERM_MAX_WIDTH; j++)
        for (int e = 0; e < 4; e++) XD->apow_mm[j][e] = PD.apow_mm[j][e];
    for (int e = 0; e < 4; e++) XD->gamma_m[e] = PD.gamma_m[e];
    auto code = [&](uint32_t v) { return xop_code(v, W); };
    for (uint32_t a = 0; a < xargs->count; a++) {
        const smi_air_xarg &s = xargs->arg[a];
        XD->kind[a] = s.kind & 0xffu;
        XD->m[a] = s.width;
        XD->mcol[a] = XD->kind[a] == SMI_ARG_LOOKUP ? s.mult_col : 0;
        XD->asel[a] = code(s.a_sel);
        XD->bsel[a] = code(s.b_sel);
        for (uint32_t j = 0; j < s.width; j++) XD->aop[a][j] = code(s.a_var[j]), XD->bop[a][j] = code(s.b_var[j]);
    }
    // the place of column j's raw values in per.vals: the groups hold the columns of one period in the AIR's order
    for (const AirPeriodGroup &gr : per.groups) {
        uint32_t k = 0;
        for (uint32_t j = 0; j < air->n_periodic; j++)
            if (air->periodic_log_period[j] == gr.log_period) {
                XD->plog[j] = gr.log_period;
                XD->pfirst[j] = (uint32_t)(gr.in_off + ((size_t)k++ << gr.log_period));
            }
    }
    XD->pvals = nullptr;
}
// A validated plain list (smi_air_args) in the operand form: the same kind, width and mult_col, its columns as operands, no
// selector.  The plain entry points build their tables from this with xargs_build over an empty AirPeriodic (air = nullptr: a
// plain list has no periodic operand and the AIR's periodic columns are not looked at) and run the kernels below.
struct XArgsOfPlain {
    smi_air_xarg arg[SMI_ARGS_MAX];
    smi_air_xargs list;
    explicit XArgsOfPlain(const smi_air_args *args) : list{args->count, 0, arg} {
        for (uint32_t a = 0; a < args->count; a++) {
            const smi_air_arg &s = args->arg[a];
            arg[a] = smi_air_xarg{s.kind, s.width, s.mult_col, 0, s.a_col, s.b_col, SMI_ARG_NO_SELECTOR, SMI_ARG_NO_SELECTOR};
        }
    }
    XArgsOfPlain(const XArgsOfPlain &) = delete;   // list.arg points into this object
};
// the tuples of a validated list as the shared instantiations read them; -> does the list have a shared lookup at all?
inline bool xshared_build(const smi_air_xargs *xargs, uint32_t W, XSharedDev *SH) {
    auto code = [&](uint32_t v) { return xop_code(v, W); };
    *SH = XSharedDev{};
    bool any = false;
    for (uint32_t a = 0; a < xargs->count; a++) {
        const smi_air_xarg &s = xargs->arg[a];
        const uint32_t J = xarg_tuples(s), m = s.width;
        SH->J[a] = J;
        for (uint32_t j = 0; j < J; j++) {
            SH->sel[a][j] = J > 1 ? code(s.a_var[J * m + j]) : code(s.a_sel);
            for (uint32_t i = 0; i < m; i++) SH->op[a][j][i] = code(s.a_var[j * m + i]);
        }
        any = any || J > 1;
    }
    return any;
}
// operands a shared list reads per row on top of what XArgsDev shows (the byte counts of the profile)
inline double xshared_cols_read(const XArgsDev &XD, const XSharedDev &SH) {
    double cols = 0;
    for (uint32_t a = 0; a < XD.A; a++)
        for (uint32_t j = 0; SH.J[a] > 1 && j < SH.J[a]; j++) cols += (j ? XD.m[a] : 0) + (SH.sel[a][j] != SMI_ARG_NO_SELECTOR);
    return cols;
}
// the periodic plan of air on the trace itself (no extension): what the column build and the helper upload
inline void xargs_periodic_plan(uint32_t p, const smi_air *air, uint32_t log_n, AirPeriodic *per) {
    smi_stark_cfg cfg{};
    cfg.log_n = log_n;
    air_periodic_plan(p, &cfg, air, true, per);
}

// ------------------------------------------------------------------------------------------------ out-of-domain sampling
// include/stark_mi.h, "Out-of-domain sampling with an argument list".
// smi_air_plan_deep_xargs: xargs_plan's checks without its bound on E, d by its rule, then deep_plan's three refusals with
// deep_plan's sentences
inline int deep_xargs_plan(uint64_t p, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_xargs *xargs, uint32_t *degree, uint32_t *segments,
                           std::string *why) {
    auto fail = [&](int code, const std::string &s) {
        if (why) *why = s;
        return code;
    };
    uint32_t d = 0;
    const int rc = air_validate(p, cfg, air, &d, nullptr, why, false, true);
    if (rc != SMI_OK) return rc;
    const int arc = xargs_validate(xargs, cfg->n_cols, air->n_periodic, why);
    if (arc != SMI_OK) return arc;
    if ((p & 3) != 1) return fail(SMI_ERR_BAD_ARG, "xargs: p = 3 (mod 4): the quartic extension does not exist");
    const int src = xargs_shared_rows(p, xargs, cfg->log_n, why);
    if (src != SMI_OK) return src;
    for (uint32_t a = 0; a < xargs->count; a++) d = std::max(d, xarg_degree(xargs->arg[a], false));
    const uint64_t B = 1ull << cfg->log_blowup;
    uint64_t D = 1;
    while (D < (uint64_t)d - 1 && D < (1ull << 32)) D <<= 1;
    if (D > B)
        return fail(SMI_ERR_BAD_ARG, "deep: D > 2^log_blowup: the composition of a degree-" + std::to_string(d) + " constraint has degree >= N and does not fit the evaluation domain");
    if (B < 4) return fail(SMI_ERR_EXPANSION_TOO_SMALL, "deep: 2^log_blowup < 4 (Fri::new's assert on the expansion factor)");
    if (4 * D > 64) return fail(SMI_ERR_BAD_ARG, "deep: 4 D > 64: a row of the segment tree is wider than the leaf hash takes");
    if (degree) *degree = d;
    if (segments) *segments = (uint32_t)D;
    return SMI_OK;
}

// The two auxiliary quotients of argument g at a point z outside F_p, over F_q operands: what XArgAux (verify.hip) computes
// from an opened row at a point of the coset, with u[c] = f_c(z) for a trace operand c, per[j] = pi_j(z) for a periodic
// operand, ca = c_a(z), cb = c_a(z w).  alpha, gamma: the shared challenges; ixt = 1 / (z - tau), izt = 1 / (z^n - tau^n).
// un[c] = f_c(z w) and pern[j] = pi_j(z w): what a next-row operand reads ("Argument list: next-row operands"); a caller
// whose lists have none (the zero-knowledge variant refuses them in its plan) passes nullptr.
inline void xargs_aux_at_z(uint32_t p, uint32_t g, uint32_t W, const smi_air_xarg &arg, const FqH &alpha, const FqH &gamma, const FqH *u, const FqH *per,
                           const FqH *un, const FqH *pern, const FqH &ca, const FqH &cb, const FqH &ixt, const FqH &izt, FqH *bq, FqH *wq) {
    const FqH one = fqh(1 % p);
    auto val = [&](uint32_t v) {
        if (v == SMI_ARG_NO_SELECTOR) return one;
        const bool next = (v & SMI_ARG_NEXT_ROW) != 0;
        v &= ~SMI_ARG_NEXT_ROW;
        return v < W ? (next ? un : u)[v] : (next ? pern : per)[v - 2 * W];
    };
    const uint32_t J = xarg_tuples(arg), m = arg.width;
    if (J > 1) {   // (s' - s) P f_T - Nn f_T + M S_b P over the fold of the tuples
        FqH P = one, Nn = fqh(0), ft = gamma, pw = one;
        for (uint32_t i = 0; i < m; i++) {
            ft = fqh_add(ft, fqh_mul(pw, val(arg.b_var[i]), p, g), p);
            pw = fqh_mul(pw, alpha, p, g);
        }
        for (uint32_t j = 0; j < J; j++) {
            FqH f = gamma;
            pw = one;
            for (uint32_t i = 0; i < m; i++) {
                f = fqh_add(f, fqh_mul(pw, val(arg.a_var[j * m + i]), p, g), p);
                pw = fqh_mul(pw, alpha, p, g);
            }
            Nn = fqh_add(fqh_mul(Nn, f, p, g), fqh_mul(val(arg.a_var[J * m + j]), P, p, g), p);
            P = fqh_mul(P, f, p, g);
        }
        const FqH ms = fqh_mul(u[arg.mult_col], val(arg.b_sel), p, g);
        FqH num = fqh_mul(fqh_sub(cb, ca, p), fqh_mul(P, ft, p, g), p, g);
        num = fqh_add(fqh_sub(num, fqh_mul(Nn, ft, p, g), p), fqh_mul(ms, P, p, g), p);
        *bq = fqh_mul(ca, ixt, p, g);
        *wq = fqh_mul(num, izt, p, g);
        return;
    }
    FqH fl = gamma, fr = gamma, pw = one;
    for (uint32_t j = 0; j < arg.width; j++) {
        fl = fqh_add(fl, fqh_mul(pw, val(arg.a_var[j]), p, g), p);
        fr = fqh_add(fr, fqh_mul(pw, val(arg.b_var[j]), p, g), p);
        pw = fqh_mul(pw, alpha, p, g);
    }
    const FqH sa = val(arg.a_sel), sb = val(arg.b_sel);
    if ((arg.kind & 0xffu) == SMI_ARG_PERM) {   // g = 1 + S (f - 1)
        const FqH gl = fqh_add(one, fqh_mul(sa, fqh_sub(fl, one, p), p, g), p), gr = fqh_add(one, fqh_mul(sb, fqh_sub(fr, one, p), p, g), p);
        *bq = fqh_mul(fqh_sub(ca, one, p), ixt, p, g);
        *wq = fqh_mul(fqh_sub(fqh_mul(cb, gr, p, g), fqh_mul(ca, gl, p, g), p), izt, p, g);
    } else {   // (s' - s) f_L f_T - S_a f_T + M S_b f_L
        const FqH m = fqh_mul(u[arg.mult_col], sb, p, g);
        FqH num = fqh_mul(fqh_sub(cb, ca, p), fqh_mul(fl, fr, p, g), p, g);
        num = fqh_add(fqh_sub(num, fqh_mul(sa, fr, p, g), p), fqh_mul(m, fl, p, g), p);
        *bq = fqh_mul(ca, ixt, p, g);
        *wq = fqh_mul(num, izt, p, g);
    }
}

// Both sides of the extended consistency check: deep_ood_sides over u, v, s of the record, plus the 2 A auxiliary quotients at
// z under the weights W + K + 2 a and W + K + 2 a + 1.  ch: alpha, gamma (8 unreduced); weights: the 4 (W + K + 2 A) unreduced
// challenges; ood: the record's 4 (2 W + 2 A + D) canonical values.
inline void deep_xargs_ood_sides(uint32_t p, uint32_t g, const smi_stark_cfg *cfg, const smi_air *air, const smi_air_xargs *xargs, uint32_t D, uint32_t w_n,
                                 const uint64_t ch[8], const uint64_t *weights, const FqH &z, const uint64_t *ood, FqH *lhs, FqH *rhs) {
    const uint32_t W = cfg->n_cols, K = air->n_constraints, Q = air->n_periodic, A = xargs->count, tau = (uint32_t)cfg->trace_offset;
    const uint64_t n = 1ull << cfg->log_n;
    std::vector<uint64_t> plain(ood, ood + 8 * (size_t)W);   // u, v, s: the record of the plain variant
    plain.insert(plain.end(), ood + 4 * (2 * (size_t)W + 2 * (size_t)A), ood + deep_args_record(W, A, D));
    deep_ood_sides(p, g, cfg, air, D, w_n, weights, z, plain.data(), lhs, rhs);
    std::vector<FqH> u(W), per(Q), un(W), pern(Q);   // at z, and at z w for the next-row operands
    const FqH zw = fqh_scale(z, w_n, p);
    for (uint32_t c = 0; c < W; c++) u[c] = fqh_of(ood + 4 * (size_t)c, p), un[c] = fqh_of(ood + 4 * ((size_t)W + c), p);
    for (uint32_t j = 0, at = 0; j < Q; at += 1u << air->periodic_log_period[j], j++) {
        per[j] = deep_periodic_at(air, j, air->periodic_value + at, cfg->log_n, tau, w_n, z, p, g);
        pern[j] = deep_periodic_at(air, j, air->periodic_value + at, cfg->log_n, tau, w_n, zw, p, g);
    }
    uint32_t al[4], ga[4];
    perm_challenges(p, ch, al, ga);
    const FqH alpha{{al[0], al[1], al[2], al[3]}}, gamma{{ga[0], ga[1], ga[2], ga[3]}};
    const FqH ixt = fqh_inv(fqh_sub(z, fqh(tau % p), p), p, g);
    const FqH izt = fqh_inv(fqh_sub(fqh_pow(z, n, p, g), fqh(host_powmod(tau, n, p)), p), p, g);
    FqH acc = *lhs;
    for (uint32_t a = 0; a < A; a++) {
        FqH bq, wq;
        xargs_aux_at_z(p, g, W, xargs->arg[a], alpha, gamma, u.data(), per.data(), un.data(), pern.data(), fqh_of(ood + 4 * (2 * (size_t)W + a), p),
                       fqh_of(ood + 4 * (2 * (size_t)W + A + a), p), ixt, izt, &bq, &wq);
        const uint64_t *wa = weights + 4 * ((size_t)W + K + 2 * (size_t)a);
        acc = fqh_add(acc, fqh_add(fqh_mul(fqh_of(wa, p), bq, p, g), fqh_mul(fqh_of(wa + 4, p), wq, p, g), p), p);
    }
    *lhs = acc;
}
