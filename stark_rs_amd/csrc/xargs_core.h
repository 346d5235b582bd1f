// xargs_core.h -- the argument list with selectors and periodic members (include/stark_mi.h, "Argument list with selectors
// and periodic members"): args_core.h's layer with operands in place of columns.  An operand is a trace column or a periodic
// column of the AIR; every argument has two optional selectors.  Shared by the HIP kernels (xargs.hip), the verifier
// (verify.hip, host) and the CPU emulator (emu_xargs.cpp), which runs the same lane batching and block split.
//
// Number forms are args_core.h's.  A selector cell is a plain residue S: g = 1 + S (f - 1) is formed in Montgomery form
// (S goes through to_mont once per row), S f_T and M S_b are plain products.  XArgsDev travels as a kernel argument and is
// indexed with the argument number and the tuple member only, both wave-uniform, and so is the kind of an operand: every
// table read stays a scalar load and every branch on it is taken by the whole wave.
#pragma once
#include "args_core.h"
#include "deep_core.h"

#define XOP_PER 0x100u   // operand code: trace column c is c (< 64), periodic column j is XOP_PER | j

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

SMI_HD bool xop_periodic(uint32_t op) { return (op & XOP_PER) != 0; }
// the four values of periodic column j at the rows row0 .. row0 + 3 of the trace: v_j[(row0 + q) mod P_j], word by word --
// with P_j = 1 or 2 the wrap falls inside the lane
SMI_HD void xargs_periodic_rows(const XArgsDev &XD, uint32_t j, uint64_t row0, uint32_t v[PERM_ROWS]) {
    const uint32_t mask = (1u << XD.plog[j]) - 1u;
    const uint32_t *src = XD.pvals + XD.pfirst[j];
#pragma unroll
    for (int q = 0; q < PERM_ROWS; q++) v[q] = src[(uint32_t)(row0 + q) & mask];
}
// one cell of an operand on the trace (the multiplicity helper)
SMI_HD uint32_t xargs_cell(const XArgsDev &XD, const uint32_t *trace, uint64_t n, uint32_t op, uint64_t row) {
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
// One lane of the block launch for argument a: args_lane_column with operands and selectors.  load4(op, v): the four cells
// of operand op at the lane's rows (anything for rows at or above n).  A permutation goes through perm_lane_ratios with
// g_L and g_R in place of f_L and f_R; a lookup through xlookup_lane_deltas.  *key as in args_lane_column.
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

// ------------------------------------------------------------------------------------------------ the multiplicity helper
// lookup_core.h's helper over operands: the hash and the comparison read cells through xargs_cell, an unselected row takes
// no part.  The hash is lookup_hash's function of the values.
SMI_HD uint32_t xlookup_hash(const XArgsDev &XD, const uint32_t *trace, uint64_t n, const uint32_t *ops, uint32_t m, uint64_t row) {
    uint32_t h = 0x9e3779b9u;
    for (uint32_t j = 0; j < m; j++) {
        h ^= xargs_cell(XD, trace, n, ops[j], row);
        h *= 0x85ebca6bu;
        h ^= h >> 15;
    }
    return h;
}
SMI_HD bool xlookup_same(const XArgsDev &XD, const uint32_t *trace, uint64_t n, const uint32_t *aops, uint64_t arow, const uint32_t *bops, uint64_t brow,
                         uint32_t m) {
    for (uint32_t j = 0; j < m; j++)
        if (xargs_cell(XD, trace, n, aops[j], arow) != xargs_cell(XD, trace, n, bops[j], brow)) return false;
    return true;
}
SMI_HD bool xargs_selected(const XArgsDev &XD, const uint32_t *trace, uint64_t n, uint32_t sel, uint64_t row) {
    return sel == SMI_ARG_NO_SELECTOR || xargs_cell(XD, trace, n, sel, row) != 0;
}
// Insert launch, lane t (lookup_insert_lane): a table row with S_b = 0 is not inserted.
template <class Atomics>
SMI_HD bool xlookup_insert_lane(const XArgsDev &XD, uint32_t a, const uint32_t *trace, uint64_t n, uint32_t *tab, uint32_t cap, uint32_t t, Atomics at) {
    if (!xargs_selected(XD, trace, n, XD.bsel[a], t)) return true;
    const uint32_t *bops = XD.bop[a], m = XD.m[a];
    uint32_t slot = xlookup_hash(XD, trace, n, bops, m, t) & (cap - 1);
    for (uint32_t i = 0; i < cap; i++) {
        const uint32_t old = at.cas(tab + slot, LOOKUP_EMPTY, t);
        if (old == LOOKUP_EMPTY) return true;
        if (xlookup_same(XD, trace, n, bops, old, bops, t, m)) {   // a slot keeps its tuple: any occupant it ever had serves
            at.min(tab + slot, t);
            return true;
        }
        slot = (slot + 1) & (cap - 1);
    }
    return false;
}
// Count launch, lane r (lookup_count_lane): 0 counted or not selected, 1 the tuple is in no selected table row, 2 the probe
// ran through the whole table.
template <class Atomics>
SMI_HD int xlookup_count_lane(const XArgsDev &XD, uint32_t a, const uint32_t *trace, uint64_t n, const uint32_t *tab, uint32_t cap, uint32_t r,
                              uint32_t *mult, Atomics at) {
    if (!xargs_selected(XD, trace, n, XD.asel[a], r)) return 0;
    const uint32_t *aops = XD.aop[a], *bops = XD.bop[a], m = XD.m[a];
    uint32_t slot = xlookup_hash(XD, trace, n, aops, m, r) & (cap - 1);
    for (uint32_t i = 0; i < cap; i++) {
        const uint32_t t = tab[slot];
        if (t == LOOKUP_EMPTY) return 1;
        if (xlookup_same(XD, trace, n, bops, t, aops, r, m)) {
            at.add(mult + t, 1u);
            return 0;
        }
        slot = (slot + 1) & (cap - 1);
    }
    return 2;
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

// One lane and trip of the streaming launch: args_compose_points with operands and selectors.  load4(op, v): operand op at
// the four points -- an extended trace column, or the extended periodic table read modulo its length.  Everything else as
// there: 1 / (x_i - tau) and the four entries of 1 / (x^n - tau^n) once per trip, the accumulator in registers across the
// arguments.
template <class Load4, class LoadC>
SMI_HD void xargs_compose_points(const XArgsDev &XD, const Fp &F, const uint64_t *w, uint32_t tau_m, const uint32_t *izt_m, uint32_t B, uint64_t i0,
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
            if (v < W || (v >= 2 * W && v < 2 * W + Q)) return "";
            if (v < 2 * W || v < 2 * W + 2 * Q) return std::string(what) + " is a next-row variable: only this-row operands (c < n_cols, or 2 n_cols + j)";
            return std::string(what) + " must be a variable of the AIR (< 2 n_cols + 2 n_periodic)";
        };
        if (g.kind != SMI_ARG_PERM && g.kind != SMI_ARG_LOOKUP) return fail(who + "kind must be SMI_ARG_PERM (0) or SMI_ARG_LOOKUP (1)");
        if (g.width < 1 || g.width > SMI_PERM_MAX_WIDTH) return fail(who + "width must be in 1 .. 8");
        if (!g.a_var || !g.b_var) return fail(who + "null operand list");
        for (uint32_t j = 0; j < g.width; j++) {
            std::string e = operand(g.a_var[j], "a_var");
            if (e.empty()) e = operand(g.b_var[j], "b_var");
            if (!e.empty()) return fail(who + e);
        }
        const uint32_t sel[2] = {g.a_sel, g.b_sel};
        for (int k = 0; k < 2; k++)
            if (sel[k] != SMI_ARG_NO_SELECTOR) {
                const std::string e = operand(sel[k], k ? "b_sel" : "a_sel");
                if (!e.empty()) return fail(who + e);
            }
        if (g.kind == SMI_ARG_LOOKUP) {
            if (g.mult_col >= W) return fail(who + "mult_col must be < n_cols");
            for (uint32_t j = 0; j < g.width; j++)
                if (g.a_var[j] == g.mult_col || g.b_var[j] == g.mult_col) return fail(who + "mult_col must be none of the tuple operands");
            if (g.a_sel == g.mult_col || g.b_sel == g.mult_col) return fail(who + "mult_col must be none of the selectors");
        }
    }
    return SMI_OK;
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
    for (uint32_t a = 0; a < xargs->count; a++) {
        const smi_air_xarg &g = xargs->arg[a];
        const bool sel = g.a_sel != SMI_ARG_NO_SELECTOR || g.b_sel != SMI_ARG_NO_SELECTOR;
        const uint32_t da = (g.kind == SMI_ARG_LOOKUP || sel) ? 3 : 2;
        if (d < da) d = da;
    }
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
    auto code = [&](uint32_t v) { return v == SMI_ARG_NO_SELECTOR ? v : v < W ? v : (XOP_PER | (v - 2 * W)); };
    for (uint32_t a = 0; a < xargs->count; a++) {
        const smi_air_xarg &s = xargs->arg[a];
        XD->kind[a] = s.kind;
        XD->m[a] = s.width;
        XD->mcol[a] = s.kind == SMI_ARG_LOOKUP ? s.mult_col : 0;
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
    for (uint32_t a = 0; a < xargs->count; a++) {
        const smi_air_xarg &g = xargs->arg[a];
        const bool sel = g.a_sel != SMI_ARG_NO_SELECTOR || g.b_sel != SMI_ARG_NO_SELECTOR;
        const uint32_t da = (g.kind == SMI_ARG_LOOKUP || sel) ? 3 : 2;
        if (d < da) d = da;
    }
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
inline void xargs_aux_at_z(uint32_t p, uint32_t g, uint32_t W, const smi_air_xarg &arg, const FqH &alpha, const FqH &gamma, const FqH *u, const FqH *per,
                           const FqH &ca, const FqH &cb, const FqH &ixt, const FqH &izt, FqH *bq, FqH *wq) {
    const FqH one = fqh(1 % p);
    auto val = [&](uint32_t v) { return v == SMI_ARG_NO_SELECTOR ? one : v < W ? u[v] : per[v - 2 * W]; };
    FqH fl = gamma, fr = gamma, pw = one;
    for (uint32_t j = 0; j < arg.width; j++) {
        fl = fqh_add(fl, fqh_mul(pw, val(arg.a_var[j]), p, g), p);
        fr = fqh_add(fr, fqh_mul(pw, val(arg.b_var[j]), p, g), p);
        pw = fqh_mul(pw, alpha, p, g);
    }
    const FqH sa = val(arg.a_sel), sb = val(arg.b_sel);
    if (arg.kind == SMI_ARG_PERM) {   // g = 1 + S (f - 1)
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
    std::vector<FqH> u(W), per(Q);
    for (uint32_t c = 0; c < W; c++) u[c] = fqh_of(ood + 4 * (size_t)c, p);
    for (uint32_t j = 0, at = 0; j < Q; at += 1u << air->periodic_log_period[j], j++)
        per[j] = deep_periodic_at(air, j, air->periodic_value + at, cfg->log_n, tau, w_n, z, p, g);
    uint32_t al[4], ga[4];
    perm_challenges(p, ch, al, ga);
    const FqH alpha{{al[0], al[1], al[2], al[3]}}, gamma{{ga[0], ga[1], ga[2], ga[3]}};
    const FqH ixt = fqh_inv(fqh_sub(z, fqh(tau % p), p), p, g);
    const FqH izt = fqh_inv(fqh_sub(fqh_pow(z, n, p, g), fqh(host_powmod(tau, n, p)), p), p, g);
    FqH acc = *lhs;
    for (uint32_t a = 0; a < A; a++) {
        FqH bq, wq;
        xargs_aux_at_z(p, g, W, xargs->arg[a], alpha, gamma, u.data(), per.data(), fqh_of(ood + 4 * (2 * (size_t)W + a), p),
                       fqh_of(ood + 4 * (2 * (size_t)W + A + a), p), ixt, izt, &bq, &wq);
        const uint64_t *wa = weights + 4 * ((size_t)W + K + 2 * (size_t)a);
        acc = fqh_add(acc, fqh_add(fqh_mul(fqh_of(wa, p), bq, p, g), fqh_mul(fqh_of(wa + 4, p), wq, p, g), p), p);
    }
    *lhs = acc;
}
