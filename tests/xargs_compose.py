"""The checker of the argument list with selectors and periodic members (include/stark_mi.h, "Argument list with selectors
and periodic members"), restated in Python over the oracle's primitives and tests/args_compose.py, tests/lookup_compose.py and
tests/perm_compose.py.  An argument is an entry of mirror.Air.args: ("perm", left, right[, left_sel, right_sel]) or ("lookup",
columns, table columns, multiplicity column[, sel, table_sel]); a member or selector is an int (trace column) or ("per", j).

The route is not the library's.  A periodic column is taken for what it is as a polynomial: the trace column of n values
v_j[r mod P_j].  `widen` appends the Q periodic columns to the W trace columns, operand ("per", j) is column W + j of the
widened trace, and its values on the evaluation coset are the ordinary extension of that full column -- where the library
extends P_j values to a table of P_j B and reads it modulo its length.  The columns come from the recurrences cell by cell.
Not a test module: imported by tests/test_xargs_host.py, tests/test_xargs_emu.py and tests/test_gpu_xargs.py."""
import numpy as np

import air_compose as ac
import air_rows as ar
import args_compose as agc
import ext_compose as xc
import lookup_compose as lc
import perm_compose as pm
import pow_compose as pw

ONE, ZERO = [1, 0, 0, 0], [0, 0, 0, 0]


def widen(cols, air, p):
    """-> the (W + Q, n) trace with the periodic columns written out"""
    n = len(cols[0])
    return [list(c) for c in cols] + [[v[r % len(v)] % p for r in range(n)] for v in air.periodics]


def norm(arg, W):
    """-> (is_perm, a indices, b indices, mult column or None, a_sel index or None, b_sel index or None) into the widened trace"""
    ix = lambda c: None if c is None else W + c[1] if isinstance(c, tuple) else c
    k = 3 if arg[0] == "perm" else 4
    sa, sb = (arg[k], arg[k + 1]) if len(arg) > k else (None, None)
    return arg[0] == "perm", [ix(c) for c in arg[1]], [ix(c) for c in arg[2]], (None if arg[0] == "perm" else arg[3]), ix(sa), ix(sb)


def extended(args):
    return any(len(g) > (3 if g[0] == "perm" else 4) or any(isinstance(c, tuple) for c in g[1] + g[2]) for g in args)


# ---------------------------------------------------------------------------------------------- the columns
def column(wide, arg, ch, p, g, W):
    """one argument by its recurrence, row by row -> (column (4, n), closes, None) or (None, None, (row, side))"""
    perm, ai, bi, mc, sa, sb = norm(arg, W)
    n = len(wide[0])
    alpha, gamma = pm.alpha_gamma(ch, p)
    apow = pm.alpha_powers(alpha, len(ai), p, g)
    rows = [[c[r] for c in wide] for r in range(n)]
    fl = [pm.tuple_value(row, ai, apow, gamma, p) for row in rows]
    fr = [pm.tuple_value(row, bi, apow, gamma, p) for row in rows]
    Sa = [1 if sa is None else rows[r][sa] % p for r in range(n)]
    Sb = [1 if sb is None else rows[r][sb] % p for r in range(n)]
    out = np.zeros((4, n), dtype=np.uint64)
    if perm:
        gl = [xc.add(ONE, xc.scale(xc.sub(fl[r], ONE, p), Sa[r], p), p) for r in range(n)]
        gr = [xc.add(ONE, xc.scale(xc.sub(fr[r], ONE, p), Sb[r], p), p) for r in range(n)]
        zeros = [r for r in range(n) if not any(gr[r])]
        if zeros:
            return None, None, (zeros[0], 1)
        z = list(ONE)
        for r in range(n):
            out[:, r] = z
            z = xc.mul(xc.mul(z, gl[r], p, g), xc.inv(gr[r], p, g), p, g)
        return out, z == ONE, None
    zeros = [(r, s) for r in range(n) for s, f in ((0, fl[r]), (1, fr[r])) if not any(f)]
    if zeros:
        return None, None, min(zeros)
    s = list(ZERO)
    for r in range(n):
        out[:, r] = s
        s = xc.add(s, xc.scale(xc.inv(fl[r], p, g), Sa[r], p), p)
        s = xc.sub(s, xc.scale(xc.inv(fr[r], p, g), rows[r][mc] % p * Sb[r] % p, p), p)
    return out, s == ZERO, None


def columns(wide, args, ch, p, g, W):
    """agc.columns over `column`: (c (4 A, n), [closes], None) or (None, None, the smallest key 16 row + 2 a + side)"""
    return agc.columns(wide, args, ch, p, g, column_of=lambda cols, arg, ch_, p_, g_: column(cols, arg, ch_, p_, g_, W))


def _sel_vec(wide, s, p):
    n = np.asarray(wide).shape[1]
    return np.ones(n, dtype=np.uint64) if s is None else np.asarray(wide, dtype=np.uint64)[s] % np.uint64(p)


def _g_vec(f, S, p):
    """1 + S (f - 1) for (4, n) f and (n,) S"""
    P = np.uint64(p)
    out = f * S % P
    out[0] = (out[0] + P + np.uint64(1) - S) % P
    return out


def recurrences_hold(c, wide, args, ch, p, g, W):
    """-> [(holds, closes) of argument a]: the section's recurrences with the denominators multiplied out, vectorised over the
    rows (for traces too long to build row by row).  With every denominator non-zero they determine the column."""
    P = np.uint64(p)
    wide = np.asarray(wide, dtype=np.uint64)
    out = []
    for a, arg in enumerate(args):
        perm, ai, bi, mc, sa, sb = norm(arg, W)
        ca = np.asarray(c[4 * a:4 * a + 4], dtype=np.uint64)
        nxt = np.roll(ca, -1, axis=1)   # the wrap: column n - 1 against the start value
        fl, fr = pm.tuples_vec(wide, ai, ch, p, g), pm.tuples_vec(wide, bi, ch, p, g)
        Sa, Sb = _sel_vec(wide, sa, p), _sel_vec(wide, sb, p)
        if perm:
            first = [int(v) for v in ca[:, 0]] == ONE
            eq = pm.mul_vec(nxt, _g_vec(fr, Sb, p), p, g) == pm.mul_vec(ca, _g_vec(fl, Sa, p), p, g)
        else:
            first = [int(v) for v in ca[:, 0]] == ZERO
            lt = pm.mul_vec(fl, fr, p, g)
            lhs = pm.mul_vec((nxt + P - ca) % P, lt, p, g)
            rhs = (fr * Sa % P + P - fl * (wide[mc] % P * Sb % P) % P) % P
            eq = lhs == rhs
        ok = eq.all(axis=0)
        out.append((bool(first and ok[:-1].all()), bool(ok[-1])))
    return out


# ---------------------------------------------------------------------------------------------- the multiplicities
def multiplicities(wide, arg, W):
    """by a dictionary -> (M as a list of n ints, the smallest selected row whose tuple is in no selected table row or None)"""
    perm, ai, bi, _mc, sa, sb = norm(arg, W)
    assert not perm
    n = len(wide[0])
    where = {}
    for t in range(n - 1, -1, -1):
        if sb is None or wide[sb][t]:
            where[tuple(wide[c][t] for c in bi)] = t   # the lowest row wins
    M, missing = [0] * n, None
    for r in range(n):
        if sa is not None and not wide[sa][r]:
            continue
        t = where.get(tuple(wide[c][r] for c in ai))
        if t is None:
            missing = r if missing is None else missing
        else:
            M[t] += 1
    return M, missing


# ---------------------------------------------------------------------------------------------- the auxiliary quotients
def aux_terms_at(idx, lde_at, c_at, c_next, args, ch, wch_aux, p, g, wN, log_n, tau, h, W):
    """the 2 A auxiliary quotients at the points of idx, as (4, len(idx)).  lde_at: (W + Q, len(idx)), the extension of the
    WIDENED trace at idx; the other arguments as agc.aux_terms_at"""
    P = np.uint64(p)
    lde_at = np.asarray(lde_at, dtype=np.uint64)
    ixt, izt = pm.point_inverses(idx, p, wN, log_n, tau, h)
    total = np.zeros((4, len(idx)), dtype=np.uint64)
    for a, arg in enumerate(args):
        perm, ai, bi, mc, sa, sb = norm(arg, W)
        wb, wt = [int(v) % p for v in wch_aux[8 * a:8 * a + 4]], [int(v) % p for v in wch_aux[8 * a + 4:8 * a + 8]]
        ca, cn = np.asarray(c_at[4 * a:4 * a + 4], dtype=np.uint64), np.asarray(c_next[4 * a:4 * a + 4], dtype=np.uint64)
        fl, fr = pm.tuples_vec(lde_at, ai, ch, p, g), pm.tuples_vec(lde_at, bi, ch, p, g)
        Sa, Sb = _sel_vec(lde_at, sa, p), _sel_vec(lde_at, sb, p)
        if perm:
            tq = (pm.mul_vec(cn, _g_vec(fr, Sb, p), p, g) + P - pm.mul_vec(ca, _g_vec(fl, Sa, p), p, g)) % P * izt % P
            bq = ca.copy()
            bq[0] = (bq[0] + P - np.uint64(1)) % P
            bq = bq * ixt % P
        else:
            num = (pm.mul_vec((cn + P - ca) % P, pm.mul_vec(fl, fr, p, g), p, g) + P - fr * Sa % P + fl * (lde_at[mc] * Sb % P) % P) % P
            tq = num * izt % P
            bq = ca * ixt % P
        total = (total + xc.mul_arr(bq, wb, p, g) + xc.mul_arr(tq, wt, p, g)) % P
    return total


def aux_terms(o, lde_wide, cl, args, ch, wch_aux, p, g, log_n, lb, tau, h, W):
    B, N = 1 << lb, 1 << (log_n + lb)
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cl = np.asarray(cl, dtype=np.uint64)
    return aux_terms_at(np.arange(N), lde_wide, cl, np.roll(cl, -B, axis=1), args, ch, wch_aux, p, g, wN, log_n, tau, h, W)


# ---------------------------------------------------------------------------------------------- plan, prover, verifier
def plan(air, args, lb):
    """-> (d, D, E) of smi_air_plan_xargs"""
    contrib = lambda g: 3 if g[0] == "lookup" or len(g) > 3 else 2
    d = max([air.degree] + [contrib(g) for g in args])
    D = 1
    while D < d - 1:
        D *= 2
    return d, D, (1 << lb) // D


def prove(o, air, args, cols, p, g, log_n, lb, t, tau, h, E, bits, honest=True):
    """agc.prove with the columns and quotients of this module -> dict(roots, proof, top, nonce, closes, ch, wch, c, cw)"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K, A = len(cols), len(air.constraints), len(args)
    wide = widen(cols, air, p)
    lde_wide = ac.lde(o, wide, p, g, log_n, lb, tau, h)
    shown = [np.asarray(c, dtype=np.uint64) for c in lde_wide[:W]]   # the periodic columns are not committed
    nodes1 = o.merkle_new(ar.row_leaves(o, shown))
    root1 = bytes(nodes1[-1])
    tr, ch = pm.challenges(o, root1)
    c, closes, zero = columns(wide, args, ch, p, g, W)
    assert zero is None, zero
    cl = ac.lde(o, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)
    cshown = [np.asarray(col, dtype=np.uint64) for col in cl]
    nodes2 = o.merkle_new(ar.row_leaves(o, cshown))
    root2 = bytes(nodes2[-1])
    tr, wch = pm.weights(o, tr, root2, W + K + 2 * A)
    assert len(tr) == agc.transcript_len(W, K, A)
    cw = pm.main_codeword(o, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h, honest)
    cw = (cw + aux_terms(o, np.asarray(lde_wide, dtype=np.uint64), cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W)) % np.uint64(p)
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    fri, top, nonce = pw.prove(o, cfg_o, cw, g, bytes(tr), bits)
    proof = fri + ar.openings_bytes(o, shown, top, N, B, True, nodes1) + ar.openings_bytes(o, cshown, top, N, B, True, nodes2)
    return dict(roots=root1 + root2, proof=proof, top=top, nonce=nonce, closes=closes, ch=ch, wch=wch, c=c, cw=cw)


def verify(o, air, args, roots, proof, p, g, log_n, lb, t, tau, h, E, bits):
    """agc.verify with the quotients of this module; the periodic operands at the opened points come from the extension of
    the written-out periodic columns -> (accept, reason class)"""
    n, B = 1 << log_n, 1 << lb
    N, log_N = n * B, log_n + lb
    W, K, A = air.n_cols, len(air.constraints), len(args)
    root1, root2 = bytes(roots[:32]), bytes(roots[32:64])
    tr, ch = pm.challenges(o, root1)
    tr, wch = pm.weights(o, tr, root2, W + K + 2 * A)
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    ok, pv, used, top, _why = pw.verify(o, cfg_o, proof, g, bytes(tr), bits)
    if not ok:
        return False, "fri"
    rest = proof[used:]
    if len(rest) != agc.opening_len(W, A, log_N, t):
        return False, "length"
    positions = [i for s in top for i in ar.positions(s, N, B, True)]
    len1 = t * 4 * (9 + 8 * W) + t * 4 * (9 + 32 * log_N)
    for sec, width in ((rest[:len1], W), (rest[len1:], 4 * A)):
        rec, prec, m = 9 + 8 * width, 9 + 32 * log_N, 4 * t
        for q in range(m):
            if sec[q * rec] != 2 or int.from_bytes(sec[q * rec + 1:q * rec + 9], "little") != width:
                return False, "record"
            at = m * rec + q * prec
            if sec[at] != 3 or int.from_bytes(sec[at + 1:at + 9], "little") != log_N:
                return False, "record"
    rows, why = pm._section(o, rest[:len1], W, log_N, positions, root1, p)
    if rows is None:
        return False, why
    crows, why = pm._section(o, rest[len1:], 4 * A, log_N, positions, root2, p)
    if crows is None:
        return False, why
    if any(v >= p for r in rows + crows for v in r):
        return False, "canonical"
    per_lde = ac.lde(o, widen([[0] * n], air, p)[1:], p, g, log_n, lb, tau, h) if air.periodics else []
    for s in range(t):
        for k in range(2):
            i = positions[4 * s + k]
            cur, nxt = rows[4 * s + k], rows[4 * s + k + 2]
            per_cur, per_nxt = [int(c[i]) for c in per_lde], [int(c[(i + B) % N]) for c in per_lde]
            got = [air.compose_at(p, log_n, lb, tau, h, wN, i, cur, nxt, xc.weight_vector(wch[:4 * (W + K)], e), per_cur, per_nxt) for e in range(4)]
            at_i = np.array([[int(v)] for v in list(cur) + per_cur], dtype=np.uint64)
            cc = np.array([[int(v)] for v in crows[4 * s + k]], dtype=np.uint64)
            cn = np.array([[int(v)] for v in crows[4 * s + k + 2]], dtype=np.uint64)
            aux = aux_terms_at([i], at_i, cc, cn, args, ch, wch[4 * (W + K):], p, g, wN, log_n, tau, h, W)
            got = [(got[e] + int(aux[e][0])) % p for e in range(4)]
            if got != [v % p for v in pv[2 * s + k][1]]:
                return False, "composition"
    return True, ""


# ---------------------------------------------------------------------------------------------- lists and traces
def mirror_air(air, args):
    """appends args to a mirror.Air's list"""
    for g in args:
        if g[0] == "perm":
            air.add_permutation(*g[1:])
        else:
            air.add_lookup(*g[1:])
    return air


W_SCENE = 20


def scene(n, p, periods, seed=5, edge=None, A=8):
    """-> (air with three periodic columns and no constraint, cols, args): ONE trace of W_SCENE columns over which the first A
    of the eight arguments below hold, with the multiplicity columns filled by `multiplicities`.  periods = (P0, P1, P2):
      per 0, per 1: the two columns of a public table (row t holds (v0[t mod P0], v1[t mod P1]));  per 2: a public 0 / 1 selector.
    Columns: c0, c5 = the table's two columns at a row of the lane's choice (a row per 2 selects); c14 = c0 where c6 is set,
    a value outside the table elsewhere; c1, c2 free, c3, c4 their rows in another order; c6, c7 trace selectors; c10 = the
    cells of c1 that c6 selects, in another order, in rows that c7 selects; c12 = per 0 written out where per 2 is set;
    c16, c17 = per 1, per 0 written out; c8, c9, c11, c13, c18, c19, c15 multiplicities.
      0  lookup  [c14] in [per 0], sel c6                    width 1, fully periodic table, trace selector
      1  perm    [c1, c2] ~ [c3, c4]                         old style
      2  lookup  [c0, c5] in [per 0, per 1], sel per 2       width 2, fully periodic table, periodic selector
      3  perm    [c1] sel c6 ~ [c10] sel c7                  selectors on both sides, which select different rows
      4  lookup  [c1] in [c3]                                old style
      5  lookup  [c0] in [c12], table_sel per 2              a table selector
      6  lookup  [c0, c5] in [per 0, c16]                    a periodic member at position 0
      7  lookup  [c0, c5] in [c17, per 1], sel c7            a periodic member at the last position
    A = 3 is new, old, new.  edge: None (random cells), "sel0" / "sel1" (the trace selectors all 0 / all 1; with "sel1" per 2
    too), "pm1" (the free cells and one table value are p - 1)."""
    from stark_rs_amd.mirror import Air
    rng = np.random.default_rng(seed)
    P0, P1, P2 = periods
    v0 = [int(v) for v in rng.permutation(4 * n)[:P0]]
    v1 = [int(v) for v in rng.integers(0, p, P1)]
    s2 = [1] * P2 if edge == "sel1" else [int(v) for v in rng.integers(0, 2, P2)]
    if not any(s2):
        s2[int(rng.integers(0, P2))] = 1
    if edge == "pm1":
        v0[0] = v1[-1] = p - 1
    air = Air(W_SCENE)
    j0, j1, j2 = air.periodic(v0), air.periodic(v1), air.periodic(s2)
    free = (lambda: [p - 1] * n) if edge == "pm1" else (lambda: [int(v) for v in rng.integers(0, p, n)])
    bits = {"sel0": lambda: [0] * n, "sel1": lambda: [1] * n}.get(edge, lambda: [int(v) for v in rng.integers(0, 2, n)])
    cols = [[0] * n for _ in range(W_SCENE)]
    good = [r for r in range(n) if s2[r % P2]]
    pick = [good[int(i)] for i in rng.integers(0, len(good), n)]
    cols[0], cols[5] = [v0[r % P0] for r in pick], [v1[r % P1] for r in pick]
    cols[6] = bits()
    cols[14] = [cols[0][r] if cols[6][r] else p - 2 - r % 5 for r in range(n)]
    cols[1], cols[2] = free(), free()
    order = [int(i) for i in rng.permutation(n)]
    cols[3], cols[4] = [cols[1][i] for i in order], [cols[2][i] for i in order]
    chosen = [cols[1][r] for r in range(n) if cols[6][r]]
    chosen = [chosen[int(i)] for i in rng.permutation(len(chosen))]
    cols[10] = free()
    for v, r in zip(chosen, sorted(int(i) for i in rng.permutation(n)[:len(chosen)])):
        cols[10][r], cols[7][r] = v, 1
    cols[12] = [v0[r % P0] if s2[r % P2] else p - 3 for r in range(n)]
    cols[16], cols[17] = [v1[r % P1] for r in range(n)], [v0[r % P0] for r in range(n)]
    args = [("lookup", [14], [("per", j0)], 8, 6, None),
            ("perm", [1, 2], [3, 4]),
            ("lookup", [0, 5], [("per", j0), ("per", j1)], 9, ("per", j2), None),
            ("perm", [1], [10], 6, 7),
            ("lookup", [1], [3], 11),
            ("lookup", [0], [12], 13, None, ("per", j2)),
            ("lookup", [0, 5], [("per", j0), 16], 18),
            ("lookup", [0, 5], [17, ("per", j1)], 19, 7, None)][:A]
    wide = widen(cols, air, p)
    for a, g in enumerate(args):
        if g[0] == "lookup":
            M, missing = multiplicities(wide, g, W_SCENE)
            assert missing is None, (a, missing)
            cols[g[3]] = wide[g[3]] = M
    return air, cols, args
