"""The checker of shared-table lookups (include/stark_mi.h, "Shared-table lookups"), restated in Python over
tests/xargs_compose.py.  An argument is an entry of mirror.Air.args; the new kind is
    ("lookups", [columns_0, .., columns_{J-1}], table columns, multiplicity column, [sel_0, .., sel_{J-1}], table_sel)
with members and selectors as everywhere: an int (trace column), ("per", j), or None for the constant 1.

The route is not the library's, which folds the tuples into one fraction Nn / P per row:
  * the shared column is the coordinate-wise sum mod p of the J columns that xargs_compose.column gives for the J SINGLE lookups
    `singles(arg)`, each over a trace whose multiplicity column holds that tuple's own share of the multiplicities;
  * the shares come from one Python dictionary count per tuple (xargs_compose.multiplicities);
  * the quotients come from the recurrence with the denominators multiplied out term by term -- sum_j S_j prod_{i != j} f_i,
    no fold -- as xargs_compose.recurrences_hold does for the other kinds.
Not a test module: imported by the tests/test_*shared_lookup*.py files."""
import numpy as np

import air_compose as ac
import deep_compose as dc
import ext_compose as xc
import perm_compose as pm
import xargs_compose as xg
import zk_args_compose as za

ZERO = [0, 0, 0, 0]


def is_shared(arg):
    return arg[0] == "lookups"


def singles(arg):
    """the J single lookups of a shared one, all with its multiplicity column"""
    _k, tuples, table, mc, sels, tsel = arg
    return [("lookup", list(t), list(table), mc, s, tsel) for t, s in zip(tuples, sels)]


def fewer(arg, J):
    """the shared lookup cut to its first J tuples (J = 1: the single lookup)"""
    return singles(arg)[0] if J == 1 else ("lookups", arg[1][:J], arg[2], arg[3], arg[4][:J], arg[5])


def mirror_air(air, args):
    """appends args to a mirror.Air's list"""
    for g in args:
        if is_shared(g):
            air.add_lookups(g[1], g[2], g[3], g[4], g[5])
        else:
            xg.mirror_air(air, [g])
    return air


# ---------------------------------------------------------------------------------------------- the multiplicities
def shares(wide, arg, W):
    """-> ([M_j as a list of n ints], the smallest (row, tuple) that is selected and in no selected table row, or None)"""
    out, missing = [], []
    for j, one in enumerate(singles(arg)):
        M, miss = xg.multiplicities(wide, one, W)
        out.append(M)
        if miss is not None:
            missing.append((miss, j))
    return out, (min(missing) if missing else None)


def multiplicities(wide, arg, W):
    """-> (M = the sum of the shares, the smallest missing (row, tuple) or None)"""
    Ms, missing = shares(wide, arg, W)
    return [sum(v) for v in zip(*Ms)], missing


# ---------------------------------------------------------------------------------------------- the columns
def column(wide, arg, ch, p, g, W, Ms=None):
    """one shared lookup -> (column (4, n), None) or (None, (row, side)) with side = j for f_j and J for f_T.  Ms: the shares
    the J single columns are built over; by default those of the dictionary count, and whatever the multiplicity column holds
    beyond their sum goes to tuple 0 (the column is linear in M, so the sum is the column of the trace as it stands)."""
    J, mc = len(arg[1]), arg[3]
    if Ms is None:
        Ms, _missing = shares(wide, arg, W)
        rest = [(int(wide[mc][r]) - sum(M[r] for M in Ms)) % p for r in range(len(wide[0]))]
        Ms = [[(a + b) % p for a, b in zip(Ms[0], rest)]] + Ms[1:]
    total, zeros = np.zeros((4, len(wide[0])), dtype=np.uint64), []
    for j, one in enumerate(singles(arg)):
        w_j = [list(c) for c in wide]
        w_j[mc] = [int(v) % p for v in Ms[j]]
        c, _closes, zero = xg.column(w_j, one, ch, p, g, W)
        if zero is not None:
            rows = [[col[r] for col in w_j] for r in range(len(wide[0]))]
            alpha, gamma = pm.alpha_gamma(ch, p)
            apow = pm.alpha_powers(alpha, len(one[1]), p, g)
            _perm, ai, bi, _mc, _sa, _sb = xg.norm(one, W)
            zeros += [(r, j) for r, row in enumerate(rows) if not any(pm.tuple_value(row, ai, apow, gamma, p))]
            zeros += [(r, J) for r, row in enumerate(rows) if not any(pm.tuple_value(row, bi, apow, gamma, p))]
            continue
        total = (total + c) % np.uint64(p)
    if zeros:
        return None, min(zeros)
    return total, None


def columns(wide, args, ch, p, g, W):
    """the A columns of a list that may hold shared lookups -> (c (4 A, n), [closes], None) or (None, None, (row, a, side)), the
    smallest triple in that order.  closes comes from the multiplied-out recurrence's wrap (recurrences_hold)."""
    n = len(wide[0])
    out, zeros = np.zeros((4 * len(args), n), dtype=np.uint64), []
    for a, arg in enumerate(args):
        if is_shared(arg):
            c, zero = column(wide, arg, ch, p, g, W)
        else:
            c, _closes, zero = xg.column(wide, arg, ch, p, g, W)   # a single lookup: (row, 0) for f_L, (row, 1) for f_T = (row, J)
        if zero is not None:
            zeros.append((zero[0], a, zero[1]))
        else:
            out[4 * a:4 * a + 4] = c
    if zeros:
        return None, None, min(zeros)
    return out, [wraps for _holds, wraps in recurrences_hold(out, wide, args, ch, p, g, W)], None


def key_of(zero):
    """the key the shared instantiation of the block launch reports for (row, a, side)"""
    return 64 * zero[0] + 8 * zero[1] + zero[2]


def _products(fs, p, g):
    """[prod_{i != j} f_i for j], prod_i f_i -- term by term"""
    one = np.zeros_like(fs[0])
    one[0] = 1
    others = []
    for j in range(len(fs)):
        acc = one
        for i, f in enumerate(fs):
            if i != j:
                acc = pm.mul_vec(acc, f, p, g)
        others.append(acc)
    return others, pm.mul_vec(others[0], fs[0], p, g)


def _numerator(vals, arg, ch, p, g, W, ca, cn):
    """(s' - s) P f_T - sum_j S_j prod_{i != j} f_i f_T + M S_b P at the points whose operand values are vals (W + Q, k)"""
    P = np.uint64(p)
    ix = lambda c: W + c[1] if isinstance(c, tuple) else c
    fs = [pm.tuples_vec(vals, [ix(c) for c in t], ch, p, g) for t in arg[1]]
    ft = pm.tuples_vec(vals, [ix(c) for c in arg[2]], ch, p, g)
    others, prod = _products(fs, p, g)
    Nn = np.zeros_like(ft)
    for other, s in zip(others, arg[4]):
        Nn = (Nn + other * xg._sel_vec(vals, None if s is None else ix(s), p) % P) % P
    ms = vals[arg[3]] % P * xg._sel_vec(vals, None if arg[5] is None else ix(arg[5]), p) % P
    lhs = pm.mul_vec((cn + P - ca) % P, pm.mul_vec(prod, ft, p, g), p, g)
    return (lhs + P - pm.mul_vec(Nn, ft, p, g) + prod * ms % P) % P


def recurrences_hold(c, wide, args, ch, p, g, W):
    """xargs_compose.recurrences_hold over a list that may hold shared lookups -> [(holds, closes) of argument a]"""
    wide = np.asarray(wide, dtype=np.uint64)
    out = []
    for a, arg in enumerate(args):
        ca = np.asarray(c[4 * a:4 * a + 4], dtype=np.uint64)
        if not is_shared(arg):
            out += xg.recurrences_hold(ca, wide, [arg], ch, p, g, W)
            continue
        ok = (_numerator(wide, arg, ch, p, g, W, ca, np.roll(ca, -1, axis=1)) == 0).all(axis=0)
        out.append((bool([int(v) for v in ca[:, 0]] == ZERO and ok[:-1].all()), bool(ok[-1])))
    return out


# ---------------------------------------------------------------------------------------------- the auxiliary quotients
def aux_terms_at(idx, lde_at, c_at, c_next, args, ch, wch_aux, p, g, wN, log_n, tau, h, W):
    """xargs_compose.aux_terms_at over a list that may hold shared lookups: the 2 A quotients at the points idx as (4, len(idx))"""
    P = np.uint64(p)
    lde_at = np.asarray(lde_at, dtype=np.uint64)
    ixt, izt = pm.point_inverses(idx, p, wN, log_n, tau, h)
    total = np.zeros((4, len(idx)), dtype=np.uint64)
    for a, arg in enumerate(args):
        ca, cn = np.asarray(c_at[4 * a:4 * a + 4], dtype=np.uint64), np.asarray(c_next[4 * a:4 * a + 4], dtype=np.uint64)
        wa = list(wch_aux[8 * a:8 * a + 8])
        if not is_shared(arg):
            total = (total + xg.aux_terms_at(idx, lde_at, ca, cn, [arg], ch, wa, p, g, wN, log_n, tau, h, W)) % P
            continue
        tq = _numerator(lde_at, arg, ch, p, g, W, ca, cn) * izt % P
        bq = ca * ixt % P
        total = (total + xc.mul_arr(bq, [int(v) % p for v in wa[:4]], p, g) + xc.mul_arr(tq, [int(v) % p for v in wa[4:]], p, g)) % P
    return total


def aux_terms(o, lde_wide, cl, args, ch, wch_aux, p, g, log_n, lb, tau, h, W):
    B, N = 1 << lb, 1 << (log_n + lb)
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cl = np.asarray(cl, dtype=np.uint64)
    return aux_terms_at(np.arange(N), lde_wide, cl, np.roll(cl, -B, axis=1), args, ch, wch_aux, p, g, wN, log_n, tau, h, W)


def zk_aux_terms(o, lde_wide, cl, args, ch, wch_aux, p, g, log_n, lb, tau, h, W, t, ea_index):
    """zk_args_compose.aux_terms over a list that may hold shared lookups: the 3 A quotients under the weights 12 a, 12 a + 4,
    12 a + 8.  lde_wide: the extension of the widened trace of the DERIVED AIR, whose row ea_index is E_A's."""
    P = np.uint64(p)
    n, B, N = 1 << log_n, 1 << lb, 1 << (log_n + lb)
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    lde_wide, cl = np.asarray(lde_wide, dtype=np.uint64), np.asarray(cl, dtype=np.uint64)
    nxt = np.roll(cl, -B, axis=1)
    idx = np.arange(N)
    x = dc.points(o, p, g, log_n, lb, h)
    tna = tau * pow(w, n - za.k_t(t), p) % p
    ict = np.array([pow((int(xi) - tna) % p, p - 2, p) for xi in x], dtype=np.uint64)
    total = np.zeros((4, N), dtype=np.uint64)
    for a, arg in enumerate(args):
        wb, wt, wc = (list(wch_aux[12 * a + 4 * k:12 * a + 4 * k + 4]) for k in range(3))
        ca, cn = cl[4 * a:4 * a + 4], nxt[4 * a:4 * a + 4]
        bq = aux_terms_at(idx, lde_wide, ca, cn, [arg], ch, wb + ZERO, p, g, wN, log_n, tau, h, W)
        wq = aux_terms_at(idx, lde_wide, ca, cn, [arg], ch, ZERO + wt, p, g, wN, log_n, tau, h, W) * lde_wide[ea_index] % P
        num = ca.copy()
        if arg[0] == "perm":
            num[0] = (num[0] + P - np.uint64(1)) % P
        total = (total + bq + wq + xc.mul_arr(num * ict % P, [int(v) % p for v in wc], p, g)) % P
    return total


# ---------------------------------------------------------------------------------------------- the plans
def contribution(arg, zk=False):
    if is_shared(arg):
        return len(arg[1]) + 2 + zk
    return (3 if arg[0] == "lookup" or len(arg) > 3 else 2) + zk


def segments(d):
    D = 1
    while D < d - 1:
        D *= 2
    return D


# ---------------------------------------------------------------------------------------------- lists and traces
def scene(n, p, J, m, sels="none", periodic=True, seed=9, cell=None, rows=None, extra=False):
    """-> (air, cols, args): ONE trace of W = m (J + 1) + 4 columns and a list of one shared lookup of J tuples of width m that
    holds.  Columns 0 .. m - 1: the table (its last member is periodic column 0, of period min(n, 8), when `periodic`); columns
    m (j + 1) ..: tuple j, which reads a table row of the lane's choice -- tuple 1 the SAME row as tuple 0 on every even row, and
    the rows 0 .. min(n, 64) - 1 of tuple 0 all read table row 0, so that the lanes of a whole wave count into one word.
    sels: "none", "trace" (columns W - 4 + j mod 3), "periodic" (periodic column 1 for every tuple), "mixed" (None, trace,
    periodic, trace); an unselected cell holds a value outside the table.  Column W - 1: the multiplicities.
    cell(rng, k) -> k table cells (default: random below p - 4; the values p - 3 .. p - 1 stay outside the table).
    rows: every tuple reads a table row below `rows` and the multiplicities are counted over the rows below it alone (the
    active rows of a zero-knowledge proof).
    extra: four more columns W .. W + 3 and two more arguments BEHIND the shared lookup -- a permutation [W] ~ [W + 1] and a
    single lookup [W + 2] in [W] with the multiplicities in W + 3 -- that hold over the rows below `rows` too."""
    from stark_rs_amd.mirror import Air
    rng = np.random.default_rng(seed + 16 * J + m)
    cell = cell or (lambda rng_, k: [int(v) for v in rng_.integers(0, p - 4, k)])
    W = m * (J + 1) + 4
    rows = n if rows is None else rows
    air = Air(W + (4 if extra else 0))
    Pn = min(n, 8)
    cols = [[0] * n for _ in range(air.n_cols)]
    for i in range(m):
        cols[i] = cell(rng, n)
    table = list(range(m))
    if periodic:
        table[m - 1] = ("per", air.periodic(cell(rng, Pn)))
        cols[m - 1] = [0] * n
    psel = air.periodic([int(v) for v in rng.integers(0, 2, Pn)] if Pn > 1 else [1])
    trow = lambda r, i: air.periodics[table[i][1]][r % Pn] if isinstance(table[i], tuple) else cols[i][r]
    tuples, sel_list, first_pick, sel_cols = [], [], None, {}
    for j in range(J):
        pick = [int(v) for v in rng.integers(0, rows, n)]
        if j == 0:
            pick[:min(n, 64)] = [0] * min(n, 64)
            first_pick = pick
        if j == 1:
            pick = [first_pick[r] if r % 2 == 0 else pick[r] for r in range(n)]
        kind = {"none": None, "trace": "t", "periodic": "p", "mixed": [None, "t", "p", "t"][j]}[sels]
        on, sel = [1] * n, None
        if kind == "t":
            sel = W - 4 + (j + 1) % 3
            if sel not in sel_cols:
                sel_cols[sel] = cols[sel] = [int(v) for v in rng.integers(0, 2, n)]
            on = sel_cols[sel]
        elif kind == "p":
            on, sel = [air.periodics[psel][r % Pn] for r in range(n)], ("per", psel)
        members = [m * (j + 1) + i for i in range(m)]
        for i, c in enumerate(members):
            cols[c] = [trow(pick[r], i) if on[r] else p - 1 - (r + i) % 3 for r in range(n)]
        tuples.append(members)
        sel_list.append(sel)
    args = [("lookups", tuples, table, W - 1, sel_list, None)]
    if extra:
        order = [int(i) for i in rng.permutation(rows)] + list(range(rows, n))
        cols[W] = [int(v) for v in rng.permutation(min(p - 8, 1 << 20))[:n]]
        cols[W + 1] = [cols[W][i] for i in order]
        cols[W + 2] = [cols[W][int(i)] for i in rng.integers(0, rows, n)]
        args += [("perm", [W], [W + 1]), ("lookup", [W + 2], [W], W + 3)]
    head = [c[:rows] for c in xg.widen(cols, air, p)]
    for g in args:
        if g[0] != "perm":
            M, missing = (multiplicities if is_shared(g) else xg.multiplicities)(head, g, air.n_cols)
            assert missing is None, missing
            cols[g[3]] = M + [0] * (n - rows)
    return air, cols, args
