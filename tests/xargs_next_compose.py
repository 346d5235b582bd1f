"""The checker of next-row operands in argument lists (include/stark_mi.h, "Argument list: next-row operands"), restated over
the checkers that exist: tests/xargs_compose.py, tests/shared_lookup_compose.py and tests/deep_args_compose.py, unedited.

A next-row list over the trace T is the plain list over the widened trace T | rot(T), rot(c)[r] = c[(r + 1) mod n]; the same
holds for a periodic column written out in full and rotated.  `restate` rewrites a list that way: the rotated columns join
the AIR as PUBLIC columns of period n behind its own periodic columns (so that the existing provers commit the real trace
alone), operand ("next", c) becomes ("per", Q + c) and ("next", ("per", j)) becomes ("per", Q + W + j).

The route is not the library's.  The restatement extends every rotated column as a polynomial of its own (an inverse and a
forward transform of the n rotated values); the library reads lde[(i + B) mod N], or the extended periodic table B entries
further.  Not a test module: imported by tests/test_xargs_next_*.py and tests/test_gpu_xargs_next.py."""
import copy

import numpy as np

import shared_lookup_compose as sl
import xargs_compose as xg

NEXT_ROW = 0x40000000   # SMI_ARG_NEXT_ROW


def is_next(c):
    return isinstance(c, tuple) and c[0] == "next"


def _map_arg(arg, f):
    """arg with f applied to every member and selector (None stays None)"""
    m = lambda c: None if c is None else f(c)
    if arg[0] == "lookups":
        return ("lookups", [[m(c) for c in t] for t in arg[1]], [m(c) for c in arg[2]], arg[3], [m(s) for s in arg[4]], m(arg[5]))
    k = 3 if arg[0] == "perm" else 4
    head = (arg[0], [m(c) for c in arg[1]], [m(c) for c in arg[2]]) + tuple(arg[3:k])
    return head + tuple(m(s) for s in arg[k:])


def operands(arg):
    """every member and selector of arg that is not None"""
    out = []
    _map_arg(arg, lambda c: out.append(c) or c)
    return out


def has_next(args):
    return any(is_next(c) for g in args for c in operands(g))


def strip(args):
    """the list with every ("next", x) replaced by x: the same shape, degrees and layouts"""
    return [_map_arg(g, lambda c: c[1] if is_next(c) else c) for g in args]


def rot(v):
    return list(v[1:]) + [v[0]]


def restate(air, args, cols, p):
    """-> (air2, args2): air2 is air with W + Q more periodic columns of period n, rot(T) and then the rotated written-out
    periodic columns; args2 names them in place of the next-row operands.  air2 carries no list of its own."""
    W, Q, n = air.n_cols, len(air.periodics), len(cols[0])
    air2 = copy.copy(air)
    air2.args = []
    air2.periodics = [list(v) for v in air.periodics]
    for c in cols:
        air2.periodics.append(rot([int(v) % p for v in c]))
    for v in air.periodics:
        air2.periodics.append(rot([int(v[r % len(v)]) % p for r in range(n)]))

    def f(c):
        if not is_next(c):
            return c
        return ("per", Q + W + c[1][1]) if isinstance(c[1], tuple) else ("per", Q + c[1])
    return air2, [_map_arg(g, f) for g in args]


def widen(cols, air, p):
    """the widened trace of the restatement: T | the periodic columns | rot(T) | the rotated periodic columns"""
    air2, _ = restate(air, [], cols, p)
    return xg.widen(cols, air2, p)


def widened_trace(cols, air, args, p):
    """-> (cols2, args2): the SAME statement as a plain list over a real trace T | rot(T) | rotated periodic columns written out
    (W + W + Q columns), for running the existing GPU path word for word.  The AIR's periodic columns keep their numbers."""
    W, Q, n = air.n_cols, len(air.periodics), len(cols[0])
    cols2 = [list(c) for c in cols] + [rot(list(c)) for c in cols] + [rot([int(v[r % len(v)]) % p for r in range(n)]) for v in air.periodics]

    def f(c):
        if not is_next(c):
            return c
        return 2 * W + c[1][1] if isinstance(c[1], tuple) else W + c[1]
    return cols2, [_map_arg(g, f) for g in args]


def columns(cols, air, args, ch, p, g):
    """the A auxiliary columns by the recurrences over the widened trace -> shared_lookup_compose.columns's triple for a list
    with a shared lookup (zero key (row, a, side)), xargs_compose.columns's otherwise (key 16 row + 2 a + side)"""
    air2, args2 = restate(air, args, cols, p)
    wide = xg.widen(cols, air2, p)
    if any(sl.is_shared(g) for g in args2):
        return sl.columns(wide, args2, ch, p, g, air.n_cols)
    return xg.columns(wide, args2, ch, p, g, air.n_cols)


def multiplicities(cols, air, arg, p):
    """-> (M, missing): xargs_compose.multiplicities (missing: a row) or shared_lookup_compose.multiplicities ((row, tuple))"""
    air2, (arg2,) = restate(air, [arg], cols, p)
    wide = xg.widen(cols, air2, p)
    return (sl if sl.is_shared(arg2) else xg).multiplicities(wide, arg2, air.n_cols)


def aux_terms(o, cols, air, args, cl, ch, wch_aux, p, g, log_n, lb, tau, h):
    """the 2 A auxiliary quotients over the evaluation coset, (4, N): every rotated column extended on its own"""
    import air_compose as ac
    air2, args2 = restate(air, args, cols, p)
    lde_wide = np.asarray(ac.lde(o, xg.widen(cols, air2, p), p, g, log_n, lb, tau, h), dtype=np.uint64)
    mod = sl if any(sl.is_shared(a) for a in args2) else xg
    return mod.aux_terms(o, lde_wide, cl, args2, ch, wch_aux, p, g, log_n, lb, tau, h, air.n_cols)


# ---------------------------------------------------------------------------------------------- lists and traces
def mirror(air, args):
    """a copy of air (its periodic columns and constraints) carrying args, flattened to smi_air_xargs whatever args holds"""
    a = copy.copy(air)
    a.args, a.xargs_always = [], True
    return sl.mirror_air(a, args)


W_SCENE = 10


def scene(n, p, P, seed=11, shared=True):
    """-> (air, cols, args): ONE trace of W_SCENE columns over which the list below holds.  per 0: a public table of period
    min(P, n) with distinct values; per 1: a public 0 / 1 selector of the same period.
      0  perm    [c0] ~ [next c0]                              a column against its own shift: closes for any column
      1  lookup  [next c1] in [per 0], mult c2                 a next-row trace member
      2  lookup  [c3] in [next per 0], mult c4                 a next-row periodic member: the table one row later
      3  perm    [c5] sel next c6 ~ [c7] sel next per 1        next-row selectors, trace and periodic (c6 = per 1 written out)
      4  lookups [next c1], [c3] sel next c6 in [per 0], mult c8     a J = 2 shared lookup (shared=True)
    c0 holds p - 1 at the rows 0, 3, 4 and n - 1; c9 stays zero."""
    from stark_rs_amd.mirror import Air
    rng = np.random.default_rng(seed + n + 64 * P)
    P = min(P, n)
    v0 = [int(v) for v in rng.permutation(4 * n + 8)[:P]]
    s = [int(v) for v in rng.integers(0, 2, P)] if P > 1 else [1]
    if not any(s):
        s[-1] = 1
    air = Air(W_SCENE)
    j0, j1 = air.periodic(v0), air.periodic(s)
    rnd = lambda: [int(v) for v in rng.integers(0, p, n)]
    cols = [[0] * n for _ in range(W_SCENE)]
    cols[0] = rnd()
    for r in (0, 3, 4, n - 1):
        cols[0][r % n] = p - 1
    cols[1] = [v0[int(i)] for i in rng.integers(0, P, n)]
    cols[3] = [v0[int(i)] for i in rng.integers(0, P, n)]
    cols[5], cols[7] = rnd(), rnd()
    cols[6] = [s[r % P] for r in range(n)]
    R = [r for r in range(n) if s[(r + 1) % P]]
    for r, q in zip(R, rng.permutation(len(R))):
        cols[7][r] = cols[5][R[int(q)]]
    args = [("perm", [0], [("next", 0)]),
            ("lookup", [("next", 1)], [("per", j0)], 2),
            ("lookup", [3], [("next", ("per", j0))], 4),
            ("perm", [5], [7], ("next", 6), ("next", ("per", j1)))]
    if shared:
        args.append(("lookups", [[("next", 1)], [3]], [("per", j0)], 8, [None, ("next", 6)], None))
    for arg in args:
        if arg[0] != "perm":
            M, missing = multiplicities(cols, air, arg, p)
            assert missing is None, (arg, missing)
            cols[arg[3]] = M
    return air, cols, args
