"""The permutation argument, the lookup argument and the argument list at the moduli of tests/test_gpu_boundary_primes.py, where
the range bounds of their F_q code are tight: fq_mul and fq_inv hand ext_mul_prepared's one reduction a sum of four products
next to 4 (p - 1)^2 against p 2^32, and tuples_of, lookup_lane_deltas and the two scans chain fp_add / fp_sub on values that
are canonical only if every step before them was.  Operands on the bounds: the edge values as trace cells, every cell p - 1
where that has a meaning, and the unreduced u64 challenges a transcript can hand over.
References: tests/perm_compose.py, tests/lookup_compose.py, tests/args_compose.py, which take (p, g).  Every comparison is
exact.  Without a GPU the kernels' lane code runs in the CPU emulator; `pytest -m gpu` for the kernels and the verifiers."""
import numpy as np
import pytest

import air_compose as ac
import args_compose as agc
import ext_compose as xc
import lookup_compose as lc
import perm_compose as pm
from test_args_emu import LISTS, SPECS, restated_column, case as args_case, emu as emu_args, emu_columns as emu_args_columns, emu_compose as emu_args_compose  # noqa: F401
from test_gpu_boundary_primes import ADICITY, ALL, GEN, KINDS, LARGE, THREE, U64, engines, operands, u64_set  # noqa: F401  (engines is a fixture)
from test_lookup_emu import emu as emu_lookup, emu_column as emu_lookup_column, emu_compose as emu_lookup_compose, emu_mult, fib_case  # noqa: F401
from test_perm_emu import chall, emu as emu_perm, emu_column as emu_perm_column, emu_compose as emu_perm_compose  # noqa: F401

NO_INVERSE = -1
LB, TAU = 3, 1
R = 1 << 32                                     # the Montgomery radix of the kernels
CH_NAMES = ["random", "u64 set", "2^64 - 1", "p - 1"]
WIDTHS = [1, 2, 8]
CPU_LOGS = [1, 2, 5, 11]
GPU_LOGS = [1, 2, 10, 11]                       # below one lane's four rows (twice), exactly one workgroup, the first with two
EMU_ONLY_LOG = 13
LIST_NAMES = ["PL", "LPL", "EIGHT"]        # of test_args_emu.LISTS
PERM_KINDS = [k for k in KINDS if k != "extreme"]   # a permutation of cells that are all p - 1 says nothing


def challenge_sets(p, seed):
    return [chall(seed), u64_set(p)[1:9], [U64] * 8, [p - 1] * 8]


def column_cases(p, logs, kinds=PERM_KINDS):
    """-> [(log_n, width, kind of cells, index of the challenge set, challenges, seed)]: every log_n x width x kind under each
    of the four challenge sets; the extreme cells (lookups only) at one width per size"""
    out = []
    for log_n in logs:
        for wi, m in enumerate(WIDTHS):
            for kind in kinds:
                if kind == "extreme" and wi != log_n % 3:
                    continue
                seed = 100 * log_n + m
                out += [(log_n, m, kind, c, ch, seed) for c, ch in enumerate(challenge_sets(p, seed))]
    return out


# ---------------------------------------------------------------------------------------------- traces
def perm_trace(o, kind, n, m, p, seed):
    """-> (cols, left, right); "edge": the edge set tiled, column j rolled by j, against the same rows shuffled"""
    if kind == "random":
        return pm.shuffled_copy(n, m, p, seed)
    rng = np.random.default_rng(seed)
    tile = operands(o, "edge", n, p)
    left = np.stack([np.roll(tile, j) for j in range(m)])
    right = left[:, rng.permutation(n)]
    cols = [[int(v) for v in r] for r in left] + [[int(v) for v in r] for r in right] + [[int(v) for v in rng.integers(0, p, n)]]
    return cols, list(range(m)), list(range(m, 2 * m))


def lookup_trace(o, kind, n, m, p, seed):
    """-> (cols, lookup, table, mult_col) with the multiplicities filled by the restatement.  "edge": the looked-up tuples are
    the edge set tiled (column j rolled by j), the table the same rows shuffled -- at most six distinct tuples, each credited
    to its lowest row; "extreme": every looked-up cell is p - 1 and table row n / 3 alone holds that tuple, M = n in one cell"""
    if kind == "random":
        return lc.shaped("range", n, p, seed, m=m)
    rng = np.random.default_rng(seed)
    if kind == "edge":
        tile = operands(o, "edge", n, p)
        look = np.stack([np.roll(tile, j) for j in range(m)])
        tab = look[:, rng.permutation(n)]
    else:
        look = np.full((m, n), p - 1, dtype=np.uint64)
        tab = rng.integers(0, p - 1, (m, n)).astype(np.uint64)
        tab[:, n // 3] = p - 1
    cols = [[int(v) for v in r] for r in look] + [[int(v) for v in r] for r in tab] + [[0] * n] + [[int(v) for v in rng.integers(0, p, n)]]
    M, missing = lc.multiplicities(cols, list(range(m)), list(range(m, 2 * m)))
    assert missing is None and max(M) < p
    cols[2 * m] = M
    return cols, list(range(m)), list(range(m, 2 * m)), 2 * m


def edge_pool(o, n, p, seed, spec):
    """agc.pool's layout over the edge set: mm columns of the tiled set (column j rolled by j), the same as the looked-up
    columns, the same rows shuffled as the table, then every argument's own columns -> (cols, arguments)"""
    rng = np.random.default_rng(seed)
    mm = max(m for _k, m in spec)
    tile = operands(o, "edge", n, p)
    src = np.stack([np.roll(tile, j) for j in range(mm)])
    tab = src[:, rng.permutation(n)]
    cols = [[int(v) for v in r] for r in src] * 2 + [[int(v) for v in r] for r in tab]
    args = []
    for kind, m in spec:
        W = len(cols)
        if kind == "perm":
            order = rng.permutation(n)
            cols += [[int(v) for v in src[j][order]] for j in range(m)]
            args.append(("perm", list(range(m)), list(range(W, W + m))))
        else:
            M, missing = lc.multiplicities(cols, list(range(mm, mm + m)), list(range(2 * mm, 2 * mm + m)))
            assert missing is None and max(M) < p
            cols.append(M)
            args.append(("lookup", list(range(mm, mm + m)), list(range(2 * mm, 2 * mm + m)), W))
    return cols, args


_pools = {}


def pooled(o, kind, log_n, p, name):
    """-> (cols, arguments of the list `name`) over one pool per (kind, size, prime)"""
    key = (kind, log_n, p)
    if key not in _pools:
        n = 1 << log_n
        _pools[key] = agc.pool(n, p, seed=log_n) if kind == "random" else edge_pool(o, n, p, log_n, agc.EIGHT)
    cols, eight = _pools[key]
    return cols, [eight[i] for i in LISTS[name]]


def list_cases(p, logs):
    """-> [(log_n, list, kind, challenges)]: every list x size x kind of cells under two of the four challenge sets -- the
    random and the 2^64 - 1 words for one kind of cells, the u64 set and the p - 1 words for the other, swapping from size
    to size.  So every list meets all four sets at every size, but a kind of cells only two of them: the restatement of
    eight columns is the slow part of these tests, and the lists of one size share it (restated_column)"""
    out = []
    for log_n in logs:
        for name in LIST_NAMES:
            for ki, kind in enumerate(PERM_KINDS):
                sets = challenge_sets(p, 100 * log_n)
                c = (log_n + ki) % 2
                out += [(log_n, name, kind, sets[c]), (log_n, name, kind, sets[c + 2])]
    return out


# ---------------------------------------------------------------------------------------------- without a GPU: the columns
@pytest.mark.parametrize("p", ALL)
def test_the_inputs_of_the_gpu_tests_need_no_other_seed(oracle, p):
    """every case the CPU and the GPU tests run, at every prime of the table and up to 2^13 rows, from the tuple values alone
    (numpy): no zero denominator, and no looked-up tuple the table lacks (lookup_trace and edge_pool assert that where they
    fill the multiplicities).  A case that failed here would get another seed"""
    g = GEN[p]
    logs = sorted(set(CPU_LOGS + GPU_LOGS + [EMU_ONLY_LOG]))

    def zero_in(cols, idx, ch):
        f = pm.tuples_vec(np.array(cols, dtype=np.uint64), idx, ch, p, g)
        return bool(np.any(~np.any(f, axis=0)))

    for log_n, m, kind, c, ch, seed in column_cases(p, logs, KINDS):
        n, what = 1 << log_n, (log_n, m, kind, CH_NAMES[c])
        if kind in PERM_KINDS:
            cols, left, right = perm_trace(oracle, kind, n, m, p, seed)
            assert not zero_in(cols, right, ch), what
        cols, lookup, table, _mc = lookup_trace(oracle, kind, n, m, p, seed)
        assert not zero_in(cols, lookup, ch) and not zero_in(cols, table, ch), what
    for log_n, name, kind, ch in list_cases(p, logs):
        cols, args = pooled(oracle, kind, log_n, p, name)
        for a in args:
            assert not zero_in(cols, a[2], ch) and (agc.is_perm(a) or not zero_in(cols, a[1], ch)), (log_n, name, kind)


@pytest.mark.parametrize("p", ALL)
def test_emu_perm_column_equals_the_restatement(oracle, emu_perm, p):
    g = GEN[p]
    for log_n, m, kind, c, ch, seed in column_cases(p, CPU_LOGS):
        cols, left, right = perm_trace(oracle, kind, 1 << log_n, m, p, seed)
        want, closes, zero = pm.column(cols, left, right, ch, p, g)
        st, z, got_closes, _row = emu_perm_column(emu_perm, cols, left, right, ch, p, g, z_stride=(1 << log_n) + log_n % 3)
        assert zero is None, (log_n, m, kind, CH_NAMES[c])
        assert st == 0 and np.array_equal(z, want), (log_n, m, kind, CH_NAMES[c])
        assert closes and got_closes == 1, (log_n, m, kind, CH_NAMES[c])


@pytest.mark.parametrize("p", ALL)
def test_emu_lookup_multiplicities_and_column_equal_the_restatement(oracle, emu_lookup, p):
    g = GEN[p]
    for log_n, m, kind, c, ch, seed in column_cases(p, CPU_LOGS, KINDS):
        n, what = 1 << log_n, (log_n, m, kind, CH_NAMES[c])
        cols, lookup, table, mult_col = lookup_trace(oracle, kind, n, m, p, seed)
        blank = [list(col) for col in cols]
        blank[mult_col] = [0x5a5a5a5 % p] * n
        st, M, missing = emu_mult(emu_lookup, blank, lookup, table, mult_col, p, g)
        assert st == 0 and missing == U64 and M == cols[mult_col], what
        assert kind != "extreme" or M[n // 3] == n
        want, closes, zero = lc.column(cols, lookup, table, mult_col, ch, p, g)
        st, s, got_closes, _at = emu_lookup_column(emu_lookup, cols, lookup, table, mult_col, ch, p, g, s_stride=n + log_n % 3)
        assert zero is None, what
        assert st == 0 and np.array_equal(s, want), what
        assert closes and got_closes == 1, what


@pytest.mark.parametrize("p", ALL)
def test_emu_args_columns_equal_the_restatement(oracle, emu_args, p):
    g = GEN[p]
    for log_n, name, kind, ch in list_cases(p, CPU_LOGS):
        cols, args = pooled(oracle, kind, log_n, p, name)
        want, closes, zero = agc.columns(cols, args, ch, p, g, column_of=restated_column)
        st, c, got_closes, _key = emu_args_columns(emu_args, cols, args, ch, p, g, c_stride=(1 << log_n) + log_n % 3)
        assert zero is None, (log_n, name, kind)
        assert st == 0 and np.array_equal(c, want), (log_n, name, kind)
        assert all(closes) and got_closes == [True] * len(args), (log_n, name, kind)


# ---------------------------------------------------------------------------------------------- without a GPU: the composition
def weights(p, count, shift=0):
    u = u64_set(p)
    return [u[(shift + 2 * j) % len(u)] for j in range(count)]


def compose_case(o, family, p, log_n):
    """-> (air, cols, aux (4 A, n), arguments as agc tuples, ch): a satisfied AIR beside its argument(s) under the challenges
    u64_set(p)[1:9]; the column(s) come from the restatement"""
    g, n, ch = GEN[p], 1 << log_n, u64_set(p)[1:9]
    if family == "perm":
        air, cols = pm.with_permutation(*ac.make("mixer", n, p), 2, p)
        args = [("perm",) + tuple(air.perm)]
    elif family == "lookup":
        air, cols = fib_case(n, p)
        args = [("lookup",) + tuple(air.lookup_arg)]
    else:
        air, cols, args = args_case(n, p, SPECS["LPL"])
    aux, closes, zero = agc.columns(cols, args, ch, p, g)
    assert zero is None and all(closes)
    return air, cols, aux, args, ch


def restated_composition(o, air, cols, aux, args, ch, wch, p, log_n):
    """-> (extended trace, extended auxiliary columns, main + aux codeword (4, N)) as the existing tests build it"""
    g = GEN[p]
    W, K = len(cols), len(air.constraints)
    lde = np.array(ac.lde(o, cols, p, g, log_n, LB, TAU, g), dtype=np.uint64)
    al = np.array(ac.lde(o, [[int(v) for v in row] for row in aux], p, g, log_n, LB, TAU, g), dtype=np.uint64)
    want = pm.main_codeword(o, air, cols, wch[:4 * (W + K)], p, g, log_n, LB, TAU, g)
    want = (want + agc.aux_terms(o, lde, al, args, ch, wch[4 * (W + K):], p, g, log_n, LB, TAU, g)) % np.uint64(p)
    return lde, al, want


EMU_COMPOSE = {"perm": (emu_perm_compose, "z_stride"), "lookup": (emu_lookup_compose, "s_stride"), "args": (emu_args_compose, "c_stride")}


@pytest.mark.parametrize("family", ["perm", "lookup", "args"])
@pytest.mark.parametrize("p", ALL)
def test_emu_compose_under_unreduced_weights_equals_the_restatement(oracle, emu_perm, emu_lookup, emu_args, p, family):
    """2^6 rows, blowup 8 (2^9 points: within the two-adicity of 12289), weights and challenges from u64_set; the 16-byte
    layout, the odd strides of the 4-byte path, and a grid of one workgroup that makes every lane loop"""
    g, log_n = GEN[p], 6
    N = 1 << (log_n + LB)
    air, cols, aux, args, ch = compose_case(oracle, family, p, log_n)
    wch = weights(p, 4 * (len(cols) + len(air.constraints) + 2 * len(args)), 1)
    lde, al, want = restated_composition(oracle, air, cols, aux, args, ch, wch, p, log_n)
    emu = {"perm": emu_perm, "lookup": emu_lookup, "args": emu_args}[family]
    fn, aux_stride = EMU_COMPOSE[family]
    assert np.array_equal(fn(emu, air, lde, al, ch, wch, p, g, log_n, LB, TAU, g), want)
    assert np.array_equal(fn(emu, air, lde, al, ch, wch, p, g, log_n, LB, TAU, g, stride=N + 1, out_stride=N + 5, **{aux_stride: N + 3}), want)
    assert np.array_equal(fn(emu, air, lde, al, ch, wch, p, g, log_n, LB, TAU, g, force_direct=1, grid=1), want)


def bound_case(family, p, N, aux_kind="top"):
    """-> (air, lde (W, N), aux (4 A, N), arguments, ch) that put ext_mul_prepared's sum on its largest value in the argument's
    own products.  The trace columns are constants, the same two on either side of the argument, and gamma = t - sum_j alpha^j
    v_j with t = (p - 1) 2^-32 in every coordinate, so that every MONTGOMERY coordinate of f_L = f_R (= f_T) is p - 1.  The
    auxiliary column is p - 1 in every coordinate at every point ("top"), or p - 1 and 0 in alternating rows of B points
    ("steps": s(w x) - s(x) = p - 1 in every other row, the factor of f_L f_T in the lookup's transition).  With both factors'
    coordinates p - 1, coordinate 3 of the product -- the one without a factor g -- is the reduction of exactly 4 (p - 1)^2:
      permutation   z(w x) * f_R and z(x) * f_L;
      lookup        f_L * f_T; "steps" adds a first factor of p - 1 in every coordinate to (s(w x) - s(x)) * (f_L f_T).
    The compose kernels work point by point: these inputs are the extension of no trace"""
    from stark_rs_amd.mirror import Air
    g = GEN[p]
    v = [p - 1, p - 2, p - 1, p - 2, p - 1]                                # columns 0, 1 = columns 2, 3; column 4: the multiplicities
    alpha = [c % p for c in u64_set(p)[1:5]]
    apow = pm.alpha_powers(alpha, 2, p, g)
    t = (p - 1) * pow(R, -1, p) % p
    s = pm.tuple_value(v, [2, 3], apow, [0, 0, 0, 0], p)
    gamma = [(t - s[e]) % p for e in range(4)]
    ch = u64_set(p)[1:5] + [gamma[0], gamma[1] + p, gamma[2] + (U64 - gamma[2]) // p * p, gamma[3] + (p << 31)]
    assert all(c < 1 << 64 for c in ch) and pm.alpha_gamma(ch, p) == (alpha, gamma)
    for idx in ([0, 1], [2, 3]):                                           # on Python ints: every Montgomery coordinate is p - 1
        f = pm.tuple_value(v, idx, apow, gamma, p)
        assert [c * R % p for c in f] == [p - 1] * 4
        assert sum((p - 1) * (c * R % p) for c in f) == 4 * (p - 1) ** 2  # coordinate 3 of (p - 1, ..) * f before its reduction
    W = 5 if family != "perm" else 4
    args = {"perm": [("perm", [0, 1], [2, 3])], "lookup": [("lookup", [0, 1], [2, 3], 4)],
            "args": [("perm", [0, 1], [2, 3]), ("lookup", [0, 1], [2, 3], 4)]}[family]
    air = Air(W)
    if family == "perm":
        air.permutation([0, 1], [2, 3])
    elif family == "lookup":
        air.lookup([0, 1], [2, 3], 4)
    else:
        agc.mirror_air(air, args)
    lde = np.stack([np.full(N, v[c], dtype=np.uint64) for c in range(W)])
    if aux_kind == "top":
        aux = np.full((4 * len(args), N), p - 1, dtype=np.uint64)
    else:
        aux = np.tile(np.where((np.arange(N) >> LB) % 2 == 1, p - 1, 0).astype(np.uint64), (4 * len(args), 1))
        ds = (np.roll(aux, -(1 << LB), axis=1) + np.uint64(p) - aux) % np.uint64(p)
        assert np.all(ds[:, :N:2 << LB] == p - 1)
    return air, lde, aux, args, ch


def solve_mod(vectors, rhs, p):
    """-> d with sum_j d_j vectors[j] = rhs (mod p), by elimination, or None where the vectors are dependent"""
    k = len(rhs)
    A = [[vectors[j][i] % p for j in range(k)] + [rhs[i] % p] for i in range(k)]
    for c in range(k):
        piv = next((r for r in range(c, k) if A[r][c]), None)
        if piv is None:
            return None
        A[c], A[piv] = A[piv], A[c]
        inv = pow(A[c][c], -1, p)
        A[c] = [v * inv % p for v in A[c]]
        for r in range(k):
            if r != c and A[r][c]:
                A[r] = [(vr - A[r][c] * vc) % p for vr, vc in zip(A[r], A[c])]
    return [A[i][k] for i in range(k)]


def bound_product_case(family, p, N):
    """-> (air, lde, aux, arguments, ch) for the lookup's widest product, (s(w x) - s(x)) * (f_L f_T): the lookup of width 4
    over constant columns with f_L a chosen unit and f_T = t / f_L, t = (p - 1) 2^-32 in every coordinate, so that every
    Montgomery coordinate of f_L f_T is p - 1.  gamma = f_L - sum_j alpha^j c_j places f_L; the table constants c_j + d_j
    place f_T, with f_T - f_L = sum_j alpha^j d_j solved for d (1, alpha, alpha^2, alpha^3 span F_q).  The auxiliary column is
    p - 1 and 0 in alternating rows of B points: in every other row the first factor is p - 1 in every coordinate too"""
    from stark_rs_amd.mirror import Air
    g = GEN[p]
    alpha = [c % p for c in u64_set(p)[1:5]]
    apow = pm.alpha_powers(alpha, 4, p, g)
    t = (p - 1) * pow(R, -1, p) % p
    fl = [p - 2, 1, (p - 1) // 2, p - 1]
    ft = xc.mul([t] * 4, xc.inv(fl, p, g), p, g)
    d = solve_mod(apow, xc.sub(ft, fl, p), p)
    assert d is not None
    cl = [p - 1, p - 2, 1, (p + 1) // 2]
    v = cl + [(a + b) % p for a, b in zip(cl, d)] + [p - 1]                # lookup columns, table columns, the multiplicities
    gamma = xc.sub(fl, pm.tuple_value(v, [0, 1, 2, 3], apow, [0, 0, 0, 0], p), p)
    ch = u64_set(p)[1:5] + [gamma[0], gamma[1] + p, gamma[2] + (U64 - gamma[2]) // p * p, gamma[3] + (p << 31)]
    assert all(c < 1 << 64 for c in ch) and pm.alpha_gamma(ch, p) == (alpha, gamma)
    assert pm.tuple_value(v, [0, 1, 2, 3], apow, gamma, p) == fl and pm.tuple_value(v, [4, 5, 6, 7], apow, gamma, p) == ft
    lt = xc.mul(fl, ft, p, g)
    assert [c * R % p for c in lt] == [p - 1] * 4                          # on Python ints: every Montgomery coordinate of f_L f_T
    assert sum((p - 1) * (c * R % p) for c in lt) == 4 * (p - 1) ** 2      # coordinate 3 of (p - 1, ..) * (f_L f_T) before its reduction
    args = [("lookup", [0, 1, 2, 3], [4, 5, 6, 7], 8)] + ([("perm", [4, 5, 6, 7], [0, 1, 2, 3])] if family == "args" else [])
    air = Air(9)
    if family == "lookup":
        air.lookup([0, 1, 2, 3], [4, 5, 6, 7], 8)
    else:
        agc.mirror_air(air, args)
    lde = np.stack([np.full(N, c, dtype=np.uint64) for c in v])
    aux = np.tile(np.where((np.arange(N) >> LB) % 2 == 1, p - 1, 0).astype(np.uint64), (4 * len(args), 1))
    return air, lde, aux, args, ch


def bound_cases(family, p, N):
    """-> [(name, air, lde, aux, arguments, ch)]"""
    out = [(kind,) + bound_case(family, p, N, kind) for kind in ("top", "steps")]
    if family != "perm":
        out.append(("product",) + bound_product_case(family, p, N))
    return out


def pointwise_composition(air, lde, aux, args, ch, wch, p, log_n):
    """main + aux for inputs that extend nothing: mirror.Air.compose_at under each weight vector plus agc.aux_terms_at"""
    g = GEN[p]
    W, K, N, B = len(lde), len(air.constraints), lde.shape[1], 1 << LB
    wN = pow(g, (p - 1) // N, p)
    main = np.zeros((4, N), dtype=np.uint64)
    for e in range(4):
        we = xc.weight_vector(wch[:4 * (W + K)], e)
        for i in range(N):
            main[e, i] = air.compose_at(p, log_n, LB, TAU, g, wN, i, [int(x) for x in lde[:, i]], [int(x) for x in lde[:, (i + B) % N]], we)
    idx = np.arange(N)
    return (main + agc.aux_terms_at(idx, lde, aux, np.roll(aux, -B, axis=1), args, ch, wch[4 * (W + K):], p, g, wN, log_n, TAU, g)) % np.uint64(p)


@pytest.mark.parametrize("family", ["perm", "lookup", "args"])
@pytest.mark.parametrize("p", LARGE)
def test_emu_compose_with_every_factor_at_its_bound(emu_perm, emu_lookup, emu_args, p, family):
    g, log_n = GEN[p], 4
    N = 1 << (log_n + LB)
    emu = {"perm": emu_perm, "lookup": emu_lookup, "args": emu_args}[family]
    fn, _ = EMU_COMPOSE[family]
    for aux_kind, air, lde, aux, args, ch in bound_cases(family, p, N):
        for shift in (0, 3):
            wch = weights(p, 4 * (len(lde) + 2 * len(args)), shift) if shift else [p - 1] * (4 * (len(lde) + 2 * len(args)))
            want = pointwise_composition(air, lde, aux, args, ch, wch, p, log_n)
            assert np.array_equal(fn(emu, air, lde, aux, ch, wch, p, g, log_n, LB, TAU, g), want), (aux_kind, shift)


# ---------------------------------------------------------------------------------------------- on the GPU: the columns
gpu = pytest.mark.gpu


def _shapes_4_byte(n):
    """a stride that is no multiple of 4, then a base that is one word off 16 bytes"""
    return (dict(stride=n + 1), dict(stride=n + 4, lead=1))


@gpu
@pytest.mark.parametrize("log_n", GPU_LOGS + [EMU_ONLY_LOG])
@pytest.mark.parametrize("p", LARGE)
def test_dev_perm_column_equals_the_restatement_and_the_emulator(engines, oracle, emu_perm, p, log_n):
    from test_gpu_perm import gpu_column
    eng, g, n = engines[p], GEN[p], 1 << log_n
    for _l, m, kind, c, ch, seed in column_cases(p, [log_n]):
        what = (m, kind, CH_NAMES[c])
        cols, left, right = perm_trace(oracle, kind, n, m, p, seed)
        st, ze, closes_e, _row = emu_perm_column(emu_perm, cols, left, right, ch, p, g)
        if log_n != EMU_ONLY_LOG:
            want, closes, zero = pm.column(cols, left, right, ch, p, g)
            assert zero is None, what
        z, got = gpu_column(eng, cols, left, right, ch)
        assert st == 0 and np.array_equal(z, ze) and got is True and closes_e == 1, what
        if log_n != EMU_ONLY_LOG:
            assert closes and np.array_equal(z, want), what
    for kw in _shapes_4_byte(n):                                          # the last case
        z4, got = gpu_column(eng, cols, left, right, ch, z_stride=kw["stride"], lead=kw.get("lead", 0))
        assert np.array_equal(z4, z) and got, kw


@gpu
@pytest.mark.parametrize("log_n", GPU_LOGS + [EMU_ONLY_LOG])
@pytest.mark.parametrize("p", LARGE)
def test_dev_lookup_multiplicities_and_column_equal_the_restatement_and_the_emulator(engines, oracle, emu_lookup, p, log_n):
    from test_gpu_lookup import gpu_column, gpu_mult
    eng, g, n = engines[p], GEN[p], 1 << log_n
    for _l, m, kind, c, ch, seed in column_cases(p, [log_n], KINDS):
        what = (m, kind, CH_NAMES[c])
        cols, lookup, table, mult_col = lookup_trace(oracle, kind, n, m, p, seed)
        blank = [list(col) for col in cols]
        blank[mult_col] = [0x5a5a5a5 % p] * n
        assert gpu_mult(eng, blank, lookup, table, mult_col) == cols[mult_col], what
        st, se, closes_e, _at = emu_lookup_column(emu_lookup, cols, lookup, table, mult_col, ch, p, g)
        if log_n != EMU_ONLY_LOG:
            want, closes, zero = lc.column(cols, lookup, table, mult_col, ch, p, g)
            assert zero is None, what
        sg, got = gpu_column(eng, cols, lookup, table, mult_col, ch)
        assert st == 0 and np.array_equal(sg, se) and got is True and closes_e == 1, what
        if log_n != EMU_ONLY_LOG:
            assert closes and np.array_equal(sg, want), what
    for kw in _shapes_4_byte(n):                                          # the last case
        s4, got = gpu_column(eng, cols, lookup, table, mult_col, ch, s_stride=kw["stride"], lead=kw.get("lead", 0))
        assert np.array_equal(s4, sg) and got, kw


@gpu
@pytest.mark.parametrize("log_n", GPU_LOGS + [EMU_ONLY_LOG])
@pytest.mark.parametrize("p", LARGE)
def test_dev_args_columns_equal_the_restatement_and_the_emulator(engines, oracle, emu_args, p, log_n):
    from test_gpu_args import gpu_columns
    eng, g, n = engines[p], GEN[p], 1 << log_n
    for _l, name, kind, ch in list_cases(p, [log_n]):
        cols, args = pooled(oracle, kind, log_n, p, name)
        st, ce, closes_e, _key = emu_args_columns(emu_args, cols, args, ch, p, g)
        if log_n != EMU_ONLY_LOG:
            want, closes, zero = agc.columns(cols, args, ch, p, g, column_of=restated_column)
            assert zero is None, (name, kind)
        c, got = gpu_columns(eng, cols, args, ch)
        assert st == 0 and np.array_equal(c, ce) and got == closes_e == [True] * len(args), (name, kind)
        if log_n != EMU_ONLY_LOG:
            assert all(closes) and np.array_equal(c, want), (name, kind)
    for kw in _shapes_4_byte(n):
        c4, got = gpu_columns(eng, cols, args, ch, c_stride=kw["stride"], lead=kw.get("lead", 0))
        assert np.array_equal(c4, c) and all(got), kw


@gpu
@pytest.mark.parametrize("p", LARGE)
def test_a_zero_denominator_names_its_row_and_the_next_call_succeeds(engines, oracle, emu_args, p):
    """through pm.gamma_for_zero at 2^11 rows: the row of the permutation, the row and the side of the lookup, and the
    argument, side and row of the list equal the restatement's; the context stays usable"""
    import stark_rs_amd as s
    from test_gpu_args import gpu_columns
    from test_gpu_lookup import gpu_column as gpu_lookup_column
    from test_gpu_perm import gpu_column as gpu_perm_column
    eng, g, log_n = engines[p], GEN[p], 11
    n = 1 << log_n
    cols, left, right = pm.shuffled_copy(n, 2, p, 8)
    for row in (0, 6, n - 1):
        ch = pm.gamma_for_zero(cols, right, chall(4), row, p, g)
        assert pm.column(cols, left, right, ch, p, g) == (None, None, row)
        with pytest.raises(s.StarkMiError) as ei:
            gpu_perm_column(eng, cols, left, right, ch)
        assert ei.value.status == -1 and "no inverse" in str(ei.value) and f"row {row}:" in str(ei.value)
    z, _closes = gpu_perm_column(eng, cols, left, right, chall(4))
    assert np.array_equal(z, pm.column(cols, left, right, chall(4), p, g)[0])
    for side, row in (("f_L", 0), ("f_T", 6), ("f_L", n - 1)):
        cols, lookup, table, mult_col = lc.shaped("range", n, p, 8)
        idx = lookup if side == "f_L" else table
        cols[idx[0]][row] = lc.absent_value(cols, table)                  # a tuple no other row holds on either side
        ch = lc.gamma_for_zero(cols, idx, chall(4), row, p, g)
        assert lc.column(cols, lookup, table, mult_col, ch, p, g) == (None, None, (row, side))
        with pytest.raises(s.StarkMiError) as ei:
            gpu_lookup_column(eng, cols, lookup, table, mult_col, ch)
        assert ei.value.status == -1 and "no inverse" in str(ei.value) and f"{side} is zero in row {row}:" in str(ei.value)
        sg, _closes = gpu_lookup_column(eng, cols, lookup, table, mult_col, chall(4))
        assert np.array_equal(sg, lc.column(cols, lookup, table, mult_col, chall(4), p, g)[0])
    cols, eight = agc.pool(n, p, seed=log_n)
    args = [eight[0], eight[3], eight[6]]                                 # perm m = 1, lookup m = 1, perm m = 1
    r0, r2 = eight[0][2], eight[6][2]
    for row in (0, 5, n - 1):
        ch = pm.gamma_for_zero(cols, r2, chall(4), row, p, g)             # f_R of argument 2 in `row`, of argument 0 where it holds that value
        key = agc.columns(cols, args, ch, p, g)[2]
        value = cols[r2[0]][row]
        assert key == min(16 * cols[r0[0]].index(value) + 1, 16 * cols[r2[0]].index(value) + 4 + 1)
        assert emu_args_columns(emu_args, cols, args, ch, p, g)[3] == key
        with pytest.raises(s.StarkMiError) as ei:
            gpu_columns(eng, cols, args, ch)
        assert ei.value.status == -1 and f"argument {(key & 15) >> 1}: f_R is zero in row {key >> 4}:" in str(ei.value)
    c, closes = gpu_columns(eng, cols, args, chall(4))
    assert all(closes) and np.array_equal(c, agc.columns(cols, args, chall(4), p, g)[0])


# ---------------------------------------------------------------------------------------------- on the GPU: the composition
AUX_STRIDE = {"perm": "z_stride", "lookup": "s_stride", "args": "c_stride"}


def gpu_compose(eng, family, air, lde, aux, ch, wch, log_n, stride=None, aux_stride=None, out_stride=None, lead=0, main_only=False):
    """-> the (4, N) output of smi_dev_air_compose_perm / _lookup / _args (main_only: of smi_dev_air_compose_ext); the words
    between and behind the output columns stay untouched"""
    from test_gpu_air import Dev
    from test_gpu_ext import _dev_cols
    W, N = lde.shape
    stride, aux_stride, out_stride = (N if v is None else v for v in (stride, aux_stride, out_stride))
    with Dev(eng) as dev:
        lt, d_lde = _dev_cols(lde.astype(np.uint32), stride, lead)
        at, d_aux = _dev_cols(aux.astype(np.uint32), aux_stride, lead)
        ot, d_out = _dev_cols(np.zeros((4, N), dtype=np.uint32), out_stride, lead)
        d_w = dev.upload_u64(wch)
        if main_only:
            eng.dev_air_compose_ext(air, d_lde, W, log_n, LB, d_w, d_out, stride=stride, out_stride=out_stride)
        else:
            getattr(eng, "dev_air_compose_" + family)(air, d_lde, d_aux, W, log_n, LB, ch, d_w, d_out, stride=stride, out_stride=out_stride,
                                                      **{AUX_STRIDE[family]: aux_stride})
        eng.sync()
        host = ot.cpu().numpy().view(np.uint32)[lead:]
    for e in range(4):
        assert np.all(host[e * out_stride + N:(e + 1) * out_stride] == 0x7fffffff)
    return np.stack([host[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)


@gpu
@pytest.mark.parametrize("family", ["perm", "lookup", "args"])
@pytest.mark.parametrize("p", LARGE)
def test_dev_air_compose_under_unreduced_weights_equals_the_restatement(engines, oracle, p, family):
    """2^7 rows, blowup 8: main + aux as tests/test_gpu_perm.py, test_gpu_lookup.py and test_gpu_args.py build it, weights and
    challenges from u64_set; aligned, every stride odd, bases off 16 bytes"""
    eng, log_n = engines[p], 7
    N = 1 << (log_n + LB)
    air, cols, aux, args, ch = compose_case(oracle, family, p, log_n)
    wch = weights(p, 4 * (len(cols) + len(air.constraints) + 2 * len(args)), 1)
    lde, al, want = restated_composition(oracle, air, cols, aux, args, ch, wch, p, log_n)
    for stride, aux_stride, out_stride, lead in ((N, N, N, 0), (N + 1, N + 3, N + 5, 0), (N + 4, N + 4, N + 4, 1)):
        got = gpu_compose(eng, family, air, lde, al, ch, wch, log_n, stride, aux_stride, out_stride, lead)
        assert np.array_equal(got, want), (stride, lead)


@gpu
@pytest.mark.parametrize("family", ["perm", "lookup", "args"])
@pytest.mark.parametrize("p", LARGE)
def test_dev_air_compose_with_every_factor_at_its_bound(engines, p, family):
    """bound_case on the GPU: (compose - compose_ext) mod p is the restated auxiliary part, and compose is compose_at plus it"""
    eng, g, log_n = engines[p], GEN[p], 7
    N, B, P = 1 << (log_n + LB), 1 << LB, np.uint64(p)
    wN = pow(g, (p - 1) // N, p)
    for aux_kind, air, lde, aux, args, ch in bound_cases(family, p, N):
        for shift in (0, 3):
            count = 4 * (len(lde) + 2 * len(args))
            wch = weights(p, count, shift) if shift else [p - 1] * count
            main = gpu_compose(eng, family, air, lde, aux, ch, wch, log_n, main_only=True)
            want = agc.aux_terms_at(np.arange(N), lde, aux, np.roll(aux, -B, axis=1), args, ch, wch[4 * len(lde):], p, g, wN, log_n, TAU, g)
            got = gpu_compose(eng, family, air, lde, aux, ch, wch, log_n)
            assert np.array_equal((got + P - main) % P, want), (aux_kind, shift)
            got = gpu_compose(eng, family, air, lde, aux, ch, wch, log_n, N + 1, N + 3, N + 5)
            assert np.array_equal((got + P - main) % P, want), (aux_kind, shift, "4-byte path")
        if aux_kind == "top":
            assert np.array_equal(got, pointwise_composition(air, lde, aux, args, ch, wch, p, log_n))


# ---------------------------------------------------------------------------------------------- on the GPU: whole proofs
KW = dict(row_leaves=True, ext=True)


def proof_case(family, n, p):
    """-> (air, cols, prove(oracle, E, bits) -> dict, verify(oracle, air, roots, proof, E, bits) -> (ok, class), reason_class,
    width of the second section's rows)"""
    g, log_n = GEN[p], n.bit_length() - 1
    if family == "perm":
        air, cols = pm.with_permutation(*ac.make("fib", n, p), 2, p)
        left, right = air.perm
        return (air, cols, lambda o, E, bits: pm.prove(o, air, left, right, cols, p, g, log_n, LB, 4, TAU, g, E, bits),
                lambda o, roots, proof, E, bits: pm.verify(o, air, left, right, roots, proof, p, g, log_n, LB, 4, TAU, g, E, bits), pm.reason_class, 4)
    if family == "lookup":
        air, cols = fib_case(n, p)
        lk = air.lookup_arg
        return (air, cols, lambda o, E, bits: lc.prove(o, air, lk[0], lk[1], lk[2], cols, p, g, log_n, LB, 4, TAU, g, E, bits),
                lambda o, roots, proof, E, bits: lc.verify(o, air, lk[0], lk[1], lk[2], roots, proof, p, g, log_n, LB, 4, TAU, g, E, bits), lc.reason_class, 4)
    air, cols, args = args_case(n, p, SPECS["LPL"])
    return (air, cols, lambda o, E, bits: agc.prove(o, air, args, cols, p, g, log_n, LB, 4, TAU, g, E, bits),
            lambda o, roots, proof, E, bits: agc.verify(o, air, args, roots, proof, p, g, log_n, LB, 4, TAU, g, E, bits), agc.reason_class, 4 * len(args))


@gpu
@pytest.mark.parametrize("bits", [0, 8])
@pytest.mark.parametrize("family", ["perm", "lookup", "args"])
@pytest.mark.parametrize("p", THREE)
def test_prove_bytes_equal_the_restatement_and_the_verifier_agrees(engines, oracle, p, family, bits):
    """2^8 rows, blowup 8, t = 4: smi_dev_air_prove_perm / _lookup / _args against the restated provers, smi_air_verify_* accepts,
    and a flipped bit in an opened auxiliary value and in root_2 are rejected with the restatement's class of reason"""
    from test_gpu_air import Dev
    eng, log_n, t = engines[p], 8, 4
    air, cols, prove, verify, reason_class, aux_width = proof_case(family, 1 << log_n, p)
    W = len(cols)
    _d, E = eng.air_plan(air, W, log_n, LB)
    with Dev(eng) as dev:
        res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, LB, t, grind_bits=bits, **KW)
    want = prove(oracle, E, bits)
    assert np.all(want["closes"]) and np.all(res["closes"])
    assert res["column_roots"].tobytes() == want["roots"]
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    assert verify(oracle, want["roots"], want["proof"], E, bits) == (True, "")
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert ok, why
    proof, roots = res["proof"], want["roots"]
    rec2, prec = 9 + 8 * aux_width, 9 + 32 * (log_n + LB)
    s2 = len(proof) - 4 * t * (rec2 + prec)                               # the second section: 4 t rows, then 4 t paths
    bad = bytearray(proof)
    bad[s2 + 6 * rec2 + 9 + 8 * (aux_width - 2)] ^= 1                     # a coordinate of the auxiliary column(s) in row 6
    wrong = bytearray(roots)
    wrong[40] ^= 1                                                        # root_2
    for name, bad_proof, bad_roots, cls in (("an auxiliary value", bytes(bad), roots, "path"), ("root_2", proof, bytes(wrong), "fri")):
        assert verify(oracle, bad_roots, bad_proof, E, bits) == (False, cls), name
        ok, why = eng.air_verify(air, bad_proof, [bad_roots[:32], bad_roots[32:]], W, log_n, LB, t, grind_bits=bits, **KW)
        assert not ok and reason_class(why) == cls, (name, why)
