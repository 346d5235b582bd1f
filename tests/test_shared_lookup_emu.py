"""CPU: the lane code of shared-table lookups (csrc/xargs_core.h: xshared_fold, xshared_lane_deltas, xshared_compose_point,
xshared_count_lane; csrc/zkargs_core.h) run by the emulator library for every lane, workgroup and argument with the kernels'
lane batching and block split, against the Python restatement (tests/shared_lookup_compose.py), whose shared column is the
sum of J single-lookup columns and whose quotients multiply the denominators out without a fold.  Every comparison is exact,
at both project primes.

log_n 1, 2, 5, 10, 11: under a lane's four rows, one lane, a few lanes, exactly one workgroup, two workgroups; J 2, 3, 4; widths
1, 2, 8; trace and periodic members; selectors none, trace, periodic, mixed.  The zero-knowledge composition needs
k_t = 8 t + 16 < n / 2 and so starts at log_n 6.  Every case asserts first that the restatement meets no zero denominator."""
import copy
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import deep_compose as dc
import ext_compose as xc
import perm_compose as pm
import shared_lookup_compose as sl
import xargs_compose as xg
import zk_args_compose as za
from test_lookup_emu import chall, degree_below

U64_MAX = (1 << 64) - 1
NO_INVERSE, BAD_ARG, LOOKUP_MISSING = -1, -50, -56
SELS = ["none", "trace", "periodic", "mixed"]


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.emu_xargs_columns.argtypes = [u64, u64, C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), vp, u32, u32, vp, vp, u64, C.POINTER(u32), C.POINTER(u64)]
    L.emu_xargs_multiplicities.argtypes = [u64, u64, C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), u32, vp, u32, u32, vp, C.c_int, C.POINTER(u64)]
    L.emu_xargs_multiplicities_rows.argtypes = [u64, u64, C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), u32, vp, u32, u32, u64, vp, C.c_int, C.POINTER(u64)]
    L.emu_air_compose_xargs.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), vp, u64, vp, u64, vp, vp, vp,
                                        u64, C.c_int, u32]
    L.emu_air_compose_zk_xargs.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), vp, u64, vp, u64, vp, vp, vp,
                                           u64, C.c_int, u32]
    return L


def with_args(air, args):
    """a copy of air (its periodic columns and constraints) carrying args"""
    a = copy.copy(air)
    a.args = []
    return sl.mirror_air(a, args)


def flat(air, args, p):
    f = with_args(air, args).flatten(p)
    assert f.xargs is not None and f.args is None
    return f


def emu_columns(emu, air, cols, args, ch, p, g, c_stride=None):
    """-> (status, c (4 A, n) uint64, closes, key)"""
    cols = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    n_cols, n = cols.shape
    A = len(args)
    c_stride = n if c_stride is None else c_stride
    c = np.full(4 * A * c_stride, 0xdeadbeef, dtype=np.uint32)
    cha = np.array(ch, dtype=np.uint64)
    mask, key = C.c_uint32(0), C.c_uint64(0)
    f = flat(air, args, p)
    st = emu.emu_xargs_columns(p, g, C.byref(f), C.byref(f.xargs), cols.ctypes.data, n_cols, n.bit_length() - 1, cha.ctypes.data, c.ctypes.data, c_stride,
                               C.byref(mask), C.byref(key))
    for e in range(4 * A):   # nothing written between the columns
        assert np.all(c[e * c_stride + n:(e + 1) * c_stride] == 0xdeadbeef)
    out = np.stack([c[e * c_stride:e * c_stride + n] for e in range(4 * A)]).astype(np.uint64)
    return st, out, [bool(mask.value >> a & 1) for a in range(A)], key.value


def emu_mult(emu, air, cols, args, a, p, g, order, rows=None):
    cols = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    n_cols, n = cols.shape
    f = flat(air, args, p)
    M = np.full(n + 2, 0xdeadbeef, dtype=np.uint32)
    missing = C.c_uint64(0)
    if rows is None:
        st = emu.emu_xargs_multiplicities(p, g, C.byref(f), C.byref(f.xargs), a, cols.ctypes.data, n_cols, n.bit_length() - 1, M[1:].ctypes.data, order,
                                          C.byref(missing))
    else:
        st = emu.emu_xargs_multiplicities_rows(p, g, C.byref(f), C.byref(f.xargs), a, cols.ctypes.data, n_cols, n.bit_length() - 1, rows, M[1:].ctypes.data,
                                               order, C.byref(missing))
    assert M[0] == M[-1] == 0xdeadbeef
    return st, [int(v) for v in M[1:-1]], missing.value


def emu_compose(emu, air, args, cols_lde, cl, ch, wch, p, g, log_n, lb, tau, h, t=None, stride=None, c_stride=None, out_stride=None, force_direct=0, grid=0):
    """emu_air_compose_xargs, or with t emu_air_compose_zk_xargs"""
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    n_cols, CW = len(cols_lde), len(cl)
    stride, c_stride, out_stride = (N if v is None else v for v in (stride, c_stride, out_stride))
    f = flat(air, args, p)
    cfg = _lib.StarkCfg(log_n, lb, n_cols, 1, tau, h, t or 0, 1)
    lde = np.zeros(n_cols * stride, dtype=np.uint32)
    for c in range(n_cols):
        lde[c * stride:c * stride + N] = cols_lde[c]
    cb = np.zeros(CW * c_stride, dtype=np.uint32)
    for e in range(CW):
        cb[e * c_stride:e * c_stride + N] = cl[e]
    out = np.full(4 * out_stride, 0xdeadbeef, dtype=np.uint32)
    cha, wa = np.array(ch, dtype=np.uint64), np.array(wch, dtype=np.uint64)
    fn = emu.emu_air_compose_xargs if t is None else emu.emu_air_compose_zk_xargs
    st = fn(p, g, C.byref(cfg), C.byref(f), C.byref(f.xargs), lde.ctypes.data, stride, cb.ctypes.data, c_stride, cha.ctypes.data, wa.ctypes.data,
            out.ctypes.data, out_stride, force_direct, grid)
    assert st == 0, st
    for e in range(4):
        assert np.all(out[e * out_stride + N:(e + 1) * out_stride] == 0xdeadbeef)
    return np.stack([out[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)


_scenes = {}


def scene(log_n, p, J, m, sels="none", periodic=True, **kw):
    key = (log_n, p, J, m, sels, periodic, tuple(sorted(kw.items())))
    if key not in _scenes:
        _scenes[key] = sl.scene(1 << log_n, p, J, m, sels, periodic, seed=log_n + 3, **kw)
    return _scenes[key]


def column_cases():
    """(log_n, J, m, sels, periodic): every J x m x sels at one lane and at a few lanes, every log_n with every J and every m"""
    out = [(log_n, J, m, sels, True) for log_n in (2, 5) for J in (2, 3, 4) for m in (1, 2, 8) for sels in SELS]
    out += [(log_n, 2 + (log_n + m) % 3, m, SELS[(log_n + m) % 4], m != 2) for log_n in (1, 10, 11) for m in (1, 2, 8)]
    out += [(1, J, 1, "mixed", False) for J in (2, 3, 4)] + [(11, 4, 2, "mixed", True), (10, 3, 8, "trace", False)]
    return out


COLUMN_CASES = column_cases()


# ---------------------------------------------------------------------------------------------- columns and multiplicities
@pytest.mark.parametrize("log_n,J,m,sels,periodic", COLUMN_CASES)
def test_emu_columns_and_multiplicities_equal_the_restatement(emu, log_n, J, m, sels, periodic):
    p, g = xc.PRIMES[(log_n + J) % 2]
    n = 1 << log_n
    air, cols, args = scene(log_n, p, J, m, sels, periodic)
    W = air.n_cols
    ch = chall(log_n + J)
    wide = xg.widen(cols, air, p)
    M, missing = sl.multiplicities(wide, args[0], W)
    assert missing is None and M == cols[W - 1]
    for order in (0, 1):
        st, got, _ = emu_mult(emu, air, cols, args, 0, p, g, order)
        assert st == 0 and got == M, order
    st, c, closes, _ = emu_columns(emu, air, cols, args, ch, p, g, c_stride=n + (log_n % 3))
    assert st == 0 and closes == [True]
    assert sl.recurrences_hold(c, wide, args, ch, p, g, W) == [(True, True)]
    if log_n <= 5:                                                       # row by row in Python ints: the sum of the J single columns
        want, want_closes, zero = sl.columns(wide, args, ch, p, g, W)
        assert zero is None and want_closes == [True] and np.array_equal(c, want)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_two_tuples_of_a_row_and_the_rows_of_a_wave_hit_one_table_row(emu, p, g):
    """the scene's tuple 1 reads tuple 0's table row on every even row, and the first 64 rows of tuple 0 read table row 0"""
    air, cols, args = scene(10, p, 2, 2)
    W = air.n_cols
    t0, t1 = args[0][1]
    assert all(cols[t0[0]][r] == cols[t1[0]][r] and cols[t0[1]][r] == cols[t1[1]][r] for r in range(0, 1 << 10, 2))
    assert all(cols[t0[i]][r] == cols[t0[i]][0] for r in range(64) for i in range(2)) and cols[W - 1][0] >= 64 + 32
    st, M, _ = emu_mult(emu, air, cols, args, 0, p, g, 0)
    assert st == 0 and M == cols[W - 1] and sum(M) == 2 << 10


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("J", [2, 4])
def test_the_shared_column_is_the_sum_of_the_librarys_single_columns(emu, p, g, J):
    """in the library's own terms: the J single lookups as a list of J arguments over a trace with J multiplicity columns that
    hold the shares -- their columns add up to the shared column, coordinate by coordinate"""
    log_n, m = 5, 2
    n = 1 << log_n
    air, cols, args = scene(log_n, p, J, m, "mixed")
    W = air.n_cols
    ch = chall(9)
    st, c, closes, _ = emu_columns(emu, air, cols, args, ch, p, g)
    assert st == 0 and closes == [True]
    Ms, _ = sl.shares(xg.widen(cols, air, p), args[0], W)
    from stark_rs_amd.mirror import Air
    split = Air(W + J)
    split.periodics = air.periodics
    singles = [one[:3] + (W + j,) + one[4:] for j, one in enumerate(sl.singles(args[0]))]
    st, cs, closes, _ = emu_columns(emu, split, [list(col) for col in cols] + Ms, singles, ch, p, g)
    assert st == 0 and closes == [True] * J
    total = np.zeros((4, n), dtype=np.uint64)
    for j in range(J):
        total = (total + cs[4 * j:4 * j + 4]) % np.uint64(p)
    assert np.array_equal(total, c)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_a_corrupted_multiplicity_cell_clears_closes(emu, p, g):
    air, cols, args = scene(5, p, 3, 2, "trace")
    W = air.n_cols
    bad = [list(c) for c in cols]
    bad[W - 1][7] = (bad[W - 1][7] + 1) % p
    ch = chall(3)
    st, c, closes, _ = emu_columns(emu, air, bad, args, ch, p, g)
    want, want_closes, zero = sl.columns(xg.widen(bad, air, p), args, ch, p, g, W)
    assert st == 0 and zero is None and closes == want_closes == [False] and np.array_equal(c, want)


# ---------------------------------------------------------------------------------------------- refusals
def zero_cases(air, cols, args, W, n, p, g):
    """-> [(challenges, (row, a, side))]: f_j of every tuple and f_T made zero in a first, a middle and the last row"""
    wide = xg.widen(cols, air, p)
    ix = lambda c: W + c[1] if isinstance(c, tuple) else c
    out = []
    for a, arg in enumerate(args):
        if not sl.is_shared(arg):
            continue
        sides = [[ix(c) for c in t] for t in arg[1]] + [[ix(c) for c in arg[2]]]
        val = lambda k, r: tuple(wide[c][r] for c in sides[k])
        for k, side_cols in enumerate(sides):
            # row 0, the last row, and the first row whose value no smaller (row, side) holds: there this side is the one named
            own = next(r for r in range(n) if not any(val(k2, r2) == val(k, r) for r2 in range(r + 1) for k2 in range(len(sides)) if (r2, k2) < (r, k)))
            for row in sorted({0, own, n - 1}):
                ch = pm.gamma_for_zero(wide, side_cols, chall(4 + k), row, p, g)
                _c, _cl, zero = sl.columns(wide, args, ch, p, g, W)
                assert zero is not None and zero <= (row, a, k) and (row != own or zero == (row, a, k)), (zero, row, k)
                out.append((ch, zero))
    return out


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,J", [(2, 2), (5, 4)])
def test_the_smallest_zero_denominator_is_named_by_row_argument_side(emu, p, g, log_n, J):
    """the key of a list with a shared lookup is 64 row + 8 a + side with side = j for f_j and J for f_T; the next call succeeds"""
    n = 1 << log_n
    air, cols, args = scene(log_n, p, J, 1, periodic=False, extra=True)  # a table of n random values: every side has a row of its own
    args = [args[1], args[0], args[2]]                                   # the shared lookup in the middle: a = 1
    W = air.n_cols
    seen = set()
    for ch, zero in zero_cases(air, cols, args, W, n, p, g):
        st, _c, _closes, key = emu_columns(emu, air, cols, args, ch, p, g)
        assert st == NO_INVERSE and key == sl.key_of(zero), (key, zero)
        seen.add(zero[2])
    assert seen == set(range(J + 1))
    st, c, closes, _ = emu_columns(emu, air, cols, args, chall(4), p, g)
    assert st == 0 and all(closes) and np.array_equal(c, sl.columns(xg.widen(cols, air, p), args, chall(4), p, g, W)[0])


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_a_missing_tuple_is_named_by_row_and_tuple_and_an_unselected_one_is_not(emu, p, g):
    air, cols, args = scene(5, p, 3, 2, "trace")
    W = air.n_cols
    arg = args[0]
    sel1 = cols[arg[4][1]]
    off, on = sel1.index(0), [r for r in range(32) if sel1[r]]
    assert cols[arg[1][1][0]][off] >= p - 3                              # an unselected cell holds a value outside the table: not missed
    bad = [list(c) for c in cols]
    on2 = [r for r in range(32) if cols[arg[4][2]][r]]
    for j, r in ((2, on2[-1]), (1, on[1]), (2, on[1]), (1, on[2])):      # the smallest: (on[1], 1)
        bad[arg[1][j][0]][r] = p - 2
    want, first = sl.multiplicities(xg.widen(bad, air, p), arg, W)
    assert first == (on[1], 1)
    for order in (0, 1):
        st, M, missing = emu_mult(emu, air, bad, args, 0, p, g, order)
        assert st == LOOKUP_MISSING and missing == 4 * first[0] + first[1] and M == want


def test_multiplicities_that_could_wrap_are_refused(emu):
    """J n >= p at the smallest modulus the context accepts, 12289 = 3 * 2^12 + 1, with 2^12 rows: J = 3 gives 12288 < p and is
    taken, J = 4 gives 16384 and is refused; 2^11 rows take J = 4"""
    p, g = 12289, 11
    for J, log_n, ok in ((3, 12, True), (4, 12, False), (4, 11, True)):
        air, cols, args = sl.scene(1 << log_n, p, J, 1, periodic=False, seed=1)
        st, _c, closes, _ = emu_columns(emu, air, cols, args, chall(2), p, g)
        assert (st, closes) == ((0, [True]) if ok else (BAD_ARG, [False])), (J, log_n, st)
        st, M, _ = emu_mult(emu, air, cols, args, 0, p, g, 0)
        assert st == (0 if ok else BAD_ARG) and (not ok or M == cols[air.n_cols - 1])


# ---------------------------------------------------------------------------------------------- the compositions
def compose_inputs(oracle, air, cols, args, p, g, log_n, lb, tau, h, per_arg, dair=None, ch=None, weights=None, closed=True):
    """-> (W, K, ch, wch, lde_wide, cl): the restated columns of a trace and their extensions; per_arg weights an argument.
    ch, weights(count): other challenges and weights than the seeded ones; closed: the arguments are to close"""
    W, A = air.n_cols, len(args)
    src = dair or air
    K = len(src.constraints)
    ch = chall(11) if ch is None else ch
    count = 4 * (W + K + per_arg * A)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, count, dtype=np.uint64)] if weights is None else weights(count)
    wide = xg.widen(cols, src, p)
    c, closes, zero = sl.columns(wide, args, ch, p, g, W)
    assert zero is None and (all(closes) or not closed)
    lde_wide = np.asarray(ac.lde(oracle, wide, p, g, log_n, lb, tau, h), dtype=np.uint64)
    cl = np.asarray(ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h), dtype=np.uint64)
    return W, K, ch, wch, lde_wide, cl


COMPOSE_CASES = [(3, 2, 2, 1, "none"), (4, 3, 3, 2, "trace"), (5, 3, 4, 1, "mixed"), (5, 2, 3, 8, "periodic"), (6, 2, 2, 2, "mixed"), (7, 3, 4, 2, "mixed"), (5, 4, 4, 2, "mixed")]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,lb,J,m,sels", COMPOSE_CASES)
def test_emu_air_compose_xargs_equals_the_restatement(oracle, emu, p, g, log_n, lb, J, m, sels):
    """the list holds the shared lookup, a permutation and a single lookup; the composition of an honest trace equals the
    restatement's and, where D n < N, stays below D n -- and with one tuple dropped from the list it does not"""
    tau, h = 1, g
    n, N = 1 << log_n, 1 << (log_n + lb)
    air, cols, args = scene(log_n, p, J, m, sels, extra=True)
    W, K, ch, wch, lde_wide, cl = compose_inputs(oracle, air, cols, args, p, g, log_n, lb, tau, h, 2)
    want = pm.main_codeword(oracle, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
    want = (want + sl.aux_terms(oracle, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W)) % np.uint64(p)
    got = emu_compose(emu, air, args, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, tau, h)
    assert np.array_equal(got, want)
    assert np.array_equal(emu_compose(emu, air, args, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, tau, h, stride=N + 1, c_stride=N + 3, out_stride=N + 5), want)
    assert np.array_equal(emu_compose(emu, air, args, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, tau, h, force_direct=1, grid=1), want)
    D = sl.segments(J + 2)
    if D * n < N:
        assert degree_below(oracle, got, D * n, p, g, log_n + lb, h)
        other = [sl.fewer(args[0], J - 1)] + args[1:]
        assert not degree_below(oracle, emu_compose(emu, air, other, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, tau, h), D * n, p, g, log_n + lb, h)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,lb,J,m,sels", [(6, 2, 2, 1, "mixed"), (6, 3, 4, 2, "mixed"), (7, 3, 3, 8, "trace"), (7, 2, 2, 2, "periodic")])
def test_emu_air_compose_zk_xargs_equals_the_restatement(oracle, emu, p, g, log_n, lb, J, m, sels):
    """the derived AIR's composition plus the 3 A quotients (E_A on the wrapping transition, the closing quotient) over the
    columns of the whole trace: a composition is a function of its inputs point by point"""
    tau, h, t = 1, g, 1
    N = 1 << (log_n + lb)
    air, cols, args = scene(log_n, p, J, m, sels, extra=True)
    dair = za.derived_air(air, log_n, t, p, tau, oracle.ff_prim_nth_root_g(1 << log_n, p, g))
    W, K, ch, wch, lde_wide, cl = compose_inputs(oracle, air, cols, args, p, g, log_n, lb, tau, h, 3, dair)
    want = dc.composition(oracle, dair, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
    want = (want + sl.zk_aux_terms(oracle, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W, t, len(lde_wide) - 1)) % np.uint64(p)
    got = emu_compose(emu, air, args, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, tau, h, t=t)
    assert np.array_equal(got, want)
    assert np.array_equal(emu_compose(emu, air, args, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, tau, h, t=t, stride=N + 1, c_stride=N + 3,
                                      out_stride=N + 5, grid=1), want)
