"""CPU: next-row operands in argument lists (include/stark_mi.h, "Argument list: next-row operands") at the level of the lane
code -- csrc/xargs_core.h run by the emulator library (csrc/emu_xargs.cpp) with the kernels' lane batching and block split --
against the restatement of tests/xargs_next_compose.py, which rewrites the list as a plain one over the widened trace
T | rot(T) and hands it to the existing checkers.  Every comparison is exact, at both project primes.

log_n 1, 2, 5: each cell on its own (n < 4), the wrap inside the one lane (n = 4), several lanes; log_n 11 for the column
against its own shift: two workgroups, the last lane of the last one wraps to row 0.  Periods 1, 2 (the wrap inside a lane),
8 and n."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import ext_compose as xc
import perm_compose as pm
import shared_lookup_compose as sl
import xargs_compose as xg
import xargs_next_compose as xn
from test_lookup_emu import chall, degree_below

U64_MAX = (1 << 64) - 1
NO_INVERSE, LOOKUP_MISSING, BAD_ARG = -1, -56, -50
W = xn.W_SCENE
PERIODS = [1, 2, 8, 1 << 20]   # cut to n by the scene


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
    return L


_scenes = {}


def scene(log_n, p, P, shared=True):
    key = (log_n, p, P, shared)
    if key not in _scenes:
        _scenes[key] = xn.scene(1 << log_n, p, P, shared=shared)
    return _scenes[key]


def emu_columns(emu, air, cols, args, ch, p, g, c_stride=None):
    """-> (status, c (4 A, n) uint64, closes, key)"""
    cols = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    n_cols, n = cols.shape
    A = len(args)
    c_stride = n if c_stride is None else c_stride
    c = np.full(4 * A * c_stride, 0xdeadbeef, dtype=np.uint32)
    cha = np.array(ch, dtype=np.uint64)
    mask, key = C.c_uint32(0), C.c_uint64(0)
    f = xn.mirror(air, args).flatten(p)
    st = emu.emu_xargs_columns(p, g, C.byref(f), C.byref(f.xargs), cols.ctypes.data, n_cols, n.bit_length() - 1, cha.ctypes.data, c.ctypes.data, c_stride,
                               C.byref(mask), C.byref(key))
    for e in range(4 * A):   # nothing written between the columns
        assert np.all(c[e * c_stride + n:(e + 1) * c_stride] == 0xdeadbeef)
    out = np.stack([c[e * c_stride:e * c_stride + n] for e in range(4 * A)]).astype(np.uint64)
    return st, out, [bool(mask.value >> a & 1) for a in range(A)], key.value


def emu_mult(emu, air, cols, args, a, p, g, order):
    """-> (status, M, missing)"""
    cols = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    n_cols, n = cols.shape
    f = xn.mirror(air, args).flatten(p)
    M = np.full(n + 2, 0xdeadbeef, dtype=np.uint32)
    missing = C.c_uint64(0)
    st = emu.emu_xargs_multiplicities(p, g, C.byref(f), C.byref(f.xargs), a, cols.ctypes.data, n_cols, n.bit_length() - 1, M[1:].ctypes.data, order,
                                      C.byref(missing))
    assert M[0] == M[-1] == 0xdeadbeef
    return st, [int(v) for v in M[1:-1]], missing.value


def emu_compose(emu, air, args, cols_lde, cl, ch, wch, p, g, log_n, lb, tau, h, stride=None, c_stride=None, out_stride=None, force_direct=0, grid=0):
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    n_cols, CW = len(cols_lde), len(cl)
    stride, c_stride, out_stride = (N if v is None else v for v in (stride, c_stride, out_stride))
    f = xn.mirror(air, args).flatten(p)
    cfg = _lib.StarkCfg(log_n, lb, n_cols, 1, tau, h, 0, 1)
    lde = np.zeros(n_cols * stride, dtype=np.uint32)
    for c in range(n_cols):
        lde[c * stride:c * stride + N] = cols_lde[c]
    cb = np.zeros(CW * c_stride, dtype=np.uint32)
    for e in range(CW):
        cb[e * c_stride:e * c_stride + N] = cl[e]
    out = np.full(4 * out_stride, 0xdeadbeef, dtype=np.uint32)
    cha, wa = np.array(ch, dtype=np.uint64), np.array(wch, dtype=np.uint64)
    st = emu.emu_air_compose_xargs(p, g, C.byref(cfg), C.byref(f), C.byref(f.xargs), lde.ctypes.data, stride, cb.ctypes.data, c_stride, cha.ctypes.data,
                                   wa.ctypes.data, out.ctypes.data, out_stride, force_direct, grid)
    assert st == 0
    for e in range(4):
        assert np.all(out[e * out_stride + N:(e + 1) * out_stride] == 0xdeadbeef)
    return np.stack([out[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)


# ---------------------------------------------------------------------------------------------- columns and multiplicities
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("log_n", [1, 2, 5])
def test_emu_columns_and_multiplicities_equal_the_restatement(emu, p, g, log_n, P):
    """a permutation, two lookups and a J = 2 shared lookup with next-row operands as members and as selectors, trace and
    periodic: the columns word for word, every argument closes, the helper's counts are the dictionary's in either lane order"""
    air, cols, args = scene(log_n, p, P)
    n, ch = 1 << log_n, chall(log_n)
    want, closes, zero = xn.columns(cols, air, args, ch, p, g)
    assert zero is None and all(closes)
    st, c, got, _ = emu_columns(emu, air, cols, args, ch, p, g, c_stride=n + (log_n % 3))
    assert st == 0 and got == [True] * len(args)
    assert np.array_equal(c, want)
    for a, arg in enumerate(args):
        if arg[0] == "perm":
            continue
        M, missing = xn.multiplicities(cols, air, arg, p)
        assert missing is None and M == cols[arg[3]]
        for order in (0, 1):
            st, got_M, _ = emu_mult(emu, air, cols, args, a, p, g, order)
            assert st == 0 and got_M == M, (a, order)
    # the same list with its flags removed is the list it always was
    plain = xn.strip(args)
    want, closes, zero = xn.columns(cols, air, plain, ch, p, g)
    st, c, got, _ = emu_columns(emu, air, cols, plain, ch, p, g)
    assert zero is None and st == 0 and got == closes and np.array_equal(c, want)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", [1, 2, 5, 11])
def test_a_column_is_a_permutation_of_its_own_shift(emu, p, g, log_n):
    """add_permutation([0], [("next", 0)]) closes for a random column; at log_n = 11 row 1023 reads its successor from the
    other workgroup and row 2047 wraps to row 0"""
    from stark_rs_amd.mirror import Air
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    cols = [[int(v) for v in rng.integers(0, p, n)], [int(v) for v in rng.integers(0, p, n)]]
    args = [("perm", [0], [("next", 0)]), ("perm", [0, ("next", 1)], [("next", 0), 1])]   # the second: pairs (c0[r], c1[r+1]) against (c0[r+1], c1[r])
    ch = chall(40 + log_n)
    st, c, closes, _ = emu_columns(emu, Air(2), cols, args, ch, p, g)
    assert st == 0 and closes == [True, n == 2]
    wide = np.array(xn.widen(cols, Air(2), p), dtype=np.uint64)
    _air2, args2 = xn.restate(Air(2), args, cols, p)
    assert xg.recurrences_hold(c, wide, args2, ch, p, g, 2) == [(True, True), (True, n == 2)]
    if log_n <= 5:
        assert np.array_equal(c, xn.columns(cols, Air(2), args, ch, p, g)[0])


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", [2, 5])
def test_zero_denominators_and_missing_rows_name_the_same_row_argument_and_side(emu, p, g, log_n):
    n = 1 << log_n
    air, cols, args = scene(log_n, p, 8, shared=False)
    air2, args2 = xn.restate(air, args, cols, p)
    wide = xg.widen(cols, air2, p)
    for a, side in ((1, 1), (2, 2), (3, 2)):   # f_L of a next-row member, f_T of a next-row periodic member, g_R under a next-row selector
        side_cols = xg.norm(args2[a], W)[side]   # norm -> (perm, a members, b members, ..)
        for row in (0, n - 1):
            if a == 3:
                row = next(r for r in range(n) if wide[xg.norm(args2[3], W)[5]][r])   # a row the right selector selects: g_R = f_R there
            ch = pm.gamma_for_zero(wide, side_cols, chall(4), row, p, g)
            want = xg.columns(wide, args2, ch, p, g, W)[2]
            assert want is not None and want >> 4 <= row
            st, _c, _closes, key = emu_columns(emu, air, cols, args, ch, p, g)
            assert st == NO_INVERSE and key == want
    # a wrong successor: next(c1) at row r is c1[r + 1]; row n - 1 reads row 0
    for at, named in ((7 % n, 7 % n - 1), (0, n - 1)):
        bad = [list(c) for c in cols]
        bad[1][at] = p - 2
        want, first = xn.multiplicities(bad, air, args[1], p)
        assert first == named
        for order in (0, 1):
            st, M, missing = emu_mult(emu, air, bad, args, 1, p, g, order)
            assert st == LOOKUP_MISSING and missing == named and M == want
    # a shared lookup names (row, tuple): 4 row + tuple
    air, cols, args = scene(log_n, p, 8)
    bad = [list(c) for c in cols]
    bad[1][3] = p - 2
    want, first = xn.multiplicities(bad, air, args[4], p)
    assert first == (2, 0)
    st, M, missing = emu_mult(emu, air, bad, args, 4, p, g, 0)
    assert st == LOOKUP_MISSING and missing == 4 * 2 + 0 and M == want


def test_the_helper_over_a_row_bound_refuses(emu):
    p, g = xc.PRIMES[0]
    air, cols, args = scene(5, p, 8)
    arr = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    M, missing = np.zeros(32, dtype=np.uint32), C.c_uint64(0)
    for lst, want in ((args, BAD_ARG), (xn.strip(args), 0)):   # without the flag c1 is still in the table
        f = xn.mirror(air, lst).flatten(p)
        st = emu.emu_xargs_multiplicities_rows(p, g, C.byref(f), C.byref(f.xargs), 1, arr.ctypes.data, W, 5, 32, M.ctypes.data, 0, C.byref(missing))
        assert st == want


# ---------------------------------------------------------------------------------------------- the composition
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,lb,P", [(1, 2, 2), (2, 2, 1), (3, 2, 2), (5, 3, 8), (7, 2, 1 << 20)])
def test_emu_air_compose_xargs_equals_the_restatement(oracle, emu, p, g, log_n, lb, P):
    """f_c(w x) is read as lde[c][(i + B) mod N] and pi_j(w x) B entries further in the extended table; the restatement
    extends the rotated columns on their own.  The composition stays below its degree bound; with the flags removed it does not"""
    tau, h = 1, g
    n, N = 1 << log_n, 1 << (log_n + lb)
    air, cols, args = scene(log_n, p, P)
    A = len(args)
    D = sl.segments(max(sl.contribution(a) for a in args))
    ch = chall(11)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + 2 * A), dtype=np.uint64)]
    c, closes, zero = xn.columns(cols, air, args, ch, p, g)
    assert zero is None and all(closes)
    lde = np.asarray(ac.lde(oracle, cols, p, g, log_n, lb, tau, h), dtype=np.uint64)
    cl = ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)
    want = pm.main_codeword(oracle, air, cols, wch[:4 * W], p, g, log_n, lb, tau, h)
    want = (want + xn.aux_terms(oracle, cols, air, args, cl, ch, wch[4 * W:], p, g, log_n, lb, tau, h)) % np.uint64(p)
    got = emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, lb, tau, h)
    assert np.array_equal(got, want)
    assert degree_below(oracle, got, D * n, p, g, log_n + lb, h)
    assert np.array_equal(emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, lb, tau, h, stride=N + 1, c_stride=N + 3, out_stride=N + 5), want)
    assert np.array_equal(emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, lb, tau, h, force_direct=1, grid=1), want)
    if D * n < N and P > 1:
        assert not degree_below(oracle, emu_compose(emu, air, xn.strip(args), lde, cl, ch, wch, p, g, log_n, lb, tau, h), D * n, p, g, log_n + lb, h)
