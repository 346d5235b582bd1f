"""CPU: the lane code of the argument list with selectors and periodic members (csrc/xargs_core.h over args_core.h), run by
the emulator library (csrc/emu_xargs.cpp) for every lane, workgroup and argument with the kernels' lane batching and block
split, against the Python restatement (tests/xargs_compose.py), which takes a periodic column as the written-out trace
column it is.  Every comparison is exact, at both project primes.

log_n 1, 2, 5, 11: under a lane's four rows, one lane, under one workgroup, two workgroups.  The periods put the wrap of a
periodic column inside a lane (1, 2), at a lane's edge (4), at several lanes (8) and nowhere (n, a fully public column).
Every case asserts first that the restatement meets no zero denominator under its challenges."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import args_compose as agc
import ext_compose as xc
import perm_compose as pm
import xargs_compose as xg
from test_lookup_emu import chall, degree_below

U64_MAX = (1 << 64) - 1
NO_INVERSE, LOOKUP_MISSING = -1, -56
W = xg.W_SCENE


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.emu_xargs_columns.argtypes = [u64, u64, C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), vp, u32, u32, vp, vp, u64, C.POINTER(u32), C.POINTER(u64)]
    L.emu_xargs_multiplicities.argtypes = [u64, u64, C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), u32, vp, u32, u32, vp, C.c_int, C.POINTER(u64)]
    L.emu_air_compose_xargs.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), vp, u64, vp, u64, vp, vp, vp,
                                        u64, C.c_int, u32]
    L.emu_args_columns.argtypes = [u64, u64, C.POINTER(_lib.AirArgs), vp, u32, u32, vp, vp, u64, C.POINTER(u32), C.POINTER(u64)]
    return L


def flat(air, args, p):
    """-> the flattened AIR carrying `args` as an smi_air_xargs (also when the list is plain)"""
    import copy
    a = copy.copy(air)
    a.args, a.xargs_always = [], True
    f = xg.mirror_air(a, args).flatten(p)
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


def periods_of(kind, n):
    """(P0, P1, P2) by name, cut to n"""
    return tuple(min(P, n) for P in {"in-lane": (1, 2, 2), "lane-edge": (4, 2, 4), "lanes": (8, 4, 1), "public": (n, n, n), "mixed": (2, 8, n)}[kind])


PERIODS = ["in-lane", "lane-edge", "lanes", "public", "mixed"]
_scenes = {}


def scene(log_n, p, kind, edge=None, A=8):
    key = (log_n, p, kind, edge, A)
    if key not in _scenes:
        _scenes[key] = xg.scene(1 << log_n, p, periods_of(kind, 1 << log_n), seed=log_n + 3, edge=edge, A=A)
    return _scenes[key]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,A,kind", [(log_n, A, kind) for log_n, A in [(1, 8), (2, 8), (5, 8), (5, 3)] for kind in PERIODS] +
                         [(11, 3, "in-lane"), (11, 3, "public")])   # two workgroups: the wrap inside a lane, a fully public column
def test_emu_columns_equal_the_restatement(emu, p, g, log_n, A, kind):
    air, cols, args = scene(log_n, p, kind, A=A)
    ch = chall(log_n)
    wide = xg.widen(cols, air, p)
    want, closes, zero = xg.columns(wide, args, ch, p, g, W)
    assert zero is None and all(closes)
    n = 1 << log_n
    st, c, got_closes, _ = emu_columns(emu, air, cols, args, ch, p, g, c_stride=n + (log_n % 3))
    assert st == 0
    assert np.array_equal(c, want)
    assert got_closes == [True] * len(args)
    assert xg.recurrences_hold(c, wide, args, ch, p, g, W) == [(True, True)] * len(args)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("edge", ["sel0", "sel1", "pm1"])
@pytest.mark.parametrize("log_n", [2, 5])
def test_emu_columns_on_edge_cells(emu, p, g, log_n, edge):
    air, cols, args = scene(log_n, p, "mixed", edge)
    ch = chall(20 + log_n)
    wide = xg.widen(cols, air, p)
    want, closes, zero = xg.columns(wide, args, ch, p, g, W)
    assert zero is None and all(closes)
    st, c, got_closes, _ = emu_columns(emu, air, cols, args, ch, p, g)
    assert st == 0 and np.array_equal(c, want) and all(got_closes)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", [2, 5])
def test_a_selector_decides_whether_an_argument_closes(emu, p, g, log_n):
    """a value outside the table in an UNSELECTED row leaves the lookup closed; with that row's selector set it does not
    close; a selector moved to the other side, or dropped, opens the permutation"""
    air, cols, args = scene(log_n, p, "mixed")
    ch = chall(31)
    row = cols[6].index(0)
    assert cols[14][row] not in air.periodics[0]
    bad = [list(c) for c in cols]
    bad[6][row] = 1
    wide = xg.widen(bad, air, p)
    want, closes, zero = xg.columns(wide, args, ch, p, g, W)
    assert zero is None and not closes[0] and not closes[3] and all(closes[a] for a in (1, 2, 4, 5, 6))
    st, c, got, _ = emu_columns(emu, air, bad, args, ch, p, g)
    assert st == 0 and got == closes and np.array_equal(c, want)
    for swap in (("perm", [1], [10], 7, 6), ("perm", [1], [10], 6, None), ("perm", [1], [10])):
        other = args[:3] + [swap] + args[4:]
        wide = xg.widen(cols, air, p)
        want, closes, zero = xg.columns(wide, other, ch, p, g, W)
        assert zero is None
        st, c, got, _ = emu_columns(emu, air, cols, other, ch, p, g)
        assert st == 0 and got == closes and not got[3] and np.array_equal(c, want)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", [2, 5, 11])
def test_a_plain_list_gives_the_columns_of_the_argument_list(emu, p, g, log_n):
    """the anchor at the level of the lane code: no selector, no periodic member -> emu_args_columns's words"""
    from test_args_emu import emu_columns as old_columns
    cols, eight = agc.pool(1 << log_n, p, seed=log_n)
    args = eight if log_n < 11 else eight[:3]
    from stark_rs_amd.mirror import Air
    ch = chall(log_n)
    st0, want, closes0, _ = old_columns(emu, cols, args, ch, p, g)
    st, c, closes, _ = emu_columns(emu, Air(len(cols)), cols, args, ch, p, g)
    assert st == st0 == 0 and closes == closes0 and np.array_equal(c, want)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", [2, 5])
def test_the_smallest_zero_denominator_key_is_named(emu, p, g, log_n):
    """f_T of argument 0 (a periodic table) made zero in a row: the key is 16 row + 2 a + side, whatever the selectors hold;
    a zero g_R of the selected permutation likewise; the next call succeeds"""
    n = 1 << log_n
    air, cols, args = scene(log_n, p, "mixed")
    wide = xg.widen(cols, air, p)
    for a, side_cols in ((0, xg.norm(args[0], W)[2]), (2, xg.norm(args[2], W)[1])):
        for row in (0, n - 1):
            ch = pm.gamma_for_zero(wide, side_cols, chall(4), row, p, g)
            _c, _cl, want = xg.columns(wide, args, ch, p, g, W)
            assert want is not None and want >> 4 <= row
            st, _c, _closes, key = emu_columns(emu, air, cols, args, ch, p, g)
            assert st == NO_INVERSE and key == want
    row = cols[7].index(1)                                               # a selected right row of argument 3: g_R = f_R there
    ch = pm.gamma_for_zero(wide, [10], chall(4), row, p, g)
    _c, _cl, want = xg.columns(wide, args, ch, p, g, W)
    st, _c, _closes, key = emu_columns(emu, air, cols, args, ch, p, g)
    assert st == NO_INVERSE and key == want and want is not None
    st, c, _closes, _ = emu_columns(emu, air, cols, args, chall(4), p, g)
    assert st == 0 and np.array_equal(c, xg.columns(wide, args, chall(4), p, g, W)[0])


# ---------------------------------------------------------------------------------------------- the multiplicities
def emu_mult(emu, air, cols, args, a, p, g, order):
    cols = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    n_cols, n = cols.shape
    f = flat(air, args, p)
    M = np.full(n + 2, 0xdeadbeef, dtype=np.uint32)
    missing = C.c_uint64(0)
    st = emu.emu_xargs_multiplicities(p, g, C.byref(f), C.byref(f.xargs), a, cols.ctypes.data, n_cols, n.bit_length() - 1, M[1:].ctypes.data, order,
                                      C.byref(missing))
    assert M[0] == M[-1] == 0xdeadbeef
    return st, [int(v) for v in M[1:-1]], missing.value


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,kind", [(log_n, kind) for log_n in (1, 2, 5) for kind in PERIODS] + [(11, "in-lane")])
def test_emu_multiplicities_equal_the_dictionary(emu, p, g, log_n, kind):
    air, cols, args = scene(log_n, p, kind)
    wide = xg.widen(cols, air, p)
    for a, arg in enumerate(args):
        if arg[0] != "lookup":
            st, _M, _ = emu_mult(emu, air, cols, args, a, p, g, 0)
            assert st == -50                                             # SMI_ERR_BAD_ARG: a permutation has no multiplicities
            continue
        want, missing = xg.multiplicities(wide, arg, W)
        assert missing is None and want == cols[arg[3]]
        for order in (0, 1):
            st, M, _ = emu_mult(emu, air, cols, args, a, p, g, order)
            assert st == 0 and M == want, (a, order)
        if len(arg) > 4 and arg[5] is not None:                         # a table selector: an unselected table row counts nothing
            sel = wide[xg.norm(arg, W)[5]]
            assert all(M[t] == 0 for t in range(len(M)) if not sel[t])


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_a_missing_selected_row_is_named_and_an_unselected_one_is_not(emu, p, g):
    air, cols, args = scene(5, p, "mixed")
    off = [r for r in range(32) if not cols[6][r]]
    on = [r for r in range(32) if cols[6][r]]
    st, _M, missing = emu_mult(emu, air, cols, args, 0, p, g, 0)          # the unselected rows hold values outside the table
    assert st == 0 and off and all(cols[14][r] not in air.periodics[0] for r in off)
    bad = [list(c) for c in cols]
    for r in on[1:3]:
        bad[14][r] = p - 2
    want, first = xg.multiplicities(xg.widen(bad, air, p), args[0], W)
    assert first == on[1]
    for order in (0, 1):
        st, M, missing = emu_mult(emu, air, bad, args, 0, p, g, order)
        assert st == LOOKUP_MISSING and missing == on[1] and M == want


# ---------------------------------------------------------------------------------------------- the composition
def emu_compose(emu, air, args, cols_lde, cl, ch, wch, p, g, log_n, lb, tau, h, stride=None, c_stride=None, out_stride=None, force_direct=0, grid=0):
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    n_cols, CW = len(cols_lde), len(cl)
    stride, c_stride, out_stride = (N if v is None else v for v in (stride, c_stride, out_stride))
    f = flat(air, args, p)
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


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,kind,A", [(3, "in-lane", 8), (4, "lane-edge", 3), (5, "mixed", 8), (6, "public", 3), (7, "lanes", 3)])
def test_emu_air_compose_xargs_equals_the_restatement(oracle, emu, p, g, log_n, kind, A):
    """the composition of an honest trace equals the restatement's and stays within its degree bound; with a selector dropped
    from the list the composition of the same columns exceeds it"""
    lb, tau, h = 3, 1, g
    n, N = 1 << log_n, 1 << (log_n + lb)
    air, cols, args = scene(log_n, p, kind, A=A)
    K = len(air.constraints)
    _d, D, _E = xg.plan(air, args, lb)
    ch = chall(11)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 2 * A), dtype=np.uint64)]
    wide = xg.widen(cols, air, p)
    c, closes, zero = xg.columns(wide, args, ch, p, g, W)
    assert zero is None and all(closes)
    lde_wide = np.asarray(ac.lde(oracle, wide, p, g, log_n, lb, tau, h), dtype=np.uint64)
    lde = lde_wide[:W]
    cl = ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)
    want = pm.main_codeword(oracle, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
    want = (want + xg.aux_terms(oracle, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W)) % np.uint64(p)
    got = emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, lb, tau, h)
    assert np.array_equal(got, want)
    assert degree_below(oracle, got, D * n, p, g, log_n + lb, h)
    assert np.array_equal(emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, lb, tau, h, stride=N + 1, c_stride=N + 3, out_stride=N + 5), want)
    assert np.array_equal(emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, lb, tau, h, force_direct=1, grid=1), want)
    other = [("lookup", [14], [("per", 0)], 8)] + args[1:]              # argument 0 without its selector
    assert not degree_below(oracle, emu_compose(emu, air, other, lde, cl, ch, wch, p, g, log_n, lb, tau, h), D * n, p, g, log_n + lb, h)
