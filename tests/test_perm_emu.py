"""CPU: the permutation argument's kernels' own lane code (csrc/perm_core.h), run by the emulator library with the
kernels' lane batching and block split, against the Python restatement (tests/perm_compose.py)."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import ext_compose as xc
import perm_compose as pm

U64_MAX = (1 << 64) - 1
NO_INVERSE = -1


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp = C.c_void_p
    L.emu_perm_column.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.AirPerm), vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64,
                                  C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.emu_air_compose_perm.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.POINTER(_lib.AirPerm), vp, C.c_uint64,
                                       vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_int, C.c_uint32]
    return L


def make_perm(left, right):
    from stark_rs_amd import _lib
    la, ra = np.array(left, dtype=np.uint32), np.array(right, dtype=np.uint32)
    out = _lib.AirPerm(len(la), 0, la.ctypes.data_as(_lib.u32p), ra.ctypes.data_as(_lib.u32p))
    out._keep = (la, ra)
    return out


def emu_column(emu, cols, left, right, ch, p, g, z_stride=None):
    """-> (status, z (4, n) uint64, closes, zero row)"""
    cols = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    W, n = cols.shape
    z_stride = n if z_stride is None else z_stride
    z = np.full(4 * z_stride, 0xdeadbeef, dtype=np.uint32)
    cha = np.array(ch, dtype=np.uint64)
    closes, zero = C.c_int(-1), C.c_uint64(0)
    st = emu.emu_perm_column(p, g, C.byref(make_perm(left, right)), cols.ctypes.data, W, n.bit_length() - 1, cha.ctypes.data, z.ctypes.data, z_stride,
                             C.byref(closes), C.byref(zero))
    for e in range(4):   # nothing written between the columns
        assert np.all(z[e * z_stride + n:(e + 1) * z_stride] == 0xdeadbeef)
    return st, np.stack([z[e * z_stride:e * z_stride + n] for e in range(4)]).astype(np.uint64), closes.value, zero.value


def chall(seed):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(1 << 62, U64_MAX, 8, dtype=np.uint64)]


SHAPES = ["m1", "m2", "m8", "overlap"]


def shaped(kind, n, p, seed):
    if kind == "overlap":
        rng = np.random.default_rng(seed)
        return [[int(v) for v in rng.integers(0, p, n)] for _ in range(4)], [0, 1, 2], [2, 0, 3]
    return pm.shuffled_copy(n, int(kind[1:]), p, seed)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("kind", SHAPES)
@pytest.mark.parametrize("log_n", range(1, 14))
def test_emu_perm_column_equals_the_restatement(emu, p, g, log_n, kind):
    n = 1 << log_n
    cols, left, right = shaped(kind, n, p, log_n)
    ch = chall(log_n)
    want, closes, zero = pm.column(cols, left, right, ch, p, g)
    assert zero is None
    st, z, got_closes, _ = emu_column(emu, cols, left, right, ch, p, g, z_stride=n + (log_n % 3))
    assert st == 0
    assert np.array_equal(z, want)
    assert got_closes == int(closes)
    assert closes == (kind != "overlap")       # a shuffled copy closes
    if log_n == 7:
        assert pm.recurrence_holds(z, cols, left, right, ch, p, g)
        bad = z.copy()
        bad[2, 5] = (bad[2, 5] + 1) % p
        assert not pm.recurrence_holds(bad, cols, left, right, ch, p, g)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("kind", ["cell", "multiplicity", "columnwise"])
@pytest.mark.parametrize("log_n", [2, 6, 11])
def test_the_product_does_not_close_when_the_multisets_differ(emu, p, g, log_n, kind):
    n = 1 << log_n
    cols, left, right = pm.non_closing(kind, n, p)
    ch = chall(3)
    want, closes, zero = pm.column(cols, left, right, ch, p, g)
    assert zero is None and not closes
    st, z, got_closes, _ = emu_column(emu, cols, left, right, ch, p, g)
    assert st == 0 and got_closes == 0
    assert np.array_equal(z, want)
    if kind == "columnwise":   # each column alone IS a permutation: only alpha tells the tuples apart
        for j in range(2):
            assert pm.column(cols, [left[j]], [right[j]], ch, p, g)[1]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", [3, 11])
@pytest.mark.parametrize("where", ["first", "last", "inside", "two"])
def test_a_zero_denominator_is_no_inverse_naming_the_smallest_row(emu, p, g, log_n, where):
    n = 1 << log_n
    cols, left, right = pm.shuffled_copy(n, 2, p, 8)
    rows = {"first": [0], "last": [n - 1], "inside": [6], "two": [n // 2 + 1, 5]}[where]
    for r in rows[1:]:                         # the same right tuple in both rows: one gamma makes both denominators zero
        for c in right:
            cols[c][r] = cols[c][rows[0]]
    ch = pm.gamma_for_zero(cols, right, chall(4), rows[0], p, g)
    assert pm.column(cols, left, right, ch, p, g) == (None, None, min(rows))
    st, _z, _closes, zero = emu_column(emu, cols, left, right, ch, p, g)
    assert st == NO_INVERSE and zero == min(rows)
    st, z, _closes, _ = emu_column(emu, cols, left, right, chall(4), p, g)       # the next call succeeds
    assert st == 0 and np.array_equal(z, pm.column(cols, left, right, chall(4), p, g)[0])


# ---------------------------------------------------------------------------------------------- the composition
def emu_compose(emu, air, cols_lde, zl, ch, wch, p, g, log_n, lb, tau, h, stride=None, z_stride=None, out_stride=None, force_direct=0, grid=0):
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    W = len(cols_lde)
    stride, z_stride, out_stride = (N if v is None else v for v in (stride, z_stride, out_stride))
    a = air.flatten(p)
    cfg = _lib.StarkCfg(log_n, lb, W, 1, tau, h, 0, 1)
    lde = np.zeros(W * stride, dtype=np.uint32)
    for c in range(W):
        lde[c * stride:c * stride + N] = cols_lde[c]
    zb = np.zeros(4 * z_stride, dtype=np.uint32)
    for e in range(4):
        zb[e * z_stride:e * z_stride + N] = zl[e]
    out = np.full(4 * out_stride, 0xdeadbeef, dtype=np.uint32)
    cha, wa = np.array(ch, dtype=np.uint64), np.array(wch, dtype=np.uint64)
    st = emu.emu_air_compose_perm(p, g, C.byref(cfg), C.byref(a), C.byref(a.perm), lde.ctypes.data, stride, zb.ctypes.data, z_stride, cha.ctypes.data,
                                  wa.ctypes.data, out.ctypes.data, out_stride, force_direct, grid)
    assert st == 0
    for e in range(4):
        assert np.all(out[e * out_stride + N:(e + 1) * out_stride] == 0xdeadbeef)
    return np.stack([out[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)


def degree_below(o, cw, bound, p, g, log_N, h):
    """every coordinate of cw, interpolated on the coset, has degree < bound"""
    wN = o.ff_prim_nth_root_g(1 << log_N, p, g)
    return all(not np.any(np.asarray(o.fast_intt(np.asarray(cw[e], dtype=np.uint64), wN, h, p))[bound:]) for e in range(4))


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name,m", [("empty", 1), ("fib", 2), ("mixer", 2)])
def test_emu_air_compose_perm_equals_the_restatement(oracle, emu, p, g, name, m):
    log_n, lb, tau, h = 7, 3, 1, g
    n, N = 1 << log_n, 1 << (log_n + lb)
    for spoil in (False, True):
        air, cols = ac.make(name, n, p)
        air, cols = pm.with_permutation(air, cols, m, p, spoil=spoil)
        W, K = len(cols), len(air.constraints)
        left, right = air.perm
        ch = chall(11)
        z, closes, zero = pm.column(cols, left, right, ch, p, g)
        assert zero is None and closes == (not spoil)
        lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
        zl = ac.lde(oracle, [[int(v) for v in z[e]] for e in range(4)], p, g, log_n, lb, tau, h)
        wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 2), dtype=np.uint64)]
        want = pm.main_codeword(oracle, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
        want = (want + pm.aux_terms(oracle, lde, zl, left, right, ch, wch[4 * (W + K):4 * (W + K) + 4], wch[4 * (W + K) + 4:], p, g, log_n, lb, tau, h)) % np.uint64(p)
        got = emu_compose(emu, air, lde, zl, ch, wch, p, g, log_n, lb, tau, h)
        assert np.array_equal(got, want), (name, spoil)
        d = max(air.degree, 2)
        D = 1
        while D < d - 1:
            D *= 2
        assert degree_below(oracle, got, D * n, p, g, log_n + lb, h) == (not spoil)
        if not spoil:   # the shapes of the 4-byte path and a grid that makes every lane loop
            assert np.array_equal(emu_compose(emu, air, lde, zl, ch, wch, p, g, log_n, lb, tau, h, stride=N + 1, z_stride=N + 3, out_stride=N + 5), want)
            assert np.array_equal(emu_compose(emu, air, lde, zl, ch, wch, p, g, log_n, lb, tau, h, force_direct=1, grid=1), want)
