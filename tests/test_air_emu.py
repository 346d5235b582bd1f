"""CPU: the AIR composition of csrc/air_core.h (the kernels' own per-thread code, run by the emulator library with
the kernel's tiling) against the oracle's polynomial route, the trace checker, smi_air_plan's host logic through
libstarkmi.so (no context, no GPU), and the Python mirror's pointwise evaluator."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp = C.c_void_p
    L.emu_air_compose.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), vp, C.c_uint64, vp, vp, C.c_int]
    L.emu_air_check.argtypes = [C.c_uint64, C.POINTER(_lib.Air), C.c_uint32, C.c_uint32, vp, C.POINTER(C.c_int),
                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    return L


def emu_compose(emu, air, lde, weights, p, g, log_n, lb, tau, h, direct=False):
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    cols = np.ascontiguousarray(np.stack(lde).astype(np.uint32))
    wts = np.array(weights, dtype=np.uint64)
    out = np.zeros(N, dtype=np.uint32)
    cfg = _lib.StarkCfg(log_n, lb, len(lde), 0, tau, h, 0, 1)
    a = air.flatten(p)
    st = emu.emu_air_compose(p, g, C.byref(cfg), C.byref(a), cols.ctypes.data, N, wts.ctypes.data, out.ctypes.data, 1 if direct else 0)
    assert st == 0, st
    return out.astype(np.uint64)


def emu_check(emu, air, cols, p, log_n):
    a = air.flatten(p)
    tr = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    ok, con, row = C.c_int(), C.c_uint32(), C.c_uint64()
    assert emu.emu_air_check(p, C.byref(a), len(cols), log_n, tr.ctypes.data, C.byref(ok), C.byref(con), C.byref(row)) == 0
    return (True, None, None) if ok.value else (False, con.value, row.value)


CASES = [(4, 3, 1, None), (6, 3, 1, None), (6, 4, 1, None), (10, 3, 1, None), (10, 4, 5, 7), (4, 4, 5, 7)]


@pytest.mark.parametrize("name", ["mixer", "fib", "wide4"])
@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("log_n,lb,tau,h", CASES)
def test_emu_compose_equals_the_polynomial_route(oracle, emu, name, p, g, log_n, lb, tau, h):
    h = g if h is None else h
    air, cols = ac.make(name, 1 << log_n, p)
    wts = ac.weights_for(air)
    assert all(w > p for w in wts)
    want, _ = ac.codeword_poly_route(oracle, air, cols, wts, p, g, log_n, lb, tau, h)
    lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
    got = emu_compose(emu, air, lde, wts, p, g, log_n, lb, tau, h)
    assert np.array_equal(got, np.asarray(want, dtype=np.uint64))
    if log_n <= 6:   # the path without a tile computes the same codeword
        assert np.array_equal(emu_compose(emu, air, lde, wts, p, g, log_n, lb, tau, h, direct=True), got)


@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_emu_compose_of_the_empty_air_is_the_weighted_sum(oracle, emu, p, g):
    log_n, lb = 6, 3
    air, cols = ac.make("empty", 1 << log_n, p)
    wts = ac.weights_for(air)
    lde = ac.lde(oracle, cols, p, g, log_n, lb, 1, g)
    got = emu_compose(emu, air, lde, wts, p, g, log_n, lb, 1, g)
    want = sum((w % p) * np.asarray(col, dtype=object) for w, col in zip(wts, lde)) % p
    assert [int(v) for v in got] == [int(v) for v in want]


@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_emu_compose_wide_synthetic_air_equals_the_mirror(oracle, emu, p, g):
    """W = 64, 32 constraints: the smallest tile, several inversion batches, the caps' neighbourhood"""
    from stark_rs_amd.mirror import Air  # noqa: F401
    log_n, lb = 6, 3
    n, N, B = 1 << log_n, 1 << (log_n + lb), 1 << lb
    air, cols = ac.synthetic(64, 32, p, n)
    wts = ac.weights_for(air)
    lde = ac.lde(oracle, cols, p, g, log_n, lb, 1, g)
    got = emu_compose(emu, air, lde, wts, p, g, log_n, lb, 1, g)
    _, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
    for i in list(range(0, N, 37)) + list(range(N - B, N)):
        want = air.compose_at(p, log_n, lb, 1, g, wN, i, [col[i] for col in lde], [col[(i + B) % N] for col in lde], wts)
        assert int(got[i]) == want, i


@pytest.mark.parametrize("name", ["mixer", "fib", "wide4"])
@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_mirror_pointwise_evaluator_equals_the_polynomial_route(oracle, name, p, g):
    log_n, lb, tau, h = 6, 3, 5, 7
    N, B = 1 << (log_n + lb), 1 << lb
    air, cols = ac.make(name, 1 << log_n, p)
    wts = ac.weights_for(air)
    want, _ = ac.codeword_poly_route(oracle, air, cols, wts, p, g, log_n, lb, tau, h)
    lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
    _, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
    for i in range(N):
        got = air.compose_at(p, log_n, lb, tau, h, wN, i, [col[i] for col in lde], [col[(i + B) % N] for col in lde], wts)
        assert got == int(want[i]), i


@pytest.mark.parametrize("name", ["mixer", "fib", "wide4"])
@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_emu_check_names_the_first_violation(emu, name, p, g):
    log_n = 6
    n = 1 << log_n
    air, cols = ac.make(name, n, p)
    assert emu_check(emu, air, cols, p, log_n) == (True, None, None)
    assert air.first_violation(p, cols) is None
    nb = len(air.boundaries)
    # one cell changed in the middle: the first violated (constraint, row), computed independently in Python
    bad = [list(c) for c in cols]
    bad[1][20] = (bad[1][20] + 1) % p
    want = None
    for k in range(len(air.constraints)):
        rows = [r for r in range(n - 1) if air.constraint_value(k, p, [c[r] for c in bad], [c[r + 1] for c in bad])]
        if rows:
            want = (nb + k, rows[0])
            break
    assert want is not None
    assert emu_check(emu, air, bad, p, log_n) == (False,) + want
    assert air.first_violation(p, bad) == want
    # a wrong boundary value is reported before any transition violation
    bad[0][0] = (bad[0][0] + 1) % p
    assert emu_check(emu, air, bad, p, log_n) == (False, 0, 0)


def _plan(air_flat, p, log_n, lb, W, tau=1, h=3):
    from stark_rs_amd import _lib
    L = _lib.lib()
    cfg = _lib.StarkCfg(log_n, lb, W, 0, tau, h, 8, 1)
    d, e = C.c_uint32(), C.c_uint64()
    st = L.smi_air_plan(p, C.byref(cfg), C.byref(air_flat), C.byref(d), C.byref(e))
    return st, d.value, e.value, L.smi_air_last_error().decode()


def test_air_plan_host_logic():
    from stark_rs_amd.mirror import Air
    BAD_ARG, NON_CANONICAL, TOO_SMALL = -50, -51, -10
    p = 998244353
    n = 64
    for name, W, d, E in [("mixer", 4, 3, 4), ("fib", 2, 1, 8), ("wide4", 4, 3, 4), ("empty", 4, 1, 8)]:
        air, _ = ac.make(name, n, p)
        assert _plan(air.flatten(p), p, 6, 3, W)[:3] == (0, d, E), name
    mixer, _ = ac.make("mixer", n, p)
    st, _, _, why = _plan(mixer.flatten(p), p, 6, 2, 4)
    assert st == TOO_SMALL and "FRI degree bound" in why
    st, _, _, why = _plan(mixer.flatten(p), p, 6, 3, 4, h=1)
    assert st == BAD_ARG and "lde_offset^N == 1" in why
    a = Air(4).boundary(1, 5, 2).boundary(1, 5, 2)
    st, _, _, why = _plan(a.flatten(p), p, 6, 3, 4)
    assert st == BAD_ARG and "twice" in why
    a = Air(4).transition({("cur", 0): 1})
    f = a.flatten(p)
    f._keep[3][0] = 8                                       # factor_var >= 2 W
    st, _, _, why = _plan(f, p, 6, 3, 4)
    assert st == BAD_ARG and "factor_var" in why
    f = a.flatten(p)
    f._keep[4][0] = 0                                       # exponent 0
    st, _, _, why = _plan(f, p, 6, 3, 4)
    assert st == BAD_ARG and "factor_exp" in why
    f = a.flatten(p)
    f._keep[1][0] = p                                       # non-canonical coefficient
    assert _plan(f, p, 6, 3, 4)[0] == NON_CANONICAL
    a = Air(4).boundary(0, 0, 1)
    f = a.flatten(p)
    f._keep[7][0] = p                                       # non-canonical boundary value
    assert _plan(f, p, 6, 3, 4)[0] == NON_CANONICAL
    # the documented caps, each met and then exceeded by one
    def with_constraints(k):
        a = Air(4)
        for _ in range(k):
            a.transition({("cur", 0): 1})
        return a
    assert _plan(with_constraints(64).flatten(p), p, 6, 3, 4)[0] == 0
    st, _, _, why = _plan(with_constraints(65).flatten(p), p, 6, 3, 4)
    assert st == BAD_ARG and "SMI_AIR_MAX_CONSTRAINTS" in why
    many = lambda t: Air(4).transition({(("cur", i % 4, 1 + i // 16), ("next", (i // 4) % 4)): 1 for i in range(t)})
    assert _plan(many(1024).flatten(p), p, 6, 12, 4)[0] == 0
    st, _, _, why = _plan(many(1025).flatten(p), p, 6, 12, 4)
    assert st == BAD_ARG and "SMI_AIR_MAX_TERMS" in why
    factors = lambda k: Air(64).transition({tuple(("cur", i) for i in range(k)): 1})
    assert _plan(factors(8).flatten(p), p, 6, 5, 64)[0] == 0
    st, _, _, why = _plan(factors(9).flatten(p), p, 6, 6, 64)
    assert st == BAD_ARG and "SMI_AIR_MAX_TERM_FACTORS" in why
    def points(k):
        a = Air(4)
        for r in range(k):
            a.boundary(2, r, r)
        return a
    assert _plan(points(16).flatten(p), p, 6, 3, 4)[0] == 0
    st, _, _, why = _plan(points(17).flatten(p), p, 6, 3, 4)
    assert st == BAD_ARG and "SMI_AIR_MAX_BOUNDARY_PER_COL" in why
    st, _, _, why = _plan(Air(65).flatten(p), p, 6, 3, 65)
    assert st == BAD_ARG and "64 columns" in why
    st, _, _, why = _plan(Air(4).transition({("cur", 0, 256): 1}).flatten(p), p, 6, 12, 4)
    assert st == BAD_ARG and "SMI_AIR_MAX_EXP" in why
