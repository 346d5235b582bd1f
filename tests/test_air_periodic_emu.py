"""CPU: periodic columns of the AIR (include/stark_mi.h, "AIR").  smi_air_plan's host logic through libstarkmi.so (no
context, no GPU); the emulator, which runs the kernels' own per-thread code, staging and table indexing, against the
oracle's polynomial route on the augmented AIR (tests/air_periodic.py); the trace checker; the Python mirror."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
from test_air_emu import _plan, emu, emu_check, emu_compose  # noqa: F401  (emu is a fixture)

BAD_ARG, NON_CANONICAL, TOO_SMALL = -50, -51, -10


def test_air_plan_with_periodic_columns():
    from stark_rs_amd.mirror import Air
    p, n = 998244353, 64
    for name in ap.NAMES:
        air, _ = ap.make(name, n, p)
        assert air.degree == 3
        assert _plan(air.flatten(p), p, 6, 3, ap.W_OF[name])[:3] == (0, 3, 4), name
        assert _plan(air.flatten(p), p, 6, 4, ap.W_OF[name], tau=5, h=7)[:3] == (0, 3, 8), name
    d4 = ap.degree4()
    st, _, _, why = _plan(d4.flatten(p), p, 6, 3, 1)
    assert st == TOO_SMALL and "degree-4" in why
    assert _plan(d4.flatten(p), p, 6, 4, 1)[:3] == (0, 4, 4)
    # the period divides the trace length: l_j <= log_n
    a = Air(1)
    a.periodic(list(range(128)))
    st, _, _, why = _plan(a.flatten(p), p, 6, 3, 1)
    assert st == BAD_ARG and "periodic_log_period" in why
    a = Air(1)
    a.periodic(list(range(64)))
    assert _plan(a.flatten(p), p, 6, 3, 1)[0] == 0
    # SMI_AIR_MAX_PERIODIC met, then exceeded by one
    def many(q):
        a = Air(2)
        for j in range(q):
            a.periodic([j, j + 1])
        return a
    assert _plan(many(16).flatten(p), p, 6, 3, 2)[0] == 0
    st, _, _, why = _plan(many(17).flatten(p), p, 6, 3, 2)
    assert st == BAD_ARG and "SMI_AIR_MAX_PERIODIC" in why
    # a value >= p
    a = Air(1)
    a.periodic([1, 2, 3, 4])
    f = a.flatten(p)
    f._keep[9][2] = p
    st, _, _, why = _plan(f, p, 6, 3, 1)
    assert st == NON_CANONICAL and "periodic value" in why
    # var < 2 W + 2 Q
    a = Air(2)
    k = a.periodic([1, 2])
    a.transition({("per_next", k): 1})
    f = a.flatten(p)
    assert f._keep[3][0] == 2 * 2 + 1 and _plan(f, p, 6, 3, 2)[0] == 0
    f._keep[3][0] = 2 * 2 + 2 * 1
    st, _, _, why = _plan(f, p, 6, 3, 2)
    assert st == BAD_ARG and "factor_var" in why and "n_periodic" in why
    # Q > 0 and a null table
    f = a.flatten(p)
    f.periodic_value = C.POINTER(C.c_uint64)()
    st, _, _, why = _plan(f, p, 6, 3, 2)
    assert st == BAD_ARG and "null table" in why
    f = a.flatten(p)
    f.periodic_log_period = C.POINTER(C.c_uint32)()
    st, _, _, why = _plan(f, p, 6, 3, 2)
    assert st == BAD_ARG and "null table" in why
    # Q = 0: what it gives today, the var >= 2 W refusal included
    for name, W, d, E in [("mixer", 4, 3, 4), ("fib", 2, 1, 8), ("wide4", 4, 3, 4), ("empty", 4, 1, 8)]:
        air, _ = ac.make(name, n, p)
        f = air.flatten(p)
        assert f.n_periodic == 0
        assert _plan(f, p, 6, 3, W)[:3] == (0, d, E), name
    f = Air(4).transition({("cur", 0): 1}).flatten(p)
    f._keep[3][0] = 8
    st, _, _, why = _plan(f, p, 6, 3, 4)
    assert st == BAD_ARG and "factor_var" in why


# (example, log_n): with W + Q tile rows, N = 2^(log_n + lb) gives points per thread P = 1 (N <= 256), 2 (N = 512) and
# 4 (N >= 1024).  switch: tables of 2 B values, far shorter than any tile; mimc at 2^10: 64 B < T = 1024; public: a table
# of N values, longer than any tile, next to one of B values
SHAPES = [("switch", 4), ("public", 4), ("public", 5), ("mimc", 6), ("switch", 6), ("public", 6), ("mimc", 10), ("switch", 10), ("public", 10)]


@pytest.mark.parametrize("name,log_n", SHAPES)
@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("lb,tau,h", ap.CASES)
def test_emu_compose_equals_the_augmented_polynomial_route(oracle, emu, name, log_n, p, g, lb, tau, h):
    h = g if h is None else h
    air, cols = ap.make(name, 1 << log_n, p)
    wts = ac.weights_for(air)
    want, _ = ap.route(oracle, air, cols, wts, p, g, log_n, lb, tau, h)
    lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
    got = emu_compose(emu, air, lde, wts, p, g, log_n, lb, tau, h)
    assert np.array_equal(got, np.asarray(want, dtype=np.uint64))
    if log_n <= 6:   # the kernel without tiles reads the tables from memory, modulo their length
        assert np.array_equal(emu_compose(emu, air, lde, wts, p, g, log_n, lb, tau, h, direct=True), got)


def test_the_shapes_reach_every_tile_kernel():
    """the tile rule of csrc/air_core.h (air_tile), restated: T the largest power of two in 64 .. 1024 with T <= N and
    (W + Q) (T + B) 4 + 4 (64 + 64) <= 65536 bytes; 256 threads, P = T / 256 points per thread"""
    seen = set()
    for name, log_n in SHAPES:
        rows = ap.W_OF[name] + len(ap.make(name, 1 << max(log_n, 6), 998244353)[0].periodics)
        for lb, _, _ in ap.CASES:
            N, B = 1 << (log_n + lb), 1 << lb
            T = next(T for T in (1024, 512, 256, 128, 64) if T <= N and rows * (T + B) * 4 + 512 <= 65536)
            seen.add(max(1, T // 256))
    assert seen == {1, 2, 4}


@pytest.mark.parametrize("name", ["mimc", "public"])
def test_emu_compose_equals_its_augmented_air_at_2_16(oracle, emu, name):
    """2^16 rows x blowup 8: the periodic AIR against the same statement with the periodic columns as trace columns
    under weight 0 -- the tables (emulator transforms, read modulo their length) against extended columns"""
    p, g = ac.PRIMES[1]
    log_n, lb = 16, 3
    air, cols = ap.make(name, 1 << log_n, p)
    wts = ac.weights_for(air)
    aug, acols, awts = ap.augment(air, cols, wts, p)
    alde = ac.lde(oracle, acols, p, g, log_n, lb, 1, g)
    got = emu_compose(emu, air, alde[:air.n_cols], wts, p, g, log_n, lb, 1, g)
    want = emu_compose(emu, aug, alde, awts, p, g, log_n, lb, 1, g)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ap.NAMES)
@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_emu_check_with_periodic_columns(emu, name, p, g):
    log_n = 7
    n = 1 << log_n
    air, cols = ap.make(name, n, p)
    assert air.first_violation(p, cols) is None
    assert emu_check(emu, air, cols, p, log_n) == (True, None, None)
    bad = [list(c) for c in cols]
    bad[0][77] = (bad[0][77] + 1) % p
    want = air.first_violation(p, bad)
    assert want is not None and want[1] in (76, 77)
    assert emu_check(emu, air, bad, p, log_n) == (False,) + want
    # the same trace under a statement with one periodic value changed
    other, _ = ap.make(name, n, p)
    other.periodics[0][0] += 1   # (the last value of a period-n column meets no row pair)
    want = other.first_violation(p, cols)
    assert want is not None
    assert emu_check(emu, other, cols, p, log_n) == (False,) + want


@pytest.mark.parametrize("name", ap.NAMES)
@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("lb,tau,h", ap.CASES)
def test_mirror_compose_at_equals_the_route(oracle, name, p, g, lb, tau, h):
    h = g if h is None else h
    log_n = 6
    N, B = 1 << (log_n + lb), 1 << lb
    air, cols = ap.make(name, 1 << log_n, p)
    wts = ac.weights_for(air)
    want, _ = ap.route(oracle, air, cols, wts, p, g, log_n, lb, tau, h)
    lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
    _, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
    for i in list(range(0, N, 5)) + list(range(N - B, N)):
        got = air.compose_at(p, log_n, lb, tau, h, wN, i, [col[i] for col in lde], [col[(i + B) % N] for col in lde], wts)
        assert got == int(want[i]), i


@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_two_spellings_of_one_statement_give_one_codeword(oracle, emu, p, g):
    """period 2 [a, b] and period 4 [a, b, a, b]"""
    log_n, lb = 6, 3
    n = 1 << log_n
    air2, cols = ap.make("switch", n, p)
    air4, _ = ap.make("switch", n, p)
    air4.periodics[0] = air4.periodics[0] * 2
    assert air2.flatten(p)._keep[8][0] == 1 and air4.flatten(p)._keep[8][0] == 2
    wts = ac.weights_for(air2)
    lde = ac.lde(oracle, cols, p, g, log_n, lb, 1, g)
    want, _ = ap.route(oracle, air2, cols, wts, p, g, log_n, lb, 1, g)
    for direct in (False, True):
        c2 = emu_compose(emu, air2, lde, wts, p, g, log_n, lb, 1, g, direct=direct)
        c4 = emu_compose(emu, air4, lde, wts, p, g, log_n, lb, 1, g, direct=direct)
        assert np.array_equal(c2, c4) and np.array_equal(c2, np.asarray(want, dtype=np.uint64))
    assert emu_check(emu, air4, cols, p, log_n) == (True, None, None)


@pytest.mark.parametrize("name", ap.NAMES)
@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("lb,tau,h", ap.CASES)
def test_fast_route_equals_the_polynomial_route(oracle, name, p, g, lb, tau, h):
    """the checker of the 2^16-row GPU proof (air_periodic.fast_route) against the schoolbook route, where both run"""
    h = g if h is None else h
    log_n = 8
    air, cols = ap.make(name, 1 << log_n, p)
    wts = ac.weights_for(air)
    want, _ = ap.route(oracle, air, cols, wts, p, g, log_n, lb, tau, h)
    got = ap.fast_route(oracle, air, cols, wts, p, g, log_n, lb, tau, h)
    assert np.array_equal(np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64))
    bad = [list(c) for c in cols]
    bad[0][100] = (bad[0][100] + 1) % p
    with pytest.raises(AssertionError, match="remainder"):
        ap.fast_route(oracle, air, bad, wts, p, g, log_n, lb, tau, h)
