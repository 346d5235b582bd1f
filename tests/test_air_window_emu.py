"""CPU: the point functions of transition windows (csrc/air_core.h, csrc/deep_core.h), run by the emulator library with the
kernels' own tiling, halo and lane bodies, against the Python restatement (tests/window_compose.py), at log_N <= 8.  Every
comparison is exact.  The restatement itself is pinned to the two-row routes it extends (ap.route, dc.q_codeword)."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import deep_compose as dc
import ext_compose as xc
import window_compose as wc
from test_gpu_boundary_primes import GEN, THREE, u64_set

PRIMES = list(xc.PRIMES)
FIELDS = PRIMES + [(p, GEN[p]) for p in THREE]   # with the boundary moduli, where tests/test_deep_emu.py runs them: the lane bodies


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.emu_air_compose.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), vp, u64, vp, vp, C.c_int]
    L.emu_air_compose_ext.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), vp, u64, vp, vp, u64, C.c_int]
    L.emu_air_check.argtypes = [u64, C.POINTER(_lib.Air), u32, u32, vp, C.POINTER(C.c_int), C.POINTER(u32), C.POINTER(u64)]
    L.emu_poly_eval_ext.argtypes = [u64, u64, vp, u32, u64, u64, vp, u32, vp]
    L.emu_poly_eval_ext_shifts.argtypes = [u64, u64, vp, u32, u64, u64, vp, u64, u32, vp]
    L.emu_deep_compose.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), u32, vp, u64, vp, u64, vp, vp, vp, vp, u64, u32]
    L.emu_deep_compose_window.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), u32, u32, vp, u64, vp, u64, vp, vp, vp, vp, u64, u32]
    L.emu_deep_ood_sides.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), vp, vp, vp, vp, vp]
    L.emu_deep_q_at_window.argtypes = [u64, u64, u32, u32, u32, u64, u64, vp, vp, vp, vp, vp, vp]
    return L


def _u64(v):
    return np.array([int(x) for x in v], dtype=np.uint64)


def emu_compose(emu, air, lde, weights, p, g, log_n, lb, tau, h, direct=False, ext=False, pad=0):
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    stride = N + pad
    host = np.full(len(lde) * stride, 0x7fffffff, dtype=np.uint32)
    for c, col in enumerate(lde):
        host[c * stride:c * stride + N] = np.asarray(col, dtype=np.uint32)
    wts = _u64(weights)
    out = np.zeros(4 * N if ext else N, dtype=np.uint32)
    cfg = _lib.StarkCfg(log_n, lb, len(lde), 0, tau, h, 0, 1)
    a = air.flatten(p)
    if ext:
        st = emu.emu_air_compose_ext(p, g, C.byref(cfg), C.byref(a), host.ctypes.data, stride, wts.ctypes.data, out.ctypes.data, N, 1 if direct else 0)
    else:
        st = emu.emu_air_compose(p, g, C.byref(cfg), C.byref(a), host.ctypes.data, stride, wts.ctypes.data, out.ctypes.data, 1 if direct else 0)
    assert st == 0, st
    return out.astype(np.uint64).reshape(4, N) if ext else out.astype(np.uint64)


def test_restatement_at_two_rows_is_the_existing_route(oracle):
    """window_compose.compose on a two-row AIR gives what the polynomial route of tests/air_periodic.py gives"""
    o = oracle
    p, g = xc.PRIMES[0]
    for name in ("mimc", "switch"):
        air, cols = ap.make(name, 64, p)
        assert air.window == 2
        wts = ac.weights_for(air)
        want = np.asarray(ap.route(o, air, cols, wts, p, g, 6, 3, 1, g)[0], dtype=np.uint64)
        assert np.array_equal(wc.compose(o, air, cols, wts, p, g, 6, 3, 1, g), want), name


def test_composition_of_a_satisfying_trace_has_the_planned_degree(oracle):
    """the four proof AIRs: H has no coefficient at or above D n, and for the pairs whose D doubles it has some at or above
    D n / 2 -- the doubling is needed, not a safety margin"""
    o = oracle
    p, g = xc.PRIMES[0]
    log_n, lb = 5, 3
    for name in ("fib1", "sq", "tap4", "wide"):
        air, cols = wc.make(name, 1 << log_n, p)
        d, D = wc.plan(air, log_n)
        assert air.first_violation(p, cols) is None
        H = wc.compose_ext(o, air, cols, xc.ext_weights_for(air), p, g, log_n, lb, 5, g)
        hc, _seg = dc.segments(o, H, D, p, g, log_n, lb, g)
        assert not hc[:, D << log_n:].any(), name
        if (d, air.window) in ((2, 3), (2, 4), (3, 4)):
            assert hc[:, (D // 2) << log_n:].any(), name


def test_synthetic_keeps_its_default_and_its_shape_when_extreme():
    """extreme=False is the statement the tests have always composed (pinned by digest); extreme=True has the same operands,
    exponents, boundary rows and periods, and every value p - 1"""
    import hashlib
    p = xc.PRIMES[0][0]
    air, cols = wc.synthetic(5, 2, 4, 2, p, 16)
    told = repr((cols, air.constraints, air.boundaries, air.periodics, air.window, air.degree)).encode()
    assert hashlib.sha256(told).hexdigest() == "aeba049f6293ee5713c0ea7e5816a1eb5e94dd53cc740e405822f5afbb179292"
    top, tcols = wc.synthetic(5, 2, 4, 2, p, 16, extreme=True)
    assert (top.window, top.degree) == (air.window, air.degree) == (4, 2)
    assert [[f for _cf, f in con] for con in top.constraints] == [[f for _cf, f in con] for con in air.constraints]
    assert [(c, r) for c, r, _v in top.boundaries] == [(c, r) for c, r, _v in air.boundaries]
    assert [len(v) for v in top.periodics] == [len(v) for v in air.periodics] == [2, 16]
    values = [v for c in tcols for v in c] + [v for per in top.periodics for v in per] + [v for _c, _r, v in top.boundaries]
    assert all(v % p == p - 1 for v in values + [cf for con in top.constraints for cf, _f in con])


@pytest.mark.parametrize("p,g", FIELDS)
@pytest.mark.parametrize("S", [3, 4])
def test_emu_compose_window(emu, oracle, p, g, S):
    """base and extension weights, tiled and direct, B in {4, 8, 16}, the halo longer than, equal to and shorter than a tile;
    at log_N = 8, for every B, the statement with every value p - 1 as well"""
    o = oracle
    seen, extremes = set(), set()
    for lb in (2, 3, 4):
        for log_N in range(((S << lb) - 1).bit_length(), 9):   # from N = S B on, where the halo is all of the domain but B points
            log_n = log_N - lb
            if (1 << log_n) < S:
                continue
            W, Q = [(1, 0), (5, 2), (64, 0), (1, 2), (5, 0), (64, 2)][(log_N + lb + S) % 6]
            if Q == 2 and log_n < 1:
                continue
            for extreme in ((False, True) if log_N == 8 else (False,)):
                air, cols = wc.synthetic(W, Q, S, 1 if lb == 2 else 2, p, 1 << log_n, extreme=extreme)
                lde = ac.lde(o, cols, p, g, log_n, lb, 5, g)
                wts, xw = ac.weights_for(air), xc.ext_weights_for(air)
                want, want_x = wc.compose(o, air, cols, wts, p, g, log_n, lb, 5, g), wc.compose_ext(o, air, cols, xw, p, g, log_n, lb, 5, g)
                seen.add(wc.air_tile(W + Q, 1 << lb, 1 << log_N, 1, S))
                extremes |= {(S, lb)} if extreme else set()
                for direct, pad in ((False, 0), (True, 0), (False, 3)):
                    got = emu_compose(emu, air, lde, wts, p, g, log_n, lb, 5, g, direct, False, pad)
                    assert np.array_equal(got, want), (S, lb, log_N, W, Q, extreme, direct, pad, int(np.flatnonzero(got != want)[0]))
                    got = emu_compose(emu, air, lde, xw, p, g, log_n, lb, 5, g, direct, True, pad)
                    assert np.array_equal(got, want_x), (S, lb, log_N, W, Q, extreme, direct, pad)
    assert {0, 64, 128, 256} <= seen, seen
    assert extremes == {(S, 2), (S, 3), (S, 4)}


def test_emu_check_window(emu):
    """a trace that breaks only the window starting at row n - S is refused naming that row; the windows that would start at
    n - S + 1 .. n - 1 (and wrap) are violated by every one of these traces and are not checked: the exemption is exact"""
    p, _g = xc.PRIMES[0]
    n, log_n = 32, 5
    for name, col in (("fib1", 0), ("sq", 0), ("tap4", 0), ("wide", 2)):
        air, cols = wc.make(name, n, p)
        S, a = air.window, air.flatten(p)

        def check(cs):
            tr = np.ascontiguousarray(np.array(cs, dtype=np.uint32))
            ok, con, row = C.c_int(), C.c_uint32(), C.c_uint64()
            assert emu.emu_air_check(p, C.byref(a), len(cs), log_n, tr.ctypes.data, C.byref(ok), C.byref(con), C.byref(row)) == 0
            return (True, None, None) if ok.value else (False, con.value, row.value)
        assert wc.wrapped_violations(air, p, cols) == list(range(n - S + 1, n)), name
        assert check(cols) == (True, None, None), name
        bad = [list(c) for c in cols]
        bad[col][n - 1] = (bad[col][n - 1] + 1) % p      # row n - 1 is read at shift S - 1 by the window of n - S alone
        ok, con, row = check(bad)
        assert not ok and row == n - S and (con, row) == air.first_violation(p, bad), name


@pytest.mark.parametrize("p,g", FIELDS)
def test_emu_poly_eval_shifts(emu, oracle, p, g):
    o = oracle
    rng = np.random.default_rng(5)
    z = [int(v) for v in rng.integers(1, p, 4)]
    for n_coeffs, m in ((1, 1), (255, 3), (256, 1), (257, 3), (1025, 2)):
        cols = rng.integers(0, p, (m, n_coeffs)).astype(np.uint32)
        w = o.ff_prim_nth_root_g(256, p, g)
        for S in (1, 2, 3, 4):
            out, za = np.zeros(4 * m * S, dtype=np.uint64), _u64(z)
            st = emu.emu_poly_eval_ext_shifts(p, g, cols.ctypes.data, m, n_coeffs, n_coeffs, za.ctypes.data, w, S, out.ctypes.data)
            assert st == 0
            pts = wc.shifts_of(z, w, S, p)
            for c in range(m):
                for s in range(S):
                    assert [int(v) for v in out[4 * (c * S + s):4 * (c * S + s) + 4]] == dc.horner([int(v) for v in cols[c]], pts[s], p, g), (n_coeffs, c, s)
            if S <= 2:
                old = np.zeros(4 * m * S, dtype=np.uint64)
                flat = _u64([v for pt in pts for v in pt])
                assert emu.emu_poly_eval_ext(p, g, cols.ctypes.data, m, n_coeffs, n_coeffs, flat.ctypes.data, S, old.ctypes.data) == 0
                assert np.array_equal(old, out)


def _codeword_inputs(o, W, D, S, log_n, lb, p, g, extreme, seed=3):
    rng = np.random.default_rng(seed + W + D + S)
    N = 1 << (log_n + lb)
    hi = p - 1
    lde = rng.integers(0, p, (W, N)).astype(np.uint32) if not extreme else np.full((W, N), hi, dtype=np.uint32)
    seg = rng.integers(0, p, (4 * D, N)).astype(np.uint32) if not extreme else np.full((4 * D, N), hi, dtype=np.uint32)
    cnt = 4 * (S * W + D)
    z = [int(v) for v in rng.integers(1, p, 4)]
    ood = [int(v) for v in rng.integers(0, p, cnt)] if not extreme else [hi] * cnt
    u = u64_set(p)
    ch = [int(v) for v in rng.integers(1 << 62, (1 << 64) - 1, cnt, dtype=np.uint64)] if not extreme else [u[(3 * i + seed) % len(u)] for i in range(cnt)]
    return lde, seg, z, ood, ch


def emu_window(emu, S, lde, seg, log_n, lb, z, ood, ch, p, g, h, grid=0, pad=0):
    from stark_rs_amd import _lib
    W, N = lde.shape
    stride = N + pad

    def spread(a):
        host = np.full(a.shape[0] * stride, 0x7fffffff, dtype=np.uint32)
        for c in range(a.shape[0]):
            host[c * stride:c * stride + N] = a[c]
        return host
    hl, hs, out = spread(lde), spread(seg), np.zeros(4 * stride, dtype=np.uint32)
    cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, h, 0, 1)
    za, oa, ca = _u64(z), _u64(ood), _u64(ch)   # named: the arrays must outlive the call
    st = emu.emu_deep_compose_window(p, g, C.byref(cfg), S, seg.shape[0] // 4, hl.ctypes.data, stride, hs.ctypes.data, stride, za.ctypes.data,
                                     oa.ctypes.data, ca.ctypes.data, out.ctypes.data, stride, grid)
    assert st == 0, st
    return np.stack([out[e * stride:e * stride + N] for e in range(4)]).astype(np.uint64)


@pytest.mark.parametrize("p,g", FIELDS)
@pytest.mark.parametrize("S", [2, 3, 4])
def test_emu_deep_compose_window(emu, oracle, p, g, S):
    o = oracle
    for log_N in (6, 7, 8):
        for lb, W, D in dc.compose_combos(log_N)[:2]:
            log_n = log_N - lb
            w = o.ff_prim_nth_root_g(1 << log_n, p, g)
            for extreme in (False, True):
                lde, seg, z, ood, ch = _codeword_inputs(o, W, D, S, log_n, lb, p, g, extreme)
                want = wc.q_codeword(lde, seg, dc.points(o, p, g, log_n, lb, g), z, ood, ch, w, S, p, g)
                if S == 2:
                    assert np.array_equal(want, dc.q_codeword(lde, seg, dc.points(o, p, g, log_n, lb, g), z, ood, ch, w, p, g))
                for grid, pad in ((0, 0), (1, 3)):
                    got = emu_window(emu, S, lde, seg, log_n, lb, z, ood, ch, p, g, g, grid, pad)
                    assert np.array_equal(got, want), (S, log_N, lb, W, D, extreme, grid, pad)
                # the verifier's Q at one point
                i = 5 % (1 << log_N)
                x = int(dc.points(o, p, g, log_n, lb, g)[i])
                out, za, oa, ca, ta, sa = np.zeros(4, dtype=np.uint64), _u64(z), _u64(ood), _u64(ch), _u64(lde[:, i]), _u64(seg[:, i])
                st = emu.emu_deep_q_at_window(p, g, W, D, S, w, x, za.ctypes.data, oa.ctypes.data, ca.ctypes.data, ta.ctypes.data, sa.ctypes.data,
                                              out.ctypes.data)
                assert st == 0 and [int(v) for v in out] == [int(v) for v in want[:, i]]


@pytest.mark.parametrize("p,g", FIELDS)
@pytest.mark.parametrize("name", ["fib1", "sq", "tap4", "wide"])
def test_emu_ood_sides_window(emu, oracle, name, p, g):
    """the verifier's consistency check at z: both sides equal the restatement's, and equal each other on an honest record"""
    from stark_rs_amd import _lib
    o = oracle
    log_n, lb, tau, h = 5, 3, 5, g
    air, cols = wc.make(name, 1 << log_n, p)
    W, K, S = len(cols), len(air.constraints), air.window
    _d, D = wc.plan(air, log_n)
    ch = xc.ext_weights_for(air)
    H = wc.compose_ext(o, air, cols, ch, p, g, log_n, lb, tau, h)
    hc, _seg = dc.segments(o, H, D, p, g, log_n, lb, h)
    z = [5, 7, 11, p - 1]
    ood = wc.ood_values(o, cols, hc, D, S, z, p, g, log_n, tau)
    lhs, rhs = wc.ood_sides(o, air, W, D, ch, z, ood, p, g, log_n, tau)
    assert lhs == rhs
    cfg = _lib.StarkCfg(log_n, lb, W, 1, tau, h, 0, 1)
    a = air.flatten(p)
    l, r, ca, za, oa = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64), _u64(ch), _u64(z), _u64(ood)
    st = emu.emu_deep_ood_sides(p, g, C.byref(cfg), C.byref(a), ca.ctypes.data, za.ctypes.data, oa.ctypes.data, l.ctypes.data, r.ctypes.data)
    assert st == 0 and [int(v) for v in l] == lhs and [int(v) for v in r] == rhs
    ood[4 * (2 * W)] = (ood[4 * (2 * W)] + 1) % p            # u_{2,0}
    oa = _u64(ood)
    st = emu.emu_deep_ood_sides(p, g, C.byref(cfg), C.byref(a), ca.ctypes.data, za.ctypes.data, oa.ctypes.data, l.ctypes.data, r.ctypes.data)
    assert st == 0 and [int(v) for v in l] != [int(v) for v in r]
