"""CPU: the lane bodies of the out-of-domain sampling kernels (csrc/deep_core.h), run by the emulator library with the
kernels' block split, and the verifier's host arithmetic, against the Python restatement (tests/deep_compose.py).  Every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import deep_compose as dc
import ext_compose as xc
from test_deep_host import quartic
from test_gpu_boundary_primes import GEN, THREE, u64_set

FIELDS = list(xc.PRIMES) + [(p, GEN[p]) for p in THREE]
ADICITY = {998244353: 23, 469762049: 26, 1073692673: 14, 536813569: 13, 536903681: 15}


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.emu_poly_eval_ext.argtypes = [u64, u64, vp, u32, u64, u64, vp, u32, vp]
    L.emu_deep_compose.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), u32, vp, u64, vp, u64, vp, vp, vp, vp, u64, u32]
    L.emu_deep_ood_sides.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), vp, vp, vp, vp, vp]
    L.emu_deep_constraint.argtypes = [u64, u64, C.POINTER(_lib.Air), u32, vp, u32, vp]
    L.emu_deep_q_at.argtypes = [u64, u64, u32, u32, u64, u64, vp, vp, vp, vp, vp, vp]
    return L


def _u64(v):
    return np.array([int(x) for x in v], dtype=np.uint64)


def emu_eval(emu, cols, points, p, g, stride=None):
    cols = np.asarray(cols, dtype=np.uint32)
    m, n = cols.shape
    stride = n if stride is None else stride
    host = np.full(m * stride, 0x7fffffff, dtype=np.uint32)
    for c in range(m):
        host[c * stride:c * stride + n] = cols[c]
    pts, out = _u64([v for pt in points for v in pt]), np.zeros(4 * m * len(points), dtype=np.uint64)
    st = emu.emu_poly_eval_ext(p, g, host.ctypes.data, m, n, stride, pts.ctypes.data, len(points), out.ctypes.data)
    assert st == 0, st
    return [[[int(out[4 * (c * len(points) + k) + e]) for e in range(4)] for k in range(len(points))] for c in range(m)]


def emu_compose(emu, lde, seg, log_n, lb, z, ood, ch, p, g, h, grid=0, pad=0):
    from stark_rs_amd import _lib
    lde, seg = np.asarray(lde, dtype=np.uint32), np.asarray(seg, dtype=np.uint32)
    W, N = lde.shape
    stride = N + pad

    def spread(a):
        host = np.full(a.shape[0] * stride, 0x7fffffff, dtype=np.uint32)
        for c in range(a.shape[0]):
            host[c * stride:c * stride + N] = a[c]
        return host
    hl, hs, out = spread(lde), spread(seg), np.full(4 * stride, 0xdeadbeef, dtype=np.uint32)
    cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, h, 0, 1)
    za, oa, ca = _u64(z), _u64(ood), _u64(ch)
    st = emu.emu_deep_compose(p, g, C.byref(cfg), seg.shape[0] // 4, hl.ctypes.data, stride, hs.ctypes.data, stride, za.ctypes.data, oa.ctypes.data,
                              ca.ctypes.data, out.ctypes.data, stride, grid)
    assert st == 0, st
    for e in range(4):
        assert np.all(out[e * stride + N:(e + 1) * stride] == 0xdeadbeef)
    return np.stack([out[e * stride:e * stride + N] for e in range(4)]).astype(np.uint64)


@pytest.mark.parametrize("p,g", FIELDS)
@pytest.mark.parametrize("n_coeffs", [1, 2, 63, 64, 65, 257, 4097])
def test_emulated_evaluation_equals_the_restatement(emu, p, g, n_coeffs):
    rng = np.random.default_rng(n_coeffs)
    cols = rng.integers(0, p, (3, n_coeffs), dtype=np.uint64)
    cols[1] = p - 1
    z, top = [int(v) for v in rng.integers(0, p, 4)], [p - 1] * 4
    for pts in ([z], [z, dc.scale_q(z, 5, p)], [top, top]):
        want = [[dc.eval_cols(cols, pt, p, g)[c] for pt in pts] for c in range(3)]
        assert emu_eval(emu, cols, pts, p, g) == want
        assert emu_eval(emu, cols, pts, p, g, stride=n_coeffs + 3) == want
    if n_coeffs <= 257:                                                      # Horner itself, where Python ints reach
        assert emu_eval(emu, cols, [z], p, g) == [[dc.horner([int(v) for v in c], z, p, g)] for c in cols]


def compose_inputs(p, W, D, N, kind, seed=1):
    """-> (lde, seg, z, ood, ch): random, or every operand p - 1 under challenges of the u64 set"""
    rng = np.random.default_rng(seed)
    cnt = 4 * (2 * W + D)
    if kind == "extreme":
        u = u64_set(p)
        return (np.full((W, N), p - 1, dtype=np.uint64), np.full((4 * D, N), p - 1, dtype=np.uint64), [p - 1] * 4, [p - 1] * cnt,
                [u[(3 * i + seed) % len(u)] for i in range(cnt)])
    return (rng.integers(0, p, (W, N), dtype=np.uint64), rng.integers(0, p, (4 * D, N), dtype=np.uint64), [int(v) for v in rng.integers(1, p, 4)],
            [int(v) for v in rng.integers(0, p, cnt)], [int(v) for v in rng.integers(1 << 62, (1 << 64) - 1, cnt, dtype=np.uint64)])


@pytest.mark.parametrize("p,g", FIELDS)
@pytest.mark.parametrize("log_N", range(6, 11))
def test_emulated_compose_equals_the_restatement(emu, oracle, p, g, log_N):
    """every B and every D at every size (D need not fit B for the point function), W rotating through 1, 4, 12, 64"""
    N = 1 << log_N
    for k, (lb, D) in enumerate([(2, 1), (3, 2), (4, 4), (2, 16), (3, 16), (4, 1)]):
        W = [1, 4, 12, 64][(k + log_N) % 4]
        log_n = log_N - lb
        w, _wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
        x = dc.points(oracle, p, g, log_n, lb, g)
        for kind in ("random", "extreme"):
            lde, seg, z, ood, ch = compose_inputs(p, W, D, N, kind, seed=k)
            want = dc.q_codeword(lde, seg, x, z, ood, ch, w, p, g)
            assert np.array_equal(emu_compose(emu, lde, seg, log_n, lb, z, ood, ch, p, g, g), want), (lb, D, W, kind)
        assert np.array_equal(emu_compose(emu, lde, seg, log_n, lb, z, ood, ch, p, g, g, grid=1, pad=3), want)   # the grid-stride loop
        for i in (0, N - 1):                                                 # ... and the verifier's point function
            got = np.zeros(4, dtype=np.uint64)
            za, oa, ca, tr, sr = _u64(z), _u64(ood), _u64(ch), _u64(lde[:, i]), _u64(seg[:, i])
            assert emu.emu_deep_q_at(p, g, W, D, w, int(x[i]), za.ctypes.data, oa.ctypes.data, ca.ctypes.data, tr.ctypes.data, sr.ctypes.data,
                                     got.ctypes.data) == 0
            assert [int(v) for v in got] == [int(v) for v in want[:, i]]


@pytest.mark.parametrize("p,g", FIELDS)
def test_the_constraint_evaluator_over_f_q_on_embedded_operands_is_the_mirror_s(emu, p, g):
    rng = np.random.default_rng(2)
    n = 64
    for name, (air, cols) in (("mixer", ac.make("mixer", n, p)), ("mimc", ap.make("mimc", n, p)), ("switch", ap.make("switch", n, p)),
                              ("quartic", quartic(n, p)), ("synthetic", ap.synthetic(4, 3, 5, p, n))):
        W, Q = air.n_cols, len(air.periodics)
        flat = air.flatten(p)
        for trial in range(3):
            vals = [p - 1] * (2 * W + 2 * Q) if trial == 0 else [int(v) for v in rng.integers(0, p, 2 * W + 2 * Q)]
            ops = _u64([c for v in vals for c in (v, 0, 0, 0)])
            for k in range(len(air.constraints)):
                out = np.zeros(4, dtype=np.uint64)
                assert emu.emu_deep_constraint(p, g, C.byref(flat), k, ops.ctypes.data, 2 * W + 2 * Q, out.ctypes.data) == 0
                want = air.constraint_value(k, p, vals[:W], vals[W:2 * W], vals[2 * W:2 * W + Q], vals[2 * W + Q:])
                assert [int(v) for v in out] == [want, 0, 0, 0], (name, k)
            # ... and on operands outside the base field it is the restatement's
            xs = [[int(v) for v in rng.integers(0, p, 4)] for _ in range(2 * W + 2 * Q)]
            ops = _u64([c for el in xs for c in el])
            for k in range(len(air.constraints)):
                out = np.zeros(4, dtype=np.uint64)
                assert emu.emu_deep_constraint(p, g, C.byref(flat), k, ops.ctypes.data, 2 * W + 2 * Q, out.ctypes.data) == 0
                assert [int(v) for v in out] == dc.constraint_q(air, k, xs, p, g), (name, k)


@pytest.mark.parametrize("p,g", FIELDS)
def test_the_consistency_check_holds_for_an_honest_record_and_is_the_restatement_s(emu, oracle, p, g):
    from stark_rs_amd import _lib
    log_n, t = 6, 2
    for name, (air, cols), lb in (("fib", ac.make("fib", 64, p), 3), ("mimc", ap.make("mimc", 64, p), 2), ("public", ap.make("public", 64, p), 3),
                                  ("quartic", quartic(64, p), 3)):
        if log_n + lb > ADICITY[p]:
            continue
        W, K = len(cols), len(air.constraints)
        _d, D = dc.plan(air)
        res = dc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g)
        _tr, weights = xc.air_transcript(oracle, W, K, res["roots"][0])
        cfg, flat = _lib.StarkCfg(log_n, lb, W, 1, 1, g, t, 1), air.flatten(p)
        for ood, same in ((res["ood"], True), (res["ood"][:5] + [(res["ood"][5] + 1) % p] + res["ood"][6:], False)):
            lhs, rhs = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
            wa, za, oa = _u64(weights), _u64(res["z"]), _u64(ood)
            assert emu.emu_deep_ood_sides(p, g, C.byref(cfg), C.byref(flat), wa.ctypes.data, za.ctypes.data, oa.ctypes.data, lhs.ctypes.data,
                                          rhs.ctypes.data) == 0
            want = dc.ood_sides(oracle, air, W, D, weights, res["z"], ood, p, g, log_n, 1)
            assert ([int(v) for v in lhs], [int(v) for v in rhs]) == want, name
            assert (want[0] == want[1]) == same, name


def test_the_point_function_cases_cover_every_value_and_run_in_the_emulator(emu, oracle):
    """dc.compose_combos, which the GPU tests take their shapes from: every B, W and D over the sizes 2^10 .. 2^16; the five
    combinations of 2^10 through the emulated kernel"""
    seen = [set(), set(), set()]
    for log_N in range(10, 17):
        for combo in dc.compose_combos(log_N):
            for s, v in zip(seen, combo):
                s.add(v)
    assert seen == [{2, 3, 4}, {1, 4, 12, 64}, {1, 2, 4, 16}]
    p, g = xc.PRIMES[1]
    for k, (lb, W, D) in enumerate(dc.compose_combos(10)):
        w, _wN = ac.roots_of_unity(oracle, p, g, 10 - lb, lb)
        lde, seg, z, ood, ch = compose_inputs(p, W, D, 1 << 10, "random", seed=k)
        want = dc.q_codeword(lde, seg, dc.points(oracle, p, g, 10 - lb, lb, g), z, ood, ch, w, p, g)
        assert np.array_equal(emu_compose(emu, lde, seg, 10 - lb, lb, z, ood, ch, p, g, g), want), (lb, W, D)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_the_numpy_helpers_equal_python_int_arithmetic_and_the_emulator(emu, p, g):
    """eval_cols (halving) against Horner on Python ints and against the emulated kernels; inv_vec and _mul_const against
    xc.inv and xc.mul, and through them q_codeword against the verifier's point function (emu_deep_q_at)"""
    rng = np.random.default_rng(3)
    z = [int(v) for v in rng.integers(0, p, 4)]
    for n in (1, 2, 3, 63, 64, 65, 257):
        cols = rng.integers(0, p, (3, n), dtype=np.uint64)
        cols[2] = p - 1
        for pt in (z, [p - 1] * 4):
            got = dc.eval_cols(cols, pt, p, g)
            assert got == [dc.horner([int(v) for v in c], pt, p, g) for c in cols], n
            assert [[v] for v in got] == emu_eval(emu, cols, [pt], p, g), n
    a = rng.integers(0, p, (4, 9), dtype=np.uint64)
    a[:, 0], a[1:, 1], a[:, 2] = p - 1, 0, [0, 1, 0, 0]
    got = dc.inv_vec(a, p, g)
    for i in range(9):
        assert [int(v) for v in got[:, i]] == xc.inv([int(v) for v in a[:, i]], p, g), i
    b = [int(v) for v in rng.integers(0, p, 4)]
    got = dc._mul_const(a, b, p, g)
    for i in range(9):
        assert [int(v) for v in got[:, i]] == xc.mul([int(v) for v in a[:, i]], b, p, g)
    W, D, N, w = 3, 2, 16, 5
    lde, seg, zz, ood, ch = compose_inputs(p, W, D, N, "random", seed=9)
    x = rng.integers(1, p, N, dtype=np.uint64)
    Q = dc.q_codeword(lde, seg, x, zz, ood, ch, w, p, g)
    for i in range(N):
        out = np.zeros(4, dtype=np.uint64)
        za, oa, ca, tr, sr = _u64(zz), _u64(ood), _u64(ch), _u64(lde[:, i]), _u64(seg[:, i])
        assert emu.emu_deep_q_at(p, g, W, D, w, int(x[i]), za.ctypes.data, oa.ctypes.data, ca.ctypes.data, tr.ctypes.data, sr.ctypes.data, out.ctypes.data) == 0
        assert [int(v) for v in out] == [int(v) for v in Q[:, i]] == dc.q_at(lde[:, i], seg[:, i], int(x[i]), zz, ood, ch, w, p, g), i


def _cases(p):
    yield "fib", ac.make("fib", 64, p), 3
    yield "mimc", ap.make("mimc", 64, p), 2
    yield "quartic", quartic(64, p), 3


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_the_restated_prover_and_verifier_agree_with_each_other_and_the_emulator(emu, oracle, p, g):
    """an honest restated proof is accepted by the restated verifier, has the formula's length and the library's layout
    length, its out-of-domain values and its Q are what the emulated kernels compute from its columns, deg Q < n, and every
    defect below is rejected for its own reason"""
    from test_deep_host import plan as lib_plan
    log_n, t = 6, 4
    for name, (air, cols), lb in _cases(p):
        W, N, n = len(cols), 1 << (log_n + lb), 1 << log_n
        _d, D = dc.plan(air)
        res = dc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g)
        proof, roots = res["proof"], res["roots"]
        assert len(proof) == dc.proof_len(oracle, W, D, log_n, lb, t, p, g, g) == lib_plan(p, g, air, W, log_n, lb, t)[2], name
        assert dc.verify(oracle, air, proof, roots, p, g, W, log_n, lb, t, 1, g) == (True, ""), name
        w, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
        # the emulated kernels on the restatement's columns: u and v from the trace coefficients, Q from the columns
        polys = np.stack([np.asarray(oracle.fast_intt(np.array(c, dtype=np.uint64), w, 1, p), dtype=np.uint64) for c in cols])
        got = emu_eval(emu, polys, [res["z"], dc.scale_q(res["z"], w, p)], p, g)
        assert [c for k in range(2) for col in got for c in col[k]] == res["ood"][:8 * W], name
        assert np.array_equal(emu_compose(emu, np.array(res["lde"]), res["seg"], log_n, lb, res["z"], res["ood"], res["gammas"], p, g, g), res["Q"]), name
        for i in (0, 1, N // 2 + 3, N - 1):
            want = dc.q_at([int(c[i]) for c in res["lde"]], [int(c[i]) for c in res["seg"]], g * pow(wN, i, p) % p, res["z"], res["ood"], res["gammas"], w, p, g)
            assert [int(v) for v in res["Q"][:, i]] == want, (name, i)
        coeffs = [oracle.fast_intt(res["Q"][e], wN, g, p) for e in range(4)]
        assert not any(np.asarray(c)[n:].any() for c in coeffs), name      # deg Q < n
        bad = bytearray(proof)
        bad[9 + 8 * 5] ^= 1                                                 # coordinate 1 of u_1 or v_0
        assert dc.verify(oracle, air, bytes(bad), roots, p, g, W, log_n, lb, t, 1, g) == (False, "consistency"), name
        bad = bytearray(proof)
        bad[9:17] = xc._u64(int.from_bytes(proof[9:17], "little") + p)
        assert dc.verify(oracle, air, bytes(bad), roots, p, g, W, log_n, lb, t, 1, g) == (False, "record canonical"), name
        bad = bytearray(proof)
        bad[1] ^= 1
        assert dc.verify(oracle, air, bytes(bad), roots, p, g, W, log_n, lb, t, 1, g) == (False, "record"), name
        assert dc.verify(oracle, air, proof, roots[::-1], p, g, W, log_n, lb, t, 1, g) == (False, "consistency"), name
        bad = bytearray(proof)
        bad[-5] ^= 1
        assert dc.verify(oracle, air, bytes(bad), roots, p, g, W, log_n, lb, t, 1, g) == (False, "auth"), name
        assert dc.verify(oracle, air, proof[:-1], roots, p, g, W, log_n, lb, t, 1, g) == (False, "length"), name
    # a trace that violates the AIR in one cell: the composition is no polynomial of degree < D n
    air, cols = ac.make("fib", 64, p)
    cols = [list(c) for c in cols]
    cols[1][17] = (cols[1][17] + 1) % p
    with pytest.raises(AssertionError):
        dc.prove(oracle, air, cols, p, g, log_n, 3, t, 1, g)
