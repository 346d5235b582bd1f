"""CPU: the quartic-extension kernels' own per-element code (csrc/fri_core.h fold_element_ext, csrc/air_core.h
air_compose_points_ext), run by the emulator library with the kernels' indexing, against the Python restatement
(tests/ext_compose.py) and against the base-field emulator coordinate by coordinate."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import air_rows as ar
import ext_compose as xc

U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp = C.c_void_p
    L.emu_fold_ext.argtypes = [C.c_uint64, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64]
    L.emu_fs_rounds_ext.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_uint32, vp]
    L.emu_fs_rounds_ext.restype = C.c_uint64
    L.emu_air_compose.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), vp, C.c_uint64, vp, vp, C.c_int]
    L.emu_air_compose_ext.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), vp, C.c_uint64, vp, vp,
                                      C.c_uint64, C.c_int]
    return L


def emu_fold(emu, cw, alpha, offset, omega, p, g, stride=None, out_stride=None):
    L = cw.shape[1]
    stride = L if stride is None else stride
    out_stride = L // 2 if out_stride is None else out_stride
    buf = np.full(4 * stride, 0xdeadbeef, dtype=np.uint32)
    for e in range(4):
        buf[e * stride:e * stride + L] = cw[e]
    out = np.full(4 * out_stride, 0xdeadbeef, dtype=np.uint32)
    al = np.array(alpha, dtype=np.uint64)
    assert emu.emu_fold_ext(p, g, buf.ctypes.data, L, stride, al.ctypes.data, offset, omega, out.ctypes.data, out_stride) == 0
    got = np.stack([out[e * out_stride:e * out_stride + L // 2] for e in range(4)]).astype(np.uint64)
    for e in range(4):   # nothing written between the columns
        assert np.all(out[e * out_stride + L // 2:(e + 1) * out_stride] == 0xdeadbeef)
    return got


def alphas(p):
    return [[U64_MAX] * 4, [p, p + 1, U64_MAX - 1, 2 * p - 1], [0, 0, 0, 0], [5, 0, 0, 0], [0, 0, 0, 1], [1 << 63, 12345, p - 1, 1 << 32]]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_len", range(1, 13))
def test_emu_fold_ext_equals_the_restatement(oracle, emu, p, g, log_len):
    L = 1 << log_len
    rng = np.random.default_rng(log_len)
    cw = rng.integers(0, p, (4, L), dtype=np.uint64)
    cw[:, 0] = p - 1                                       # all coordinates p - 1 among the operands
    cw[:, L // 2] = [0, p - 1, 0, p - 1]
    omega, offset = oracle.ff_prim_nth_root_g(L, p, g), [g, 7, 1][log_len % 3]
    for al in alphas(p)[:3] + [alphas(p)[3 + log_len % 3]]:
        want = xc.fold(cw, al, offset, omega, p, g)
        assert np.array_equal(emu_fold(emu, cw, al, offset, omega, p, g), want), al
    al = alphas(p)[1]
    assert np.array_equal(emu_fold(emu, cw, al, offset, omega, p, g, stride=L + 3, out_stride=L // 2 + 5), xc.fold(cw, al, offset, omega, p, g))


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_fold_restatement_is_the_definition_element_by_element(oracle, p, g):
    """the vectorised restatement against scalar F_q arithmetic, and a base-field alpha folds every coordinate as
    Fri::fold_codeword does"""
    L = 64
    rng = np.random.default_rng(3)
    cw = rng.integers(0, p, (4, L), dtype=np.uint64)
    omega, offset = oracle.ff_prim_nth_root_g(L, p, g), g
    al = [U64_MAX, p + 3, 17, U64_MAX - 5]
    got = xc.fold(cw, al, offset, omega, p, g)
    inv2 = pow(2, -1, p)
    for i in range(L // 2):
        lo, hi = [int(v) for v in cw[:, i]], [int(v) for v in cw[:, i + L // 2]]
        xi = pow(offset * pow(omega, i, p) % p, -1, p)
        want = xc.add(xc.scale(xc.add(lo, hi, p), inv2, p), xc.mul([a % p for a in al], xc.scale(xc.sub(lo, hi, p), inv2 * xi % p, p), p, g), p)
        assert [int(v) for v in got[:, i]] == want, i
    a0 = 0xfedcba9876543210
    got = xc.fold(cw, [a0, 0, 0, 0], offset, omega, p, g)
    cfg = oracle.fri_cfg(omega, offset, L, 4, 1, p)
    for e in range(4):
        assert np.array_equal(got[e], np.asarray(oracle.fri_fold_codeword(cfg, cw[e], a0, offset, omega), dtype=np.uint64))


def _emu_compose_pair(emu, air, lde, ch, p, g, log_n, lb, tau, h, direct):
    """-> (the four coordinates from emu_air_compose_ext, the four base-field codewords from emu_air_compose)"""
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    cols = np.ascontiguousarray(np.stack(lde).astype(np.uint32))
    cfg, a = _lib.StarkCfg(log_n, lb, len(lde), 0, tau, h, 0, 1), air.flatten(p)
    out_stride = N + 4
    out = np.full(4 * out_stride, 0xdeadbeef, dtype=np.uint32)
    w = np.array(ch, dtype=np.uint64)
    st = emu.emu_air_compose_ext(p, g, C.byref(cfg), C.byref(a), cols.ctypes.data, N, w.ctypes.data, out.ctypes.data, out_stride, 1 if direct else 0)
    assert st == 0, st
    got = [out[e * out_stride:e * out_stride + N].copy() for e in range(4)]
    assert all(np.all(out[e * out_stride + N:(e + 1) * out_stride] == 0xdeadbeef) for e in range(4))
    want = []
    for e in range(4):
        we, o1 = np.array(xc.weight_vector(ch, e), dtype=np.uint64), np.zeros(N, dtype=np.uint32)
        assert emu.emu_air_compose(p, g, C.byref(cfg), C.byref(a), cols.ctypes.data, N, we.ctypes.data, o1.ctypes.data, 1 if direct else 0) == 0
        want.append(o1)
    return got, want


def _airs(p, n):
    yield "fib", ac.make("fib", n, p)
    yield "mixer", ac.make("mixer", n, p)
    yield "empty", ac.make("empty", n, p)
    yield "mimc", ap.make("mimc", n, p)
    yield "public", ap.make("public", n, p)
    yield "wide64", ar.wide(64, 20, p, n)
    yield "wide20", ar.wide(20, 8, p, n)      # twenty tile rows: T = 512, two points per thread (emu_tiles_ext<2>)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("log_n,lb,tau,h", [(7, 3, 1, None), (6, 4, 5, 7)])
def test_emu_compose_ext_coordinate_e_is_the_base_composition_under_weights_e(oracle, emu, p, g, direct, log_n, lb, tau, h):
    h = g if h is None else h
    for name, (air, cols) in _airs(p, 1 << log_n):
        ch = xc.ext_weights_for(air)
        ch[0], ch[5] = U64_MAX, p                          # an extreme and a zero weight coordinate
        lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
        got, want = _emu_compose_pair(emu, air, lde, ch, p, g, log_n, lb, tau, h, direct)
        for e in range(4):
            assert np.array_equal(got[e], want[e]), (name, e)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_emu_compose_ext_equals_the_polynomial_route(oracle, emu, p, g):
    """not only equal to the sibling emulator: coordinate e is the oracle's polynomial-route codeword under weights e"""
    log_n, lb, tau, h = 5, 3, 5, 7
    air, cols = ac.make("mixer", 1 << log_n, p)
    ch = xc.ext_weights_for(air)
    lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
    got, _ = _emu_compose_pair(emu, air, lde, ch, p, g, log_n, lb, tau, h, False)
    for e in range(4):
        want, _ = ac.codeword_poly_route(oracle, air, cols, xc.weight_vector(ch, e), p, g, log_n, lb, tau, h)
        assert np.array_equal(got[e].astype(np.uint64), np.asarray(want, dtype=np.uint64)), e


@pytest.mark.parametrize("prefix_len", [0, 5, 8, 24, 31, 32, 37, 64, 100])
def test_emu_transcript_rounds_equal_the_restatement(oracle, emu, prefix_len):
    """the four-lane Fiat-Shamir round of fs_round_ext_kernel (hash_core.h fs_round_ext_lane) at every kind of phase: a
    counter that fits the pending chunk, one that completes it, one that straddles two"""
    rng = np.random.default_rng(prefix_len)
    prefix = bytes(rng.integers(0, 256, prefix_len, dtype=np.uint8))
    R = 5
    roots = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(R)]
    alphas = np.zeros(4 * (R - 1), dtype=np.uint64)
    seed_ch = emu.emu_fs_rounds_ext(prefix, prefix_len, b"".join(roots), R, alphas.ctypes.data)
    tr, want = bytearray(prefix), []
    for r in range(R):
        tr += roots[r]
        if r < R - 1:
            want += xc.round_alpha(oracle, tr)
    assert [int(a) for a in alphas] == want
    assert seed_ch == xc.challenge(oracle, tr)
    assert len(tr) == prefix_len + 32 * R + 32 * (R - 1)


def test_the_tile_choices_of_the_test_airs_cover_every_points_per_thread():
    """what air_tile (air_core.h) picks for the shapes above: P = 4, 2 and 1 are all run by the comparisons in this file"""
    def tile(rows, B, N, weight_vecs=4):
        for T in (1024, 512, 256, 128, 64):
            if T <= N and rows * (T + B) * 4 + weight_vecs * 128 * 4 <= 65536:
                return T, T // min(T, 256)
        return 0, 0
    assert tile(4, 8, 1024) == (1024, 4) and tile(20, 8, 1024) == (512, 2) and tile(64, 8, 1024) == (128, 1)
    assert tile(20, 16, 1024) == (512, 2)
