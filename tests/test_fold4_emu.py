"""CPU: the fold-by-4 kernel's lane body (csrc/fri_core.h fold4_element_ext), run by the emulator library with both of the
kernel's batchings, against the Lagrange restatement (tests/fold4_compose.py): every length 4 .. 2^10, operands on the
bounds, the project primes and the boundary moduli of tests/test_gpu_boundary_primes.py."""
import ctypes as C

import numpy as np
import pytest

import ext_compose as xc
import fold4_compose as f4
from test_gpu_boundary_primes import GEN, LARGE, u64_set

U64_MAX = (1 << 64) - 1
FILL = 0xdeadbeef


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp = C.c_void_p
    L.emu_fold4_ext.argtypes = [C.c_uint64, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_int]
    L.emu_fold4_layout.argtypes = [C.POINTER(_lib.FriCfg), vp]
    L.emu_fold4_layout.restype = None
    return L


def emu_fold4(emu, cw, alpha, offset, omega, p, g, vec, stride=None, out_stride=None):
    L = cw.shape[1]
    q = L // 4
    stride = L if stride is None else stride
    out_stride = q if out_stride is None else out_stride
    buf = np.full(4 * stride, FILL, dtype=np.uint32)
    for e in range(4):
        buf[e * stride:e * stride + L] = cw[e]
    out = np.full(4 * out_stride, FILL, dtype=np.uint32)
    al = np.array(alpha, dtype=np.uint64)
    assert emu.emu_fold4_ext(p, g, buf.ctypes.data, L, stride, al.ctypes.data, offset, omega, out.ctypes.data, out_stride, vec) == 0
    for e in range(4):   # nothing written between the columns
        assert np.all(out[e * out_stride + q:(e + 1) * out_stride] == FILL)
    return np.stack([out[e * out_stride:e * out_stride + q] for e in range(4)]).astype(np.uint64)


def batchings(L):
    return (0, 1) if L >= 16 else (0,)   # the 16-byte variant wants q = L / 4 a multiple of 4


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_len", range(2, 11))
def test_emu_fold4_equals_the_restatement(oracle, emu, p, g, log_len):
    L = 1 << log_len
    rng = np.random.default_rng(log_len)
    cw = rng.integers(0, p, (4, L), dtype=np.uint64)
    cw[:, 0] = p - 1
    cw[:, L // 4] = [0, p - 1, 0, p - 1]
    omega, offset = oracle.ff_prim_nth_root_g(L, p, g), [g, 7, 1][log_len % 3]
    for al in ([U64_MAX] * 4, [p, p + 1, U64_MAX - 1, 2 * p - 1], [[0] * 4, [5, 0, 0, 0], [1 << 63, 12345, p - 1, 1 << 32]][log_len % 3]):
        want = f4.fold4(cw, al, offset, omega, p, g)
        for vec in batchings(L):
            assert np.array_equal(emu_fold4(emu, cw, al, offset, omega, p, g, vec), want), (al, vec)
    top = np.full((4, L), p - 1, dtype=np.uint64)          # every coordinate p - 1, every alpha coordinate 2^64 - 1
    want = f4.fold4(top, [U64_MAX] * 4, offset, omega, p, g)
    for vec in batchings(L):
        assert np.array_equal(emu_fold4(emu, top, [U64_MAX] * 4, offset, omega, p, g, vec), want), vec
    al = [3, U64_MAX, p - 1, 1 << 32]                       # strides wider than the codeword: odd for the 4-byte variant
    want = f4.fold4(cw, al, offset, omega, p, g)
    assert np.array_equal(emu_fold4(emu, cw, al, offset, omega, p, g, 0, stride=L + 3, out_stride=L // 4 + 5), want)
    if L >= 16:
        assert np.array_equal(emu_fold4(emu, cw, al, offset, omega, p, g, 1, stride=L + 8, out_stride=L // 4 + 4), want)


@pytest.mark.parametrize("p", LARGE)
def test_emu_fold4_at_the_boundary_moduli(oracle, emu, p):
    g = GEN[p]
    for L in (4, 16, 1 << 8):
        omega = oracle.ff_prim_nth_root_g(L, p, g)
        rng = np.random.default_rng(L)
        for cw in (np.full((4, L), p - 1, dtype=np.uint64), rng.integers(0, p, (4, L), dtype=np.uint64),
                   np.resize(np.array([0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2], dtype=np.uint64), (4, L))):
            for al in ([p - 1] * 4, u64_set(p)[5:9], [U64_MAX] * 4):
                want = f4.fold4(cw, al, g, omega, p, g)
                for vec in batchings(L):
                    assert np.array_equal(emu_fold4(emu, cw, al, g, omega, p, g, vec), want), (L, al, vec)


def test_emu_fold4_refuses_what_the_launcher_refuses(emu):
    p, g = xc.PRIMES[0]
    buf = np.zeros(64, dtype=np.uint32)
    al = np.zeros(4, dtype=np.uint64)
    for L, stride, out_stride, vec in [(2, 2, 1, 0), (12, 12, 3, 0), (16, 15, 4, 0), (16, 16, 3, 0)]:
        assert emu.emu_fold4_ext(p, g, buf.ctypes.data, L, stride, al.ctypes.data, 3, 5, buf.ctypes.data, out_stride, vec) == -1
    assert emu.emu_fold4_ext(p, g, buf.ctypes.data, 8, 8, al.ctypes.data, 3, 5, buf.ctypes.data, 2, 1) == -2   # q = 2: no 16-byte variant


def test_emu_layout_export_equals_the_restatement(emu):
    from stark_rs_amd import _lib
    for ln in range(3, 15):
        for E in (4, 8, 16):
            for t in (1, 2, 5, 32):
                cfg, out = _lib.FriCfg(1, 1, 1 << ln, E, t), np.zeros(4, dtype=np.uint64)
                emu.emu_fold4_layout(C.byref(cfg), out.ctypes.data)
                assert tuple(int(v) for v in out) == f4.layout(1 << ln, E, t), (ln, E, t)
