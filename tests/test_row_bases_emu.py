"""CPU: the address forms and the unmasked step-twiddle indices of the NTT passes (csrc/ntt_core.h) through the emulator, which is
built with SMI_EMU_CHECKS -- every running twiddle index is asserted to stay inside its table -- at the shapes of
tests/test_gpu_ntt_row_bases.py up to 2^21, and the bound of the indices checked directly for every step of Steps<>."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ntt_matrix as nm

u32p = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd as s
    s.build()
    from stark_rs_amd._lib import EMU_PATH as path
    L = C.CDLL(path)
    L.emu_ntt.argtypes = [C.c_uint64, C.c_uint64, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                          C.c_int, C.c_uint64, C.c_uint64]
    return L


def _leg(batch, inverse, offset, post=1, nin=(0, 0)):
    return {"batch": batch, "inverse": inverse, "offset": offset, "post": post, "nin": nin, "strided": False, "inplace": False}


def _emu(emu, prime, L, leg, cols, in_gap=0, out_gap=0):
    p, g, _ = nm.PRIMES[prime]
    n, batch = 1 << L, leg["batch"]
    si, so = n + in_gap, n + out_gap
    x = np.full(batch * si, nm.SENTINEL, dtype=np.uint32)
    for i, c in enumerate(cols):
        x[i * si:i * si + n] = nm.column(p, L, c)
    out = np.full(batch * so, nm.SENTINEL, dtype=np.uint32)
    rc = emu.emu_ntt(p, g, x.ctypes.data_as(u32p), out.ctypes.data_as(u32p), L, nm.n_in_of(leg, n), batch, si, so,
                     1 if leg["inverse"] else 0, leg["offset"], leg["post"])
    assert rc == 0
    out = out.reshape(batch, so)
    assert (out[:, n:] == nm.SENTINEL).all(), "a store left its column"
    return out[:, :n].astype(np.uint64)


@pytest.mark.parametrize("prime", ["ref", "p2"])
def test_emulated_two_pass_plan_with_column_strides(emu, oracle, prime):
    for leg in (_leg(3, False, 5), _leg(3, True, 3, 5)):
        got = _emu(emu, prime, 13, leg, (0, 1, 2), in_gap=32, out_gap=64)
        for c in range(3):
            assert np.array_equal(got[c], nm.oracle_column(oracle, prime, 13, leg, c))


@pytest.mark.parametrize("prime", ["ref", "p2"])
def test_emulated_three_pass_plan_column_groups_of_four_and_one(emu, oracle, prime):
    leg = _leg(5, False, 5)
    emu.emu_set_share_cols(2)
    try:
        got = _emu(emu, prime, 21, leg, range(5))
    finally:
        emu.emu_set_share_cols(1)
    for c in range(5):
        assert np.array_equal(got[c], nm.oracle_column(oracle, prime, 21, leg, c))


@pytest.mark.parametrize("prime", ["ref", "p2"])
def test_emulated_extension(emu, oracle, prime):
    o = oracle
    p, g, _ = nm.PRIMES[prime]
    logn, lb = 13, 3
    n, N = 1 << logn, 1 << (logn + lb)
    inv = _leg(3, True, 1, g)                       # coefficients scaled by the coset offset's powers
    coef = _emu(emu, prime, logn, inv, (0, 2, 5))
    x = np.ascontiguousarray(coef.reshape(-1), dtype=np.uint32)
    out = np.zeros(3 * N, dtype=np.uint32)
    assert emu.emu_ntt(p, g, x.ctypes.data_as(u32p), out.ctypes.data_as(u32p), logn + lb, n, 3, n, N, 0, 1, 1) == 0
    w, Wn = o.ff_prim_nth_root_g(n, p, g), o.ff_prim_nth_root_g(N, p, g)
    for i, c in enumerate((0, 2, 5)):
        want = o.fast_coset_ntt(o.fast_intt(nm.column(p, logn, c), w, 1, p), N, Wn, g, p)
        assert np.array_equal(out.reshape(3, N)[i].astype(np.uint64), want), (prime, c)


def _steps():
    """Steps<LOGR> of csrc/ntt_core.h -> {LOGR: (s0, s1, s2)}"""
    with open(os.path.join(nm.ROOT, "stark_rs_amd", "csrc", "ntt_core.h")) as f:
        text = f.read()
    out = {int(m.group(1)): tuple(int(v) for v in m.group(2, 3, 4))
           for m in re.finditer(r"struct Steps<(\d+)>\s*\{ enum \{ n = \d, s0 = (\d+), s1 = (\d+), s2 = (\d+) \}", text)}
    assert out and all(sum(s) == lr and s[0] == 4 for lr, s in out.items())
    return out


def test_step_twiddle_indices_need_no_mask():
    """every step that multiplies by step twiddles -- step 0 (S = 4, MLOG = LOGR) and the middle step of a three-step tile
    (S = s1, MLOG = LOGR - 4) -- for all pos < 2^(MLOG - S) and kk < 2^S: the masked index of the table of R entries is the
    plain product, which is what the running sum pos, 2 pos, 3 pos, ... reaches"""
    for logr, (s0, s1, s2) in sorted(_steps().items()):
        R = 1 << logr
        cases = [(s0, logr)] + ([(s1, logr - s0)] if s2 else [])
        for S, mlog in cases:
            pos = np.arange(1 << (mlog - S), dtype=np.uint64)[:, None]
            kk = np.arange(1 << S, dtype=np.uint64)[None, :]
            plain = (pos * kk) << np.uint64(logr - mlog)
            assert np.array_equal(plain & np.uint64(R - 1), plain), (logr, S, mlog)
            assert int(plain.max()) < R
            running = np.cumsum(np.broadcast_to(pos << np.uint64(logr - mlog), plain.shape), axis=1, dtype=np.uint64) - (pos << np.uint64(logr - mlog))
            assert np.array_equal(running, plain), (logr, S, mlog)
