"""CPU: a plain argument list runs the operand list's code (csrc/xargs_core.h XArgsOfPlain in front of the column build and the
streaming launch).  For every list of tests/test_args_emu.py the plain entry points of the emulator -- their own checks, then
the conversion -- and the operand list's entry points over the same list flattened in Python give the same words.  Both sides
stand against the restatement in their own files (test_args_emu.py, test_xargs_emu.py); every comparison is exact."""
import numpy as np
import pytest

import air_compose as ac
import args_compose as agc
import ext_compose as xc
from test_args_emu import LISTS, SPECS, case, emu_columns as plain_columns, emu_compose as plain_compose, pooled
from test_lookup_emu import chall
from test_xargs_emu import emu_columns as operand_columns, emu_compose as operand_compose

U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def emu():
    """the emulator with the four entry points declared as tests/test_args_emu.py and tests/test_xargs_emu.py declare them"""
    import ctypes as C
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    for fn, lst in ((L.emu_args_columns, _lib.AirArgs), (L.emu_xargs_columns, _lib.AirXArgs)):
        fn.argtypes = [u64, u64] + ([C.POINTER(_lib.Air)] if lst is _lib.AirXArgs else []) + [C.POINTER(lst), vp, u32, u32, vp, vp, u64, C.POINTER(u32), C.POINTER(u64)]
    for fn, lst in ((L.emu_air_compose_args, _lib.AirArgs), (L.emu_air_compose_xargs, _lib.AirXArgs)):
        fn.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.POINTER(lst), vp, u64, vp, u64, vp, vp, vp, u64, C.c_int, u32]
    return L


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("log_n", [1, 2, 5])
def test_both_routes_build_the_same_columns(emu, p, g, log_n, name):
    """n = 2 and 4: at most one lane's four rows; 32: several lanes.  An odd stride on either side."""
    from stark_rs_amd.mirror import Air
    cols, eight = pooled(log_n, p)
    args = [eight[i] for i in LISTS[name]]
    ch = chall(log_n)
    c_stride = (1 << log_n) + 1
    st0, want, closes0, key0 = plain_columns(emu, cols, args, ch, p, g, c_stride=c_stride)
    st, c, closes, key = operand_columns(emu, Air(len(cols)), cols, args, ch, p, g, c_stride=c_stride)
    assert st == st0 == 0 and key == key0
    assert closes == closes0 == [True] * len(args)
    assert np.array_equal(c, want)
    bad = agc.spoil(cols, args[-1], p)                                   # the last argument does not close: the same mask, the same words
    st0, want, closes0, _ = plain_columns(emu, bad, args, ch, p, g)
    st, c, closes, _ = operand_columns(emu, Air(len(cols)), bad, args, ch, p, g)
    assert st == st0 == 0 and closes == closes0 and not closes[-1] and np.array_equal(c, want)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("log_n", [1, 2, 5])
def test_both_routes_compose_the_same_codeword(oracle, emu, p, g, log_n, name):
    lb, tau, h = 3, 1, g
    N = 1 << (log_n + lb)
    air, cols, args = case(1 << log_n, p, SPECS[name])
    W, K, A = len(cols), len(air.constraints), len(args)
    ch = chall(11)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 2 * A), dtype=np.uint64)]
    c, closes, zero = agc.columns(cols, args, ch, p, g)
    assert zero is None and all(closes)
    lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
    cl = ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)
    for kw in (dict(), dict(stride=N + 1, c_stride=N + 3, out_stride=N + 5), dict(force_direct=1, grid=1)):
        want = plain_compose(emu, air, lde, cl, ch, wch, p, g, log_n, lb, tau, h, **kw)
        got = operand_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, lb, tau, h, **kw)
        assert np.array_equal(got, want), kw
