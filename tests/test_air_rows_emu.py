"""CPU: the two kernels of the row-committed AIR path as the emulator library runs them -- the wide-row leaf hash
(hash_core.h row_hash_wide2 under the kernel's own indexing of a lane's two rows and its chunk loop) against the
oracle's Hash::from_field_elements, and the row-opening records (mgpu_core.h mg_row_open_write) against a restatement
built from the oracle's MerkleTree -- and the declarations of the two new entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import air_compose as ac
import air_rows as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp = C.c_void_p
    L.emu_row_hash_wide.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int, vp]
    L.emu_row_hash_wide.restype = None
    L.emu_row_hash.argtypes = [vp, C.c_size_t, C.c_int, vp]
    L.emu_row_hash.restype = None
    L.emu_air_row_open.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp]
    L.emu_air_row_open.restype = C.c_uint64
    return L


def wide(emu, cols, n, W, stride):
    """cols: (W, stride) uint32 -> (n, 32) digests"""
    out = np.zeros((n, 32), dtype=np.uint8)
    emu.emu_row_hash_wide(cols.ctypes.data, stride, n, W, out.ctypes.data)
    return out


def columns(p, W, n, stride, seed):
    """W columns `stride` apart; rows 0 and 1 (where they exist) hold p-1 and 0 throughout, the padding beyond n is
    poisoned with values no row may pick up"""
    rng = np.random.default_rng(seed)
    cols = np.full((W, stride), 0xFFFFFFFF, dtype=np.uint32)
    cols[:, :n] = rng.integers(0, p, (W, n), dtype=np.int64).astype(np.uint32)
    cols[:, 0] = p - 1
    if n > 1:
        cols[:, 1] = 0
    if n > 2:
        cols[::2, n - 1] = p - 1
    return cols


# one lane (n = 1), one pair (n = 2), less than a wave, a wave, half a workgroup's rows, exactly one workgroup (2 x 256 rows),
# two and eight workgroups
SIZES = [1, 2, 4, 64, 128, 256, 512, 1024, 4096]


@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("W", range(1, 65))
def test_wide_row_hash_equals_the_oracle(emu, oracle, W, p, g):
    o = oracle
    for n in SIZES:
        if n == 4096 and W not in (1, 4, 5, 8, 9, 33, 63, 64):
            continue   # the widths around the chunk boundaries and the ends at the largest size; every width at the others
        stride = n + (0 if n in (64, 1024) else 3)
        cols = columns(p, W, n, stride, 1000 * W + n)
        got = wide(emu, cols, n, W, stride)
        want = o.row_hashes(cols[:, :n].astype(np.uint64))
        assert np.array_equal(got, want), (W, n)
    # the oracle's one-row call on the extreme rows: all p-1, all 0
    assert bytes(got[0]) == o.hash_from_field_elements([p - 1] * W)
    assert bytes(got[1]) == o.hash_from_field_elements([0] * W)


@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_wide_row_hash_equals_the_fused_paths_row_hash(emu, W):
    p = ac.PRIMES[0][0]
    n, stride = 130, 133
    cols = columns(p, W, n, stride, W)
    n = 128
    got = wide(emu, cols, n, W, stride)
    rows = np.ascontiguousarray(cols[:, :n].T)
    want = np.zeros((n, 32), dtype=np.uint8)
    emu.emu_row_hash(rows.ctypes.data, n, W, want.ctypes.data)
    assert np.array_equal(got, want)


def row_open(emu, lde, nodes, N, top, R, B):
    W = len(lde)
    cols = np.ascontiguousarray(np.array(lde, dtype=np.uint64).astype(np.uint32))
    tp = np.array(top, dtype=np.uint64)
    depth = N.bit_length() - 1
    size = len(top) * R * (9 + 8 * W) + len(top) * R * (9 + 32 * depth)
    out = np.full(size + 16, 0xEE, dtype=np.uint8)   # a guard behind the section
    nd = np.ascontiguousarray(nodes)
    used = emu.emu_air_row_open(cols.ctypes.data, N, W, nd.ctypes.data, N, tp.ctypes.data, len(top), R, B, out.ctypes.data)
    assert used == size and (out[size:] == 0xEE).all()
    return bytes(out[:size])


@pytest.mark.parametrize("W", [1, 4, 5, 64])
@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("log_N,B", [(6, 4), (9, 8), (1, 2)])
def test_row_opening_records_equal_the_restatement(emu, oracle, W, R, log_N, B):
    o = oracle
    p = ac.PRIMES[1][0]
    N = 1 << log_N
    if B >= N and R == 4:
        B = 1
    rng = np.random.default_rng(W * 100 + log_N)
    lde = [[int(x) for x in rng.integers(0, p, N)] for _ in range(W)]
    nodes = o.merkle_new(ar.row_leaves(o, lde))
    half = N // 2
    # a + B and b + B both wrap for the last positions; top-level indices above N/2 are reduced
    top = sorted({0, half - 1, max(half - B, 0), N - 1, N - B, int(rng.integers(0, N)), int(rng.integers(0, N))})
    got = row_open(emu, lde, nodes, N, top, R, B)
    assert len(got) == ar.opening_len(W, R == 4, log_N, len(top))
    assert got == ar.openings_bytes(o, lde, top, N, B, R == 4, nodes)
    if R == 4 and log_N > 1:
        assert any((t % half) + half + B >= N for t in top)   # a position that wraps at N is among them


def test_the_entry_points_are_declared_and_bound():
    import stark_rs_amd
    from stark_rs_amd import _lib
    names = {"smi_dev_air_prove_rows", "smi_air_verify_rows"}
    assert names <= set(stark_rs_amd.declared_symbols())
    stark_rs_amd.build()
    L = _lib.lib()
    for nm in names:
        assert getattr(L, nm).argtypes is not None, nm
    assert len(L.smi_dev_air_prove_rows.argtypes) == 9 and len(L.smi_air_verify_rows.argtypes) == 7
    # the Rust side: declared in the generated block, which is current, and wrapped
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_rust_bindings", os.path.join(ROOT, "tools", "gen_rust_bindings.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    src = open(os.path.join(ROOT, "bindings", "stark_mi.rs")).read()
    a, b = src.index("// BEGIN GENERATED"), src.index("// END GENERATED") + len("// END GENERATED")
    assert src[a:b] == gen.generate()
    for nm in names:
        assert f"pub fn {nm}(" in src[a:b] and f"{nm}(ctx.raw" in src[b:], nm


def test_air_plan_does_not_read_row_leaves():
    """limits, degree and expansion factor are those of the column-tree calls"""
    from stark_rs_amd import _lib
    from stark_rs_amd.engine import air_plan
    for p, g in ac.PRIMES:
        for name, want in (("empty", (1, 8)), ("fib", (1, 8)), ("mixer", (3, 4))):
            air, _ = ac.make(name, 1 << 10, p)
            got = [air_plan(p, air.flatten(p), _lib.StarkCfg(10, 3, air.n_cols, rl, 1, g, 8, 1)) for rl in (0, 1)]
            assert got == [want, want], (name, got)
    assert C.sizeof(_lib.StarkCfg) == 48
