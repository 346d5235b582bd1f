"""CPU: the coset-leaf hash as the emulator library runs it (hash_core.h coset_leaf_hash2 under the kernel's grid and its
choice of a lane's two leaves) against the oracle's Hash::from_field_elements over a leaf's 4 V values, and against the
wide-row hash over the same buffer read as 4 V columns q apart where that kernel reaches; the opening sections as the
emulated writer of coset_open_kernel lays them out (mgpu_core.h mg_coset_open_write) against the restatement's
(tests/deep_fold4_compose.py); and the restated provers and verifier: accepted as proved, every tampering class rejected with
its sentence."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import deep_args_compose as da
import deep_compose as dc
import deep_fold4_compose as d4


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp = C.c_void_p
    L.emu_coset_leaf_hash.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int, vp]
    L.emu_coset_leaf_hash.restype = None
    L.emu_row_hash_wide.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_int, vp]
    L.emu_row_hash_wide.restype = None
    L.emu_coset_open.argtypes = [C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint32, vp]
    L.emu_coset_open.restype = C.c_uint64
    return L


def coset_view(cols, n):
    """(V, stride) columns -> (4 V, q): row 4 c + j is column c at the indices j q .. j q + q - 1, a leaf's value order"""
    V, q = cols.shape[0], n // 4
    return np.ascontiguousarray(cols[:, :n].reshape(V, 4, q).reshape(4 * V, q))


def columns(p, V, n, stride, seed, fill=None):
    """V columns `stride` apart, the padding beyond n poisoned with values no leaf may pick up"""
    rng = np.random.default_rng(seed)
    cols = np.full((V, stride), 0xFFFFFFFF, dtype=np.uint32)
    if fill is None:
        cols[:, :n] = rng.integers(0, p, (V, n), dtype=np.int64).astype(np.uint32)
        cols[0, 0] = p - 1
        cols[V - 1, n - 1] = 0
    else:
        cols[:, :n] = fill
    return cols


def coset_hash(emu, cols, n, V, stride):
    q = n // 4
    out = np.full((q + 1, 32), 0xEE, dtype=np.uint8)   # a guard digest behind the leaves
    emu.emu_coset_leaf_hash(cols.ctypes.data, stride, n, V, out.ctypes.data)
    assert (out[q] == 0xEE).all()
    return out[:q]


# one leaf, one pair, fewer leaves than a workgroup, half a workgroup's leaves, exactly one workgroup's 2 x 256, two workgroups
QS = [1, 2, 4, 256, 512, 1024]
# 4, 8, 64, 68 (the first width past the row hash's 64 values) and 256 values a leaf
WIDTHS = [1, 2, 16, 17, 64]


@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("V", WIDTHS)
@pytest.mark.parametrize("pad", [0, 1])
def test_coset_leaf_hash_equals_the_oracle(emu, oracle, V, pad, p, g):
    for q in QS:
        n = 4 * q
        stride = n + pad
        cols = columns(p, V, n, stride, 100 * V + q + pad)
        got = coset_hash(emu, cols, n, V, stride)
        want = oracle.row_hashes(coset_view(cols, n).astype(np.uint64))
        assert np.array_equal(got, want), (V, q)
        # the oracle's one-leaf call on the first leaf, value 4 c + j = column c at j q
        first = [int(cols[c, j * q]) for c in range(V) for j in range(4)]
        assert bytes(got[0]) == oracle.hash_from_field_elements(first)
        if 4 * V <= 64 and pad == 0:
            wide = np.zeros((q, 32), dtype=np.uint8)
            emu.emu_row_hash_wide(cols.ctypes.data, q, q, 4 * V, wide.ctypes.data)
            assert np.array_equal(got, wide), (V, q)


@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("V", WIDTHS)
def test_coset_leaf_hash_of_the_largest_residue(emu, oracle, V, p, g):
    for q in (1, 2, 512):
        n = 4 * q
        cols = columns(p, V, n, n + 1, 0, fill=p - 1)
        got = coset_hash(emu, cols, n, V, n + 1)
        assert all(bytes(d) == oracle.hash_from_field_elements([p - 1] * (4 * V)) for d in got), (V, q)


def test_the_entry_point_is_declared_and_bound():
    import stark_rs_amd
    from stark_rs_amd import _lib
    assert "smi_dev_merkle_build_cosets" in stark_rs_amd.declared_symbols()
    stark_rs_amd.build()
    assert len(_lib.lib().smi_dev_merkle_build_cosets.argtypes) == 6
    from stark_rs_amd.engine import Engine
    assert callable(Engine.dev_merkle_build_cosets)


# ---------------------------------------------------------------------------------------------- the opening sections
def emu_sections(emu, groups, trees, top, N):
    """groups: per group a list of V columns of N values; trees: their coset trees -> the sections' bytes"""
    G, t, log_N = len(groups), len(top), N.bit_length() - 1
    cols = [np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.uint64) for c in gp]).astype(np.uint32)) for gp in groups]
    nodes = [np.ascontiguousarray(nd) for nd in trees]
    ptr = lambda arrs: (C.c_void_p * G)(*[a.ctypes.data for a in arrs])
    stride = (C.c_uint64 * G)(*[N] * G)
    V = (C.c_uint32 * G)(*[len(gp) for gp in groups])
    tp = np.array(top, dtype=np.uint64)
    size = sum(d4.section_len(len(gp), t, log_N) for gp in groups)
    out = np.full(size + 16, 0xEE, dtype=np.uint8)   # a guard behind the sections
    used = emu.emu_coset_open(G, ptr(cols), stride, V, ptr(nodes), N, tp.ctypes.data, t, out.ctypes.data)
    assert used == size and (out[size:] == 0xEE).all()
    return bytes(out[:size])


@pytest.mark.parametrize("widths", [[1, 4], [4, 8], [9, 12, 8], [64, 32, 64]])
@pytest.mark.parametrize("log_N", [3, 6, 9])
def test_opening_sections_equal_the_restatement(emu, oracle, widths, log_N):
    p = ac.PRIMES[1][0]
    N = 1 << log_N
    q = N // 4
    rng = np.random.default_rng(log_N * 100 + sum(widths))
    groups = [[rng.integers(0, p, N, dtype=np.uint64) for _ in range(V)] for V in widths]
    trees = [d4.coset_tree(oracle, gp, N) for gp in groups]
    # the first and the last leaf, indices at and above N / 4 (reduced), random ones
    top = [0, q - 1, q, N - 1] + [int(v) for v in rng.integers(0, N, 3)]
    got = emu_sections(emu, groups, trees, top, N)
    want = b"".join(d4.section(oracle, gp, nd, top, N) for gp, nd in zip(groups, trees))
    assert got == want
    assert len(got) == sum(len(top) * (9 + 32 * V) + len(top) * (9 + 32 * (log_N - 2)) for V in widths)


# ---------------------------------------------------------------------------------------------- the restated proofs
@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_restated_plain_proofs_verify_and_every_tampering_is_rejected(emu, oracle, p, g):
    t = 4
    for name, log_n, lb in (("fib", 4, 3), ("mixer", 5, 2)):
        air, cols = ac.make(name, 1 << log_n, p)
        W, D = len(cols), dc.plan(air)[1]
        args = (p, g, W, log_n, lb, t, 1, g)
        res = d4.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g)
        assert d4.verify(oracle, air, None, res["proof"], res["roots"], *args) == (True, "")
        # the sections of the proof are the emulated writer's
        assert emu_sections(emu, res["groups"], res["trees"], res["top"], 1 << (log_n + lb)) == b"".join(res["sections"])
        muts = d4.mutations(res["proof"], W, 0, D, log_n, lb, t, p)
        assert {m[2] for m in muts} >= set(d4.WORDS[k] for k in ("length", "record", "path", "auth")) and any(m[0].startswith("swap") for m in muts)
        for nm, m, why in muts:
            assert d4.verify(oracle, air, None, m, res["roots"], *args) == (False, why), nm
        # what only one check can refuse: a column committed as value + p, a column committed with two coset points exchanged
        for k, V in enumerate((W, 4 * D)):
            bad = d4.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, commit_as=d4.plus_p(k, V - 1, p))
            assert d4.verify(oracle, air, None, bad["proof"], bad["roots"], *args) == (False, d4.WORDS["canonical"])
            bad = d4.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, commit_as=d4.swapped(k, 0))
            assert d4.verify(oracle, air, None, bad["proof"], bad["roots"], *args) == (False, d4.WORDS["quotient"])
        # another statement, other roots, the wrong difficulty, a proof of the folding-2 variant
        other = ac.make(name, 1 << log_n, p)[0]
        c, r, v = other.boundaries[0]
        other.boundaries[0] = (c, r, (v + 1) % p)
        assert d4.verify(oracle, other, None, res["proof"], res["roots"], *args) == (False, d4.FRONT["consistency"])
        assert d4.verify(oracle, air, None, res["proof"], res["roots"][::-1], *args) == (False, d4.FRONT["consistency"])
        assert d4.verify(oracle, air, None, res["proof"], res["roots"], *args, bits=20) == (False, "proof of work")
        old = dc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g)
        ok, why = d4.verify(oracle, air, None, old["proof"], old["roots"], *args)
        assert not ok and why in d4.SENTENCES
        ok, why = dc.verify(oracle, air, res["proof"], res["roots"], *args)
        assert not ok
    # a shape without a fold: the verifier's sentence (the prover has no layer-0 coset to open against)
    air, cols = ac.make("fib", 8, p)
    old = dc.prove(oracle, air, cols, p, g, 3, 3, t, 1, g)
    assert d4.folds(3, 3, t) == 0
    assert d4.verify(oracle, air, None, old["proof"], old["roots"], p, g, 2, 3, 3, t, 1, g) == (False, d4.FRONT["no layer"])


@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_restated_list_proofs_verify_and_every_tampering_is_rejected(oracle, p, g):
    log_n, lb, t = 4, 3, 4
    for name in ("lookup", "perm_sel"):
        air, cols, lst = da.small_lists(1 << log_n, p)[name]
        W, A, D = len(cols), len(lst), da.plan(air, lst)[1]
        args = (p, g, W, log_n, lb, t, 1, g)
        res = d4.prove_args(oracle, air, lst, cols, p, g, log_n, lb, t, 1, g)
        assert res["closes"] == [True] * A
        assert d4.verify(oracle, air, lst, res["proof"], res["roots"], *args) == (True, "")
        for nm, m, why in d4.mutations(res["proof"], W, A, D, log_n, lb, t, p):
            assert d4.verify(oracle, air, lst, m, res["roots"], *args) == (False, why), nm
        for k, V in enumerate((W, 4 * A, 4 * D)):
            bad = d4.prove_args(oracle, air, lst, cols, p, g, log_n, lb, t, 1, g, commit_as=d4.plus_p(k, 0, p))
            assert d4.verify(oracle, air, lst, bad["proof"], bad["roots"], *args) == (False, d4.ARGS_WORDS["canonical"])
            bad = d4.prove_args(oracle, air, lst, cols, p, g, log_n, lb, t, 1, g, commit_as=d4.swapped(k, V - 1))
            assert d4.verify(oracle, air, lst, bad["proof"], bad["roots"], *args) == (False, d4.ARGS_WORDS["quotient"])
        # a list that does not close: proved, and refused on the consistency check
        if name == "lookup":
            broken = [list(c) for c in cols]
            broken[2][broken[2].index(max(broken[2]))] -= 1              # one multiplicity too small
            bad = d4.prove_args(oracle, air, lst, broken, p, g, log_n, lb, t, 1, g, honest=False)
            assert bad["closes"] == [False]
            assert d4.verify(oracle, air, lst, bad["proof"], bad["roots"], *args) == (False, d4.FRONT["consistency args"])
        old = da.prove(oracle, air, lst, cols, p, g, log_n, lb, t, 1, g)
        ok, why = d4.verify(oracle, air, lst, old["proof"], old["roots"], *args)
        assert not ok and why in d4.SENTENCES
        assert not da.verify(oracle, air, lst, res["proof"], res["roots"], *args)[0]
