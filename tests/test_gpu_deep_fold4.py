"""GPU: out-of-domain sampling over coset leaves (include/stark_mi.h, "Out-of-domain sampling over coset leaves") --
smi_dev_merkle_build_cosets, smi_dev_air_prove_deep_fold4 / smi_air_verify_deep_fold4 and their argument-list twins -- against
the restatement over the CPU oracle's primitives (tests/deep_fold4_compose.py).  Every comparison is exact.  `pytest -m gpu`."""
import numpy as np
import pytest

import air_compose as ac
import deep_args_compose as da
import deep_compose as dc
import deep_fold4_compose as d4
import ext_compose as xc
import fold4_compose as f4
from test_deep_fold4_emu import QS, WIDTHS, columns, coset_view
from test_deep_host import quartic
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_deep import make_air
from test_gpu_deep_args import mirror, statement

pytestmark = pytest.mark.gpu
KW = dict(row_leaves=True, ext=True, deep=True, coset_leaves=True)
KWA = dict(row_leaves=True, ext=True, deep_args=True, coset_leaves=True)
BAD_ARG = -50


# ---------------------------------------------------------------------------------------------- the coset-leaf tree
def gpu_coset_tree(eng, cols, V, n, stride):
    """cols: (V, stride) uint32 -> the (2 q - 1, 32) node digests; the word behind the tree must stay as it was"""
    import torch
    q = n // 4
    t = torch.from_numpy(np.ascontiguousarray(cols).view(np.int32).reshape(-1)).cuda()
    nodes = torch.full((2 * q, 32), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.dev_merkle_build_cosets(t.data_ptr(), V, stride, n, nodes.data_ptr())
    eng.sync()
    host = nodes.cpu().numpy()
    assert (host[2 * q - 1] == 0xEE).all()
    return host[:2 * q - 1]


@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("V", WIDTHS)
def test_coset_tree_equals_the_oracle_on_every_level(engines, oracle, V, p, g):
    """one leaf, one pair, fewer leaves than a workgroup, half a workgroup's, exactly one workgroup's 2 x 256, two workgroups;
    4, 8, 64, 68 and 256 values a leaf; columns exactly n apart and one word further; all values p - 1"""
    eng = engines[p]
    for q in QS:
        for pad in (0, 1):
            n = 4 * q
            cols = columns(p, V, n, n + pad, 100 * V + q + pad)
            got = gpu_coset_tree(eng, cols, V, n, n + pad)
            want = oracle.merkle_new(oracle.row_hashes(coset_view(cols, n).astype(np.uint64)))
            assert np.array_equal(got, want), (V, q, pad)
    for q in (1, 512):
        n = 4 * q
        got = gpu_coset_tree(eng, columns(p, V, n, n + 1, 0, fill=p - 1), V, n, n + 1)
        assert all(bytes(d) == oracle.hash_from_field_elements([p - 1] * (4 * V)) for d in got[:q]), (V, q)


def test_coset_tree_at_2_22_is_the_row_tree_of_the_16_column_view(engines):
    """one launch at n = 2^22, W = 4: leaf i of the coset tree hashes the 16 values the row tree over the same buffer read as
    16 columns q apart hashes for row i, so the two trees are equal node for node"""
    import torch
    p, g = ac.PRIMES[1]
    eng, n, W = engines[p], 1 << 22, 4
    q = n // 4
    gen = torch.Generator(device="cuda").manual_seed(22)
    cols = torch.randint(0, p, (W * n,), dtype=torch.int32, device="cuda", generator=gen)
    a, b = (torch.zeros((2 * q - 1, 32), dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    eng.dev_merkle_build_cosets(cols.data_ptr(), W, n, n, a.data_ptr())
    eng.dev_merkle_build_rows(cols.data_ptr(), 4 * W, q, q, b.data_ptr())
    eng.sync()
    assert torch.equal(a, b) and int(a[-1].to(torch.int32).sum()) > 0


def test_coset_tree_refusals(engines):
    import stark_rs_amd as s
    p, g = ac.PRIMES[0]
    eng = engines[p]
    with Dev(eng) as dev:
        d_cols, d_nodes = dev.upload(np.arange(2 * 16, dtype=np.uint64)), dev.alloc(32 * 8)
        for args, word in (((2, 16, 12), "power of two"), ((2, 16, 2), "at least 4"), ((2, 16, 0), "power of two"), ((2, 15, 16), "stride"),
                           ((0, 16, 16), "1..64 columns"), ((65, 16, 16), "1..64 columns")):
            with pytest.raises(s.StarkMiError, match=word) as ei:
                eng.dev_merkle_build_cosets(d_cols, args[0], args[1], args[2], d_nodes)
            assert ei.value.status == BAD_ARG, args
        eng.dev_merkle_build_cosets(d_cols, 2, 16, 16, d_nodes)                # and the call that all of them spoil


# ---------------------------------------------------------------------------------------------- plain AIRs
def gpu_proof(eng, air, cols, log_n, lb, t, bits=0, check=True, **kw):
    with Dev(eng) as dev:
        return eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, lb, t, grind_bits=bits, check=check, **KW, **kw)


def periodic_air(n, p):
    """fib with a periodic column of period 4 added to the transition: a_next = b + pi"""
    from stark_rs_amd.mirror import Air
    vals = [3, p - 1, 0, 7]
    a, b = [1], [1]
    for r in range(n - 1):
        a.append((b[-1] + vals[r % 4]) % p)
        b.append((a[-2] + b[-1]) % p)
    air = Air(2)
    j = air.periodic(vals)
    air.transition({("next", 0): 1, ("cur", 1): -1, ("per", j): -1})
    air.transition({("next", 1): 1, ("cur", 0): -1, ("cur", 1): -1})
    air.boundary(0, 0, 1).boundary(1, 0, 1)
    return air, [a, b]


def plain_statement(name, n, p):
    if name == "periodic":
        return periodic_air(n, p)
    return make_air(name, n, p)


# (name, log_blowup, sizes): from the smallest shape with a fold at t = 4 (N = 128; mimc needs 64 rows) up to n = 2^8
PLAIN = [("fib", 3, (4, 5, 6, 7, 8)), ("mixer", 3, (4, 6, 8)), ("mimc", 3, (6, 7, 8)), ("mimc", 2, (6, 8)), ("quartic", 3, (4, 7)), ("periodic", 3, (4, 5, 8)),
         ("fib", 2, (5, 6))]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name,lb,sizes", PLAIN)
def test_plain_proofs_equal_the_restatement_and_verify(engines, oracle, p, g, name, lb, sizes):
    eng, t = engines[p], 4
    seen = set()
    for log_n in sizes:
        air, cols = plain_statement(name, 1 << log_n, p)
        W, D = len(cols), dc.plan(air)[1]
        bits = 4 if log_n == 6 else 0
        res = gpu_proof(eng, air, cols, log_n, lb, t, bits)
        want = d4.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, bits)
        assert [bytes(r) for r in res["column_roots"]] == want["roots"] and res["column_roots"].shape == (2, 32)
        assert [c for el in res["ood"] for c in el] == want["ood"] and len(res["ood"]) == 2 * W + D
        assert res["top_indices"] == want["top"]
        assert res["proof"][:len(res["proof"]) - sum(map(len, want["sections"]))] == want["proof"][:9 + 32 * (2 * W + D) + want["fri_len"]]
        assert res["proof"][-sum(map(len, want["sections"])):] == b"".join(want["sections"])      # the opening kernel's bytes
        assert res["proof"] == want["proof"]
        F, length = eng.air_deep_fold4_layout(air, W, log_n, lb, t)
        assert len(res["proof"]) == length == d4.layout(W, 0, D, log_n, lb, t)[1] and F == d4.folds(log_n, lb, t) >= 1
        seen.add((F, (f4.layout(1 << (log_n + lb), 1 << lb, t)[0] - 1) % 2))
        ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **KW)
        assert ok, why
        assert d4.verify(oracle, air, None, res["proof"], want["roots"], p, g, W, log_n, lb, t, 1, g, bits) == (True, "")
    if name == "fib" and lb == 3:
        assert seen >= {(1, 0), (1, 1), (2, 0), (2, 1)}                      # one and two folds, both parities of R2 - 1


def test_stage_names_and_the_result_keys_are_the_deep_variant_s(engines):
    p, g = xc.PRIMES[1]
    eng = engines[p]
    air, cols = quartic(1 << 6, p)
    res = gpu_proof(eng, air, cols, 6, 3, 4, timed=True)
    assert list(res["stage_ms"]) == ["lde", "commit", "compose", "segments", "ood", "fri", "open"]
    assert sorted(res) == ["column_roots", "ood", "proof", "stage_ms", "top_indices"]
    assert eng.air_deep_fold4_layout(air, 1, 6, 3, 4) == d4.layout(1, 0, 4, 6, 3, 4)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_a_shape_without_a_fold_is_refused_by_prover_and_verifier(engines, oracle, p, g):
    import stark_rs_amd as s
    eng, log_n, lb, t = engines[p], 3, 3, 4
    assert d4.folds(log_n, lb, t) == 0
    air, cols = ac.make("fib", 1 << log_n, p)
    with pytest.raises(s.StarkMiError, match="deep fold4: FRI has no fold") as ei:
        gpu_proof(eng, air, cols, log_n, lb, t)
    assert ei.value.status == BAD_ARG
    old = dc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g)              # a record that is consistent at z, whatever follows it
    ok, why = eng.air_verify(air, old["proof"], old["roots"], 2, log_n, lb, t, **KW)
    assert (ok, why) == d4.verify(oracle, air, None, old["proof"], old["roots"], p, g, 2, log_n, lb, t, 1, g) == (False, d4.FRONT["no layer"])
    air_l, cols_l, lst = statement("perm", log_n, p)
    with pytest.raises(s.StarkMiError, match="deep fold4: FRI has no fold"):
        gpu_proof_args(eng, air_l, lst, cols_l, log_n, lb, t)
    old = da.prove(oracle, air_l, lst, cols_l, p, g, log_n, lb, t, 1, g)
    ok, why = eng.air_verify(mirror(air_l, lst), old["proof"], old["roots"], len(cols_l), log_n, lb, t, **KWA)
    assert (ok, why) == (False, d4.FRONT["no layer"])


def both(eng, oracle, air, lst, proof, roots, p, g, W, log_n, lb, t, want=None, bits=0):
    """the library's verdict and the restatement's are the same sentence (want: that sentence) -> it"""
    a = mirror(air, lst) if lst is not None else air
    ok, why = eng.air_verify(a, proof, roots, W, log_n, lb, t, grind_bits=bits, **(KWA if lst is not None else KW))
    got_o = d4.verify(oracle, air, lst, proof, [bytes(r) for r in roots], p, g, W, log_n, lb, t, 1, g, bits)
    assert (ok, why) == got_o and not ok and why, ((ok, why), got_o)
    assert want is None or why == want, (why, want)
    return why


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name", ["mixer", "mimc"])
def test_plain_rejections_carry_the_restatement_s_sentence(engines, oracle, p, g, name):
    import stark_rs_amd as s
    eng, log_n, lb, t = engines[p], 6, 3, 4
    n = 1 << log_n
    air, cols = make_air(name, n, p)
    W, D = len(cols), dc.plan(air)[1]
    res = gpu_proof(eng, air, cols, log_n, lb, t)
    proof, roots = res["proof"], res["column_roots"]
    shape = (p, g, W, log_n, lb, t)
    assert eng.air_verify(air, proof, roots, W, log_n, lb, t, **KW)[0]
    # each record and path of each group, a value + p and a swapped pair in a record, the record, the length
    for nm, m, why in d4.mutations(proof, W, 0, D, log_n, lb, t, p):
        both(eng, oracle, air, None, m, roots, *shape, want=why)
    # restated proofs only one check can refuse: a column committed as value + p, two coset points of a column exchanged
    for k, V in enumerate((W, 4 * D)):
        bad = d4.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, commit_as=d4.plus_p(k, V - 1, p))
        both(eng, oracle, air, None, bad["proof"], bad["roots"], *shape, want=d4.WORDS["canonical"])
        bad = d4.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, commit_as=d4.swapped(k, 0))
        both(eng, oracle, air, None, bad["proof"], bad["roots"], *shape, want=d4.WORDS["quotient"])
    # a statement changed in one boundary value, the wrong difficulty, the roots exchanged, one trace cell changed
    other = make_air(name, n, p)[0]
    c, r, v = other.boundaries[0]
    other.boundaries[0] = (c, r, (v + 1) % p)
    both(eng, oracle, other, None, proof, roots, *shape, want=d4.FRONT["consistency"])
    both(eng, oracle, air, None, proof, roots, *shape, want="proof of work", bits=20)
    both(eng, oracle, air, None, proof, roots[::-1].copy(), *shape, want=d4.FRONT["consistency"])
    bad_cols = [list(c) for c in cols]
    bad_cols[0][n // 3] = (bad_cols[0][n // 3] + 1) % p
    forged = gpu_proof(eng, air, bad_cols, log_n, lb, t, check=False)
    both(eng, oracle, air, None, forged["proof"], forged["column_roots"], *shape, want=d4.FRONT["consistency"])
    with pytest.raises(s.StarkMiError):
        gpu_proof(eng, air, bad_cols, log_n, lb, t)
    # a layer-0 coset record of FRI changed: the walk's own sentence
    off = d4.object_offsets(W, 0, D, log_n, lb, t)
    at = off["fri"] + [a for kind, _r, a in f4.objects(1 << (log_n + lb), 1 << lb, t)[0] if kind == "coset"][0]
    m = bytearray(proof)
    m[at + 9] ^= 2
    both(eng, oracle, air, None, bytes(m), roots, *shape, want="merkle authentication path verification fails for aa")
    # cross-variant: the folding-2 DEEP proof and the fold-by-4 AIR proof here, this proof there
    with Dev(eng) as dev:
        d = dev.upload(np.array(cols, dtype=np.uint64))
        deep2 = eng.dev_air_prove(air, d, W, log_n, lb, t, grind_bits=0, row_leaves=True, ext=True, deep=True)
        air4 = eng.dev_air_prove(air, d, W, log_n, lb, t, grind_bits=0, row_leaves=True, ext=True, folding=4)
    both(eng, oracle, air, None, deep2["proof"], deep2["column_roots"], *shape)
    both(eng, oracle, air, None, air4["proof"], np.concatenate([air4["column_roots"], air4["column_roots"]]), *shape, want=d4.FRONT["record"])
    ok, why = eng.air_verify(air, proof, roots, W, log_n, lb, t, grind_bits=0, row_leaves=True, ext=True, deep=True)
    assert not ok and why
    ok, why = eng.air_verify(air, proof, roots[:1], W, log_n, lb, t, grind_bits=0, row_leaves=True, ext=True, folding=4)
    assert not ok and why


# ---------------------------------------------------------------------------------------------- argument lists
def gpu_proof_args(eng, air, lst, cols, log_n, lb, t, bits=0, check=True, fill=False, **kw):
    cols = [list(c) for c in cols]
    if fill:
        for g_ in lst:
            if g_[0] == "lookup":
                cols[g_[3]] = [0] * len(cols[0])
    with Dev(eng) as dev:
        return eng.dev_air_prove(mirror(air, lst), dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, lb, t, grind_bits=bits, check=check,
                                 fill_multiplicities=fill, **KWA, **kw)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name,lb,sizes", [("nine", 3, (4, 6, 8)), ("nine", 2, (5, 6)), ("selectors", 3, (4, 7)), ("perm", 3, (5,)), ("lookup", 2, (8,))])
def test_list_proofs_equal_the_restatement_and_verify(engines, oracle, p, g, name, lb, sizes):
    eng, t = engines[p], 4
    for log_n in sizes:
        air, cols, lst = statement(name, log_n, p)
        W, A, D = len(cols), len(lst), da.plan(air, lst)[1]
        bits = 8 if log_n == 6 else 0
        res = gpu_proof_args(eng, air, lst, cols, log_n, lb, t, bits, fill=name in ("lookup", "nine"))
        want = d4.prove_args(oracle, air, lst, cols, p, g, log_n, lb, t, 1, g, bits)
        assert [bytes(r) for r in res["column_roots"]] == want["roots"] and res["column_roots"].shape == (3, 32)
        assert [c for el in res["ood"] for c in el] == want["ood"] and len(res["ood"]) == 2 * W + 2 * A + D
        assert res["closes"] == want["closes"] == [True] * A
        assert res["top_indices"] == want["top"]
        assert res["proof"][-sum(map(len, want["sections"])):] == b"".join(want["sections"])      # the opening kernel's bytes
        assert res["proof"] == want["proof"]
        F, length = eng.air_deep_args_fold4_layout(mirror(air, lst), W, log_n, lb, t)
        assert len(res["proof"]) == length == d4.layout(W, A, D, log_n, lb, t)[1] and F == d4.folds(log_n, lb, t) >= 1
        ok, why = eng.air_verify(mirror(air, lst), res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **KWA)
        assert ok, why
        assert d4.verify(oracle, air, lst, res["proof"], want["roots"], p, g, W, log_n, lb, t, 1, g, bits) == (True, "")


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_list_rejections_carry_the_restatement_s_sentence(engines, oracle, p, g):
    import stark_rs_amd as s
    eng, log_n, lb, t = engines[p], 5, 3, 4
    air, cols, lst = statement("nine", log_n, p)
    W, A, D = len(cols), len(lst), da.plan(air, lst)[1]
    res = gpu_proof_args(eng, air, lst, cols, log_n, lb, t, timed=True)
    assert list(res["stage_ms"]) == ["lde", "commit", "args", "compose", "segments", "ood", "fri", "open"]
    assert sorted(res) == ["closes", "column_roots", "ood", "proof", "stage_ms", "top_indices"]
    proof, roots = res["proof"], res["column_roots"]
    shape = (p, g, W, log_n, lb, t)
    for nm, m, why in d4.mutations(proof, W, A, D, log_n, lb, t, p):
        both(eng, oracle, air, lst, m, roots, *shape, want=why)
    for k, V in enumerate((W, 4 * A, 4 * D)):
        bad = d4.prove_args(oracle, air, lst, cols, p, g, log_n, lb, t, 1, g, commit_as=d4.plus_p(k, V - 1, p))
        both(eng, oracle, air, lst, bad["proof"], bad["roots"], *shape, want=d4.ARGS_WORDS["canonical"])
        bad = d4.prove_args(oracle, air, lst, cols, p, g, log_n, lb, t, 1, g, commit_as=d4.swapped(k, 0))
        both(eng, oracle, air, lst, bad["proof"], bad["roots"], *shape, want=d4.ARGS_WORDS["quotient"])
    both(eng, oracle, air, lst, proof, roots, *shape, want="proof of work", bits=20)
    both(eng, oracle, air, [lst[0], lst[2], lst[1]], proof, roots, *shape, want=d4.FRONT["consistency args"])   # another statement
    # a list that does not close: proved with its bit down, the bytes the restatement's, and rejected on the consistency check
    broken = [list(c) for c in cols]
    broken[6][broken[6].index(max(broken[6]))] -= 1
    with pytest.raises(s.StarkMiError, match=r"the arguments \[1\] do not close"):
        gpu_proof_args(eng, air, lst, broken, log_n, lb, t)
    bad = gpu_proof_args(eng, air, lst, broken, log_n, lb, t, check=False)
    want = d4.prove_args(oracle, air, lst, broken, p, g, log_n, lb, t, 1, g, honest=False)
    assert bad["closes"] == want["closes"] == [True, False, True] and bad["proof"] == want["proof"]
    both(eng, oracle, air, lst, bad["proof"], bad["column_roots"], *shape, want=d4.FRONT["consistency args"])
    # cross-variant
    with Dev(eng) as dev:
        deep2 = eng.dev_air_prove(mirror(air, lst), dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, grind_bits=0, row_leaves=True, ext=True,
                                  deep_args=True)
    both(eng, oracle, air, lst, deep2["proof"], deep2["column_roots"], *shape)
    ok, why = eng.air_verify(mirror(air, lst), proof, roots, W, log_n, lb, t, grind_bits=0, row_leaves=True, ext=True, deep_args=True)
    assert not ok and why


def test_one_prove_at_2_16(engines):
    p, g = xc.PRIMES[1]
    eng, log_n, lb, t = engines[p], 16, 3, 32
    air, cols = ac.make("mixer", 1 << log_n, p)
    W, D = len(cols), dc.plan(air)[1]
    assert W == 4
    res = gpu_proof(eng, air, cols, log_n, lb, t, bits=8, check=False)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=8, **KW)
    assert ok, why
    F, length = eng.air_deep_fold4_layout(air, W, log_n, lb, t)
    assert len(res["proof"]) == length == d4.layout(W, 0, D, log_n, lb, t)[1] and F >= 1
    m = bytearray(res["proof"])
    m[-1] ^= 1
    assert eng.air_verify(air, bytes(m), res["column_roots"], W, log_n, lb, t, grind_bits=8, **KW) == (False, d4.WORDS["auth"])


# ---------------------------------------------------------------------------------------------- stage_ms of every DEEP prover
def mimc_on_the_real_rows(n, t, p):
    """air_periodic's MiMC lane with its second claim on the last real row n - k_t - 1: the zk plan refuses a claim on a
    randomiser row"""
    import air_periodic as ap
    import zk_compose as zk
    from stark_rs_amd.mirror import Air
    x = ap.make("mimc", n, p)[1][0]
    air = Air(1)
    k = air.periodic(ap.round_constants(64, p))
    air.transition({("next", 0): 1, ("cur", 0, 3): -1, (("cur", 0, 2), ("per", k)): -3, (("cur", 0), ("per", k, 2)): -3, ("per", k, 3): -1})
    real = n - zk.k_t(t)
    air.boundary(0, 0, x[0]).boundary(0, real - 1, x[real - 1])
    return air, [x]


# (entry point, the stages its section of include/stark_mi.h documents, log_blowup, statement)
STAGE_CASES = [("deep", 7, 3, "mimc"), ("deep_xargs", 8, 2, "perm"), ("deep_fold4", 7, 2, "mimc"), ("deep_xargs_fold4", 8, 3, "lookup"),
               ("deep_zk", 9, 2, "mimc")]


@pytest.mark.parametrize("entry,count,lb,name", STAGE_CASES)
def test_stage_ms_gets_exactly_the_documented_count(engines, entry, count, lb, name):
    """smi_dev_air_prove_<entry> through the library handle with a stage_ms array one double longer than documented, all NaN
    beforehand: `count` finite values >= 0, the extra double untouched, and the bytes of the same call with stage_ms null (zk:
    under the same seed).  n = 2^6, two colinearity tests."""
    import ctypes as C
    from stark_rs_amd import engine
    p, g = xc.PRIMES[0]
    eng, log_n, t, seed = engines[p], 6, 2, bytes(range(32))
    xa = None
    if name == "mimc":
        air, cols = mimc_on_the_real_rows(1 << log_n, t, p) if entry == "deep_zk" else make_air("mimc", 1 << log_n, p)
        a = eng._air(air)
    else:
        air, cols, lst = statement(name, log_n, p)
        a = eng._air(mirror(air, lst))
        xa = engine.xargs_of(a)
    cfg = eng._stark_cfg(len(cols), log_n, lb, t, 1, None, True)
    prove = getattr(eng.L, "smi_dev_air_prove_" + entry)

    def call(stage):
        roots, ood, top = np.zeros((3, 32), dtype=np.uint8), np.zeros(4096, dtype=np.uint64), np.zeros(t, dtype=np.uint64)
        proof, plen, closes = C.c_void_p(), C.c_size_t(), C.c_uint32()
        with Dev(eng) as dev:
            d = dev.upload(np.array(cols, dtype=np.uint64))
            args = [eng.h, C.byref(cfg), C.byref(a)] + ([C.byref(xa)] if xa is not None else []) + [C.c_void_p(d)] + ([seed] if entry == "deep_zk" else [])
            args += [roots.ctypes.data, ood.ctypes.data, C.byref(proof), C.byref(plen), top.ctypes.data, stage, 0] + ([C.byref(closes)] if xa is not None else [])
            status = prove(*args)
            assert status == 0, (status, eng.L.smi_last_error(eng.h))
            out = C.string_at(proof, plen.value)
            eng.L.smi_free(proof)
        return out

    stage = (C.c_double * (count + 1))(*[float("nan")] * (count + 1))
    timed = call(stage)
    got = [float(v) for v in stage]
    print(entry, got)
    assert all(np.isfinite(v) and v >= 0 for v in got[:count]), got
    assert np.isnan(got[count]), got
    assert len(timed) > 9 and timed == call(None)
