"""GPU: out-of-domain sampling over coset leaves at the boundary moduli of tests/test_gpu_boundary_primes.py (THREE: one per
range bound of the lazy reductions) -- the coset-leaf hash with all values p - 1, one proof of each variant against the
restatement (tests/deep_fold4_compose.py), and one tampered proof each.  `pytest -m gpu`."""
import numpy as np
import pytest

import air_compose as ac
import deep_args_compose as da
import deep_compose as dc
import deep_fold4_compose as d4
from test_deep_fold4_emu import columns
from test_gpu_boundary_primes import GEN, THREE, engines  # noqa: F401  (engines is a fixture)
from test_gpu_deep_fold4 import KW, KWA, gpu_coset_tree, gpu_proof, gpu_proof_args
from test_gpu_deep_args import mirror

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("V", [1, 17, 64])
def test_coset_leaf_hash_of_the_largest_residue(engines, oracle, p, V):
    for q in (1, 2, 512):
        n = 4 * q
        got = gpu_coset_tree(engines[p], columns(p, V, n, n + 1, 0, fill=p - 1), V, n, n + 1)
        assert all(bytes(d) == oracle.hash_from_field_elements([p - 1] * (4 * V)) for d in got[:q]), (V, q)
        cols = columns(p, V, n, n, V + q)
        got = gpu_coset_tree(engines[p], cols, V, n, n)
        assert np.array_equal(got, d4.coset_tree(oracle, list(cols.astype(np.uint64)), n)), (V, q)


@pytest.mark.parametrize("p", THREE)
def test_a_plain_proof_at_boundary_moduli(engines, oracle, p):
    eng, g, log_n, lb, t = engines[p], GEN[p], 5, 2, 4
    air, cols = ac.make("mixer", 1 << log_n, p)
    W = len(cols)
    res = gpu_proof(eng, air, cols, log_n, lb, t)
    want = d4.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g)
    assert res["proof"] == want["proof"] and [bytes(r) for r in res["column_roots"]] == want["roots"]
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, **KW)
    assert ok, why
    bad = d4.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, commit_as=d4.swapped(0, 1))
    assert eng.air_verify(air, bad["proof"], bad["roots"], W, log_n, lb, t, **KW) == (False, d4.WORDS["quotient"])
    m = bytearray(res["proof"])
    m[9 + 32 * (2 * W)] ^= 1                                                 # s_0
    assert eng.air_verify(air, bytes(m), res["column_roots"], W, log_n, lb, t, **KW) == (False, d4.FRONT["consistency"])
    assert dc.plan(air)[1] <= 1 << lb


@pytest.mark.parametrize("p", THREE)
def test_a_list_proof_at_boundary_moduli(engines, oracle, p):
    eng, g, log_n, lb, t = engines[p], GEN[p], 5, 2, 4
    air, cols, lst = da.readme_lists(1 << log_n, p)["nine"]
    res = gpu_proof_args(eng, air, lst, cols, log_n, lb, t)
    want = d4.prove_args(oracle, air, lst, cols, p, g, log_n, lb, t, 1, g)
    assert res["proof"] == want["proof"] and [bytes(r) for r in res["column_roots"]] == want["roots"]
    ok, why = eng.air_verify(mirror(air, lst), res["proof"], res["column_roots"], 9, log_n, lb, t, **KWA)
    assert ok, why
    bad = d4.prove_args(oracle, air, lst, cols, p, g, log_n, lb, t, 1, g, commit_as=d4.plus_p(1, 2, p))
    assert eng.air_verify(mirror(air, lst), bad["proof"], bad["roots"], 9, log_n, lb, t, **KWA) == (False, d4.ARGS_WORDS["canonical"])
    m = bytearray(res["proof"])
    m[9 + 32 * 18] ^= 1                                                      # a_0
    assert eng.air_verify(mirror(air, lst), bytes(m), res["column_roots"], 9, log_n, lb, t, **KWA) == (False, d4.FRONT["consistency args"])
