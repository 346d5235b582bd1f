"""GPU: out-of-domain sampling at the boundary moduli of tests/test_gpu_boundary_primes.py (THREE: one per range bound of
the lazy reductions) -- the two kernels under operands p - 1 and challenges of the u64 set, and one proof with its
verification.  `pytest -m gpu`."""
import numpy as np
import pytest

import air_periodic as ap
import deep_compose as dc
from test_gpu_air import Dev
from test_gpu_boundary_primes import GEN, THREE, engines  # noqa: F401  (engines is a fixture)
from test_gpu_deep import KW, check_compose, check_eval

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("n_coeffs,n_cols", [(1, 3), (257, 64), ((1 << 16) + 1, 3)])
def test_dev_poly_eval_ext_at_boundary_moduli(engines, p, n_coeffs, n_cols):
    check_eval(engines[p], p, GEN[p], n_coeffs, n_cols)


@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("log_N", [10, 12])
def test_dev_deep_compose_at_boundary_moduli(engines, oracle, p, log_N):
    check_compose(engines[p], oracle, p, GEN[p], log_N, [(2, 1, 16), (3, 12, 2), (4, 64, 4)])


@pytest.mark.parametrize("p", THREE)
def test_prove_and_verify_at_boundary_moduli(engines, oracle, p):
    eng, g, log_n, lb, t = engines[p], GEN[p], 8, 3, 4
    air, cols = ap.make("mimc", 1 << log_n, p)
    with Dev(eng) as dev:
        res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), 1, log_n, lb, t, **KW)
    want = dc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g)
    assert res["proof"] == want["proof"] and [bytes(r) for r in res["column_roots"]] == want["roots"]
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], 1, log_n, lb, t, **KW)
    assert ok, why
    bad = bytearray(res["proof"])
    bad[9] ^= 1
    ok, why = eng.air_verify(air, bytes(bad), res["column_roots"], 1, log_n, lb, t, **KW)
    assert not ok and dc.KEYWORD["consistency"] in why
