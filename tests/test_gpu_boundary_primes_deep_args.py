"""GPU: out-of-domain sampling with an argument list at the boundary moduli of tests/test_gpu_boundary_primes.py (THREE: one
per range bound of the lazy reductions) -- the compose kernel under operands p - 1 and challenges of the u64 set, 2^64 - 1 and
p - 1, and one proof with its verification.  `pytest -m gpu`."""
import numpy as np
import pytest

import deep_args_compose as da
from test_gpu_air import Dev
from test_gpu_boundary_primes import GEN, THREE, engines  # noqa: F401  (engines is a fixture)
from test_gpu_deep_args import KW, SHAPES, check_compose, mirror

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("log_N", [4, 11])
def test_dev_deep_compose_args_at_boundary_moduli(engines, oracle, p, log_N):
    check_compose(engines[p], oracle, p, GEN[p], log_N, SHAPES, ("random", "u64", "max", "pm1"))


@pytest.mark.parametrize("p", THREE)
def test_prove_and_verify_at_boundary_moduli(engines, oracle, p):
    eng, g, log_n, lb, t = engines[p], GEN[p], 6, 2, 4
    air, cols, args = da.readme_lists(1 << log_n, p)["nine"]
    with Dev(eng) as dev:
        res = eng.dev_air_prove(mirror(air, args), dev.upload(np.array(cols, dtype=np.uint64)), 9, log_n, lb, t, **KW)
    want = da.prove(oracle, air, args, cols, p, g, log_n, lb, t, 1, g)
    assert res["proof"] == want["proof"] and [bytes(r) for r in res["column_roots"]] == want["roots"]
    ok, why = eng.air_verify(mirror(air, args), res["proof"], res["column_roots"], 9, log_n, lb, t, **KW)
    assert ok, why
    bad = bytearray(res["proof"])
    bad[9 + 32 * 18] ^= 1                                                    # a_0
    ok, why = eng.air_verify(mirror(air, args), bytes(bad), res["column_roots"], 9, log_n, lb, t, **KW)
    assert not ok and da.KEYWORD["consistency"] in why
