"""CPU: out-of-domain sampling (include/stark_mi.h, "Out-of-domain sampling") without a GPU -- the plan's refusals and the
layout length (host-only entry points of the library) and the declarations."""
import ctypes as C
import os
import re

import pytest

import air_compose as ac
import air_periodic as ap
import deep_compose as dc
import ext_compose as xc
from stark_rs_amd.mirror import Air

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, TOO_SMALL = -50, -10
ENTRY_POINTS = ["smi_air_plan_deep", "smi_air_deep_layout", "smi_dev_poly_eval_ext", "smi_dev_deep_compose", "smi_dev_air_prove_deep",
                "smi_air_verify_deep"]


def quartic(n, p, period=4):
    """x' = k x^4 + 1 with k of period `period`: degree 5, so D = 4; the trace from numpy-free integer arithmetic"""
    ks = ap.round_constants(period, p, seed=5)
    x = [3]
    for r in range(n - 1):
        x.append((ks[r % period] * pow(x[-1], 4, p) + 1) % p)
    air = Air(1)
    k = air.periodic(ks)
    air.transition({("next", 0): 1, (("per", k), ("cur", 0, 4)): -1, (): -1})
    air.boundary(0, 0, 3).boundary(0, n - 1, x[-1])
    return air, [x]


def power_air(e):
    """x' = x^e: degree e"""
    return Air(1).transition({("next", 0): 1, ("cur", 0, e): -1})


def plan(p, g, air, W, log_n, lb, t=None):
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    s.build()
    cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, g, t or 0, 1)
    return s.engine.air_plan_deep(p, air.flatten(p), cfg, t is not None)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_plan_and_its_refusals(p, g):
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    n = 64
    mimc = ap.make("mimc", n, p)[0]
    assert plan(p, g, mimc, 1, 6, 3) == (3, 2)
    assert plan(p, g, mimc, 1, 6, 2) == (3, 2)                              # E = 2: refused by smi_air_plan, planned here
    with pytest.raises(s.StarkMiError) as ei:
        s.engine.air_plan(p, mimc.flatten(p), _lib.StarkCfg(6, 2, 1, 1, 1, g, 0, 1))
    assert ei.value.status == TOO_SMALL
    assert plan(p, g, ac.make("fib", n, p)[0], 2, 6, 2) == (1, 1)
    assert plan(p, g, quartic(n, p)[0], 1, 6, 3) == (5, 4)
    assert plan(p, g, quartic(n, p)[0], 1, 6, 2) == (5, 4)                  # D = B
    for air, lb, status, word in ((quartic(n, p)[0], 1, BAD_ARG, "D > 2^log_blowup"),        # D = 4 > B = 2, named before B < 4
                                  (ac.make("fib", n, p)[0], 1, TOO_SMALL, "2^log_blowup < 4"),
                                  (power_air(18), 5, BAD_ARG, "4 D > 64"),                      # D = 32 <= B = 32
                                  (power_air(34), 6, BAD_ARG, "4 D > 64"),                      # D = 64 <= B = 64
                                  (power_air(17), 3, BAD_ARG, "D > 2^log_blowup")):             # D = 16 > B = 8
        with pytest.raises(s.StarkMiError) as ei:
            plan(p, g, air, air.n_cols, 6, lb)
        assert ei.value.status == status and word in str(ei.value), (lb, str(ei.value))
    assert plan(p, g, power_air(17), 1, 6, 4) == (17, 16)                   # 4 D = 64: the widest row
    with pytest.raises(s.StarkMiError) as ei:                               # smi_air_plan's other checks apply unchanged
        plan(p, g, Air(1).transition({("next", 0): 1, ("cur", 2): -1}), 1, 6, 3)
    assert ei.value.status == BAD_ARG and "factor_var" in str(ei.value)
    with pytest.raises(s.StarkMiError, match="LDE domain too large"):
        plan(p, g, mimc, 1, 26, 3)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_layout_length_is_the_formula(oracle, p, g):
    for air, W, log_n, lb, t in ((ap.make("mimc", 64, p)[0], 1, 6, 2, 4), (ap.make("mimc", 1024, p)[0], 1, 10, 3, 8),
                                 (ac.make("mixer", 256, p)[0], 4, 8, 3, 6), (quartic(64, p)[0], 1, 6, 3, 4), (ac.make("fib", 1 << 20, p)[0], 2, 20, 3, 32)):
        d, D, length = plan(p, g, air, W, log_n, lb, t)
        assert (d, D) == dc.plan(air)
        assert length == dc.proof_len(oracle, W, D, log_n, lb, t, p, g, g), (W, log_n, lb, t)


def test_declarations():
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    s.build()
    declared = s.declared_symbols()
    header = open(os.path.join(ROOT, "include", "stark_mi.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "stark_mi.rs")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared
        assert re.search(r"pub fn " + name + r"\(", rust), name
        assert hasattr(lib, name), name
    assert "---- Out-of-domain sampling (DEEP)" in header
    core = open(os.path.join(ROOT, "stark_rs_amd", "csrc", "deep_core.h")).read()
    for word in dc.KEYWORD.values():                                        # every reason class has its sentence in the library
        assert word in core, word
