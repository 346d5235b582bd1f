"""CPU: out-of-domain sampling with an argument list (include/stark_mi.h, "Out-of-domain sampling with an argument list")
without a GPU -- the plan, its refusals and the layout length (host-only entry points of the library) against the restatement
(tests/deep_args_compose.py), and the declarations."""
import ctypes as C
import os
import re

import pytest

import deep_args_compose as da
import ext_compose as xc
import xargs_compose as xa
from stark_rs_amd.mirror import Air

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, TOO_SMALL = -50, -10
ENTRY_POINTS = ["smi_air_plan_deep_xargs", "smi_air_deep_xargs_layout", "smi_dev_deep_compose_args", "smi_dev_air_prove_deep_xargs",
                "smi_air_verify_deep_xargs"]


def plan(p, g, air, W, log_n, lb, t=None):
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    s.build()
    cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, g, t or 0, 1)
    flat = air.flatten(p)
    return s.engine.air_plan_deep_args(p, flat, s.engine.xargs_of(flat), cfg, t is not None)


def listed(air, *args):
    return xa.mirror_air(air, list(args))


PERM, SEL, LOOKUP = ("perm", [0], [1]), ("perm", [0], [1], 2, None), ("lookup", [0], [1], 2)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_plan_degrees_and_segments(p, g):
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    for args, air, want in (([PERM], Air(3), (2, 1)), ([SEL], Air(3), (3, 2)), ([LOOKUP], Air(3), (3, 2)),
                            ([LOOKUP], Air(3).transition({("next", 0): 1, ("cur", 0, 5): -1}), (5, 4))):
        assert plan(p, g, listed(air, *args), 3, 6, 3) == want == da.plan(air, args)
        flat = listed(Air(3), *args)                                         # the superset form of the same list plans alike
        flat.xargs_always = True
        assert plan(p, g, flat, 3, 6, 3)[1] == da.plan(Air(3), args)[1]
    # a lookup list at log_blowup = 2: refused by smi_air_plan_xargs and by smi_air_plan_args, planned here
    vm = listed(Air(3), LOOKUP)
    assert plan(p, g, vm, 3, 6, 2) == (3, 2)
    cfg = _lib.StarkCfg(6, 2, 3, 1, 1, g, 0, 1)
    flat = vm.flatten(p)
    for refused in (lambda: s.engine.air_plan_xargs(p, flat, s.engine.xargs_of(flat), cfg), lambda: s.engine.air_plan_args(p, flat, flat.args, cfg)):
        with pytest.raises(s.StarkMiError) as ei:
            refused()
        assert ei.value.status == TOO_SMALL


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_every_refusal_has_its_sentence(p, g):
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    quintic = lambda: Air(3).transition({("next", 0): 1, ("cur", 0, 5): -1})
    for air, lb, status, word in ((listed(quintic(), LOOKUP), 1, BAD_ARG, "D > 2^log_blowup"),          # D = 4 > B = 2, named before B < 4
                                  (listed(Air(3), PERM), 1, TOO_SMALL, "2^log_blowup < 4"),
                                  (listed(Air(3), LOOKUP), 1, TOO_SMALL, "2^log_blowup < 4"),            # D = 2 = B
                                  (listed(Air(3).transition({("next", 0): 1, ("cur", 0, 18): -1}), PERM), 5, BAD_ARG, "4 D > 64"),
                                  (listed(Air(3).transition({("next", 0): 1, ("cur", 0, 17): -1}), PERM), 3, BAD_ARG, "D > 2^log_blowup")):
        with pytest.raises(s.StarkMiError) as ei:
            plan(p, g, air, 3, 6, lb)
        assert ei.value.status == status and word in str(ei.value), (lb, str(ei.value))
    assert plan(p, g, listed(Air(3).transition({("next", 0): 1, ("cur", 0, 17): -1}), PERM), 3, 6, 4) == (17, 16)
    # every limit of the list section, through hand-made lists
    a01, b01 = (C.c_uint32 * 2)(0, 1), (C.c_uint32 * 2)(1, 0)
    flat = Air(3).flatten(p)
    cfg = _lib.StarkCfg(6, 3, 3, 1, 1, g, 0, 1)

    def one(kind=0, width=1, mult=2, a=a01, b=b01, a_sel=_lib.NO_SELECTOR, b_sel=_lib.NO_SELECTOR, count=1):
        raw = (_lib.AirXArg * max(count, 1))()
        for i in range(max(count, 1)):
            raw[i] = _lib.AirXArg(kind, width, mult, 0, C.cast(a, _lib.u32p), C.cast(b, _lib.u32p), a_sel, b_sel)
        xs = _lib.AirXArgs(count, 0, raw)
        xs._keep = raw
        return xs
    for xs, word in ((one(count=0), "count"), (one(count=9), "count"), (one(kind=2), "kind"), (one(width=0), "width"), (one(width=9), "width"),
                     (one(a=(C.c_uint32 * 1)(3)), "next-row"), (one(b=(C.c_uint32 * 1)(6)), "variable of the AIR"), (one(a_sel=4), "a_sel"),
                     (one(b_sel=7), "b_sel"), (one(kind=1, mult=3), "mult_col must be < n_cols"), (one(kind=1, mult=0), "none of the tuple operands"),
                     (one(kind=1, mult=2, a_sel=2), "none of the selectors")):
        with pytest.raises(s.StarkMiError) as ei:
            s.engine.air_plan_deep_args(p, flat, xs, cfg)
        assert ei.value.status == BAD_ARG and word in str(ei.value), (word, str(ei.value))
    null = _lib.AirXArgs(1, 0, None)
    with pytest.raises(s.StarkMiError, match="null argument array"):
        s.engine.air_plan_deep_args(p, flat, null, cfg)
    with pytest.raises(s.StarkMiError) as ei:                                # smi_air_plan's own checks apply unchanged
        plan(p, g, listed(Air(3).transition({("next", 0): 1, ("cur", 6): -1}), PERM), 3, 6, 3)
    assert ei.value.status == BAD_ARG and "factor_var" in str(ei.value)
    with pytest.raises(s.StarkMiError, match="LDE domain too large"):
        plan(p, g, listed(Air(3), PERM), 3, 26, 3)


def test_p_3_mod_4_is_refused():
    """a prime = 3 mod 4 has two-adicity 1, so smi_air_plan's own domain check answers before the plan's sentence about the
    quartic extension can (as in smi_air_plan_deep and smi_air_plan_xargs): refused it is, at the smallest shape there is"""
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    for m in (7, 1000003):
        assert m % 4 == 3
        flat = listed(Air(3), PERM).flatten(m)
        with pytest.raises(s.StarkMiError) as ei:
            s.engine.air_plan_deep_args(m, flat, s.engine.xargs_of(flat), _lib.StarkCfg(1, 2, 3, 1, 1, 2, 0, 1))
        assert ei.value.status == -52 and "LDE domain too large" in str(ei.value)
    core = open(os.path.join(ROOT, "stark_rs_amd", "csrc", "xargs_core.h")).read()
    assert core.count("p = 3 (mod 4): the quartic extension does not exist") == 2     # smi_air_plan_xargs's sentence, kept


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_layout_length_is_the_formula(oracle, p, g):
    for args, W, log_n, lb, t in (([PERM], 3, 6, 2, 4), ([LOOKUP], 3, 6, 2, 4), ([LOOKUP, PERM, SEL], 3, 10, 3, 8), ([LOOKUP] + [PERM] * 7, 3, 20, 3, 32)):
        air = listed(Air(3), *args)
        d, D, length = plan(p, g, air, W, log_n, lb, t)
        assert (d, D) == da.plan(Air(3), args)
        assert length == da.proof_len(oracle, W, len(args), D, log_n, lb, t, p, g, g), (len(args), log_n, lb, t)


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
    assert "---- Out-of-domain sampling with an argument list" in header
    core = open(os.path.join(ROOT, "stark_rs_amd", "csrc", "deep_core.h")).read()
    for word in da.KEYWORD.values():                                         # every reason class has its sentence in the library
        assert word in core, word
