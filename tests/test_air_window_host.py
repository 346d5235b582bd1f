"""CPU, no GPU: the statement side of transition windows (include/stark_mi.h, "AIR: transition windows") -- mirror.Air's row
factors, the flattening and the numbering, smi_air_plan / smi_air_plan_deep and the layouts under a window, the degree table,
and the refusal, naming the window, of every plan that a prover or verifier outside the plain DEEP variants runs first.  The
provers' and verifiers' own refusals need a context and are in tests/test_gpu_air_window.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import deep_compose as dc
import deep_fold4_compose as dfc
import ext_compose as xc
import window_compose as wc
from stark_rs_amd.mirror import Air

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -50


def cfg_of(W, log_n, lb, g, t=0):
    from stark_rs_amd import _lib
    return _lib.StarkCfg(log_n, lb, W, 1, 1, g, t, 1)


def test_flatten_and_numbering():
    p = xc.PRIMES[0][0]
    two = Air(2).transition({("next", 0): 1, ("cur", 1): -1})
    k = two.periodic([1, 2])
    two.transition({("per_next", k): 1, ("per", k): -1, ("row", 1, 1): 1, ("per_row", 0, k): 2})
    assert two.window == 2 and two.flatten(p).window == 0                    # today's bytes: the field stays 0
    assert two.constraints[1] == [(1, [(2 * 2 + 1, 1)]), (-1, [(2 * 2, 1)]), (1, [(2 + 1, 1)]), (2, [(2 * 2, 1)])]
    for S in (3, 4):
        air = Air(3)
        j0, j1 = air.periodic([5, 6]), air.periodic([7])
        air.transition({("row", S - 1, 2): 1, ("next", 1): -1, ("cur", 0, 3): 4, ("per_row", S - 1, j1): 1, ("per", j0): 1, ("per_next", j1, 2): 1})
        W, Q = 3, 2
        assert air.window == S
        flat = air.flatten(p)
        assert flat.window == S and flat.n_factors == 6
        got = [(flat.factor_var[i], flat.factor_exp[i]) for i in range(6)]
        assert got == [((S - 1) * W + 2, 1), (W + 1, 1), (0, 3), (S * W + (S - 1) * Q + j1, 1), (S * W + j0, 1), (S * W + Q + j1, 2)]
        assert air.degree == 3
        rows = [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]][:S]
        pers = [[5, 7], [6, 7], [5, 7], [6, 7]][:S]
        assert air.constraint_value_window(0, p, rows, pers) == (rows[S - 1][2] - rows[1][1] + 4 * rows[0][0] ** 3 + pers[S - 1][1] + pers[0][0] + pers[1][1] ** 2) % p
    with pytest.raises(ValueError, match="row shift"):
        Air(1).transition({("row", 4, 0): 1})
    with pytest.raises(ValueError):
        Air(2).add_permutation([("row", 2, 0)], [1])                         # tuple members stay this-row operands
    usage = Air(1).transition({("row", 2, 0): 1, ("row", 1, 0): -1, ("row", 0, 0): -1})   # the README's two lines
    assert usage.window == 3 and usage.first_violation(p, [[1, 1, 2, 3, 5, 8, 13, 21]]) is None
    assert usage.first_violation(p, [[1, 1, 2, 3, 5, 8, 13, 22]]) == (0, 5)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_window_0_and_2_plan_as_today(oracle, p, g):
    import stark_rs_amd as s
    s.build()
    for air, W, log_n in ((ac.make("fib", 64, p)[0], 2, 6), (ac.make("mixer", 64, p)[0], 4, 6), (ap.make("mimc", 64, p)[0], 1, 6)):
        flat0, flat2 = air.flatten(p), air.flatten(p)
        flat2.window = 2
        for lb in (2, 3, 4):
            cfg = cfg_of(W, log_n, lb, g, 4)
            want = s.engine.air_plan_deep(p, flat0, cfg, True)
            assert want[:2] == dc.plan(air) and want[2] == dc.proof_len(oracle, W, want[1], log_n, lb, 4, p, g, g)
            assert s.engine.air_plan_deep(p, flat2, cfg, True) == want
            assert s.engine.air_deep_fold4_layout(p, flat2, cfg) == s.engine.air_deep_fold4_layout(p, flat0, cfg)
            try:
                e0 = s.engine.air_plan(p, flat0, cfg)
            except s.StarkMiError as e:
                with pytest.raises(s.StarkMiError) as ei:
                    s.engine.air_plan(p, flat2, cfg)
                assert str(ei.value) == str(e)
            else:
                assert s.engine.air_plan(p, flat2, cfg) == e0


def power_window_air(d, S):
    """one column: a[r + S - 1] = a[r]^d"""
    return Air(1).transition({("row", S - 1, 0): 1, ("row", 0, 0, d): -1}) if S > 2 else Air(1).transition({("next", 0): 1, ("cur", 0, d): -1})


def test_degree_table():
    """D doubles for exactly (d, S) in {(2, 3), (2, 4), (3, 4)}"""
    import stark_rs_amd as s
    s.build()
    p, g = xc.PRIMES[0]
    doubles = {(2, 3), (2, 4), (3, 4)}
    for d in range(1, 10):
        for S in (2, 3, 4):
            for log_n in (2, 6, 10):
                base = 1
                while base < d - 1:
                    base <<= 1
                air = power_window_air(d, S)
                got = s.engine.air_plan_deep(p, air.flatten(p), cfg_of(1, log_n, 4, g))
                assert got == (d, base * (2 if (d, S) in doubles else 1)) == wc.plan(air, log_n), (d, S, log_n, got)
    for d, S in ((1, 3), (1, 4), (3, 3), (4, 4), (5, 4)):
        assert wc.segments_for(d, S, 64) == dc.plan(power_window_air(d, 2))[1]
    # smi_air_plan: E = B / D with the same D
    assert s.engine.air_plan(p, power_window_air(2, 3).flatten(p), cfg_of(1, 6, 3, g)) == (2, 4)
    with pytest.raises(s.StarkMiError) as ei:
        s.engine.air_plan(p, power_window_air(2, 3).flatten(p), cfg_of(1, 6, 2, g))
    assert ei.value.status == -10


def test_refusals_of_the_statement():
    import stark_rs_amd as s
    s.build()
    p, g = xc.PRIMES[0]
    fib1 = wc.make("fib1", 64, p)[0]
    for w, word in ((1, "window"), (5, "window"), (1 << 31, "window")):
        flat = fib1.flatten(p)
        flat.window = w
        for plan in (s.engine.air_plan, s.engine.air_plan_deep):
            with pytest.raises(s.StarkMiError) as ei:
                plan(p, flat, cfg_of(1, 6, 3, g))
            assert ei.value.status == BAD_ARG and word in str(ei.value)
    for S, log_n, ok in ((3, 1, False), (4, 1, False), (3, 2, True), (4, 2, True)):   # n >= S
        flat = power_window_air(1, S).flatten(p)
        if ok:
            assert s.engine.air_plan_deep(p, flat, cfg_of(1, log_n, 3, g)) == (1, 1)
        else:
            with pytest.raises(s.StarkMiError, match="window") as ei:
                s.engine.air_plan_deep(p, flat, cfg_of(1, log_n, 3, g))
            assert ei.value.status == BAD_ARG
    for S in (3, 4):                                                        # factor_var = S (W + Q) is one past the last variable
        air = Air(2)
        air.periodic([1, 2])
        air.transition({("row", S - 1, 0): 1, ("per_row", S - 1, 0): 1})
        flat = air.flatten(p)
        assert max(flat.factor_var[i] for i in range(flat.n_factors)) == S * 3 - 1
        assert s.engine.air_plan_deep(p, flat, cfg_of(2, 6, 3, g))[0] == 1
        flat.factor_var[1] = S * 3
        with pytest.raises(s.StarkMiError, match="factor_var") as ei:
            s.engine.air_plan_deep(p, flat, cfg_of(2, 6, 3, g))
        assert ei.value.status == BAD_ARG
    two = Air(1).transition({("next", 0): 1, ("cur", 0): -1}).flatten(p)     # the two-row refusal keeps its sentence
    two.factor_var[0] = 2
    with pytest.raises(s.StarkMiError, match=r"row shifts 0 and 1 only"):
        s.engine.air_plan(p, two, cfg_of(1, 6, 3, g))


def test_every_other_plan_refuses_a_window():
    """the plan that each out-of-scope prover and verifier runs first: SMI_ERR_BAD_ARG with `window` in the sentence"""
    import stark_rs_amd as s
    s.build()
    p, g = xc.PRIMES[0]
    E = s.engine

    def windowed(build=None):
        air = Air(3).transition({("row", 2, 0): 1, ("row", 1, 0): -1, ("row", 0, 0): -1})
        if build:
            build(air)
        return air.flatten(p)
    cfg = cfg_of(3, 8, 3, g, 4)
    cases = []
    f = windowed(lambda a: a.permutation([0], [1]))
    cases.append(lambda: E.air_plan_perm(p, f, f.perm, cfg))
    f2 = windowed(lambda a: a.lookup([0], [1], 2))
    cases.append(lambda: E.air_plan_lookup(p, f2, f2.lookup, cfg))
    f3 = windowed(lambda a: a.add_permutation([0], [1]))
    cases.append(lambda: E.air_plan_args(p, f3, f3.args, cfg))
    f4 = windowed(lambda a: a.add_permutation([0], [1], left_sel=2))
    cases.append(lambda: E.air_plan_xargs(p, f4, f4.xargs, cfg))
    cases.append(lambda: E.air_plan_deep_args(p, f4, f4.xargs, cfg))
    cases.append(lambda: E.air_deep_args_fold4_layout(p, f4, f4.xargs, cfg))
    cases.append(lambda: E.air_plan_deep_zk_args(p, f4, f4.xargs, cfg))
    cases.append(lambda: E.air_deep_zk_args_layout(p, f4, f4.xargs, cfg))
    f5 = windowed()
    cases.append(lambda: E.air_plan_deep_zk(p, f5, cfg))
    cases.append(lambda: E.air_deep_zk_layout(p, f5, cfg))
    for i, call in enumerate(cases):
        with pytest.raises(s.StarkMiError, match="window") as ei:
            call()
        assert ei.value.status == BAD_ARG, i
    assert E.air_plan_deep(p, f5, cfg) == (1, 1)                              # the plain DEEP plan takes it


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_layout_lengths_are_the_formula(oracle, p, g):
    import stark_rs_amd as s
    s.build()
    for name, log_n, lb, t in (("fib1", 6, 2, 4), ("sq", 8, 3, 6), ("tap4", 10, 2, 8), ("wide", 7, 3, 5), ("wide", 20, 3, 32)):
        n = 1 << min(log_n, 10)
        air = wc.make(name, n, p)[0]
        if name == "tap4":
            assert len(air.periodics[0]) == 8
        W, S = air.n_cols, air.window
        flat, cfg = air.flatten(p), cfg_of(air.n_cols, log_n, lb, g, t)
        d, D, length = s.engine.air_plan_deep(p, flat, cfg, True)
        assert (d, D) == wc.plan(air, log_n)
        assert length == wc.proof_len(oracle, W, D, S, log_n, lb, t, p, g, g) == dc.proof_len(oracle, W, D, log_n, lb, t, p, g, g) + 32 * (S - 2) * W
        folds, flen = s.engine.air_deep_fold4_layout(p, flat, cfg)
        assert (folds, flen) == wc.fold4_layout(W, D, S, log_n, lb, t)
        assert wc.transcript_len(W, len(air.constraints), D, 2) == 32 * (3 + W + len(air.constraints) + 2 * (2 * W + D))


def test_plans_and_layouts_under_a_caller_s_offsets(oracle):
    """smi_air_plan_deep with its length and smi_air_deep_fold4_layout under (trace_offset, lde_offset) other than (1, g) give
    the length of the proof made under them -- the restated proofs, which tests/test_gpu_deep_offsets.py holds the device's
    equal to -- for a two-row statement and a window statement, over row leaves and over coset leaves"""
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    s.build()
    p, g = xc.PRIMES[0]
    t = 4
    for name, window, log_n, lb in (("mimc", False, 6, 3), ("tap4", True, 5, 3)):
        air, cols = wc.make(name, 1 << log_n, p) if window else ap.make(name, 1 << log_n, p)
        W, S, flat = len(cols), air.window, air.flatten(p)
        d, D = wc.plan(air, log_n)
        assert dfc.folds(log_n, lb, t) >= 1
        for tau, h in ((5, 11), (1, 11), (5, g), (p - 1, p - 2)):
            N = 1 << (log_n + lb)
            assert pow(h, N, p) != 1 and pow(h * pow(tau, p - 2, p) % p, N, p) != 1
            cfg = _lib.StarkCfg(log_n, lb, W, 1, tau, h, t, 1)
            rows = wc.prove(oracle, air, cols, p, g, log_n, lb, t, tau, h) if window else dc.prove(oracle, air, cols, p, g, log_n, lb, t, tau, h)
            cosets = wc.prove(oracle, air, cols, p, g, log_n, lb, t, tau, h, 0, True) if window else dfc.prove(oracle, air, cols, p, g, log_n, lb, t, tau, h)
            assert s.engine.air_plan_deep(p, flat, cfg, True) == (d, D, len(rows["proof"])), (name, tau, h)
            assert len(rows["proof"]) == wc.proof_len(oracle, W, D, S, log_n, lb, t, p, g, h)
            assert s.engine.air_deep_fold4_layout(p, flat, cfg) == (dfc.folds(log_n, lb, t), len(cosets["proof"])), (name, tau, h)
            assert len(cosets["proof"]) == wc.fold4_layout(W, D, S, log_n, lb, t)[1]


def test_declarations():
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    s.build()
    declared = s.declared_symbols()
    header = open(os.path.join(ROOT, "include", "stark_mi.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "stark_mi.rs")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("smi_dev_poly_eval_ext_shifts", "smi_dev_deep_compose_window"):
        assert name in declared and hasattr(lib, name)
        assert re.search(r"pub fn " + name + r"\(", rust), name
    assert "#define SMI_AIR_MAX_WINDOW 4" in header and "pub const SMI_AIR_MAX_WINDOW: u32 = 4;" in rust
    assert "---- AIR: transition windows" in header
    assert "row shifts other than 0 and 1" not in header
    assert re.search(r"pub n_periodic: u32,\s*pub window: u32,", rust)
    assert np.dtype(np.uint32).itemsize * 2 == _lib.Air.periodic_log_period.offset - _lib.Air.n_periodic.offset   # the field kept its place
