"""CPU: the host side of the argument list with selectors and periodic members -- smi_air_plan_xargs through libstarkmi.so
without a context (degrees, E, every refusal with its reason), and how mirror.Air flattens a list: to smi_air_xargs only when
some argument has a selector or a periodic member, to smi_air_args otherwise, so that existing callers keep their path."""
import ctypes as C

import pytest

import ext_compose as xc
import xargs_compose as xg

P, G = xc.PRIMES[0]
BAD_ARG, TOO_SMALL = -50, -10


def air_of(W=6, periods=(4, 1), degree=1):
    from stark_rs_amd.mirror import Air
    air = Air(W)
    for per in periods:
        air.periodic(list(range(1, per + 1)))
    if degree > 1:
        air.transition({("next", 0): 1, ("cur", 0, degree): -1})
    return air


def plan(air, log_n=4, lb=3):
    """-> (d, E) or (status, reason)"""
    import stark_rs_amd
    from stark_rs_amd import _lib, engine
    stark_rs_amd.build()
    f = air.flatten(P)
    assert f.xargs is not None
    cfg = _lib.StarkCfg(log_n, lb, air.n_cols, 1, 1, G, 0, 1)
    try:
        return engine.air_plan_xargs(P, f, f.xargs, cfg)
    except _lib.StarkMiError as e:
        return e.status, str(e)


def test_flattening_routes_on_selectors_and_periodic_members():
    air = air_of().add_permutation([0], [1]).add_lookup([2], [3], 4)
    f = air.flatten(P)
    assert not air.extended_args and f.args is not None and f.xargs is None and f.args.count == 2
    for more in (lambda a: a.add_permutation([0], [1], left_sel=5), lambda a: a.add_lookup([2], [("per", 0)], 4),
                 lambda a: a.add_lookup([2], [3], 4, table_sel=("per", 1))):
        air = air_of().add_permutation([0], [1])
        more(air)
        f = air.flatten(P)
        assert air.extended_args and f.args is None and f.xargs.count == 2
    air = air_of().add_lookup([2, ("per", 1)], [("per", 0), 3], 4, sel=1, table_sel=("per", 1))
    g = air.flatten(P).xargs.arg[0]
    assert (g.kind, g.width, g.mult_col, g.a_sel, g.b_sel) == (1, 2, 4, 1, 2 * 6 + 1)
    assert [g.a_var[0], g.a_var[1], g.b_var[0], g.b_var[1]] == [2, 13, 12, 3]
    air = air_of().add_permutation([0], [("per", 0)])
    g = air.flatten(P).xargs.arg[0]
    assert g.a_sel == g.b_sel == 0xffffffff
    with pytest.raises(ValueError, match="next-row"):
        air_of().add_permutation([("per_next", 0)], [1])


@pytest.mark.parametrize("degree", [1, 2, 3, 5])
def test_plan_degrees(degree):
    """a permutation contributes 2 without a selector and 3 with one or two, a lookup 3; d = max(d_air, ...)"""
    cases = [(lambda a: a.add_permutation([0], [("per", 0)]), 2),
             (lambda a: a.add_permutation([0], [1], left_sel=2), 3),
             (lambda a: a.add_permutation([0], [1], left_sel=2, right_sel=("per", 1)), 3),
             (lambda a: a.add_lookup([0], [("per", 0)], 3), 3),
             (lambda a: a.add_lookup([0], [1], 3, sel=2, table_sel=4), 3)]
    for add, contrib in cases:
        air = air_of(degree=degree)
        add(air)
        d = max(degree, contrib)
        assert xg.plan(air, air.args, 4)[0] == d
        D = 1
        while D < d - 1:
            D *= 2
        assert plan(air, lb=4) == (d, 16 // D)


def test_a_selected_permutation_needs_the_blowup_of_a_lookup():
    air = air_of().add_permutation([0], [("per", 0)])
    assert plan(air, lb=2) == (2, 4)
    air = air_of().add_permutation([0], [1], left_sel=2)
    st, why = plan(air, lb=2)
    assert st == TOO_SMALL and "xargs: 2^log_blowup / D < 4" in why


def raw_plan(build):
    """smi_air_plan_xargs over a hand-made smi_air_xargs (what mirror.Air would not let through) -> (status, reason)"""
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = _lib.lib()
    f = air_of().flatten(P)   # W = 6, Q = 2: this-row variables 0 .. 5 and 12, 13
    arr = lambda v: (C.c_uint32 * len(v))(*v)
    items = build(arr)
    raw = (_lib.AirXArg * len(items))(*items)
    xs = _lib.AirXArgs(len(items), 0, raw)
    cfg = _lib.StarkCfg(4, 3, 6, 1, 1, G, 0, 1)
    d, e = C.c_uint32(), C.c_uint64()
    st = L.smi_air_plan_xargs(P, C.byref(cfg), C.byref(f), C.byref(xs), C.byref(d), C.byref(e))
    return st, L.smi_air_last_error().decode()


NONE = 0xffffffff


@pytest.mark.parametrize("name,make,needle", [
    ("next-row trace member", lambda X, arr: [X(0, 1, 0, 0, arr([6]), arr([1]), NONE, NONE)], "argument 0: a_var is a next-row variable"),
    ("next-row periodic member", lambda X, arr: [X(0, 1, 0, 0, arr([0]), arr([14]), NONE, NONE)], "argument 0: b_var is a next-row variable"),
    ("next-row selector", lambda X, arr: [X(0, 1, 0, 0, arr([0]), arr([1]), NONE, NONE), X(0, 1, 0, 0, arr([0]), arr([1]), 15, NONE)],
     "argument 1: a_sel is a next-row variable"),
    ("operand out of range", lambda X, arr: [X(1, 1, 3, 0, arr([0]), arr([16]), NONE, NONE)], "argument 0: b_var must be a variable of the AIR"),
    ("selector out of range", lambda X, arr: [X(1, 1, 3, 0, arr([0]), arr([1]), NONE, 99)], "argument 0: b_sel must be a variable of the AIR"),
    ("mult_col among the operands", lambda X, arr: [X(1, 2, 3, 0, arr([0, 3]), arr([1, 12]), NONE, NONE)], "argument 0: mult_col must be none of the tuple operands"),
    ("mult_col among the selectors", lambda X, arr: [X(1, 1, 3, 0, arr([0]), arr([12]), NONE, 3)], "argument 0: mult_col must be none of the selectors"),
    ("mult_col periodic", lambda X, arr: [X(1, 1, 12, 0, arr([0]), arr([1]), NONE, NONE)], "argument 0: mult_col must be < n_cols"),
    ("width 0", lambda X, arr: [X(0, 0, 0, 0, arr([0]), arr([1]), NONE, NONE)], "argument 0: width must be in 1 .. 8"),
    ("width 9", lambda X, arr: [X(0, 9, 0, 0, arr([0] * 9), arr([1] * 9), NONE, NONE)], "argument 0: width must be in 1 .. 8"),
    ("kind 2", lambda X, arr: [X(2, 1, 0, 0, arr([0]), arr([1]), NONE, NONE)], "argument 0: kind must be"),
    ("nine arguments", lambda X, arr: [X(0, 1, 0, 0, arr([0]), arr([1]), NONE, NONE)] * 9, "count must be in 1 .. SMI_ARGS_MAX"),
])
def test_refusals_name_the_argument(name, make, needle):
    from stark_rs_amd import _lib
    keep = []

    def arr(v):
        keep.append((C.c_uint32 * len(v))(*v))
        return C.cast(keep[-1], _lib.u32p)
    st, why = raw_plan(lambda _arr: make(_lib.AirXArg, arr))
    assert st == BAD_ARG and needle in why, (name, why)


def test_an_accepted_list_clears_the_reason():
    from stark_rs_amd import _lib
    st, why = raw_plan(lambda arr: [_lib.AirXArg(1, 1, 3, 0, C.cast(arr([0]), _lib.u32p), C.cast(arr([12]), _lib.u32p), 13, NONE)])
    assert (st, why) == (0, "")
