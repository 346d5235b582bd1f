"""CPU: the host side of next-row operands in argument lists (include/stark_mi.h, "Argument list: next-row operands") --
the plans and layouts through libstarkmi.so without a context, every refusal with its reason, and how mirror.Air spells and
flattens such an operand."""
import ctypes as C

import pytest

import ext_compose as xc
import xargs_next_compose as xn

P, G = xc.PRIMES[0]
BAD_ARG = -50
NONE, NEXT = 0xffffffff, 0x40000000
W = xn.W_SCENE


def cfg_of(log_n, lb, t=4):
    from stark_rs_amd import _lib
    return _lib.StarkCfg(log_n, lb, W, 1, 1, G, t, 1)


def every_plan(air, args, log_n, lb):
    """-> the (d, E), (d, D, proof bytes) and (folds, proof bytes) of the three layouts for air carrying args"""
    import stark_rs_amd
    from stark_rs_amd import engine
    stark_rs_amd.build()
    f = xn.mirror(air, args).flatten(P)
    cfg = cfg_of(log_n, lb)
    return (engine.air_plan_xargs(P, f, f.xargs, cfg), engine.air_plan_deep_args(P, f, f.xargs, cfg, with_length=True),
            engine.air_deep_args_fold4_layout(P, f, f.xargs, cfg))


@pytest.mark.parametrize("shared,lb", [(False, 3), (True, 4)])
def test_a_list_with_flags_plans_as_the_list_with_the_flags_stripped(shared, lb):
    air, cols, args = xn.scene(32, P, 8, shared=shared)
    assert xn.has_next(args) and not xn.has_next(xn.strip(args))
    got, want = every_plan(air, args, 5, lb), every_plan(air, xn.strip(args), 5, lb)
    assert got == want
    assert got[0][0] == (4 if shared else 3)


def test_mirror_spellings():
    from stark_rs_amd.mirror import Air
    air = Air(6)
    j = air.periodic([1, 2, 3, 4])
    air.add_lookup([0, 1, ("next", 0)], [("per", j), ("next", ("per", j)), 3], 2, sel=("next", 4), table_sel=("next", ("per", j)))
    assert air.extended_args
    g = air.flatten(P).xargs.arg[0]
    assert [g.a_var[i] for i in range(3)] == [0, 1, NEXT | 0]
    assert [g.b_var[i] for i in range(3)] == [12 + j, NEXT | (12 + j), 3]
    assert (g.a_sel, g.b_sel, g.mult_col) == (NEXT | 4, NEXT | (12 + j), 2)
    air = Air(3).add_permutation([0], [("next", 0)])   # a next-row member alone takes the smi_*_xargs route
    f = air.flatten(P)
    assert air.extended_args and f.args is None and f.xargs.arg[0].b_var[0] == NEXT
    air = Air(6)
    air.periodic([1, 2])
    air.add_lookups([[("next", 0)], [1]], [("per", 0)], 2, sels=[None, ("next", ("per", 0))])
    g = air.flatten(P).xargs.arg[0]
    assert [g.a_var[i] for i in range(4)] == [NEXT | 0, 1, NONE, NEXT | 12]
    for bad in (("per_next", 0), ("next", ("next", 0)), ("next", ("per_next", 0)), ("nxt", 0)):
        with pytest.raises(ValueError, match="next-row"):
            Air(3).add_permutation([bad], [1])


def raw_plan(build, zk=False):
    """smi_air_plan_xargs (or the zero-knowledge plan) over a hand-made smi_air_xargs -> (status, reason)"""
    import stark_rs_amd
    from stark_rs_amd import _lib
    from stark_rs_amd.mirror import Air
    stark_rs_amd.build()
    L = _lib.lib()
    air = Air(6)   # W = 6, Q = 2: this-row variables 0 .. 5 and 12, 13
    air.periodic([1, 2, 3, 4])
    air.periodic([1])
    f = air.flatten(P)
    keep = []

    def arr(v):
        keep.append((C.c_uint32 * len(v))(*v))
        return C.cast(keep[-1], _lib.u32p)
    items = build(_lib.AirXArg, arr)
    raw = (_lib.AirXArg * len(items))(*items)
    xs = _lib.AirXArgs(len(items), 0, raw)
    cfg = _lib.StarkCfg(8 if zk else 4, 3, 6, 1, 1, G, 2, 1)
    d, e, D, kt, ks = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    if zk:
        st = L.smi_air_plan_deep_zk_xargs(P, C.byref(cfg), C.byref(f), C.byref(xs), C.byref(d), C.byref(D), C.byref(kt), C.byref(ks))
    else:
        st = L.smi_air_plan_xargs(P, C.byref(cfg), C.byref(f), C.byref(xs), C.byref(d), C.byref(e))
    return st, L.smi_air_last_error().decode()


@pytest.mark.parametrize("name,make,needle", [
    ("the flag on mult_col", lambda X, arr: [X(1, 1, NEXT | 3, 0, arr([0]), arr([12]), NONE, NONE)], "argument 0: mult_col must be < n_cols"),
    ("next(mult_col) as a member", lambda X, arr: [X(1, 2, 3, 0, arr([0, NEXT | 3]), arr([1, 12]), NONE, NONE)], "argument 0: mult_col must be none of the tuple operands"),
    ("next(mult_col) as a table member", lambda X, arr: [X(1, 1, 3, 0, arr([0]), arr([NEXT | 3]), NONE, NONE)], "argument 0: mult_col must be none of the tuple operands"),
    ("next(mult_col) as a selector", lambda X, arr: [X(1, 1, 3, 0, arr([0]), arr([12]), NONE, NEXT | 3)], "argument 0: mult_col must be none of the selectors"),
    ("next(mult_col) as a tuple selector", lambda X, arr: [X(1 | 1 << 8, 1, 3, 0, arr([0, 1, NONE, NEXT | 3]), arr([12]), NONE, NONE)],
     "argument 0: mult_col must be none of the selectors"),
    ("bit 31 beside the flag", lambda X, arr: [X(0, 1, 0, 0, arr([0x80000000 | NEXT | 1]), arr([1]), NONE, NONE)], "argument 0: a_var must be a variable of the AIR"),
    ("bit 31 alone", lambda X, arr: [X(0, 1, 0, 0, arr([0]), arr([0x80000000 | 1]), NONE, NONE)], "argument 0: b_var must be a variable of the AIR"),
    ("bit 29 beside the flag", lambda X, arr: [X(0, 1, 0, 0, arr([0]), arr([1]), NEXT | 0x20000000 | 1, NONE)], "argument 0: a_sel must be a variable of the AIR"),
    ("the flag on the AIR's next-row trace variable", lambda X, arr: [X(0, 1, 0, 0, arr([NEXT | 6]), arr([1]), NONE, NONE)], "argument 0: a_var is a next-row variable"),
    ("the flag on the AIR's next-row periodic variable", lambda X, arr: [X(0, 1, 0, 0, arr([0]), arr([NEXT | 14]), NONE, NONE)], "argument 0: b_var is a next-row variable"),
    ("the flag on a column out of range", lambda X, arr: [X(0, 1, 0, 0, arr([0]), arr([NEXT | 16]), NONE, NONE)], "argument 0: b_var must be a variable of the AIR"),
])
def test_refusals_name_the_argument(name, make, needle):
    st, why = raw_plan(make)
    assert st == BAD_ARG and needle in why, (name, why)


def test_accepted_operands_clear_the_reason():
    st, why = raw_plan(lambda X, arr: [X(1, 2, 3, 0, arr([NEXT | 0, 1]), arr([NEXT | 12, 13]), NEXT | 4, NEXT | 13),
                                       X(0, 1, 0, 0, arr([0]), arr([NEXT | 0]), NONE, NONE)])
    assert st == 0 and why == ""


@pytest.mark.parametrize("name,make,needle", [
    ("a member", lambda X, arr: [X(0, 1, 0, 0, arr([0]), arr([1]), NONE, NONE), X(0, 1, 0, 0, arr([0]), arr([NEXT | 0]), NONE, NONE)], "argument 1: b_var is a next-row operand"),
    ("a selector", lambda X, arr: [X(1, 1, 3, 0, arr([0]), arr([12]), NEXT | 13, NONE)], "argument 0: a_sel is a next-row operand"),
    ("a tuple selector", lambda X, arr: [X(1 | 1 << 8, 1, 3, 0, arr([0, 1, NONE, NEXT | 4]), arr([12]), NONE, NONE)], "argument 0: a tuple selector is a next-row operand"),
])
def test_the_zero_knowledge_plan_refuses(name, make, needle):
    st, why = raw_plan(make, zk=True)
    assert st == BAD_ARG and why.startswith("zk deep argument: ") and needle in why, (name, why)
    strip = lambda X, arr: [X(g.kind, g.width, g.mult_col, 0, g.a_var, g.b_var, g.a_sel if g.a_sel == NONE else g.a_sel & ~NEXT, g.b_sel) for g in make(X, arr)]
    if name == "a selector":   # the same list without the flag is planned
        st, why = raw_plan(strip, zk=True)
        assert st == 0, why
