"""CPU: the host side of shared-table lookups (include/stark_mi.h, "Shared-table lookups") through libstarkmi.so without a
context -- the degree a shared lookup of J tuples contributes in the three plans and the D (or D') that follows, every refusal
by its sentence, the encoding of J in the second byte of kind, and how mirror.Air flattens add_lookups."""
import ctypes as C

import pytest

import ext_compose as xc
import shared_lookup_compose as sl
import zk_args_compose as za

P, G = xc.PRIMES[0]
BAD_ARG, TOO_SMALL = -50, -10
NONE = 0xffffffff


def air_of(J, W=12, degree=1):
    """J tuples of width 2 into the table (c0, per 0), multiplicities in column 11"""
    from stark_rs_amd.mirror import Air
    air = Air(W)
    air.periodic([1, 2, 3, 4])
    if degree > 1:
        air.transition({("next", 0): 1, ("cur", 0, degree): -1})
    return air.add_lookups([[1 + 2 * j, 2 + 2 * j] for j in range(J)], [0, ("per", 0)], 11, [None, 9, ("per", 0), 10][:J])


def plans(air, log_n, lb, t=1):
    """-> ((d, E) | status, (d, D) | status, (d, D', k_t, k_s) | status) of the three plan functions"""
    import stark_rs_amd
    from stark_rs_amd import _lib, engine
    stark_rs_amd.build()
    f = air.flatten(P)
    assert f.xargs is not None and f.args is None
    cfg = _lib.StarkCfg(log_n, lb, air.n_cols, 1, 1, G, t, 1)
    out = []
    for fn in (engine.air_plan_xargs, engine.air_plan_deep_args, engine.air_plan_deep_zk_args):
        try:
            out.append(fn(P, f, f.xargs, cfg))
        except _lib.StarkMiError as e:
            out.append(e.status)
    return tuple(out)


@pytest.mark.parametrize("degree", [1, 4, 7])
@pytest.mark.parametrize("J", [1, 2, 3, 4])
def test_plan_degrees_and_segments(J, degree):
    """J + 2 in smi_air_plan_xargs and smi_air_plan_deep_xargs, J + 3 in smi_air_plan_deep_zk_xargs (where the AIR's own degree
    counts one more); D is the power of two at or above d - 1, E = B / D, D' = ceil(D n / (n - k_s))"""
    log_n, lb, t = 7, 5, 1
    n = 1 << log_n
    air = air_of(J, degree=degree)
    assert sl.contribution(air.args[0]) == J + 2 and sl.contribution(air.args[0], zk=True) == J + 3
    d, dz = max(degree, J + 2), max(degree + 1 if degree > 1 else 1, J + 3)
    D, Dz = sl.segments(d), sl.segments(dz)
    assert plans(air, log_n, lb, t) == ((d, (1 << lb) // D), (d, D), (dz, -(-Dz * n // (n - za.k_s(t))), za.k_t(t), za.k_s(t)))
    if degree == 1:
        assert D == {1: 2, 2: 4, 3: 4, 4: 8}[J] and Dz == {1: 4, 2: 4, 3: 8, 4: 8}[J]


def test_the_blowup_each_variant_needs():
    """row leaves need E >= 4: J = 2, 3 log_blowup 4, J = 4 log_blowup 5; DEEP needs D <= B: J = 2, 3 log_blowup 2, J = 4
    log_blowup 3; under zk J = 2 stays at log_blowup 2 as a single lookup does, J = 3, 4 need 3"""
    need = {1: (3, 2, 2), 2: (4, 2, 2), 3: (4, 2, 3), 4: (5, 3, 3)}
    for J, lbs in need.items():
        for k, lb in enumerate(lbs):
            assert not isinstance(plans(air_of(J), 7, lb)[k], int), (J, k, lb)
            if lb > 2:
                assert plans(air_of(J), 7, lb - 1)[k] == (TOO_SMALL if k == 0 else BAD_ARG), (J, k, lb)


def test_flattening():
    from stark_rs_amd import _lib
    air = air_of(3)
    assert air.extended_args and air.args[0][0] == "lookups"
    g = air.flatten(P).xargs.arg[0]
    assert (_lib.ARG_TUPLES_SHIFT, _lib.ARG_MAX_TUPLES) == (8, 4)
    assert (g.kind, g.width, g.mult_col, g.a_sel, g.b_sel) == (1 | 2 << 8, 2, 11, NONE, NONE)
    assert [g.a_var[i] for i in range(9)] == [1, 2, 3, 4, 5, 6, NONE, 9, 2 * 12 + 0]
    assert [g.b_var[i] for i in range(2)] == [0, 24]
    one = air_of(1)                                                      # one tuple is add_lookup: the value SMI_ARG_LOOKUP itself
    assert one.args[0][0] == "lookup" and one.flatten(P).xargs.arg[0].kind == 1
    from stark_rs_amd.mirror import Air
    with pytest.raises(ValueError, match="1 .. 4 tuples"):
        Air(12).add_lookups([[1]] * 5, [0], 11)
    with pytest.raises(ValueError, match="one width"):
        Air(12).add_lookups([[1], [2, 3]], [0], 11)
    with pytest.raises(ValueError, match="one selector"):
        Air(12).add_lookups([[1], [2]], [0], 11, [None])


def raw_plan(items, log_n=4, lb=5, p=P, g=G, which="smi_air_plan_xargs"):
    """a plan function over a hand-made smi_air_xargs -> (status, reason); W = 12, Q = 1: this-row variables 0 .. 11 and 24"""
    import stark_rs_amd
    from stark_rs_amd import _lib
    from stark_rs_amd.mirror import Air
    stark_rs_amd.build()
    L = _lib.lib()
    air = Air(12)
    air.periodic([1, 2, 3, 4])
    f = air.flatten(p)
    raw = (_lib.AirXArg * len(items))(*items)
    xs = _lib.AirXArgs(len(items), 0, raw)
    cfg = _lib.StarkCfg(log_n, lb, 12, 1, 1, g, 1, 1)
    d, e, x, y = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint32()
    if which == "smi_air_plan_xargs":
        st = L.smi_air_plan_xargs(p, C.byref(cfg), C.byref(f), C.byref(xs), C.byref(d), C.byref(e))
    elif which == "smi_air_plan_deep_xargs":
        st = L.smi_air_plan_deep_xargs(p, C.byref(cfg), C.byref(f), C.byref(xs), C.byref(d), C.byref(x))
    else:
        st = L.smi_air_plan_deep_zk_xargs(p, C.byref(cfg), C.byref(f), C.byref(xs), C.byref(d), C.byref(x), C.byref(y), C.byref(y))
    return st, L.smi_air_last_error().decode(), d.value


KIND = lambda J: 1 | (J - 1) << 8


@pytest.mark.parametrize("name,make,needle", [
    ("tuple bits on a permutation", lambda X, arr: [X(0 | 1 << 8, 1, 0, 0, arr([0, 1, NONE, NONE]), arr([2]), NONE, NONE)],
     "argument 0: a permutation takes no tuple count"),
    ("five tuples", lambda X, arr: [X(KIND(5), 1, 11, 0, arr([1, 2, 3, 4, 5] + [NONE] * 5), arr([0]), NONE, NONE)],
     "argument 0: a shared lookup has at most SMI_ARG_MAX_TUPLES (4) tuples"),
    ("bits above the second byte", lambda X, arr: [X(1 | 1 << 16, 1, 11, 0, arr([1]), arr([0]), NONE, NONE)], "argument 0: kind must be SMI_ARG_PERM (0) or SMI_ARG_LOOKUP (1)"),
    ("kind 2", lambda X, arr: [X(2, 1, 11, 0, arr([1]), arr([0]), NONE, NONE)], "argument 0: kind must be SMI_ARG_PERM (0) or SMI_ARG_LOOKUP (1)"),
    ("kind 2 with tuple bits", lambda X, arr: [X(2 | 1 << 8, 1, 11, 0, arr([1, 2, NONE, NONE]), arr([0]), NONE, NONE)], "argument 0: kind must be"),
    ("a set a_sel", lambda X, arr: [X(0, 1, 0, 0, arr([0]), arr([1]), NONE, NONE), X(KIND(2), 1, 11, 0, arr([1, 2, NONE, NONE]), arr([0]), 3, NONE)],
     "argument 1: a shared lookup keeps its selectors behind the tuples in a_var: a_sel must be SMI_ARG_NO_SELECTOR"),
    ("a next-row operand in a tuple", lambda X, arr: [X(KIND(3), 2, 11, 0, arr([1, 2, 3, 4, 5, 12 + 6, NONE, NONE, NONE]), arr([0, 24]), NONE, NONE)],
     "argument 0: tuple 2: a_var is a next-row variable"),
    ("a next-row periodic operand in a tuple", lambda X, arr: [X(KIND(2), 1, 11, 0, arr([1, 25, NONE, NONE]), arr([0]), NONE, NONE)],
     "argument 0: tuple 1: a_var is a next-row variable"),
    ("a next-row selector", lambda X, arr: [X(KIND(2), 1, 11, 0, arr([1, 2, NONE, 12 + 3]), arr([0]), NONE, NONE)],
     "argument 0: tuple 1: selector is a next-row variable"),
    ("a selector out of range", lambda X, arr: [X(KIND(2), 1, 11, 0, arr([1, 2, 99, NONE]), arr([0]), NONE, NONE)],
     "argument 0: tuple 0: selector must be a variable of the AIR"),
    ("mult_col in a later tuple", lambda X, arr: [X(KIND(2), 1, 11, 0, arr([1, 11, NONE, NONE]), arr([0]), NONE, NONE)],
     "argument 0: mult_col must be none of the tuple operands"),
    ("mult_col among the tuples' selectors", lambda X, arr: [X(KIND(2), 1, 11, 0, arr([1, 2, NONE, 11]), arr([0]), NONE, NONE)],
     "argument 0: mult_col must be none of the selectors"),
])
def test_refusals_name_the_argument(name, make, needle):
    from stark_rs_amd import _lib
    keep = []

    def arr(v):
        keep.append((C.c_uint32 * len(v))(*v))
        return C.cast(keep[-1], _lib.u32p)
    for which in ("smi_air_plan_xargs", "smi_air_plan_deep_xargs", "smi_air_plan_deep_zk_xargs"):
        st, why, _d = raw_plan(make(_lib.AirXArg, arr), log_n=7, which=which)
        assert st == BAD_ARG and needle in why, (name, which, why)


def test_the_plans_cannot_meet_multiplicities_that_wrap():
    """J n >= p needs n > p / 4.  A plan runs at a blowup of 4 or more inside the two-adic part of p - 1, so n <= (p - 1) / 4
    there and J n <= p - 1: at the smallest modulus, 12289 = 3 * 2^12 + 1, the largest trace a plan takes has 2^10 rows and
    J = 4 passes.  The refusal is met through the entry points that take log_n alone (tests/test_shared_lookup_emu.py and
    tests/test_gpu_boundary_primes_shared_lookup.py, at 2^12 rows)."""
    from stark_rs_amd import _lib
    keep = []

    def arr(v):
        keep.append((C.c_uint32 * len(v))(*v))
        return C.cast(keep[-1], _lib.u32p)
    four = [_lib.AirXArg(KIND(4), 1, 11, 0, arr([1, 2, 3, 4] + [NONE] * 4), arr([0]), NONE, NONE)]
    assert raw_plan(four, log_n=9, lb=3, p=12289, g=11, which="smi_air_plan_deep_xargs") == (0, "", 6)
    st, why, _d = raw_plan(four, log_n=10, lb=3, p=12289, g=11, which="smi_air_plan_deep_xargs")
    assert st != 0 and "LDE domain too large" in why


def test_one_tuple_spelled_with_the_new_constant_is_the_lookup():
    """kind = SMI_ARG_LOOKUP | (1 - 1) << SMI_ARG_TUPLES_SHIFT is SMI_ARG_LOOKUP: same status, same degree, a_sel allowed"""
    from stark_rs_amd import _lib
    keep = []

    def arr(v):
        keep.append((C.c_uint32 * len(v))(*v))
        return C.cast(keep[-1], _lib.u32p)
    spelled = 1 | (1 - 1) << _lib.ARG_TUPLES_SHIFT
    assert spelled == 1
    a = raw_plan([_lib.AirXArg(spelled, 1, 11, 0, arr([1]), arr([0]), 3, NONE)])
    b = raw_plan([_lib.AirXArg(1, 1, 11, 0, arr([1]), arr([0]), 3, NONE)])
    assert a == b == (0, "", 3)


def test_the_constants_are_declared_everywhere():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stark_mi.h")).read()
    rust = open(os.path.join(root, "bindings", "stark_mi.rs")).read()
    assert re.search(r"#define SMI_ARG_MAX_TUPLES\s+4\b", header) and re.search(r"#define SMI_ARG_TUPLES_SHIFT\s+8\b", header)
    assert "Shared-table lookups" in header
    assert "SMI_ARG_MAX_TUPLES" in rust and "SMI_ARG_TUPLES_SHIFT" in rust
    for section in ("Argument list:", "Argument list with selectors and periodic members -"):
        body = header[header.index("/* ---- " + section):]
        left = body[body.index("Left out:"):]
        left = left[:left.index("*/")]
        assert "sharing one multiplicity column" not in left and "sharing one table" not in left, section
