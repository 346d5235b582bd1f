"""CPU: the plan table of tests/ntt_matrix.py covers what it claims -- every shape of SMI_NTT_SHAPES in every role, every
setting/family pair, every knob a variable the library reads -- and the planner (csrc/ntt_host.h, through the emulator
library) returns exactly the table's plan under each override.  The GPU half is tests/test_gpu_ntt_matrix.py; the same
table on the emulator is tests/test_emu_kernels.py::test_emulated_ntt_explicit_tile_shapes."""
import ctypes as C
import glob
import os
import re

import pytest

import ntt_matrix as nm

CSRC = os.path.join(nm.ROOT, "stark_rs_amd", "csrc")


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd as s
    s.build()
    from stark_rs_amd._lib import EMU_PATH as path
    L = C.CDLL(path)
    L.emu_ntt_plan.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def planner(emu, L, batch):
    lr, lw = (C.c_int * 4)(), (C.c_int * 4)()
    np_ = emu.emu_ntt_plan(L, batch, lr, lw)
    return [(lr[i], lw[i]) for i in range(np_)]


def roles_of(plan):
    passes = nm.parse_plan(plan)
    return [(s, "first" if i == 0 else "last" if i == len(passes) - 1 else "mid") for i, s in enumerate(passes)]


def test_every_shape_appears_in_every_role():
    shapes, table = nm.shapes(), nm.plan_table()
    assert len(shapes) >= 14 and (6, 6) in shapes and (11, 2) in shapes
    for family, role in (("first", "first"), ("last", "last"), ("middle", "mid"), ("deferred-first", "first")):
        rows = [r for r in table if r["family"] == family]
        assert [r["shape"] for r in rows] == shapes, family
        for r in rows:   # the row's plan has its shape in its role, and nothing but 64-point lines (or the 7.5 partner) beside it
            assert r["role"] == role and (r["shape"], role) in roles_of(r["plan"]), r
            assert r["primes"] == ("ref", "p2"), r
    four = [r for r in table if r["family"] == "four-pass"]
    assert [(r["L"], r["plan"], r["primes"]) for r in four] == [(24, "6.6,6.6,6.6,6.6", ("p2",))]
    assert len(table) == 4 * len(shapes) + 1 and len({r["id"] for r in table}) == len(table)
    # the smallest sizes: a first or last shape beside one 64-point pass, a middle one between two
    for r in table:
        lr = r["shape"][0]
        want = {"first": max(13, lr + 6), "last": max(13, lr + 6), "middle": lr + 12, "deferred-first": lr + 12, "four-pass": 24}
        assert r["L"] == want[r["family"]], r


def test_every_plan_of_the_table_is_valid_by_the_planners_rules():
    """a shape added to SMI_NTT_SHAPES gets its four plans from the same recipe; where the recipe gives one the planner would
    refuse (and quietly replace by the default plan), this fails"""
    kernels = nm.shapes()
    for r in nm.plan_table():
        assert nm.plan_valid(r["L"], nm.parse_plan(r["plan"]), kernels), r
        assert r["L"] <= max(nm.PRIMES[k][2] for k in r["primes"]) and r["primes"], r
    assert not nm.plan_valid(nm.INVALID_PLAN[0], nm.parse_plan(nm.INVALID_PLAN[1]), kernels)
    assert not nm.plan_valid(12, [(6, 6), (6, 7)], kernels) and not nm.plan_valid(18, [(6, 6), (6, 6), (6, 6), (6, 6), (6, 6)], kernels)


def test_the_table_follows_the_macro(monkeypatch):
    """the table follows the macro: with one more shape in it there are four more rows"""
    before = len(nm.plan_table())
    monkeypatch.setattr(nm, "shapes", lambda: [(6, 6), (7, 5), (12, 2)])
    assert len(nm.plan_table()) == 13 and before != 13
    assert {r["plan"] for r in nm.plan_table() if r["shape"] == (12, 2)} == {"12.2,6.6", "6.6,12.2", "6.6,12.2,6.6", "12.2,6.6,6.6"}


def test_every_setting_runs_its_families():
    want = {
        "defaults": ({}, {"first", "last", "middle", "four-pass"}),
        "SHARE_COLS=2-DEFER_TW=0": ({"SHARE_COLS": "2", "DEFER_TW": "0"}, {"last", "middle", "four-pass"}),
        "SHARE_COLS=2-DEFER_TW=1": ({"SHARE_COLS": "2", "DEFER_TW": "1"}, {"middle", "deferred-first", "four-pass"}),
        "SHARE_COLS=2-DEFER_TW=1-TWIN_REGS=0": ({"SHARE_COLS": "2", "DEFER_TW": "1", "TWIN_REGS": "0"}, {"middle"}),
        "SHARE_COLS=0-DEFER_TW=1-LAST_DIRECT=0": ({"SHARE_COLS": "0", "DEFER_TW": "1", "LAST_DIRECT": "0"}, {"last", "middle", "deferred-first"}),
        "SHARE_COLS=2-LAST_DIRECT=0": ({"SHARE_COLS": "2", "LAST_DIRECT": "0"}, {"last"}),
    }
    got = {name: ({k[len("SMI_NTT_"):]: v for k, v in env.items()}, set(fams)) for name, env, fams in nm.SETTINGS}
    assert got == want
    # the legs: two single-column ones everywhere, the n_in sweep of the first role, four batched ones where columns are shared
    for _name, env, fams in nm.SETTINGS:
        for fam in fams:
            names = set(nm.legs(fam, env))
            assert {"inv1", "fwd1"} <= names
            assert ({"inv6", "fwd6", "fwd6_strided", "inv6_inplace"} <= names) == (env.get("SMI_NTT_SHARE_COLS") == "2")
            assert ({"fwd1_z0", "fwd1_z1", "fwd1_z2", "fwd1_z4", "fwd1_z6", "fwd1_ragged-3", "fwd1_ragged+1", "fwd1_offset1"} <= names) == (fam == "first")
    n = 1 << 13
    L = nm.legs("first", {})
    assert [nm.n_in_of(L[k], n) for k in ("inv1", "fwd1", "fwd1_z0", "fwd1_z6", "fwd1_ragged-3", "fwd1_ragged+1")] == [n, n // 8, n, n // 64, n // 8 - 3, n // 8 + 1]
    assert (L["inv1"]["offset"], L["inv1"]["post"], L["fwd1"]["offset"], L["fwd1_offset1"]["offset"]) == (3, 5, 5, 1)


def test_every_knob_is_a_variable_the_library_reads():
    text = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(f))
    assert set(nm.KNOBS) == {"SMI_NTT_SHARE_COLS", "SMI_NTT_DEFER_TW", "SMI_NTT_TWIN_REGS", "SMI_NTT_LAST_DIRECT"}
    for k in nm.KNOBS:
        assert 'getenv("%s")' % k in text, k
    assert re.search(r'"SMI_NTT_PLAN_%u"', text) and "getenv(name)" in text


def test_the_oracle_meets_every_single_column_leg_and_a_column_of_every_group():
    need = nm.needed_keys()
    for _name, env, fams in nm.SETTINGS:
        for row, prime in nm.entries(fams):
            for leg in nm.legs(row["family"], env).values():
                cols = [c for c in range(leg["batch"]) if nm.key(prime, row["L"], leg, c) in need]
                if leg["batch"] == 1 or row["L"] <= 20:
                    assert cols == list(range(leg["batch"]))
                else:   # column groups of four: columns 0..3 and 4..5
                    assert cols == [0, 5] and {c // nm.COLS_PER_WG for c in cols} == {0, 1}


def test_predicted_kernel_names():
    share2 = {"SMI_NTT_SHARE_COLS": "2"}
    inv6, fwd6, inv1 = nm.legs("middle", share2)["inv6"], nm.legs("middle", share2)["fwd6"], nm.legs("middle", share2)["inv1"]
    assert nm.predicted_kernels("6.6,9.3,6.6", 21, inv6, share2) == {
        "ntt_pass_kernel<6,6,first>": 1, "ntt_pass_cols_kernel<9,3,mid>": 1, "ntt_pass_cols_kernel<6,6,last>": 1}
    assert nm.predicted_kernels("6.6,9.3,6.6", 21, fwd6, share2) == {   # a forward last pass has no output scale to share
        "ntt_pass_kernel<6,6,first>": 1, "ntt_pass_cols_kernel<9,3,mid>": 1, "ntt_pass_kernel<6,6,last>": 1}
    assert nm.predicted_kernels("6.6,9.3,6.6", 21, inv1, share2) == {
        "ntt_pass_kernel<6,6,first>": 1, "ntt_pass_kernel<9,3,mid>": 1, "ntt_pass_kernel<6,6,last>": 1}
    for env in ({"SMI_NTT_SHARE_COLS": "0"}, {}):   # never; the rule's threshold of 1024 workgroups: 2^18 / 2^12 tiles x 2 groups
        assert nm.predicted_kernels("6.6,6.6,6.6", 18, inv6, env) == {
            "ntt_pass_kernel<6,6,first>": 1, "ntt_pass_kernel<6,6,mid>": 1, "ntt_pass_kernel<6,6,last>": 1}
    assert nm.predicted_kernels("6.6,6.6,6.6,6.6", 24, inv6, {}) == {
        "ntt_pass_kernel<6,6,first>": 1, "ntt_pass_cols_kernel<6,6,mid>": 2, "ntt_pass_cols_kernel<6,6,last>": 1}
    assert [nm.share_mode({"SMI_NTT_SHARE_COLS": v}) for v in ("0", "1", "2", "3")] == [0, 1, 2, 1] and nm.share_mode({}) == 1


def test_the_planner_returns_the_tables_plan_under_each_override(emu):
    assert not any(k.startswith("SMI_NTT_PLAN_") for k in os.environ)
    for r in nm.plan_table():
        name = "SMI_NTT_PLAN_%d" % r["L"]
        os.environ[name] = r["plan"]
        try:
            for batch in (1, nm.BATCH):
                assert planner(emu, r["L"], batch) == nm.parse_plan(r["plan"]), r
        finally:
            del os.environ[name]


def test_the_planner_refuses_the_invalid_plan(emu):
    L, plan = nm.INVALID_PLAN
    default = {b: planner(emu, L, b) for b in (1, nm.BATCH)}
    os.environ["SMI_NTT_PLAN_%d" % L] = plan
    try:
        for b, want in default.items():
            assert planner(emu, L, b) == want != nm.parse_plan(plan)
    finally:
        del os.environ["SMI_NTT_PLAN_%d" % L]
    assert sum(lr for lr, _ in nm.parse_plan(plan)) != L and all(s in nm.shapes() for s in nm.parse_plan(plan))
