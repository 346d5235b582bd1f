"""GPU: launch_merkle_impl (csrc/hash.hip) and the FRI round driver (csrc/fri.hip, csrc/stark.hip) execute every plan the
host planners emit -- tests/test_launch_plans.py pins the plans, this module runs them.  One battery
(tests/gpu_battery.py: every stored level of every tree, every proof byte, against the CPU oracle) runs in-process at
default knobs and in one fresh child process per non-default knob setting, because the SMI_* knobs are read once per
process.  The kernel launches each item recorded must be the ones the planners emit under the same knobs: a setting
that did not reach the library (a misspelt variable) fails there.  `pytest -m gpu`."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import time

import pytest

import gpu_battery as gb
from test_launch_plans import (BY_FOLD, CHUNK, DIGESTS, ELEMENTS, KNOB_SETTINGS, R0_ALIGNED, R0_COMBINE, R0_UNALIGNED, ROWS,
                               SUB, TAIL_LEN, knobs, merkle_plan, ref_rounds, round_plan)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATTERY = os.path.join("tests", "gpu_battery.py")

# Measured on an MI355X: the default-knob battery takes 1.0 .. 1.3 s in-process over three sessions (a child 3.0 .. 4.3 s of
# wall time with the start of Python, torch and two engines; the oracle's expectations before them 13 s).  A child gets
# five times the battery's largest time and never less than 120 s -- the floor decides: the margin is for a first load of
# the code objects and a busy shared host.
BATTERY_SECONDS = 1.3
CHILD_TIMEOUT = max(120.0, 5 * BATTERY_SECONDS)


def _merkle_env(over):
    return {"SMI_MERKLE_" + k: str(v) for k, v in over.items()}


# (id, environment, Merkle knobs as the planner sees them, SMI_FRI_TAIL as the planner sees it)
SETTINGS = [("-".join("%s=%s" % kv for kv in over.items()), _merkle_env(over), over, TAIL_LEN) for over in KNOB_SETTINGS[1:]]
SETTINGS += [("FRI_TAIL=0", {"SMI_FRI_TAIL": "0"}, {}, 0),
             ("FRI_TAIL=2048", {"SMI_FRI_TAIL": "2048"}, {}, 2048),
             ("FUSE=0-FRI_TAIL=2048", {"SMI_MERKLE_FUSE": "0", "SMI_FRI_TAIL": "2048"}, dict(FUSE=0), 2048)]
# the NTT knobs change no Merkle or FRI plan: the battery's LDE items (and the extension inside the build-defined prove)
# are what they reach -- one 2^20 two-pass plan and one 2^23 plan (8.6, 6.6, 9.5) at batch 3, not the other pass kernels:
# tests/test_gpu_ntt_matrix.py runs every instantiation -- and the environment the child echoes is the only evidence here
# that they were set
NTT_SETTINGS = [{"SMI_NTT_SHARE_COLS": "0"}, {"SMI_NTT_TWIN_REGS": "0"}, {"SMI_NTT_LAST_DIRECT": "0"}, {"SMI_NTT_DEFER_TW": "0"},
                {"SMI_NTT_DEFER_TW": "1"}, {"SMI_LDE_GEO": "2", "SMI_LDE_LAYOUT": "4"}, {"SMI_LDE_GEO": "1", "SMI_LDE_LAYOUT": "3"}]
SETTINGS += [("-".join("%s=%s" % (k[4:], v) for k, v in env.items()), env, {}, TAIL_LEN) for env in NTT_SETTINGS]
assert len(SETTINGS) == 12 + 3 + 7 and len({s[0] for s in SETTINGS}) == len(SETTINGS)

_dead_child = []   # the first child that ended by a signal, an abort or a time limit: nothing is started after it


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd as s
    s.build()
    from stark_rs_amd._lib import EMU_PATH as path
    L = C.CDLL(path)
    i64p, u64p, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    L.emu_merkle_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, i64p, u64p]
    L.emu_fri_round_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, i64p, u8p, u8p, C.POINTER(C.c_uint32)]
    return L


@pytest.fixture(scope="session")
def expectations(tmp_path_factory, oracle):
    """the battery's inputs and expected outputs, computed once per session by the oracle and handed on as files"""
    out = tmp_path_factory.mktemp("battery_expectations")
    t0 = time.time()
    man = gb.expected(oracle, str(out))
    print("battery expectations: %.0f s of oracle time" % (time.time() - t0))
    yield str(out), man
    shutil.rmtree(str(out), ignore_errors=True)   # 1.1 GB of trees: not left behind in the temporary directory


# --------------------------------------------------------------------------------------- evidence of the plan
MERKLE_KERNELS = ("merkle_top_kernel", "merkle_sub_kernel<leaves>", "merkle_sub_kernel<digests>")


def planned_tree_launches(emu, ent, kn):
    n, kind = 1 << ent["logn"], ent["kind"]
    if kind == "E":
        plan = merkle_plan(emu, n, 1, ELEMENTS, 0, kn)
    elif kind == "R" and ent["W"] <= 4:
        plan = merkle_plan(emu, n, 1, ROWS, ent["W"], kn)
    else:   # digests: hashed by a launch of their own (smi_dev_hash_leaves, or the row hash of more than four columns)
        plan = merkle_plan(emu, n, 1, DIGESTS, 0, kn)
    return _merkle_counts(plan)


def _merkle_counts(plan):
    return {"merkle_top_kernel": sum(st["family"] == CHUNK for st in plan),
            "merkle_sub_kernel<leaves>": sum(st["family"] == SUB and st["from_leaves"] == 1 for st in plan),
            "merkle_sub_kernel<digests>": sum(st["family"] == SUB and st["from_leaves"] == 0 for st in plan)}


def planned_prove_launches(emu, n, expansion, t, phase, round0, kn, tail_len, commit=()):
    """fold and tail launches of the round plan, and the Merkle launches of `commit` (the plans of the trees built before
    the rounds) plus one single-tree plan per round outside the tail"""
    R = ref_rounds(n, expansion, t)
    ok, prod, _tree, tail_at = round_plan(emu, n, R, phase, round0, kn, tail_len)
    assert ok
    want = {"fri_fold_kernel": prod.count(BY_FOLD), "fri_tail_kernel": 1 if tail_at < R else 0}
    want.update(_merkle_counts(list(commit) + [st for r in range(tail_at) for st in merkle_plan(emu, n >> r, 1, ELEMENTS, 0, kn)]))
    return want


def assert_plan_evidence(emu, report, man, over, tail_len):
    """the launches every item recorded are the ones merkle_plan / fri_round_plan emit under these knobs"""
    kn = knobs(**over)
    items = report["items"]
    for name, ent in man["trees"].items():
        if name in items:
            got = {k: items[name]["launches"].get(k, 0) for k in MERKLE_KERNELS}
            assert got == planned_tree_launches(emu, ent, kn), (name, over)
    for name, ent in man["proves"].items():
        for item, round0 in ((name, R0_ALIGNED),) + (((name + "_misaligned", R0_UNALIGNED),) if name == "prove_a" else ()):
            if item not in items:
                continue
            want = planned_prove_launches(emu, 1 << ent["logn"], ent["expansion"], ent["t"], 5 if ent["prior"] else 0, round0, kn, tail_len)
            got = {k: items[item]["launches"].get(k, 0) for k in want}
            assert got == want, (item, over, tail_len)
            assert "combine_columns_kernel" not in items[item]["launches"]
    # the build-defined prove: the first tree's launch computes the column combination where the round plan lets it
    st = man["stark"]
    N, R = 1 << (st["logn"] + st["lb"]), ref_rounds(1 << (st["logn"] + st["lb"]), 1 << st["lb"], st["t"])
    fused, _, _, _ = round_plan(emu, N, R, 0, R0_COMBINE, kn, tail_len)
    for variant in ("columns", "opened", "rows"):
        if "stark_" + variant not in items:
            continue
        # the commit: W column trees in one set of launches (grid.y = W), or one tree over the rows
        commit = merkle_plan(emu, N, 1, ROWS, st["W"], kn) if variant == "rows" else merkle_plan(emu, N, st["W"], ELEMENTS, 0, kn)
        want = planned_prove_launches(emu, N, 1 << st["lb"], st["t"], 0, R0_COMBINE if fused else R0_ALIGNED, kn, tail_len, commit)
        launches = items["stark_" + variant]["launches"]
        assert ("combine_columns_kernel" not in launches) == fused, (variant, over)
        assert {k: launches.get(k, 0) for k in want} == want, (variant, over, tail_len)


def all_items(extras):
    return set(gb.tree_items(extras)) | set(gb.PROVES) | {"prove_a_misaligned", "stark_columns", "stark_opened", "stark_rows",
                                                         "lde", "lde_two_pass"}


def assert_every_item(report, names):
    bad = {k: v for k, v in report["items"].items() if not v["ok"]}
    assert not bad, "differs from the oracle: " + json.dumps(bad)[:2000]
    assert set(report["items"]) == set(names)
    assert report["ok"]


# ------------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def engines():
    import stark_rs_amd as s
    e = {"ref": s.Engine(gb.P, gb.G, 0), "p2": s.Engine(gb.P2, gb.G2, 0)}
    yield e
    for x in e.values():
        x.close()


def test_battery_at_default_knobs(engines, expectations, emu, tmp_path):
    exp_dir, man = expectations
    assert not any(k.startswith(("SMI_MERKLE_", "SMI_FRI_TAIL", "SMI_NTT_", "SMI_LDE_")) for k in os.environ), "default knobs only"
    report = gb.run(engines, exp_dir, str(tmp_path / "report.json"))
    print("default-knob battery: %.1f s" % report["seconds"])
    assert_every_item(report, all_items(True))
    assert_plan_evidence(emu, report, man, {}, TAIL_LEN)
    # the kernels the suite never compared with anything before all ran here
    ran = set().union(*(it["launches"] for it in report["items"].values()))
    assert {"merkle_top_kernel", "merkle_sub_kernel<leaves>", "merkle_sub_kernel<digests>", "fri_fold_kernel", "fri_tail_kernel",
            "lde_b_kernel"} <= ran


def run_child(env_over, exp_dir, report_path, extras, only=None):
    """one fresh process with the knobs in its environment; -> (exit status or None on a time limit, seconds, output)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith(("SMI_MERKLE_", "SMI_FRI_TAIL", "SMI_NTT_", "SMI_LDE_"))}
    env.update(env_over)
    cmd = [sys.executable, BATTERY, exp_dir, report_path] + ([] if extras else ["--no-extras"]) + (["--only=" + ",".join(only)] if only else [])
    t0 = time.time()
    try:
        done = subprocess.run(cmd, cwd=ROOT, env=env, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        return done.returncode, time.time() - t0, done.stdout.decode(errors="replace")
    except subprocess.TimeoutExpired as e:
        return None, time.time() - t0, (e.stdout or b"").decode(errors="replace")


def checked_child(name, env_over, exp_dir, tmp_path, extras, only=None):
    """run_child under the module's fault discipline -> (exit status, report, output).  After a child that ended by a
    signal, an abort or a time limit, every later call fails at once without starting GPU work; nothing is retried."""
    if _dead_child:   # fail, not skip: a card that faulted once gets no further work from this module
        pytest.fail("not started: the child for %s ended with %s" % _dead_child[0])
    report_path = str(tmp_path / "report.json")
    status, seconds, output = run_child(env_over, exp_dir, report_path, extras, only)
    print("child %s: exit %s after %.1f s" % (name, status, seconds))
    if status is None or status < 0 or status in (134, 139):
        _dead_child.append((name, "a time limit of %.0f s" % CHILD_TIMEOUT if status is None else "status %d" % status))
        pytest.fail("child %s ended with %s\n%s" % (name, _dead_child[0][1], output[-3000:]))
    assert os.path.exists(report_path), output[-3000:]
    with open(report_path) as f:
        report = json.load(f)
    assert all(report["env"].get(k) == v for k, v in env_over.items()), report["env"]
    return status, report, output


@pytest.mark.parametrize("name,env_over,over,tail_len", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_battery_in_a_child_under_knobs(name, env_over, over, tail_len, expectations, emu, tmp_path):
    exp_dir, man = expectations
    extras = over == dict(TOP_BLOCKS=1024)
    status, report, output = checked_child(name, env_over, exp_dir, tmp_path, extras)
    assert_every_item(report, all_items(extras))
    assert status == 0, output[-3000:]
    # GENERIC=1 and the NTT knobs change no launch count: for them the environment the child echoed (checked_child) is
    # the only evidence that the setting was in force
    assert_plan_evidence(emu, report, man, over, tail_len)


def test_a_misspelt_knob_fails_the_plan_evidence(expectations, emu, tmp_path):
    """the check of the checks: SMI_MERKEL_K=1 reaches no knob, every item still equals the oracle, and the launches are
    not the ones planned for K=1"""
    exp_dir, man = expectations
    only = ["E20", "D20", "R4_20", "prove_a"]
    status, report, output = checked_child("misspelt", {"SMI_MERKEL_K": "1"}, exp_dir, tmp_path, False, only)
    assert status == 0, output[-3000:]
    assert_every_item(report, only)
    assert_plan_evidence(emu, report, man, {}, TAIL_LEN)
    with pytest.raises(AssertionError):
        assert_plan_evidence(emu, report, man, dict(K=1), TAIL_LEN)


def test_a_wrong_expectation_fails_its_item_in_process_and_in_a_child(engines, expectations, tmp_path):
    """one flipped byte in an expectation file fails exactly the items that read it, with the place of the difference"""
    exp_dir, _man = expectations
    wrong = tmp_path / "wrong"
    wrong.mkdir()
    flipped = {"tree_E12.npy": -1 - 32 * 5, "prove_c.bin": 40}   # node 2^13 - 7 (level 10, index 1); the second root record
    for f in os.listdir(exp_dir):
        if f in flipped:
            data = bytearray(open(os.path.join(exp_dir, f), "rb").read())
            data[flipped[f]] ^= 0x10
            (wrong / f).write_bytes(bytes(data))
        else:
            os.symlink(os.path.join(exp_dir, f), str(wrong / f))
    only = ["E12", "D12", "E13", "R4_12", "prove_c", "prove_b"]

    def check(report):
        items = report["items"]
        assert set(items) == set(only) and not report["ok"]
        assert [k for k in only if not items[k]["ok"]] == ["E12", "D12", "prove_c"]
        for k in ("E12", "D12"):
            assert items[k]["where"] == {"level": 10, "index": 1, "differing_nodes": 1}
        assert items["prove_c"]["where"] == {"byte": 40}

    check(gb.run(engines, str(wrong), only=only))
    status, report, _output = checked_child("wrong-expectation", {}, str(wrong), tmp_path, False, only)
    assert status == 1
    check(report)
