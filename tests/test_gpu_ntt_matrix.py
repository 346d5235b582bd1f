"""GPU: every NTT pass kernel instantiation of csrc/ntt.hip runs against the CPU oracle -- tests/test_ntt_matrix_host.py pins
the plan table, this module runs it.  tests/ntt_matrix.py is started in one fresh child process per knob setting (the
SMI_NTT_* context knobs are read when a context is created, and a child keeps both the environment of this process and a
fault out of it).  Every leg of every plan must equal the oracle bit for bit, and the ntt_pass_kernel<...> /
ntt_pass_cols_kernel<...> names its profile recorded must be exactly the ones the plan and the setting predict: an override
the planner refused (it falls back to the default plan) or a knob that did not reach the library fails there.
`pytest -m gpu`.

Measured on an MI355X (seconds in the child's process / of its wall time with the start of Python, torch and two engines):
defaults 5.0 / 5.5, SHARE_COLS=2 DEFER_TW=0 10.9 / 11.5, SHARE_COLS=2 DEFER_TW=1 15.0 / 15.5, with TWIN_REGS=0 8.0 / 8.5,
SHARE_COLS=0 DEFER_TW=1 LAST_DIRECT=0 4.2 / 4.7, SHARE_COLS=2 LAST_DIRECT=0 1.9 / 2.4; the refused-plan child 2.4, the
wrong-digest child 6.8 (it recomputes one 2^24-point expectation); the oracle's 300 expectations before them 4 s on sixteen
threads; the module 62 s.  Most of a child's time is the copies to and from the host, not the transforms."""
import json
import os
import shutil
import subprocess
import sys
import time

import pytest

import ntt_matrix as nm

pytestmark = pytest.mark.gpu

ROOT = nm.ROOT
MATRIX = os.path.join("tests", "ntt_matrix.py")
# A child gets five times the largest measured in-process time and never less than 120 s (the floor decides, as in
# tests/test_gpu_plans.py: the margin is for a first load of the code objects and a busy shared host); a child that needs
# more than a quarter of that is split by family, the limit is not raised.
MATRIX_SECONDS = 15.0   # the largest in-process time above: under a quarter of the limit, so no setting is split
CHILD_TIMEOUT = max(120.0, 5 * MATRIX_SECONDS)
KNOB_PREFIXES = ("SMI_MERKLE_", "SMI_FRI_TAIL", "SMI_NTT_", "SMI_LDE_")

# one child per (setting, families): a setting whose child needs more than a quarter of the limit is split by family here
CHILDREN = [(name, env, families) for name, env, families in nm.SETTINGS]
assert len({c[0] for c in CHILDREN}) == len(CHILDREN)

_dead_child = []   # the first child that ended by a signal, an abort or a time limit: nothing is started after it


@pytest.fixture(scope="session")
def matrix_expectations(tmp_path_factory, oracle):
    """SHA-256 digests of every expected column, computed once per session by the oracle"""
    out = tmp_path_factory.mktemp("ntt_matrix_expectations")
    man = nm.expected(oracle, str(out))
    print("ntt matrix expectations: %d digests, %.0f s of oracle time" % (len(man["digests"]), man["oracle_seconds"]))
    yield os.path.join(str(out), "manifest.json"), man
    shutil.rmtree(str(out), ignore_errors=True)


def run_child(env_over, manifest, report_path, args):
    """one fresh process with the knobs in its environment; -> (exit status or None on a time limit, seconds, output)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith(KNOB_PREFIXES)}
    env.update(env_over)
    t0 = time.time()
    try:
        done = subprocess.run([sys.executable, MATRIX, manifest, report_path] + list(args), cwd=ROOT, env=env, timeout=CHILD_TIMEOUT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        return done.returncode, time.time() - t0, done.stdout.decode(errors="replace")
    except subprocess.TimeoutExpired as e:
        return None, time.time() - t0, (e.stdout or b"").decode(errors="replace")


def checked_child(name, env_over, manifest, tmp_path, args):
    """run_child under the fault discipline of tests/test_gpu_plans.py -> (exit status, report, output).  After a child that
    ended by a signal, an abort or a time limit, every later call fails at once without starting GPU work; nothing is
    retried."""
    if _dead_child:   # fail, not skip: a card that faulted once gets no further work from this module
        pytest.fail("not started: the child for %s ended with %s" % _dead_child[0])
    report_path = str(tmp_path / "report.json")
    status, seconds, output = run_child(env_over, manifest, report_path, args)
    print("child %s: exit %s after %.1f s" % (name, status, seconds))
    if status is None or status < 0 or status in (134, 139):
        _dead_child.append((name, "a time limit of %.0f s" % CHILD_TIMEOUT if status is None else "status %d" % status))
        pytest.fail("child %s ended with %s\n%s" % (name, _dead_child[0][1], output[-3000:]))
    assert os.path.exists(report_path), output[-3000:]
    with open(report_path) as f:
        report = json.load(f)
    print("child %s: %.1f s in process" % (name, report["seconds"]))
    assert {k: v for k, v in report["env"].items() if k.startswith(KNOB_PREFIXES)} == env_over, report["env"]
    return status, report, output


def assert_every_leg(report, env, families, primes=("ref", "p2")):
    """every plan of the families on every prime is in the report with all of its legs, and every leg equals the oracle"""
    assert report["error"] is None, report["error"]
    bad = {"%s %s" % (p, l): leg["where"] for p, rec in report["plans"].items() for l, leg in rec["legs"].items() if not leg["ok"]}
    assert not bad, "differs from the oracle: " + json.dumps(bad)[:3000]
    want = {"%s:%s" % (row["id"], prime): set(nm.legs(row["family"], env)) for row, prime in nm.entries(families, primes)}
    assert {p: set(rec["legs"]) for p, rec in report["plans"].items()} == want
    assert report["ok"]


def assert_kernel_evidence(report, env):
    """the ntt_* launches every leg recorded are the ones its plan string and the setting predict"""
    for name, rec in report["plans"].items():
        for leg_name, leg in nm.legs(rec["family"], env).items():
            want = nm.predicted_kernels(rec["plan"], rec["L"], leg, env)
            assert rec["legs"][leg_name]["kernels"] == want, (name, leg_name, env)


def kernels_seen(report):
    return set().union(*(leg["kernels"] for rec in report["plans"].values() for leg in rec["legs"].values()))


@pytest.mark.parametrize("name,env,families", CHILDREN, ids=[c[0] for c in CHILDREN])
def test_matrix_in_a_child(name, env, families, matrix_expectations, tmp_path):
    manifest, _man = matrix_expectations
    status, report, output = checked_child(name, env, manifest, tmp_path, ["--families=" + ",".join(families)])
    assert_every_leg(report, env, families)
    assert status == 0, output[-3000:]
    assert_kernel_evidence(report, env)
    # what the setting is there to reach did run: every shape in the role of each of its families
    seen, mode = kernels_seen(report), nm.share_mode(env)
    for s in nm.shapes():
        if "first" in families or "deferred-first" in families:
            assert "ntt_pass_kernel<%d,%d,first>" % s in seen
        if "middle" in families:
            assert "ntt_pass_kernel<%d,%d,mid>" % s in seen
            assert ("ntt_pass_cols_kernel<%d,%d,mid>" % s in seen) == (mode == 2)
        if "last" in families:
            assert "ntt_pass_kernel<%d,%d,last>" % s in seen
            assert ("ntt_pass_cols_kernel<%d,%d,last>" % s in seen) == (mode == 2)
    if "four-pass" in families:
        four = report["plans"]["four-pass:6.6@24:p2"]
        assert four["legs"]["inv1"]["kernels"]["ntt_pass_kernel<6,6,mid>"] == 2


def test_a_refused_plan_fails_the_kernel_evidence(matrix_expectations, tmp_path):
    """the check of the checks: the planner refuses 9.3,9.3,9.3 at 2^18 points (the digits sum to 27) and runs the default
    plan, whose results equal the oracle -- and whose kernels are not the ones the string predicts"""
    manifest, _man = matrix_expectations
    L, plan = nm.INVALID_PLAN
    status, report, output = checked_child("refused-plan", {}, manifest, tmp_path, ["--plan=%d=%s" % (L, plan), "--primes=ref"])
    assert status == 0 and report["ok"] and report["error"] is None, output[-3000:]
    (rec,) = report["plans"].values()
    assert (rec["L"], rec["plan"]) == (L, plan) and set(rec["legs"]) == {"inv1", "fwd1"} and all(l["ok"] for l in rec["legs"].values())
    with pytest.raises(AssertionError):
        assert_kernel_evidence(report, {})
    assert all(k.startswith("ntt_pass_kernel<9,") for k in kernels_seen(report)) and len(kernels_seen(report)) == 2


def test_a_wrong_digest_fails_exactly_its_leg(matrix_expectations, tmp_path):
    """one corrupted digest in a copy of the manifest fails the one leg that reads it (the inverse transform of the four-pass
    plan: no other plan has 2^24 points) and no other"""
    manifest, man = matrix_expectations
    leg = nm.legs("four-pass", {})["inv1"]
    k = nm.key("p2", 24, leg, 0)
    wrong = json.loads(json.dumps(man))
    wrong["digests"][k] = wrong["digests"][k][:-1] + ("0" if wrong["digests"][k][-1] != "0" else "1")
    path = str(tmp_path / "wrong_manifest.json")
    with open(path, "w") as f:
        json.dump(wrong, f)
    status, report, _output = checked_child("wrong-digest", {}, path, tmp_path, ["--families=four-pass"])
    assert status == 1 and not report["ok"] and report["error"] is None
    failed = [(p, l) for p, rec in report["plans"].items() for l, rec_leg in rec["legs"].items() if not rec_leg["ok"]]
    assert failed == [("four-pass:6.6@24:p2", "inv1")] and set(report["plans"]["four-pass:6.6@24:p2"]["legs"]) == {"inv1", "fwd1"}
    # the values are the oracle's: only the digest differs
    assert report["plans"]["four-pass:6.6@24:p2"]["legs"]["inv1"]["where"] == {"column": 0, "index": None, "differing": 0}
    assert_kernel_evidence(report, {})
