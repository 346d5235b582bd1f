"""GPU: every verifier of csrc/verify.hip against its recorded verdicts (tests/golden/verify_verdicts.json, made by
tests/golden/make_verify_verdicts.py): base and extension FRI with and without a prior transcript and grinding,
smi_stark_verify with column openings, the AIR verifiers over column trees, rows, the extension and the extension with
proof of work, and the permutation proof -- each on the untouched proof, on truncations at every object boundary, wrong
tags and counts, flipped bits, values plus p, wrong nonces and difficulties, the other variants' verifiers, and pairs of
defects that pin the order of the checks.  Status, *accept, the sentence, consumed, n_pv and the polynomial values are
compared exactly; nothing is skipped.  `pytest -m gpu`."""
import os

import pytest

import verify_verdicts as vv
from test_gpu_air import engines  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "verify_verdicts.json")


def test_every_verdict_is_the_recorded_one(engines, oracle):
    want = vv.load(FIXTURE)
    got = vv.run_all(engines, oracle)
    assert list(got) == list(want)                                  # every case, in order: the replay skips nothing
    wrong = []
    for name in want:
        assert [r[:2] for r in got[name]] == [r[:2] for r in want[name]], name
        wrong += [(name, g, w) for g, w in zip(got[name], want[name]) if g != w]
    assert not wrong, "%d verdicts differ, the first: %r" % (len(wrong), wrong[:3])


def test_the_fixture_reaches_every_reject_sentence():
    want = vv.load(FIXTURE)
    seen = {row[4] for rows in want.values() for row in rows}
    assert not [x for x in vv.SENTENCES if x not in seen and x not in vv.UNREACHABLE]
    # every honest proof is accepted by its own verifier; the one proof committed with non-canonical values is not
    for name, rows in want.items():
        assert rows[0][0] in ("ok", "as committed"), name
        assert rows[0][2:4] == ([0, 0] if "+ p committed" in name else [0, 1]), name
