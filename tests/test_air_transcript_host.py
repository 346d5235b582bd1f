"""CPU: the transcript layouts of the AIR proofs (csrc/transcript_core.h, through the emulator's emu_air_transcript) -- the
one derivation of roots -> weights -> FRI's seed that provers and verifiers share -- against the Python composers the
tests of every variant already trust: air_compose.transcript (column trees), air_rows.transcript (one row tree),
ext_compose.air_transcript (the extension) and perm_compose.challenges / weights (the permutation proof).  The
challenges and the seed (16 words and the phase) are compared; W in {1, 2, 3} and K in {0, 1, 3} leave every phase the
8-byte indices can: 0, 8, 16, 24.  The seed is compared with emu_fs_seed over the composer's transcript bytes -- hashc::fs_seed,
the function Transcript::seed() calls --, so this pins the transcript's bytes, not the seed function: that one is pinned
to the oracle by tests/test_transcript_host.py.

Also here: the list of reject sentences the recorded verdicts must reach (tests/verify_verdicts.py) against the string
literals of csrc/verify.hip, so that a sentence added to the verifier is required of the fixture."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import air_compose as ac
import air_rows as ar
import ext_compose as xc
import perm_compose as pm


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd as s
    s.build()
    from stark_rs_amd._lib import EMU_PATH
    L = C.CDLL(EMU_PATH)
    L.emu_air_transcript.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.emu_air_transcript.restype = C.c_uint64
    L.emu_fs_seed.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.emu_fs_seed.restype = None
    return L


def _roots(n, seed):
    return [np.random.default_rng(1000 * seed + c).integers(0, 256, 32, dtype=np.uint8).tobytes() for c in range(n)]


def _air(W, K):
    from stark_rs_amd.mirror import Air
    air = Air(W)
    for k in range(K):
        air.transition({("next", k % W): 1, ("cur", 0): -1})
    return air


def composed(o, layout, W, K, roots):
    """-> (transcript bytes, challenges) by the Python composer of the layout"""
    if layout == 0:
        return ac.transcript(o, _air(W, K), roots)
    if layout == 1:
        return ar.transcript(o, W, K, roots[0])
    if layout == 2:
        return xc.air_transcript(o, W, K, roots[0])
    tr, ch = pm.challenges(o, roots[0])
    tr, wts = pm.weights(o, tr, roots[1], W + K + 2)
    return bytes(tr), ch + wts


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("W", [1, 2, 3])
@pytest.mark.parametrize("K", [0, 1, 3])
def test_challenges_and_seed_equal_the_python_composers(oracle, emu, layout, W, K):
    roots = _roots(W if layout == 0 else 2, 10 * W + K)
    tr, want = composed(oracle, layout, W, K, roots)
    n = {0: W + K, 1: W + K, 2: 4 * (W + K), 3: 8 + 4 * (W + K + 2)}[layout]
    assert len(want) == n
    got, seed = np.zeros(n + 1, dtype=np.uint64), np.zeros(17, dtype=np.uint32)
    got[n] = 0x5a5a
    assert emu.emu_air_transcript(layout, b"".join(roots), W, K, got.ctypes.data, seed.ctypes.data) == n
    assert [int(x) for x in got[:n]] == [int(x) for x in want] and got[n] == 0x5a5a
    words, phase = np.zeros(16, dtype=np.uint32), C.c_uint32(99)
    emu.emu_fs_seed(bytes(tr), len(tr), words.ctypes.data, C.addressof(phase))
    assert list(seed[:16]) == list(words) and seed[16] == phase.value == len(tr) % 32


def test_the_cases_leave_every_phase():
    phases = {(32 * (W if layout == 0 else 1) + 8 * (K if layout == 0 else W + K)) % 32 for layout in (0, 1) for W in (1, 2, 3) for K in (0, 1, 3)}
    assert phases == {0, 8, 16, 24}


def test_the_sentences_the_fixture_must_reach_are_the_ones_in_verify_hip():
    """every string literal of verify.hip that is not an #include, not inside a comment and not the message of a status
    (smi_fail) is a sentence a verdict can carry"""
    import verify_verdicts as vv
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stark_rs_amd", "csrc", "verify.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines() if not line.lstrip().startswith("#include"))
    lits = []
    code = re.sub(r'"((?:[^"\\]|\\.)*)"', lambda m: lits.append(m.group(1)) or "@%d@" % (len(lits) - 1), code)   # then no ';' hides in a string
    code = re.sub(r"smi_fail\([^;]*;", "", code)
    found = {lits[int(k)] for k in re.findall(r"@(\d+)@", code)}
    assert found == set(vv.SENTENCES) | set(vv.UNREACHABLE)
