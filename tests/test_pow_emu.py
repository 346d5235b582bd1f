"""CPU: the search kernel's own per-lane code (csrc/hash_core.h grind_pair / grind_round) run by the emulator library with
the kernel's rounds and lanes (csrc/emu.cpp emu_grind), against the restatement over the oracle's hash
(tests/pow_compose.py).  The emulator visits the lanes of a round in descending order, so a larger valid nonce is published
before a smaller one: the minimum has to win, not the first writer."""
import ctypes as C

import numpy as np
import pytest

import pow_compose as pc

LENGTHS = list(range(32)) + [32, 37, 64, 200]
GRIDS = [1, 64, 4096]


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp = C.c_void_p
    L.emu_fs_seed.argtypes = [C.c_char_p, C.c_size_t, vp, vp]
    L.emu_grind.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, vp]
    L.emu_grind_pair.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, vp]
    L.emu_grind_word.argtypes = [vp, C.c_uint32, C.c_uint64, vp, vp]
    L.emu_grind_word.restype = C.c_uint64
    return L


def transcript(length, seed=0):
    return bytes(np.random.default_rng(7000 + 1000 * seed + length).integers(0, 256, length, dtype=np.uint8))


def seed_of(emu, t):
    words, phase = np.zeros(16, dtype=np.uint32), C.c_uint32()
    emu.emu_fs_seed(t, len(t), words.ctypes.data, C.addressof(phase))
    assert phase.value == len(t) % 32
    return words, phase.value


def emu_grind(emu, t, bits, lanes, max_tries=0):
    """-> the nonce, or None when the search is exhausted"""
    words, phase = seed_of(emu, t)
    out = np.zeros(1, dtype=np.uint64)
    rc = emu.emu_grind(words.ctypes.data, phase, bits, max_tries, lanes, out.ctypes.data)
    assert rc in (0, 1), rc
    return int(out[0]) if rc == 0 else None


def find(oracle, bits, want, length=5):
    """a transcript of `length` bytes whose smallest nonce at `bits` satisfies want(nonce), by the restatement"""
    for seed in range(1, 4000):
        t = transcript(length, seed)
        if want(pc.grind(oracle, t, bits)):
            return t
    raise AssertionError("no such transcript among the candidates")


@pytest.mark.parametrize("length", LENGTHS)
def test_check_words_of_a_pair_equal_the_restatement_at_every_phase(oracle, emu, length):
    """both halves of the paired-lane state, nonces whose bytes all differ, and the verifier's single-hash form"""
    t = transcript(length)
    words, phase = seed_of(emu, t)
    w = np.zeros(2, dtype=np.uint64)
    for n0, n1 in [(0, 1), (2, 3), (0xfedcba9876543210, 0x0123456789abcdef), ((1 << 64) - 2, (1 << 64) - 1), (255, 256)]:
        emu.emu_grind_pair(words.ctypes.data, phase, n0, n1, w.ctypes.data)
        assert [int(w[0]), int(w[1])] == [pc.check_word(oracle, t, n0), pc.check_word(oracle, t, n1)], (n0, n1)
        out, ph = np.zeros(16, dtype=np.uint32), C.c_uint32()
        assert emu.emu_grind_word(words.ctypes.data, phase, n0, out.ctypes.data, C.addressof(ph)) == pc.check_word(oracle, t, n0)
        after, after_phase = seed_of(emu, t + n0.to_bytes(8, "little"))     # the transcript with the nonce absorbed
        assert ph.value == after_phase == (phase + 8) % 32 and np.array_equal(out, after)


@pytest.mark.parametrize("lanes", GRIDS)
@pytest.mark.parametrize("bits", [0, 1, 4, 8, 12])
def test_emu_grind_finds_the_smallest_nonce_at_every_phase(oracle, emu, bits, lanes):
    for length in LENGTHS:
        t = transcript(length)
        assert emu_grind(emu, t, bits, lanes) == pc.grind(oracle, t, bits), length


@pytest.mark.parametrize("lanes", GRIDS)
def test_emu_grind_at_sixteen_bits(oracle, emu, lanes):
    t = transcript(37)
    assert emu_grind(emu, t, 16, lanes) == pc.grind(oracle, t, 16)


def find_smallest_is(oracle, bits, target, length=5):
    """a transcript whose smallest nonce at `bits` is exactly `target`: the one hash at `target` first, the search only then"""
    for seed in range(1, 200000):
        t = transcript(length, seed)
        if pc.pow_ok(oracle, t, target, bits) and pc.grind(oracle, t, bits) == target:
            return t
    raise AssertionError("no such transcript among the candidates")


@pytest.mark.parametrize("lanes,bits", [(1, 2), (64, 8), (4096, 13)])
def test_round_zero_a_later_round_and_a_round_boundary(oracle, emu, lanes, bits):
    S = 2 * lanes
    t = find(oracle, bits, lambda nu: nu < S - 1)
    assert emu_grind(emu, t, bits, lanes) == pc.grind(oracle, t, bits) < S
    # strictly inside a later round (with one lane every nonce is the first or the last of its round)
    later = (lambda nu: nu >= 2 * S) if lanes == 1 else (lambda nu: nu > S and nu % S not in (0, S - 1))
    t = find(oracle, bits, later)
    assert emu_grind(emu, t, bits, lanes) == pc.grind(oracle, t, bits) > S
    for target in (S - 1, S, S + 1):          # the last nonce of round 0, the first of round 1 (lane 0), its pair
        t = find_smallest_is(oracle, bits, target)
        assert pc.grind(oracle, t, bits) == target
        assert emu_grind(emu, t, bits, lanes) == target, target


def test_two_valid_nonces_in_round_zero_the_smaller_wins(oracle, emu):
    lanes, bits = 64, 4
    t = find(oracle, bits, lambda nu: nu < 40)
    valid = pc.valid_nonces(oracle, t, bits, 2 * lanes)
    assert len(valid) >= 2 and valid[1] // 2 != valid[0] // 2            # two lanes hit in round 0; the higher lane goes first
    assert emu_grind(emu, t, bits, lanes) == valid[0] == pc.grind(oracle, t, bits)
    # ... and with both in ONE lane's pair the even one wins
    t = next(x for x in (transcript(5, s) for s in range(1, 4000)) if pc.pow_ok(oracle, x, 0, 1) and pc.pow_ok(oracle, x, 1, 1))
    assert emu_grind(emu, t, 1, lanes) == 0


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("lanes", GRIDS)
def test_the_search_cap(oracle, emu, lanes, parity):
    """max_tries nonces are tried, 0 .. max_tries - 1: an odd smallest nonce is the second of its lane's pair"""
    bits = 8
    t = find(oracle, bits, lambda nu: nu > 8 and nu % 2 == parity)
    nu = pc.grind(oracle, t, bits)
    assert emu_grind(emu, t, bits, lanes, max_tries=nu + 1) == nu
    assert emu_grind(emu, t, bits, lanes, max_tries=nu) is None
    assert emu_grind(emu, t, bits, lanes, max_tries=4) is None
    assert emu_grind(emu, t, bits, lanes, max_tries=1) is None
    assert emu_grind(emu, t, bits, lanes, max_tries=(1 << 64) - 1) == nu
    assert emu_grind(emu, t, bits, lanes, max_tries=0) == nu                # the default cap 2^(bits+6) is far away
