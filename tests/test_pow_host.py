"""CPU: the host side of grinding (include/stark_mi.h, "Grinding") -- smi_grind_check through libstarkmi.so (no context, no
GPU) against the restatement over the oracle's hash (tests/pow_compose.py), the new status, and the declarations in the
header, the ctypes table and the Rust binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pow_compose as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["smi_grind_check", "smi_dev_grind", "smi_dev_fri_prove_ext_pow", "smi_fri_verify_ext_pow", "smi_dev_air_prove_ext_pow",
       "smi_air_verify_ext_pow"]
BITS = [0, 1, 7, 8, 12]


@pytest.fixture(scope="module")
def L():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    return _lib.lib()


def _check(L, t, nonce, bits):
    ok = C.c_int(-1)
    st = L.smi_grind_check(t if t else None, len(t), nonce, bits, C.byref(ok))
    return st, ok.value


def transcript(length):
    return bytes(np.random.default_rng(1000 + length).integers(0, 256, length, dtype=np.uint8))


@pytest.mark.parametrize("bits", BITS)
def test_grind_check_equals_pow_ok_at_every_transcript_length(L, oracle, bits):
    """the found nonce is accepted; the nearest smaller and the nearest larger nonce the restatement rejects are rejected"""
    for length in range(71):
        t = transcript(length)
        nu = pc.grind(oracle, t, bits)
        assert _check(L, t, nu, bits) == (0, 1), (length, nu)
        near = [nu - 1] if nu > 0 else []                               # the smallest valid nonce: everything below it fails
        if bits:
            near.append(next(v for v in range(nu + 1, nu + (1 << 20)) if not pc.pow_ok(oracle, t, v, bits)))
        for v in near:
            assert not pc.pow_ok(oracle, t, v, bits)
            assert _check(L, t, v, bits) == (0, 0), (length, v)
        for b2 in BITS:                                                 # one nonce at every difficulty: the word, not one bit
            assert _check(L, t, nu, b2) == (0, int(pc.pow_ok(oracle, t, nu, b2))), (length, nu, b2)


def test_a_proof_ground_at_b_holds_at_every_smaller_b(L, oracle):
    t = transcript(37)
    nu = pc.grind(oracle, t, 12)
    assert all(_check(L, t, nu, b) == (0, 1) for b in range(13))
    assert pc.check_word(oracle, t, nu) & 0xFFF == 0


def test_the_whole_check_word_is_read(L, oracle):
    """bits 24..32: a nonce is accepted at exactly the difficulties up to the trailing zeros of the restated word"""
    t = transcript(5)
    for nu in (0, 1, 77, (1 << 64) - 1, 1 << 63, 0x0123456789abcdef):
        w = pc.check_word(oracle, t, nu)
        for b in range(pc.MAX_BITS + 1):
            assert _check(L, t, nu, b) == (0, int(w & ((1 << b) - 1) == 0)), (nu, b)


def test_refusals_and_the_empty_transcript(L, oracle):
    assert _check(L, b"abc", 0, 33)[0] == -50                            # SMI_ERR_BAD_ARG
    assert _check(L, b"", 0, 33)[0] == -50
    ok = C.c_int()
    assert L.smi_grind_check(None, 3, 0, 4, C.byref(ok)) == -50          # NULL with a length
    assert L.smi_grind_check(b"abc", 3, 0, 4, None) == -50
    for bits in BITS:                                                    # NULL with length 0 is the empty transcript
        nu = pc.grind(oracle, b"", bits)
        assert L.smi_grind_check(None, 0, nu, bits, C.byref(ok)) == 0 and ok.value == 1
        if nu:
            assert L.smi_grind_check(None, 0, nu - 1, bits, C.byref(ok)) == 0 and ok.value == 0
    assert _check(L, b"", 5, 32)[0] == 0                                 # SMI_GRIND_MAX_BITS itself is a difficulty


def test_status_string_of_the_new_code(L):
    text = L.smi_status_string(-55).decode()
    assert "proof of work" in text and text != L.smi_status_string(-999).decode()
    from stark_rs_amd import _lib
    assert _lib.status_string(-55) == text


def test_mirror_and_engine_level_check(L, oracle):
    from stark_rs_amd import engine, mirror
    t = transcript(25)
    nu = pc.grind(oracle, t, 8)
    fs = mirror.FiatShamir()
    fs.absorb(t)
    assert fs.check_grind(nu, 8) and (nu == 0 or not fs.check_grind(nu - 1, 8))
    assert bytes(fs.transcript) == t                                     # checking absorbs nothing
    assert engine.grind_check(t, nu, 8) and engine.Engine.grind_check(t, nu, 8)
    with pytest.raises(engine.StarkMiError):
        engine.grind_check(t, nu, 33)


def test_declared_in_the_header_the_ctypes_table_and_the_rust_binding(L):
    import stark_rs_amd as s
    declared = s.declared_symbols()
    rust = open(os.path.join(ROOT, "bindings", "stark_mi.rs")).read()
    header = open(os.path.join(ROOT, "include", "stark_mi.h")).read()
    assert re.search(r"#define SMI_GRIND_MAX_BITS 32\b", header)
    assert re.search(r"SMI_ERR_GRIND_EXHAUSTED = -55\b", header)
    assert re.search(r"pub const SMI_ERR_GRIND_EXHAUSTED: c_int = -55;", rust)
    assert re.search(r"pub const SMI_GRIND_MAX_BITS: u32 = 32;", rust)
    for name in NEW:
        assert name in declared, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert re.search(r"pub fn smi_dev_grind\(ctx: \*mut smi_ctx, transcript: \*const u8, transcript_len: usize, bits: u32, max_tries: u64, "
                     r"nonce: \*mut u64\) -> c_int;", rust)
    hand = rust[rust.index("// END GENERATED"):]
    for name in ("smi_grind_check", "smi_dev_grind", "smi_dev_air_prove_ext_pow", "smi_air_verify_ext_pow"):
        assert name + "(" in hand, name                                  # safe wrappers next to the extension ones
    # the existing configuration structs keep their layout: the difficulty is an argument, not a field
    from stark_rs_amd import _lib
    assert C.sizeof(_lib.FriCfg) == 40 and C.sizeof(_lib.StarkCfg) == 48
