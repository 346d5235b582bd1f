"""GPU: proof-of-work grinding (include/stark_mi.h, "Grinding") -- smi_dev_grind, smi_dev_fri_prove_ext_pow /
smi_fri_verify_ext_pow, smi_dev_air_prove_ext_pow / smi_air_verify_ext_pow -- against the restatement over the CPU
oracle's primitives (tests/pow_compose.py) and the CPU emulator of the search kernel.  Every comparison is exact.
`pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import air_rows as ar
import ext_compose as xc
import pow_compose as pc
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_ext import _dev_cols, low_degree_codeword

pytestmark = pytest.mark.gpu

# phases 0, 5, 24, 25, 31, 0, 5, 8: both sides of the 9 / 10-mix split
LENGTHS = [0, 5, 24, 25, 31, 32, 37, 200]


def transcript(length):
    return bytes(np.random.default_rng(9000 + length).integers(0, 256, length, dtype=np.uint8))


# ---------------------------------------------------------------------------------------------- the search alone
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("bits", [0, 8, 12, 16])
def test_dev_grind_finds_the_smallest_nonce(engines, oracle, p, g, bits):
    eng = engines[p]
    for length in LENGTHS:
        t = transcript(length)
        want = pc.grind(oracle, t, bits)
        assert eng.grind(t, bits) == want, length
        assert eng.grind(t, bits, max_tries=want + 1) == want, length       # the cap is exclusive


def test_dev_grind_at_twenty_bits_against_the_host_check_and_the_emulator(engines):
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    eng = engines[xc.PRIMES[0][0]]
    t = transcript(37)
    nu = eng.grind(t, 20)
    assert s.engine.grind_check(t, nu, 20)
    emu = C.CDLL(_lib.EMU_PATH)
    emu.emu_fs_seed.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
    emu.emu_grind.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    words, phase, out = np.zeros(16, dtype=np.uint32), C.c_uint32(), np.zeros(1, dtype=np.uint64)
    emu.emu_fs_seed(t, len(t), words.ctypes.data, C.addressof(phase))
    assert emu.emu_grind(words.ctypes.data, phase.value, 20, 0, 4096, out.ctypes.data) == 0
    assert nu == int(out[0])                                                # the smallest one, not just a valid one


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_an_exhausted_search_is_a_status_and_the_context_goes_on(engines, oracle, p, g):
    import stark_rs_amd as s
    eng = engines[p]
    t = next(x for x in map(transcript, LENGTHS) if pc.grind(oracle, x, 16) > 4)
    with pytest.raises(s.StarkMiError) as ei:
        eng.grind(t, 16, max_tries=4)
    assert ei.value.status == -55 and "proof of work" in str(ei.value)
    assert eng.grind(t, 16) == pc.grind(oracle, t, 16)
    with pytest.raises(s.StarkMiError) as ei:
        eng.grind(t, 33)
    assert ei.value.status == -50 and "grind_bits" in str(ei.value)


def test_mirror_fiat_shamir_grinds_and_absorbs(engines, oracle):
    from stark_rs_amd import mirror
    fs = mirror.FiatShamir()
    fs.absorb(transcript(25))
    nu = fs.grind(12)
    assert nu == pc.grind(oracle, transcript(25), 12)
    assert bytes(fs.transcript) == transcript(25) + nu.to_bytes(8, "little")


# ---------------------------------------------------------------------------------------------- FRI over F_q with grinding
def gpu_prove(eng, cfg, cw, prior, bits):
    """bits = None: smi_dev_fri_prove_ext, the proof without grinding -> (proof, top); otherwise -> (proof, top, nonce)"""
    import torch
    t_in, d_in = _dev_cols(cw)
    torch.cuda.synchronize()
    return eng.dev_fri_prove_ext(cfg, d_in, cw.shape[1], transcript=prior, grind_bits=bits)


def after_last_root(proof, prior, R):
    """the transcript as it stands after the last root: the prefix, every root, four counters behind all but the last"""
    tr = bytearray(prior)
    for r in range(R):
        tr += proof[33 * r + 1:33 * r + 33]
        if r < R - 1:
            for e in range(4):
                tr += xc._u64(e)
    return bytes(tr)


def failing_bits(o, tr, nonce, bits):
    """the least difficulty above `bits` the nonce does not meet, by the restatement"""
    return next(b for b in range(bits + 1, pc.MAX_BITS + 1) if not pc.pow_ok(o, tr, nonce, b))


def failing_nonce(o, tr, nonce, bits):
    return next(v for v in range(nonce + 1, nonce + (1 << 20)) if not pc.pow_ok(o, tr, v, bits))


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("bits", [0, 8, 12])
@pytest.mark.parametrize("prior_len", [0, 5, 24, 25, 37])
@pytest.mark.parametrize("log_N,E,t", [(8, 4, 4), (12, 4, 8)])
def test_prove_pow_bytes_equal_the_restatement_and_verify_agrees(engines, oracle, p, g, log_N, E, t, prior_len, bits):
    """at a 25-byte prefix the nonce crosses a chunk boundary and the seed is drawn at phase 1; at 24 bytes it completes the
    chunk and the seed is drawn at phase 0, by the sixteen-lane kernel"""
    eng, N, prior = engines[p], 1 << log_N, bytes(range(prior_len))
    cw, omega = low_degree_codeword(oracle, p, g, N, E, g, log_N)
    cfg_o, cfg = oracle.fri_cfg(omega, g, N, E, t, p), eng.fri_cfg(omega, g, N, E, t)
    want, want_top, want_nonce = pc.prove(oracle, cfg_o, cw, g, prior, bits)
    got, top, nonce = gpu_prove(eng, cfg, cw, prior, bits)
    assert nonce == want_nonce
    assert top == want_top
    assert got == want
    R = oracle.fri_num_rounds(cfg_o)
    assert len(got) == pc.proof_len(N, E, t, R) == len(gpu_prove(eng, cfg, cw, prior, None)[0]) + 17
    ok_o, pv_o, used_o, _top, _why = pc.verify(oracle, cfg_o, got, g, prior, bits)
    ok, pv, used, why = eng.fri_verify_ext(cfg, got, prior, grind_bits=bits)
    assert ok_o and ok, why
    assert pv == pv_o and used == used_o == len(got)
    if bits >= 4:                                                           # a proof ground at b verifies at b' <= b
        assert eng.fri_verify_ext(cfg, got, prior, grind_bits=bits - 4)[0] and pc.verify(oracle, cfg_o, got, g, prior, bits - 4)[0]
        assert eng.fri_verify_ext(cfg, got, prior, grind_bits=0)[0]


def _both_reject(eng, oracle, cfg, cfg_o, g, proof, prior, bits, reason=None):
    ok_o = pc.verify(oracle, cfg_o, proof, g, prior, bits)[0]
    ok, _pv, used, why = eng.fri_verify_ext(cfg, proof, prior, grind_bits=bits)
    assert not ok_o and not ok and why and used == 0
    if reason:
        assert why == reason
    return why


def fri_rejections(o, tr, proof, nonce, at, bits):
    """-> [(name, proof bytes, difficulty, the reason where one is named)]: the ways a nonce record can be wrong; `at` is
    its first byte"""
    out = []
    bad = bytearray(proof)
    bad[at + 9:at + 17] = xc._u64(failing_nonce(o, tr, nonce, bits))
    out.append(("a nonce that fails", bytes(bad), bits, "proof of work"))
    out.append(("a raised difficulty", proof, failing_bits(o, tr, nonce, bits), "proof of work"))
    bad = bytearray(proof)
    bad[at + 1] = 2
    out.append(("count 2, nothing added", bytes(bad), bits, None))
    out.append(("count 2, a second value", proof[:at] + xc._elems([nonce, nonce]) + proof[at + 17:], bits, None))
    out.append(("count 0", proof[:at] + xc._elems([]) + proof[at + 17:], bits, None))
    out.append(("the record missing", proof[:at] + proof[at + 17:], bits, None))
    for k in range(8):
        bad = bytearray(proof)
        bad[at + 9 + k] ^= 0x01 if k else 0x80
        out.append(("byte %d of the nonce flipped" % k, bytes(bad), bits, None))
    for cut in (1, 8, 9, 12, 16):
        out.append(("cut %d bytes into the record" % cut, proof[:at + cut], bits, None))
    out.append(("cut behind the record", proof[:at + 17], bits, None))
    return out


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("prior", [b"", bytes(range(25))])
def test_verify_pow_rejections(engines, oracle, p, g, prior):
    eng, N, E, t, bits = engines[p], 1 << 10, 4, 6, 8
    cw, omega = low_degree_codeword(oracle, p, g, N, E, g, 4)
    cfg_o, cfg = oracle.fri_cfg(omega, g, N, E, t, p), eng.fri_cfg(omega, g, N, E, t)
    proof, _top, nonce = gpu_prove(eng, cfg, cw, prior, bits)
    R = oracle.fri_num_rounds(cfg_o)
    at, tr = pc.nonce_offset(N, R), after_last_root(proof, prior, R)
    assert proof[at:at + 17] == pc.record(nonce) and pc.pow_ok(oracle, tr, nonce, bits)
    assert eng.fri_verify_ext(cfg, proof, prior, grind_bits=bits)[0] and pc.verify(oracle, cfg_o, proof, g, prior, bits)[0]
    for name, bad, b, reason in fri_rejections(oracle, tr, proof, nonce, at, bits):
        _both_reject(eng, oracle, cfg, cfg_o, g, bad, prior, b, reason)
    # a proof without grinding offered here, and a ground proof offered to the verifier without grinding
    plain, _ = gpu_prove(eng, cfg, cw, prior, None)
    assert eng.fri_verify_ext(cfg, plain, prior)[0]
    assert "proof of work" in _both_reject(eng, oracle, cfg, cfg_o, g, plain, prior, bits)
    _both_reject(eng, oracle, cfg, cfg_o, g, plain, prior, 0)                # even at difficulty 0 the record is part of the stream
    ok, _pv, _used, why = eng.fri_verify_ext(cfg, proof, prior)
    assert not ok and why and not xc.verify(oracle, cfg_o, proof, g, prior)[0]
    import stark_rs_amd as s
    with pytest.raises(s.StarkMiError) as ei:
        eng.fri_verify_ext(cfg, proof, prior, grind_bits=33)
    assert ei.value.status == -50
    with pytest.raises(s.StarkMiError) as ei:
        gpu_prove(eng, cfg, cw, prior, 33)
    assert ei.value.status == -50


# ---------------------------------------------------------------------------------------------- the AIR proof
def _air_cases(p, n):
    yield "fib", ac.make("fib", n, p)
    yield "mixer", ac.make("mixer", n, p)
    yield "mimc", ap.make("mimc", n, p)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("bits", [8, 12])
@pytest.mark.parametrize("log_n", [8, 10])
def test_air_prove_pow_bytes_equal_the_restatement_and_verify_accepts(engines, oracle, p, g, log_n, bits):
    eng, lb, t = engines[p], 3, 4
    kw = dict(row_leaves=True, ext=True)
    for name, (air, cols) in _air_cases(p, 1 << log_n):
        W = len(cols)
        _d, E = eng.air_plan(air, W, log_n, lb)
        with Dev(eng) as dev:
            d_trace = dev.upload(np.array(cols, dtype=np.uint64))
            res = eng.dev_air_prove(air, d_trace, W, log_n, lb, t, grind_bits=bits, **kw)
            plain = eng.dev_air_prove(air, d_trace, W, log_n, lb, t, **kw)
        root, want, top, _nonce = pc.air_proof(oracle, air, cols, p, g, log_n, lb, t, 1, g, E, bits)
        assert bytes(res["column_roots"][0]) == root, name
        assert res["top_indices"] == top, name
        assert res["proof"] == want, name
        assert len(res["proof"]) == len(plain["proof"]) + 17, name
        roots = res["column_roots"]
        for b in (bits, bits - 4, 0):
            ok, why = eng.air_verify(air, res["proof"], roots, W, log_n, lb, t, grind_bits=b, **kw)
            assert ok, (name, b, why)
        ok, why = eng.air_verify(air, res["proof"], roots, W, log_n, lb, t, **kw)
        assert not ok and why, name                                         # the verifier without grinding rejects it
        ok, why = eng.air_verify(air, plain["proof"], plain["column_roots"], W, log_n, lb, t, grind_bits=bits, **kw)
        assert not ok and "proof of work" in why, name                      # ... and the other way round


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_air_verify_pow_rejections(engines, oracle, p, g):
    eng, log_n, lb, t, bits = engines[p], 9, 3, 8, 8
    n, N = 1 << log_n, 1 << (log_n + lb)
    air, cols = ac.make("mixer", n, p)
    W, K = len(cols), len(air.constraints)
    kw = dict(row_leaves=True, ext=True)
    _d, E = eng.air_plan(air, W, log_n, lb)
    with Dev(eng) as dev:
        res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, grind_bits=bits, **kw)
    roots, proof = res["column_roots"], res["proof"]
    assert eng.air_verify(air, proof, roots, W, log_n, lb, t, grind_bits=bits, **kw)[0]
    cfg = eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t)
    R = eng.fri_num_rounds(cfg)
    at = pc.nonce_offset(N, R)
    nonce = int.from_bytes(proof[at + 9:at + 17], "little")
    assert proof[at:at + 9] == b"\x02" + xc._u64(1)
    prior, _ch = xc.air_transcript(oracle, W, K, bytes(roots[0]))
    tr = after_last_root(proof, prior, R)
    assert nonce == pc.grind(oracle, tr, bits)
    for name, bad, b, reason in fri_rejections(oracle, tr, proof, nonce, at, bits):
        ok, why = eng.air_verify(air, bad, roots, W, log_n, lb, t, grind_bits=b, **kw)
        assert not ok and why, name
        if reason:
            assert why == reason, name
    bad = bytearray(proof)                                                  # the opening section is still checked
    bad[-5] ^= 1
    assert not eng.air_verify(air, bytes(bad), roots, W, log_n, lb, t, grind_bits=bits, **kw)[0]
    assert not eng.air_verify(air, proof[:-1], roots, W, log_n, lb, t, grind_bits=bits, **kw)[0]
    import stark_rs_amd as s
    with pytest.raises(s.StarkMiError, match="ext=True"):
        eng.air_verify(air, proof, roots, W, log_n, lb, t, row_leaves=True, grind_bits=bits)
    with pytest.raises(s.StarkMiError) as ei:
        eng.air_verify(air, proof, roots, W, log_n, lb, t, grind_bits=33, **kw)
    assert ei.value.status == -50


def test_air_prove_pow_headline_shape_is_accepted(engines):
    """2^22 x 4, B = 8, t = 32 on the second prime at 16 bits: accepted, and the proof has the predicted length"""
    import torch
    p, g = xc.PRIMES[1]
    eng, log_n, lb, t, W, bits = engines[p], 22, 3, 32, 4, 16
    n, N = 1 << log_n, 1 << (log_n + lb)
    rng = np.random.default_rng(1)
    y = rng.integers(0, p, n, dtype=np.int64)
    xv, yl, xs = 5, y.tolist(), [5]
    for r in range(n - 1):                                                  # x' = x y + 1: a satisfiable AIR numpy builds quickly
        xv = (xv * yl[r] + 1) % p
        xs.append(xv)
    cols = np.stack([np.array(xs, dtype=np.int64), y, rng.integers(0, p, n, dtype=np.int64), rng.integers(0, p, n, dtype=np.int64)])
    from stark_rs_amd.mirror import Air
    air = Air(W)
    air.transition({("next", 0): 1, (("cur", 0), ("cur", 1)): -1, (): -1})
    air.boundary(0, 0, 5).boundary(3, n - 1, int(cols[3][n - 1]))
    _d, E = eng.air_plan(air, W, log_n, lb)
    trace = torch.from_numpy(cols.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    kw = dict(row_leaves=True, ext=True)
    res = eng.dev_air_prove(air, trace.data_ptr(), W, log_n, lb, t, timed=True, grind_bits=bits, **kw)
    cfg = eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t)
    R = eng.fri_num_rounds(cfg)
    assert len(res["proof"]) == pc.proof_len(N, E, t, R) + ar.opening_len(W, 1, log_n + lb, t)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **kw)
    assert ok, why
    assert not eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, **kw)[0]
    print("stage_ms", res["stage_ms"])
