"""FRI with more than 32 colinearity tests: the three regimes of sample_indices_kernel (csrc/fri.hip) -- accepted indices held
in registers up to 256 tests, lane 0's loop over LDS and global memory above, and more than one batch of 64 candidates in
either -- and everything whose grid or batch size comes from t: the base and extension query kernels, the column and row
openings of the STARK / AIR provers and the batched path verification inside the verifiers.  References: oracle.fri_prove
for the base field, tests/ext_compose.py and tests/pow_compose.py for the extension, all on oracle.fri_sample_indices.
Every comparison is exact: proof bytes and top-level indices.

The reference verifier interpolates the last codeword in O(last_n^3) (16 s at last_n = 1024, two minutes at 2048, a quarter
of an hour at 4096, and last_n lies in (4t, 8t]), so oracle.fri_verify itself is called up to last_n = 256 here and once at
512; above, the same verifier is restated below (`reference_verify`, src/fri.rs:313-504 statement for statement with its
reasons) over the oracle's primitives with the interpolation through oracle.fast_intt, which tests/test_oracle_fast.py
proves equal to the O(n^3) restatement.  The non-GPU tests of this file hold the two verifiers against each other and run
every configuration through the reference alone.  `pytest -m gpu` for the rest."""
import numpy as np
import pytest

import air_compose as ac
import ext_compose as xc
import pow_compose as pc
import transcript_compose as tc
from gpu_battery import PRIOR

P, G = xc.PRIMES[0]
P2, G2 = xc.PRIMES[1]
GEN = dict(xc.PRIMES)
E, OFFSET = 4, 3
TS = [33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 512]
FIVE = [64, 65, 256, 257, 300]
BASE_CASES = [(P, t, b"") for t in TS] + [(P2, t, b"") for t in FIVE] + [(P, t, PRIOR) for t in FIVE]
EXT_CASES = [(12, 4, 65), (14, 4, 257), (14, 4, 300)]
DENSE = [(64, 4, 64), (256, 4, 256), (512, 4, 512), (256, 4, 255), (256, 128, 128)]
NO_ROUNDS, NO_ROOTS = -17, "No FRI roots extracted"
LOW_DEGREE = "last codeword does not correspond to polynomial of low enough degree"
COLINEARITY = "colinearity check failure"
PATH_FAILS = "merkle authentication path verification fails for "
FLIP_REASONS = {"last triple of the last layer": COLINEARITY, "path of test 64": PATH_FAILS + "aa", "path of test 256": PATH_FAILS + "bb",
                "last path": PATH_FAILS + "cc"}


def _case_id(c):
    return "p%d-t%d%s" % (c[0], c[1], "-prior" if c[2] else "")


# ---------------------------------------------------------------------------------------------- the plan, from fri_plan.h
def plan(N, expansion, t):
    """-> (R, last_n): rounds go on while len > E and 4 t < len (src/fri.rs:93-103)"""
    ln, R = N, 0
    while ln > expansion and 4 * t < ln:
        ln, R = ln // 2, R + 1
    return R, (N >> (R - 1) if R else N)


def log_len_for(t, layers=3):
    """the smallest k at which a 2^k codeword has `layers` query layers (R - 1) under E = 4"""
    k = 3
    while plan(1 << k, E, t)[0] - 1 < layers:
        k += 1
    return k


def base_proof_len(N, t, R):
    n = 33 * R + 9 + 8 * (N >> (R - 1))
    for r in range(R - 1):
        depth = (N >> r).bit_length() - 1
        n += 33 * t + t * (2 * (9 + 32 * depth) + 9 + 32 * (depth - 1))
    return n


# ---------------------------------------------------------------------------------------------- the reference verifier
class FastInterpolation:
    """the oracle with Polynomial::interpolate_domain on a geometric domain through its radix-2 restatement"""

    def __init__(self, o):
        self._o = o

    def __getattr__(self, name):
        return getattr(self._o, name)

    def poly_interpolate_domain(self, dom, vals, p):
        n = len(dom)
        if n <= 64:
            return self._o.poly_interpolate_domain(dom, vals, p)
        offset, omega = int(dom[0]), int(dom[1]) * pow(int(dom[0]), -1, p) % p
        assert all(int(dom[i]) == offset * pow(omega, i, p) % p for i in (2, 3, n // 2, n - 1)) and pow(omega, n, p) == 1
        c = self._o.fast_intt(np.array([int(v) for v in vals], dtype=np.uint64), omega, offset, p)
        keep = len(c)
        while keep and c[keep - 1] == 0:          # mod.rs:57-68: trailing zeros are not part of the polynomial
            keep -= 1
        return c[:keep].copy()


class FastProver:
    """the oracle with Fri::fold_codeword and the leaf hashes through their fast restatements (tests/test_oracle_fast.py and
    tests/test_oracle_kats.py hold them against the op-for-op ones): tests/transcript_compose.py's prove over it writes a
    2^21-point proof in a third of oracle.fri_prove's time, what is left being the 2^22 hashes of round 0"""

    def __init__(self, o):
        self._o = o

    def __getattr__(self, name):
        return getattr(self._o, name)

    def fri_fold_codeword(self, cfg, cw, alpha, offset, omega):
        return self._o.fast_fold(cw, alpha, offset, omega, cfg.p)

    def leaf_hashes(self, cw):
        return self._o.leaf_hashes_batched(cw)


def reference_verify(o, cfg, stream, prior=b""):
    """Fri::verify (src/fri.rs:313-504) -> (accept, reason): tests/transcript_compose.py's verify with the reference's
    rejection messages (oracle/stark_oracle.c so_fri_verify) and the fast interpolation"""
    f = FastInterpolation(o)
    fs = tc.fiat_shamir(o, prior)
    p, t, N, R = cfg.p, int(cfg.num_colinearity_tests), int(cfg.domain_length), o.fri_num_rounds(cfg)
    at, roots, alphas = 0, [], []
    for _ in range(R):
        obj = tc._pop(stream, at)
        if obj is None or obj[0] != 0:
            return False, "Failed to extract Merkle root"
        roots.append(obj[1])
        fs.absorb(obj[1])
        alphas.append(fs.challenge())
        at = obj[2]
    obj = tc._pop(stream, at)
    if obj is None or obj[0] != 2:
        return False, "Failed to extract last codeword"
    last, at = obj[1], obj[2]
    if R == 0:
        return False, NO_ROOTS
    if o.merkle_commit(o.leaf_hashes(last)) != roots[-1]:
        return False, "last codeword is not well formed"
    bound = len(last) // int(cfg.expansion_factor)
    if bound == 0:
        return False, "last codeword too small"
    omega, offset = int(cfg.omega), int(cfg.offset)
    lo, loff = omega, offset
    for _ in range(R - 1):
        lo, loff = lo * lo % p, loff * loff % p
    dom = [loff * pow(lo, i, p) % p for i in range(len(last))]
    poly = f.poly_interpolate_domain(dom, last, p)
    if len(poly) - 1 > bound - 1:
        return False, LOW_DEGREE
    top = o.fri_sample_indices(o.hash_from_u64(fs.challenge()), N >> 1, N >> (R - 1), t)
    for r in range(R - 1):
        half = N >> (r + 1)
        c_idx = [i % half for i in top]
        trip = []
        for s in range(t):
            obj = tc._pop(stream, at)
            if obj is None or obj[0] != 2:
                return False, "Failed to extract triple values"
            if len(obj[1]) != 3:
                return False, "Expected triple of values"
            at = obj[2]
            trip.append(obj[1])
            ax = offset * pow(omega, c_idx[s], p) % p
            bx = offset * pow(omega, c_idx[s] + half, p) % p
            if not o.poly_test_colinearity([(ax, obj[1][0]), (bx, obj[1][1]), (alphas[r] % p, obj[1][2])], p):
                return False, COLINEARITY
        for s in range(t):
            for which, leaf_v, idx, root in (("aa", trip[s][0], c_idx[s], roots[r]), ("bb", trip[s][1], c_idx[s] + half, roots[r]),
                                             ("cc", trip[s][2], c_idx[s], roots[r + 1])):
                obj = tc._pop(stream, at)
                if obj is None or obj[0] != 3:
                    return False, "Failed to extract path for " + which
                at = obj[2]
                if not o.merkle_verify(o.hash_from_field_elements([leaf_v]), idx, obj[1], root):
                    return False, PATH_FAILS + which
        omega, offset = omega * omega % p, offset * offset % p
    return True, ""


def sampling_trace(o, seed, size, reduced_size, t):
    """Fri::sample_indices (src/fri.rs:176-213) candidate by candidate -> (indices, candidates drawn, the number of
    accepted indices before each batch of 64 candidates)"""
    out, seen, counter, at_batch = [], set(), 0, []
    while len(out) < t:
        if counter % 64 == 0:
            at_batch.append(len(out))
        index = o.fri_sample_index(o.hash_from_bytes(seed + counter.to_bytes(4, "little")), size)
        counter += 1
        if index % reduced_size not in seen:
            seen.add(index % reduced_size)
            out.append(index)
    return out, counter, at_batch


def base_trace(o, cfg, proof, prior):
    """the sampling of a base-field proof: the seed from its roots -> sampling_trace"""
    R, N = o.fri_num_rounds(cfg), int(cfg.domain_length)
    fs = tc.fiat_shamir(o, prior)
    for r in range(R):
        fs.absorb(proof[33 * r + 1:33 * r + 33])
    return sampling_trace(o, o.hash_from_u64(fs.challenge()), N >> 1, N >> (R - 1), int(cfg.num_colinearity_tests))


# ---------------------------------------------------------------------------------------------- references, computed once
_REF = {}


def base_ref(o, p, t, prior=b"", log_N=None):
    """-> dict(N, omega, cfg, cw, proof, top) of the reference's proof of a codeword of degree < N / 4"""
    key = ("base", p, t, bytes(prior), log_N)
    if key not in _REF:
        N = 1 << (log_len_for(t) if log_N is None else log_N)
        omega = o.ff_prim_nth_root_g(N, p, GEN[p])
        cw = o.fast_coset_ntt(o.splitmix64(77 + t, N // E) % np.uint64(p), N, omega, OFFSET, p)
        cfg = o.fri_cfg(omega, OFFSET, N, E, t, p)
        if log_N is not None and log_N > 16:
            proof, top = tc.prove(FastProver(o), cfg, cw, prior)
        else:
            proof, top = tc.prove(o, cfg, cw, prior) if prior else o.fri_prove(cfg, cw)
        _REF[key] = dict(N=N, omega=omega, cfg=cfg, cw=cw, proof=proof, top=[int(v) for v in top])
    return _REF[key]


def ext_ref(o, p, log_N, expansion, t, bits=None):
    key = ("ext", p, log_N, expansion, t, bits)
    if key not in _REF:
        g, N = GEN[p], 1 << log_N
        rng = np.random.default_rng(log_N + t)
        omega = o.ff_prim_nth_root_g(N, p, g)
        cw = np.stack([np.asarray(o.fast_coset_ntt(rng.integers(0, p, N // expansion, dtype=np.uint64), N, omega, g, p), dtype=np.uint64)
                       for _ in range(4)])
        cfg = o.fri_cfg(omega, g, N, expansion, t, p)
        if bits is None:
            proof, top = xc.prove(o, cfg, cw, g, PRIOR)
            nonce = None
        else:
            proof, top, nonce = pc.prove(o, cfg, cw, g, PRIOR, bits)
        _REF[key] = dict(N=N, omega=omega, cfg=cfg, cw=cw, proof=proof, top=top, nonce=nonce)
    return _REF[key]


def records(proof):
    """-> [(tag, first byte, one byte past the end)] of a proof's objects"""
    out, at = [], 0
    while at < len(proof):
        obj = xc._pop(proof, at)
        out.append((obj[0], at, obj[2]))
        at = obj[2]
    return out


def flips(proof, R, t, extra=0):
    """item by item the corruptions of the verifier test -> [(name, proof with one payload byte flipped)]; extra: records
    between the last codeword and the first layer (the nonce)"""
    recs = records(proof)
    first = R + 1 + extra                                   # the first triple of layer 0; a layer is t triples and 3 t paths
    picks = {"last triple of the last layer": recs[first + 4 * t * (R - 2) + t - 1],
             "path of test 64": recs[first + t + 3 * 64], "path of test 256": recs[first + t + 3 * 256 + 1], "last path": recs[-1]}
    assert picks["last triple of the last layer"][0] == 2 and all(picks[k][0] == 3 for k in picks if "path" in k)
    out = []
    for name, (_tag, a, b) in picks.items():
        bad = bytearray(proof)
        bad[a + 9] ^= 0x01                                  # the low byte of the first value / the first byte of the first digest
        out.append((name, bytes(bad)))
    return out


# ---------------------------------------------------------------------------------------------- without a GPU
def test_the_restated_verifier_is_the_oracles(oracle):
    """accepts and rejects with oracle.fri_verify, reason for reason, where that one is affordable (last_n = 256, and once
    at 512): the honest proof, a flipped triple, flipped paths, a codeword of too high a degree"""
    o = oracle
    for t in (33, 64):
        ref = base_ref(o, P, t)
        R = o.fri_num_rounds(ref["cfg"])
        assert o.fri_verify(ref["cfg"], ref["proof"]) and reference_verify(o, ref["cfg"], ref["proof"]) == (True, "")
        if t == 64:
            continue
        recs = records(ref["proof"])
        for k in (R + 1, R + 1 + t + 3 * 20 + 1, len(recs) - 1):
            bad = bytearray(ref["proof"])
            bad[recs[k][1] + 9] ^= 1
            assert not o.fri_verify(ref["cfg"], bytes(bad))
            assert reference_verify(o, ref["cfg"], bytes(bad)) == (False, o.fri_last_reject())
        tight = o.fri_cfg(ref["omega"], OFFSET, ref["N"], 2 * E, t, P)   # same rounds (E does not bind), half the degree bound
        assert not o.fri_verify(tight, ref["proof"])
        assert reference_verify(o, tight, ref["proof"]) == (False, o.fri_last_reject()) == (False, LOW_DEGREE)
    f = FastInterpolation(o)
    dom = [5 * pow(o.ff_prim_nth_root(128), i, P) % P for i in range(128)]
    vals = [int(v) for v in o.splitmix64(9, 128) % np.uint64(P)]
    assert list(f.poly_interpolate_domain(dom, vals, P)) == list(o.poly_interpolate_domain(dom, vals, P))


def test_every_configuration_through_the_reference_alone(oracle):
    """the inputs of the GPU tests below are ones the reference proves and its own verifier accepts; the sampling of each,
    candidate by candidate: the plan, the regime of the kernel it selects and the batches of 64 candidates it needs"""
    o = oracle
    crossed, multi = set(), set()
    for p, t, prior in BASE_CASES:
        ref = base_ref(o, p, t, prior)
        R, last_n = plan(ref["N"], E, t)
        assert R == o.fri_num_rounds(ref["cfg"]) and R - 1 >= 3 and 4 * t < last_n <= 8 * t
        assert plan(ref["N"] // 2, E, t)[0] - 1 < 3                      # the smallest such length
        assert len(ref["proof"]) == base_proof_len(ref["N"], t, R)
        assert reference_verify(o, ref["cfg"], ref["proof"], prior) == (True, "")
        if last_n <= 256 and not prior:
            assert o.fri_verify(ref["cfg"], ref["proof"]), o.fri_last_reject()
        top, drawn, at_batch = base_trace(o, ref["cfg"], ref["proof"], prior)
        assert top == ref["top"] and len({i % last_n for i in top}) == t
        regime = "registers" if t <= 256 else "LDS+global"
        batches = len(at_batch)
        print("t=%d p=%d prior=%d: N=2^%d R=%d last_n=%d %s, %d candidates in %d batches" %
              (t, p, len(prior), ref["N"].bit_length() - 1, R, last_n, regime, drawn, batches))
        if batches > 1:
            multi.add(regime)
        for edge in (64, 128, 192, 256):                                  # a batch that starts below the edge and ends above
            if any(a < edge < b for a, b in zip(at_batch, at_batch[1:] + [t])):
                crossed.add(edge)
    assert multi == {"registers", "LDS+global"} and crossed == {64, 128, 192, 256}
    for p, _g in xc.PRIMES:
        for log_N, expansion, t in EXT_CASES:
            ref = ext_ref(o, p, log_N, expansion, t)
            R = o.fri_num_rounds(ref["cfg"])
            assert R - 1 >= 2 and len(ref["proof"]) == xc.proof_len(ref["N"], expansion, t, R)
            ok, _pv, used, top = xc.verify(FastInterpolation(o), ref["cfg"], ref["proof"], GEN[p], PRIOR)
            assert ok and used == len(ref["proof"]) and top == ref["top"]
    ref = ext_ref(o, P, 14, 4, 257, bits=8)
    assert pc.verify(FastInterpolation(o), ref["cfg"], ref["proof"], G, PRIOR, 8)[0]


def test_the_reference_rejects_each_flip_at_257_queries(oracle):
    """the corruptions of the verifier tests below, through the references alone: each is rejected, for the reason expected"""
    o, t, f = oracle, 257, FastInterpolation(oracle)
    ref = base_ref(o, P, t)
    for name, bad in flips(ref["proof"], o.fri_num_rounds(ref["cfg"]), t):
        assert reference_verify(o, ref["cfg"], bad) == (False, FLIP_REASONS[name]), name
    for bits in (None, 8):
        ref = ext_ref(o, P, 14, 4, t, bits=bits)
        for name, bad in flips(ref["proof"], o.fri_num_rounds(ref["cfg"]), t, extra=0 if bits is None else 1):
            if bits is None:
                assert not xc.verify(f, ref["cfg"], bad, G, PRIOR)[0], name
            else:
                assert pc.verify(f, ref["cfg"], bad, G, PRIOR, bits)[4] == ("colinearity" if "triple" in name else "path"), name


@pytest.mark.parametrize("N,expansion,t", DENSE)
def test_dense_sampling_has_no_rounds_in_the_reference(oracle, N, expansion, t):
    """t = last_n needs 4 t >= N, and there num_rounds() is 0, never 1: a round is only made while 4 t < len, so every
    proof with a root has last_n > 4 t.  The reference proves such a case (all of the domain sampled, no layer) and its own
    verifier rejects the proof for having no root; with t above the domain's length it panics."""
    o = oracle
    assert plan(N, expansion, t) == (0, N)
    omega = o.ff_prim_nth_root(N)
    cw = o.fast_coset_ntt(o.splitmix64(N + t, max(N // expansion, 1)) % np.uint64(P), N, omega, OFFSET)
    cfg = o.fri_cfg(omega, OFFSET, N, expansion, t)
    assert o.fri_num_rounds(cfg) == 0
    proof, top = o.fri_prove(cfg, cw)
    assert len(proof) == 9 + 8 * N and len({i % N for i in top}) == t
    assert not o.fri_verify(cfg, proof) and o.fri_last_reject() == NO_ROOTS
    with pytest.raises(o.OraclePanic, match="cannot sample more indices than available in last codeword"):
        o.fri_prove(o.fri_cfg(omega, OFFSET, N, expansion, N + 1), cw)
    with pytest.raises(o.OraclePanic, match="not enough entropy in indices wrt last codeword"):
        o.fri_prove(o.fri_cfg(omega, OFFSET, N, expansion, 2 * N + 1), cw)


# ---------------------------------------------------------------------------------------------- on the GPU
from test_gpu_air import Dev, engines  # noqa: E402,F401  (engines is a fixture)

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("case", BASE_CASES, ids=_case_id)
def test_base_prove_in_every_sampling_regime(engines, oracle, case):
    p, t, prior = case
    o, eng = oracle, engines[p]
    ref = base_ref(o, p, t, prior)
    cfg = eng.fri_cfg(ref["omega"], OFFSET, ref["N"], E, t)
    proof, top = eng.fri_prove(cfg, ref["cw"], transcript=prior)
    assert top == ref["top"]
    assert proof == ref["proof"]
    assert len(proof) == base_proof_len(ref["N"], t, eng.fri_num_rounds(cfg))
    assert reference_verify(o, ref["cfg"], proof, prior) == (True, "")
    if plan(ref["N"], E, t)[1] <= 256 and not prior:
        assert o.fri_verify(ref["cfg"], proof), o.fri_last_reject()
    ok, _pv, why = eng.fri_verify(cfg, proof, transcript=prior)
    assert ok, why


@gpu
@pytest.mark.parametrize("t", [65, 257])
def test_dev_prove_from_a_device_codeword(engines, oracle, t):
    eng, ref = engines[P], base_ref(oracle, P, t)
    cfg = eng.fri_cfg(ref["omega"], OFFSET, ref["N"], E, t)
    with Dev(eng) as dev:
        proof, top = eng.dev_fri_prove(cfg, dev.upload(ref["cw"]), ref["N"])
        d = dev.alloc(4 * ref["N"] + 16)                    # only 4-byte aligned: the other leaf source of round 0
        eng.dev_upload(ref["cw"], d + 4)
        proof2, top2 = eng.dev_fri_prove(cfg, d + 4, ref["N"])
    assert top == top2 == ref["top"]
    assert proof == ref["proof"] and proof2 == ref["proof"]


@gpu
def test_dev_prove_with_folds_computed_by_the_leaf_kernel(engines, oracle):
    """2^21 points: round 1's tree kernel folds round 0 itself from an aligned codeword, a separate fold launch serves
    one that is only 4-byte aligned (tests/test_gpu_pipeline.py) -- both launch plans at t = 257, eleven rounds"""
    t, log_N = 257, 21
    eng, ref = engines[P], base_ref(oracle, P, t, log_N=log_N)
    N = ref["N"]
    cfg = eng.fri_cfg(ref["omega"], OFFSET, N, E, t)
    assert eng.fri_num_rounds(cfg) == plan(N, E, t)[0] == 11
    with Dev(eng) as dev:
        d = dev.alloc(4 * N + 16)
        for lead in (0, 4):
            eng.dev_upload(ref["cw"], d + lead)
            proof, top = eng.dev_fri_prove(cfg, d + lead, N)
            assert top == ref["top"], lead
            assert proof == ref["proof"], lead
    assert len(ref["proof"]) == base_proof_len(N, t, 11)


@gpu
@pytest.mark.parametrize("N,expansion,t", DENSE)
def test_dense_sampling_is_refused_before_any_launch(engines, oracle, N, expansion, t):
    """num_rounds() == 0 in every case that would sample all of the last codeword (see the non-GPU test of the same cases):
    the library refuses what the reference's verifier rejects, SMI_ERR_NO_ROUNDS, and that check comes before the two
    sampling asserts, which last_n > 4 t puts out of reach of a proof with rounds.  The context goes on working."""
    import stark_rs_amd as s
    o, eng = oracle, engines[P]
    omega = o.ff_prim_nth_root(N)
    cw = o.fast_coset_ntt(o.splitmix64(N + t, max(N // expansion, 1)) % np.uint64(P), N, omega, OFFSET)
    for tt in (t, N + 1, 2 * N + 1):
        cfg = eng.fri_cfg(omega, OFFSET, N, expansion, tt)
        assert eng.fri_num_rounds(cfg) == 0
        with pytest.raises(s.StarkMiError, match=NO_ROOTS) as ei:
            eng.fri_prove(cfg, cw)
        assert ei.value.status == NO_ROUNDS
        with Dev(eng) as dev:
            with pytest.raises(s.StarkMiError) as ei:
                eng.dev_fri_prove(cfg, dev.upload(cw), N)
        assert ei.value.status == NO_ROUNDS
    ref = base_ref(o, P, 33)
    assert eng.fri_prove(eng.fri_cfg(ref["omega"], OFFSET, ref["N"], E, 33), ref["cw"]) == (ref["proof"], ref["top"])


def _ext_cols(cw):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(cw.astype(np.uint32)).view(np.int32).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t


@gpu
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_N,expansion,t", EXT_CASES)
def test_prove_ext_at_many_queries(engines, oracle, p, g, log_N, expansion, t):
    o, eng = oracle, engines[p]
    ref = ext_ref(o, p, log_N, expansion, t)
    cfg = eng.fri_cfg(ref["omega"], g, ref["N"], expansion, t)
    cols = _ext_cols(ref["cw"])
    proof, top = eng.dev_fri_prove_ext(cfg, cols.data_ptr(), ref["N"], transcript=PRIOR)
    assert top == ref["top"]
    assert proof == ref["proof"]
    ok, _pv, used, why = eng.fri_verify_ext(cfg, proof, PRIOR)
    assert ok and used == len(proof), why
    assert xc.verify(FastInterpolation(o), ref["cfg"], proof, g, PRIOR)[0]


@gpu
def test_prove_ext_with_grinding_at_257_queries(engines, oracle):
    o, eng, bits = oracle, engines[P], 8
    ref = ext_ref(o, P, 14, 4, 257, bits=bits)
    cfg = eng.fri_cfg(ref["omega"], G, ref["N"], 4, 257)
    cols = _ext_cols(ref["cw"])
    proof, top, nonce = eng.dev_fri_prove_ext(cfg, cols.data_ptr(), ref["N"], transcript=PRIOR, grind_bits=bits)
    assert (nonce, top) == (ref["nonce"], ref["top"])
    assert proof == ref["proof"]
    ok, _pv, used, why = eng.fri_verify_ext(cfg, proof, PRIOR, grind_bits=bits)
    assert ok and used == len(proof), why
    assert pc.verify(FastInterpolation(o), ref["cfg"], proof, G, PRIOR, bits)[0]


# ---------------------------------------------------------------------------------------------- the pipelines that open
@gpu
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("t", [65, 257])
def test_stark_prove_opens_every_column_at_every_sampled_position(engines, oracle, p, g, t):
    """W = 4, 2^10 rows, blowup 8: the FRI proof of the weighted column sum is the oracle's, the opening section the
    restatement of tests/conftest.py, and smi_stark_verify accepts"""
    from conftest import column_openings_bytes
    o, eng = oracle, engines[p]
    log_n, lb, W = 10, 3, 4
    n, N = 1 << log_n, 1 << (log_n + lb)
    assert plan(N, 1 << lb, t)[0] - 1 >= 2
    cols = np.stack([o.splitmix64(0x5354524B00 + c, n) % np.uint64(p) for c in range(W)])
    with Dev(eng) as dev:
        res = eng.dev_stark_prove(dev.upload(cols), W, log_n, lb, t, open_columns=True)
    w, wN = o.ff_prim_nth_root_g(n, p, g), o.ff_prim_nth_root_g(N, p, g)
    lde = [o.fast_coset_ntt(o.fast_intt(cols[c], w, 1, p), N, wN, g, p) for c in range(W)]
    roots = [o.merkle_commit(o.leaf_hashes_batched(col)) for col in lde]
    assert [bytes(r) for r in res["column_roots"]] == roots
    fs, weights = o.FiatShamir(), []
    for root in roots:
        fs.absorb(root)
        weights.append(fs.challenge() % p)
    combined = sum(lde[c] * np.uint64(weights[c]) for c in range(W)) % np.uint64(p)   # four products below 2^60
    fri, top = o.fri_prove(o.fri_cfg(wN, g, N, 1 << lb, t, p), combined)
    assert res["top_indices"] == top
    assert res["proof"][:len(fri)] == fri
    assert res["proof"][len(fri):] == column_openings_bytes(o, lde, top, N)
    ok, why = eng.stark_verify(res["proof"], res["column_roots"], W, log_n, lb, t, open_columns=True)
    assert ok, why
    bad = bytearray(res["proof"])
    bad[-1] ^= 1                                            # the last digest of the last path of the last test
    assert not eng.stark_verify(bytes(bad), res["column_roots"], W, log_n, lb, t, open_columns=True)[0]


@gpu
@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("t", [65, 257])
def test_air_prove_column_trees_at_many_queries(engines, oracle, p, g, t):
    """the mixer at 2^10 rows, blowup 8: d = 3, FRI at E = 4 on 2^13 points -- R - 1 = 4 query layers at t = 65, 2 at 257"""
    from test_gpu_air import _prove, _split
    o, eng, log_n, lb = oracle, engines[p], 10, 3
    N, B = 1 << (log_n + lb), 1 << lb
    air, cols = ac.make("mixer", 1 << log_n, p)
    W, K = air.n_cols, len(air.constraints)
    _d, exp = eng.air_plan(air, W, log_n, lb)
    assert exp == 4 and plan(N, exp, t)[0] - 1 >= 2
    with Dev(eng) as dev:
        res = _prove(eng, dev, air, cols, log_n, lb, t)
    lde = ac.lde(o, cols, p, g, log_n, lb, 1, g)
    roots = [o.merkle_commit(o.leaf_hashes(col)) for col in lde]
    assert [bytes(r) for r in res["column_roots"]] == roots
    prior, wts = ac.transcript(o, air, roots)
    codeword, _ = ac.codeword_poly_route(o, air, cols, wts, p, g, log_n, lb, 1, g)
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    want_fri, top = tc.prove(o, o.fri_cfg(wN, g, N, exp, t, p), codeword, prior)
    fri, opened = _split(res, W, K, log_n + lb, t)
    assert res["top_indices"] == [int(x) for x in top]
    assert fri == want_fri
    assert opened == ac.openings_bytes(o, lde, top, N, B, True)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t)
    assert ok, why


@gpu
@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("t", [65, 257])
def test_air_prove_rows_at_many_queries(engines, oracle, p, g, t):
    from test_gpu_air_rows import assert_proof
    o, eng, log_n, lb = oracle, engines[p], 10, 3
    air, cols = ac.make("mixer", 1 << log_n, p)
    codeword = lambda wts: ac.codeword_poly_route(o, air, cols, wts, p, g, log_n, lb, 1, g)[0]
    assert_proof(o, eng, air, cols, codeword, p, g, log_n, lb, t)


@gpu
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("t", [65, 257])
def test_air_prove_ext_at_many_queries(engines, oracle, p, g, t):
    from test_gpu_ext import restated_air_proof
    o, eng, log_n, lb = oracle, engines[p], 10, 3
    air, cols = ac.make("mixer", 1 << log_n, p)
    W = len(cols)
    _d, exp = eng.air_plan(air, W, log_n, lb)
    with Dev(eng) as dev:
        res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, row_leaves=True, ext=True)
    root, want, top = restated_air_proof(o, air, cols, p, g, log_n, lb, t, 1, g, exp)
    assert bytes(res["column_roots"][0]) == root
    assert res["top_indices"] == top
    assert res["proof"] == want
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True)
    assert ok, why
    bad = bytearray(res["proof"])
    bad[-1] ^= 1
    assert not eng.air_verify(air, bytes(bad), res["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True)[0]


# ---------------------------------------------------------------------------------------------- the verifiers at width
@gpu
def test_base_verifier_rejects_each_flip_with_the_references_reason(engines, oracle):
    """t = 257: 771 paths per layer in one smi_merkle_verify_batch; the first failure is named as the reference names it"""
    o, eng, t = oracle, engines[P], 257
    ref = base_ref(o, P, t)
    cfg = eng.fri_cfg(ref["omega"], OFFSET, ref["N"], E, t)
    R = eng.fri_num_rounds(cfg)
    assert eng.fri_verify(cfg, ref["proof"])[0]
    for name, bad in flips(ref["proof"], R, t):
        ok_o, why_o = reference_verify(o, ref["cfg"], bad)
        ok, _pv, why = eng.fri_verify(cfg, bad)
        assert not ok and not ok_o, name
        assert why == why_o == FLIP_REASONS[name], name


@gpu
@pytest.mark.parametrize("bits", [None, 8])
def test_ext_verifier_rejects_each_flip(engines, oracle, bits):
    o, eng, t = oracle, engines[P], 257
    ref = ext_ref(o, P, 14, 4, t, bits=bits)
    cfg = eng.fri_cfg(ref["omega"], G, ref["N"], 4, t)
    R = eng.fri_num_rounds(cfg)
    assert eng.fri_verify_ext(cfg, ref["proof"], PRIOR, grind_bits=bits)[0]
    f = FastInterpolation(o)
    for name, bad in flips(ref["proof"], R, t, extra=0 if bits is None else 1):
        ok, _pv, _used, why = eng.fri_verify_ext(cfg, bad, PRIOR, grind_bits=bits)
        assert not ok, name
        assert why == FLIP_REASONS[name], name
        if bits is None:
            assert not xc.verify(f, ref["cfg"], bad, G, PRIOR)[0], name
        else:
            why_o = pc.verify(f, ref["cfg"], bad, G, PRIOR, bits)[4]
            assert why_o == ("colinearity" if "triple" in name else "path"), name
