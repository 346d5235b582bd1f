"""GPU: zero-knowledge DEEP proofs (include/stark_mi.h, "Zero-knowledge DEEP proofs") at the shapes the two-column statements of
tests/test_gpu_zk_proof.py do not reach: a next-row periodic variable beside two periods, W in {1, 4, 5, 63}, D' in {3, 9, 10},
t = 5 and t = 32, grinding and offsets of the caller's; every sentence of the verifier against the restatement
(tests/zk_compose.py) with dishonest restated provers; one flipped bit in every object of a proof; the kept exemption column
across offsets; and two more statements at the boundary moduli.  Every comparison is exact.  `pytest -m gpu`."""
import functools

import pytest

import fold4_compose as f4
import zk_compose as zk
from test_gpu_boundary_primes_deep_fold4 import GEN as BOUNDARY_GEN, THREE
from test_gpu_zk import engines  # noqa: F401  (a fixture: one context per modulus)
from test_gpu_zk_proof import KW, _objects, gpu_proof
from test_zk_emu import P_REF, SEED, statement

pytestmark = pytest.mark.gpu
GEN = dict(BOUNDARY_GEN)
GEN[P_REF] = 3
# (statement, W, log_n, log_blowup, t, trace_offset, lde_offset or None for g, grind_bits)
ROWS = [("wide", 5, 7, 2, 2, 1, None, 0),          # the next-row periodic shift, two periods, odd W, D' = 3
        ("wide", 4, 7, 2, 2, 1, None, 8),          # the documented width, the nonce record
        ("wide", 63, 6, 2, 1, 1, None, 0),         # leaf 64, the widest the tree takes
        ("wide", 5, 6, 2, 1, 5, 7, 8),             # offsets in the exemption column, the extension and the DEEP points
        ("quintic", 1, 6, 3, 1, 1, None, 0),       # D' = 9, leaf 41
        ("quintic", 1, 6, 3, 2, 1, None, 0),       # D' = 10, leaf 45
        ("cubic", 2, 8, 2, 5, 1, None, 0),         # t not a power of two, k_t = 48, k_s = 21
        ("cubic", 2, 10, 2, 32, 1, None, 8)]       # k_t = 264, k_s = 129, 32 records a section, D' = 5
NUMBERS = [(3, 3, 24, 9), (3, 3, 24, 9), (3, 3, 16, 5), (3, 3, 16, 5), (6, 9, 16, 5), (6, 10, 24, 9), (4, 5, 48, 21), (4, 5, 264, 129)]


@functools.lru_cache(maxsize=None)
def reference(oracle, name, W, log_n, lb, t, tau, h, bits, p=P_REF, commit_as=None, claim_t=None):
    """statement, restated proof: made once and shared.  claim_t: the statement laid out for that many tests (its claim on
    the last real row lies k_t(claim_t) + 1 rows from the end), proved with t"""
    air, cols = statement(name, log_n, t if claim_t is None else claim_t, p, W)
    g = GEN[p]
    return air, cols, zk.prove(oracle, air, cols, SEED, p, g, log_n, lb, t, tau, g if h is None else h, bits, commit_as=commit_as)


def both(eng, oracle, air, proof, roots, W, log_n, lb, t, tau=1, h=None, bits=0, p=P_REF, lib_bits="same"):
    """-> (the library's verdict and sentence, the restatement's)"""
    g = GEN[p]
    got = eng.air_verify(air, proof, roots, W, log_n, lb, t, trace_offset=tau, lde_offset=h, grind_bits=bits if lib_bits == "same" else lib_bits, zk=True, **KW)
    return got, zk.verify(oracle, air, proof, [bytes(r) for r in roots], p, g, W, log_n, lb, t, tau, g if h is None else h, bits or 0)


# ---------------------------------------------------------------------------------------------- proofs byte for byte
@pytest.mark.parametrize("row", range(len(ROWS)), ids=["%s-W%d-%d-%d-t%d-tau%d-h%s-b%d" % r for r in ROWS])
def test_proofs_equal_the_restatement_and_verify(engines, oracle, row):
    name, W, log_n, lb, t, tau, h, bits = ROWS[row]
    p = P_REF
    eng = engines[p]
    air, cols, want = reference(oracle, name, W, log_n, lb, t, tau, h, bits)
    assert eng.air_plan_deep_zk(air, W, log_n, lb, t, tau, h) == zk.plan(air, log_n, t) == NUMBERS[row] and want["Dp"] == NUMBERS[row][1]
    res, after = gpu_proof(eng, air, cols, log_n, lb, t, SEED, bits=bits, trace_offset=tau, lde_offset=h)
    assert [bytes(r) for r in res["column_roots"]] == want["roots"]
    assert [v for el in res["ood"] for v in el] == want["ood"]
    assert res["proof"] == want["proof"] and res["top_indices"] == [int(v) for v in want["top"]]
    assert after == want["trace"] and SEED not in res["proof"]
    assert len(res["proof"]) == eng.air_deep_zk_layout(air, W, log_n, lb, t, tau, h)[1] == zk.layout(W, want["Dp"], log_n, lb, t)[1]
    verify = lambda pr: eng.air_verify(air, pr, res["column_roots"], W, log_n, lb, t, trace_offset=tau, lde_offset=h, grind_bits=bits, zk=True, **KW)
    assert verify(res["proof"]) == (True, "")
    if t < 32:
        assert zk.verify(oracle, air, res["proof"], want["roots"], p, 3, W, log_n, lb, t, tau, 3 if h is None else h, bits) == (True, "")
        return
    # t = 32: the restated verifier takes a quarter of a minute, so the library's alone; the last record of each section
    off = zk.offsets(W, want["Dp"], log_n, lb, t)
    assert off["end"] == len(res["proof"]) and len(set(res["top_indices"])) > 16
    for k, V in enumerate((W + 1, 4 * want["Dp"] + 5)):
        m = bytearray(res["proof"])
        m[off[f"rec {k}"] + (t - 1) * (9 + 32 * V) + 9] ^= 1
        assert verify(bytes(m)) == (False, zk.WORDS["auth"]), k


def test_the_kept_exemption_column_follows_the_trace_offset(engines, oracle):
    """three proofs in one process at trace offsets 1, 5, 1: the library keeps the last exemption column it made, keyed on the
    offset among others, so the third proof must equal the first and the second the restatement at offset 5"""
    name, W, log_n, lb, t = "wide", 5, 6, 2, 1
    eng = engines[P_REF]
    out = []
    for tau in (1, 5, 1):
        air, cols, want = reference(oracle, name, W, log_n, lb, t, tau, None, 0)
        res, _after = gpu_proof(eng, air, cols, log_n, lb, t, SEED, trace_offset=tau)
        assert res["proof"] == want["proof"] and [bytes(r) for r in res["column_roots"]] == want["roots"], tau
        assert eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, trace_offset=tau, zk=True, **KW) == (True, "")
        out.append(res)
    assert out[0]["proof"] == out[2]["proof"] != out[1]["proof"]
    assert bytes(out[0]["column_roots"][0]) == bytes(out[2]["column_roots"][0]) != bytes(out[1]["column_roots"][0])
    # and the verifier's copy of the column: the offset-1 proof under offset 5 and back
    air, _cols, _want = reference(oracle, name, W, log_n, lb, t, 1, None, 0)
    got, restated = both(eng, oracle, air, out[0]["proof"], out[0]["column_roots"], W, log_n, lb, t, tau=5)
    assert got == restated == (False, zk.FRONT["consistency"])
    assert eng.air_verify(air, out[0]["proof"], out[0]["column_roots"], W, log_n, lb, t, zk=True, **KW) == (True, "")


# ---------------------------------------------------------------------------------------------- every sentence
CASE = ("wide", 5, 7, 2, 2)


def put(proof, at, new):
    m = bytearray(proof)
    m[at:at + len(new)] = new
    return bytes(m)


def u64_plus(proof, at, d):
    return put(proof, at, ((int.from_bytes(proof[at:at + 8], "little") + d) % (1 << 64)).to_bytes(8, "little"))


def test_dishonest_commitments_by_their_sentences(engines, oracle):
    name, W, log_n, lb, t = CASE
    p, eng = P_REF, engines[P_REF]
    Dp = 3
    cases = [(zk.swapped(0, 1), (False, zk.WORDS["quotient"])), (zk.swapped(1, 0), (False, zk.WORDS["quotient"])),
             (zk.plus_p(0, 1, p), (False, zk.WORDS["canonical"])), (zk.plus_p(1, 2, p), (False, zk.WORDS["canonical"])),
             (zk.plus_p(1, 4 * Dp + 3, p), (False, zk.WORDS["canonical"])),                                    # a coordinate of R
             (zk.plus_p(0, W, p), (True, "")), (zk.plus_p(1, 4 * Dp + 4, p), (True, ""))]                      # the two salts
    for k, (commit_as, verdict) in enumerate(cases):
        air, _cols, bad = reference(oracle, name, W, log_n, lb, t, 1, None, 0, commit_as=commit_as)
        assert bad["Dp"] == Dp
        got, restated = both(eng, oracle, air, bad["proof"], bad["roots"], W, log_n, lb, t)
        assert got == restated == verdict, k


def test_malformed_proofs_by_their_sentences(engines, oracle):
    name, W, log_n, lb, t = CASE
    p, eng = P_REF, engines[P_REF]
    air, _cols, want = reference(oracle, name, W, log_n, lb, t, 1, None, 0)
    proof, roots, Dp = want["proof"], want["roots"], want["Dp"]
    off = zk.offsets(W, Dp, log_n, lb, t)
    assert off["end"] == len(proof) == 5366
    cases = [("ood + p", u64_plus(proof, 9, p), zk.FRONT["record canonical"]), ("last ood + p", u64_plus(proof, off["fri"] - 8, p), zk.FRONT["record canonical"]),
             ("ood count", u64_plus(proof, 1, -1), zk.FRONT["record"]), ("ood tag", put(proof, 0, b"\x03"), zk.FRONT["record"]),
             ("cut", proof[:-1], zk.WORDS["length"]), ("extended", proof + b"\x00", zk.WORDS["length"]), ("empty", b"", zk.FRONT["record"])]
    for k, V in enumerate((W + 1, 4 * Dp + 5)):
        r, pa = off[f"rec {k}"] + 9 + 32 * V, off[f"path {k}"]           # the second record, the first path
        cases += [(f"record tag {k}", put(proof, r, b"\x03"), zk.WORDS["record"]), (f"record count {k}", u64_plus(proof, r + 1, 1), zk.WORDS["record"]),
                  (f"path tag {k}", put(proof, pa, b"\x02"), zk.WORDS["path"]), (f"path depth {k}", u64_plus(proof, pa + 1, -1), zk.WORDS["path"])]
    for what, bad, sentence in cases:
        got, restated = both(eng, oracle, air, bad, roots, W, log_n, lb, t)
        assert got == restated == (False, sentence), what


def test_a_wrong_number_of_tests_and_a_wrong_difficulty(engines, oracle):
    """the statement's claim on the last real row is legal for one t only (a boundary point on a randomiser row is refused, not
    judged), so the proof verified at t - 1 and t + 1 is of the statement laid out for t + 1, proved honestly at t"""
    import stark_rs_amd as s
    name, W, log_n, lb, t = CASE
    p, eng = P_REF, engines[P_REF]
    air, _cols, want = reference(oracle, name, W, log_n, lb, t, 1, None, 0, claim_t=t + 1)
    assert both(eng, oracle, air, want["proof"], want["roots"], W, log_n, lb, t) == ((True, ""), (True, ""))
    for other in (t - 1, t + 1):
        got, restated = both(eng, oracle, air, want["proof"], want["roots"], W, log_n, lb, other)
        assert got == restated == (False, zk.FRONT["consistency"]), other          # another exemption column, another k_s in z^(j L)
    tight, _cols, honest = reference(oracle, name, W, log_n, lb, t, 1, None, 0)
    with pytest.raises(s.StarkMiError, match="a randomiser row"):
        eng.air_verify(tight, honest["proof"], honest["roots"], W, log_n, lb, t + 1, zk=True, **KW)
    # a proof ground at 8 bits: the least difficulty above 8 that its nonce misses, 9 itself, and no demand at all
    air, _cols, ground = reference(oracle, name, W, log_n, lb, t, 1, None, 8)
    assert ground["proof"] != honest["proof"] and len(ground["proof"]) == len(honest["proof"])
    assert both(eng, oracle, air, ground["proof"], ground["roots"], W, log_n, lb, t, bits=8) == ((True, ""), (True, ""))
    miss = next(b for b in range(9, 33) if zk.verify(oracle, air, ground["proof"], ground["roots"], p, 3, W, log_n, lb, t, 1, 3, b) != (True, ""))
    got, restated = both(eng, oracle, air, ground["proof"], ground["roots"], W, log_n, lb, t, bits=miss)
    assert got == restated == (False, "proof of work"), miss
    got, restated = both(eng, oracle, air, ground["proof"], ground["roots"], W, log_n, lb, t, bits=9)
    assert got == restated == ((False, "proof of work") if miss == 9 else (True, ""))
    # include/stark_mi.h, "Grinding": a proof ground at b verifies at every b' <= b, and None counts as 0
    got, restated = both(eng, oracle, air, ground["proof"], ground["roots"], W, log_n, lb, t, bits=0, lib_bits=None)
    assert got == restated == (True, "")


def test_one_flipped_bit_in_every_object(engines, oracle):
    """the first and the last byte of the payload of every object of one proof: the out-of-domain record, each FRI root, the
    last codeword, the nonce, every record and every path.  No flip is skipped, and both verifiers name the same reason."""
    name, W, log_n, lb, t = CASE
    eng = engines[P_REF]
    air, _cols, want = reference(oracle, name, W, log_n, lb, t, 1, None, 0)
    proof, roots = want["proof"], want["roots"]
    objs, at, flips, said = _objects(proof), 0, 0, {}
    F = f4.layout(1 << (log_n + lb), 1 << lb, t)[1]
    assert [o[0] for o in objs[:F + 4]] == [2] + [0] * (F + 1) + [2, 2] and objs[-1][2] == len(proof)
    assert sum(1 for o in objs if o[0] == 3) >= 4 * t and len(objs) >= 1 + (F + 1) + 2 + 4 * t
    for tag, _payload, end in objs:
        first = at + (1 if tag == 0 else 9)
        assert first < end
        for where, bit in ((first, 0), (end - 1, 7)):
            m = bytearray(proof)
            m[where] ^= 1 << bit
            got, restated = both(eng, oracle, air, bytes(m), roots, W, log_n, lb, t)
            assert got == restated and not got[0] and got[1] in zk.SENTENCES, (at, where)
            said[got[1]] = said.get(got[1], 0) + 1
            flips += 1
        at = end
    assert flips == 2 * len(objs)
    print("sentences of the sweep:", said)
    assert zk.FRONT["consistency"] in said and zk.WORDS["auth"] in said


# ---------------------------------------------------------------------------------------------- boundary moduli
@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("name,W,log_n,lb,t", [("cubic", 2, 7, 2, 1), ("wide", 5, 6, 2, 1)])
def test_two_more_statements_at_boundary_moduli(engines, oracle, p, name, W, log_n, lb, t):
    """a periodic column and D' = 5; two periods, a next-row read, five columns and D' = 3"""
    g = GEN[p]
    two_adicity = ((p - 1) & -(p - 1)).bit_length() - 1
    if two_adicity < log_n + lb:
        assert (p - 1) % (1 << (log_n + lb)) != 0
        pytest.skip(f"p = {p}: p - 1 = 2^{two_adicity} * odd has no domain of 2^{log_n + lb} points")
    eng = engines[p]
    air, cols, want = reference(oracle, name, W, log_n, lb, t, 1, None, 0, p=p)
    res, after = gpu_proof(eng, air, cols, log_n, lb, t, SEED)
    assert [bytes(r) for r in res["column_roots"]] == want["roots"] and res["proof"] == want["proof"] and after == want["trace"]
    assert want["Dp"] == {"cubic": 5, "wide": 3}[name]
    got, restated = both(eng, oracle, air, res["proof"], res["column_roots"], W, log_n, lb, t, p=p)
    assert got == restated == (True, "")
