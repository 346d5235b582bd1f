"""GPU: zero-knowledge DEEP proofs (include/stark_mi.h, "Zero-knowledge DEEP proofs") -- smi_dev_air_prove_deep_zk and
smi_air_verify_deep_zk through the engine against the restatement (tests/zk_compose.py): proofs byte for byte for a fixed
seed, every rejection with the restatement's sentence, the cross-variant rejections, the hiding shape, and the smallest shape
at the boundary moduli of tests/test_gpu_boundary_primes_deep_fold4.py.  `pytest -m gpu`."""
import functools

import numpy as np
import pytest

import deep_fold4_compose as d4
import zk_compose as zk
from test_gpu_air import Dev
from test_gpu_boundary_primes_deep_fold4 import GEN as BOUNDARY_GEN, THREE
from test_gpu_zk import engines  # noqa: F401  (a fixture: one context per modulus)
from test_zk_emu import P_REF, SEED, STATEMENTS

pytestmark = pytest.mark.gpu
KW = dict(row_leaves=True, ext=True, deep=True, coset_leaves=True)
GEN = dict(BOUNDARY_GEN)
GEN[P_REF] = 3
SEED2 = bytes(range(1, 33))
# (statement, log_n, log_blowup, t): k_t in {16, 24}, k_s in {5, 9}; the cubic's derived AIR needs B >= 4
SHAPES = [("fib", 6, 2, 1), ("fib", 7, 3, 2), ("cubic", 7, 2, 1), ("cubic", 8, 3, 2), ("fib", 8, 2, 2)]


def gpu_proof(eng, air, cols, log_n, lb, t, seed, bits=0, check=True, trace_offset=1, lde_offset=None):
    """-> (result, the device trace after the call)"""
    with Dev(eng) as dev:
        d = dev.upload(np.array(cols, dtype=np.uint64))
        res = eng.dev_air_prove(air, d, len(cols), log_n, lb, t, trace_offset=trace_offset, lde_offset=lde_offset, grind_bits=bits, check=check, zk=seed,
                                **KW)
        after = eng.dev_download(d, len(cols) << log_n).reshape(len(cols), -1)
    return res, [[int(v) for v in c] for c in after]


@functools.lru_cache(maxsize=None)
def reference(oracle, name, log_n, lb, t, p, seed):
    """statement, restated proof: made once and shared"""
    air, cols = STATEMENTS[name](log_n, t, p)
    return air, cols, zk.prove(oracle, air, cols, seed, p, GEN[p], log_n, lb, t, 1, GEN[p])


@pytest.mark.parametrize("name,log_n,lb,t", SHAPES)
def test_proofs_equal_the_restatement_and_verify(engines, oracle, name, log_n, lb, t):
    p = P_REF
    eng = engines[p]
    air, cols, want = reference(oracle, name, log_n, lb, t, p, SEED)
    res, after = gpu_proof(eng, air, cols, log_n, lb, t, SEED)
    assert [bytes(r) for r in res["column_roots"]] == want["roots"]
    assert [v for el in res["ood"] for v in el] == want["ood"]
    assert res["proof"] == want["proof"] and res["top_indices"] == [int(v) for v in want["top"]]
    assert after == want["trace"] and res["seed"] == SEED and SEED not in res["proof"]
    assert len(res["proof"]) == eng.air_deep_zk_layout(air, 2, log_n, lb, t)[1] == zk.layout(2, want["Dp"], log_n, lb, t)[1]
    assert eng.air_verify(air, res["proof"], res["column_roots"], 2, log_n, lb, t, zk=True, **KW) == (True, "")
    assert zk.verify(oracle, air, res["proof"], want["roots"], p, 3, 2, log_n, lb, t, 1, 3) == (True, "")


def test_rejections_by_their_sentences(engines, oracle):
    p, g, name, log_n, lb, t = P_REF, 3, "cubic", 7, 2, 1
    eng = engines[p]
    air, cols, want = reference(oracle, name, log_n, lb, t, p, SEED)
    proof, roots, Dp = want["proof"], want["roots"], want["Dp"]
    off = zk.offsets(2, Dp, log_n, lb, t)
    assert off["end"] == len(proof)
    both = lambda a, pr, rt: (eng.air_verify(a, pr, rt, 2, log_n, lb, t, zk=True, **KW), zk.verify(oracle, a, pr, rt, p, g, 2, log_n, lb, t, 1, g))

    def flipped(at):
        m = bytearray(proof)
        m[at] ^= 1
        return bytes(m)
    cases = {"a salt byte of tree 1": (flipped(off["rec 0"] + 9 + 8 * 4 * 2), zk.WORDS["auth"]),
             "a salt byte of tree 2": (flipped(off["rec 1"] + 9 + 8 * 4 * (4 * Dp + 4)), zk.WORDS["auth"]),
             "a value of R": (flipped(off["rec 1"] + 9 + 8 * 4 * 4 * Dp), zk.WORDS["auth"]),
             "a segment value": (flipped(off["rec 1"] + 9), zk.WORDS["auth"]),
             "s_0": (flipped(off["s0"]), zk.FRONT["consistency"]),
             "s_last": (flipped(off["s0"] + 32 * (Dp - 1) + 8), zk.FRONT["consistency"])}
    for what, (bad, sentence) in cases.items():
        got, restated = both(air, bad, roots)
        assert got == restated == (False, sentence), what
    # a prover that composes the caller's AIR, not the derived one, over the trace as it stands
    lazy = zk.prove(oracle, air, cols, SEED, p, g, log_n, lb, t, 1, g, compose_with=air)
    got, restated = both(air, lazy["proof"], lazy["roots"])
    assert got == restated and not got[0] and got[1] == zk.FRONT["consistency"]
    # the statement violated on the last real row (check=False: the prover does not look)
    n, kt = 1 << log_n, zk.k_t(t)
    broken = [list(c) for c in cols]
    broken[0][n - kt - 1] = (broken[0][n - kt - 1] + 1) % p
    res, _ = gpu_proof(eng, air, broken, log_n, lb, t, SEED, check=False)
    got, restated = both(air, res["proof"], res["column_roots"])
    assert got == restated and not got[0] and got[1].startswith("zk deep")
    import stark_rs_amd as s
    with pytest.raises(s.StarkMiError):
        gpu_proof(eng, air, broken, log_n, lb, t, SEED)
    # the two variants refuse each other's proofs
    with Dev(eng) as dev:
        plain = eng.dev_air_prove(zk.derived_air(air, log_n, t, p, 1, oracle.ff_prim_nth_root_g(n, p, g)), dev.upload(np.array(want["trace"], dtype=np.uint64)),
                                  2, log_n, lb, t, grind_bits=0, **KW)
    got, restated = both(air, plain["proof"], plain["column_roots"])
    assert got == restated == (False, zk.FRONT["record"])
    assert eng.air_verify(air, proof, roots, 2, log_n, lb, t, **KW) == (False, d4.FRONT["record"])


def test_the_engine_refuses_zk_elsewhere(engines):
    eng = engines[P_REF]
    air, cols = STATEMENTS["fib"](6, 1, P_REF)
    for kw in (dict(row_leaves=True, ext=True, deep=True), dict(row_leaves=True, ext=True), dict(row_leaves=True, ext=True, deep_args=True, coset_leaves=True)):
        with pytest.raises(ValueError, match="zk"):
            eng.dev_air_prove(air, 0, 2, 6, 2, 1, zk=SEED, **kw)
        with pytest.raises(ValueError, match="zk"):
            eng.air_verify(air, b"", [bytes(32)] * 2, 2, 6, 2, 1, zk=True, **kw)
    with pytest.raises(ValueError, match="32 bytes"):
        eng.dev_air_prove(air, 0, 2, 6, 2, 1, zk=b"short", **KW)


def test_hiding_shape(engines, oracle):
    """two witnesses of one statement: proofs of one length and one record structure; for a fixed seed the opened trace values
    are the interpolant of (real rows | generator rows) at the opened points"""
    p, g, log_n, lb, t = P_REF, 3, 7, 2, 2
    eng = engines[p]
    n, N, kt = 1 << log_n, 1 << (log_n + lb), zk.k_t(t)
    from stark_rs_amd.mirror import Air
    air = Air(2)                                             # a' = a + b with b free: many witnesses; the claim is on a alone
    air.transition({("next", 0): 1, ("cur", 0): -1, ("cur", 1): -1})
    air.boundary(0, 0, 1).boundary(0, 1, 1)
    wit = []
    for k in (0, 1):
        b = [0] + [(7 * r * r + k * r * (r - 1)) % p for r in range(1, n)]           # b[0] = 0 in both: a[1] = 1
        a = [1]
        for r in range(n - 1):
            a.append((a[-1] + b[r]) % p)
        wit.append([a, b])
    res = [gpu_proof(eng, air, w, log_n, lb, t, True)[0] for w in wit]
    assert res[0]["seed"] != res[1]["seed"] and len(res[0]["proof"]) == len(res[1]["proof"]) == eng.air_deep_zk_layout(air, 2, log_n, lb, t)[1]
    assert all(eng.air_verify(air, r["proof"], r["column_roots"], 2, log_n, lb, t, zk=True, **KW) == (True, "") for r in res)
    tags = lambda pr: [(o_[0], len(o_[1])) for o_ in _objects(pr)]
    assert tags(res[0]["proof"]) == tags(res[1]["proof"])
    got, after = gpu_proof(eng, air, wit[0], log_n, lb, t, SEED)
    rows = zk.rng(oracle, SEED, zk.STREAM_ROWS, 2 * kt, p)
    assert [c[n - kt:] for c in after] == [rows[:kt], rows[kt:]] and [c[:n - kt] for c in after] == [c[:n - kt] for c in wit[0]]
    w, wN = oracle.ff_prim_nth_root_g(n, p, g), oracle.ff_prim_nth_root_g(N, p, g)
    polys = [[int(v) for v in oracle.fast_intt(np.array(c, dtype=np.uint64), w, 1, p)] for c in after]
    off = zk.offsets(2, zk.plan(air, log_n, t)[1], log_n, lb, t)
    for s, top in enumerate(got["top_indices"]):
        rec = [int.from_bytes(got["proof"][off["rec 0"] + s * (9 + 32 * 3) + 9 + 8 * i:][:8], "little") for i in range(12)]
        for c in range(2):
            for j in range(4):
                x = g * pow(wN, top % (N // 4) + j * (N // 4), p) % p
                assert rec[4 * c + j] == sum(cf * pow(x, i, p) for i, cf in enumerate(polys[c])) % p


def _objects(proof):
    import ext_compose as xc
    out, at = [], 0
    while at < len(proof):
        obj = xc._pop(proof, at)
        assert obj is not None
        out.append(obj)
        at = obj[2]
    return out


@pytest.mark.parametrize("p", THREE)
def test_the_smallest_shape_at_boundary_moduli(engines, oracle, p):
    eng, g, name, log_n, lb, t = engines[p], GEN[p], "fib", 6, 2, 1
    air, cols, want = reference(oracle, name, log_n, lb, t, p, SEED)
    a, after_a = gpu_proof(eng, air, cols, log_n, lb, t, SEED)
    b, after_b = gpu_proof(eng, air, cols, log_n, lb, t, SEED2)
    again, _ = gpu_proof(eng, air, cols, log_n, lb, t, SEED)
    assert a["proof"] == want["proof"] == again["proof"] and [bytes(r) for r in a["column_roots"]] == want["roots"]
    assert bytes(a["column_roots"][0]) != bytes(b["column_roots"][0]) and bytes(a["column_roots"][1]) != bytes(b["column_roots"][1])
    off = zk.offsets(2, want["Dp"], log_n, lb, t)
    opened = lambda r: r["proof"][off["rec 0"] + 9:off["rec 0"] + 9 + 64]
    assert opened(a) != opened(b) and after_a != after_b
    for r in (a, b):
        assert eng.air_verify(air, r["proof"], r["column_roots"], 2, log_n, lb, t, zk=True, **KW) == (True, "")
        assert zk.verify(oracle, air, r["proof"], [bytes(x) for x in r["column_roots"]], p, g, 2, log_n, lb, t, 1, g) == (True, "")
