"""GPU: zero-knowledge DEEP proofs with an argument list (include/stark_mi.h, "Zero-knowledge DEEP proofs with an argument
list") -- smi_dev_air_prove_deep_zk_xargs and smi_air_verify_deep_zk_xargs through the engine against the restatement
(tests/zk_args_compose.py): proofs byte for byte for a fixed seed, the column build plus the tail step above one workgroup,
every rejection with the restatement's sentence, the cross-variant rejections, the hiding shape, the smallest shape at the
boundary moduli, and the stage timer.  `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_fold4_compose as d4
import ext_compose as xc
import xargs_compose as xa
import zk_args_compose as za
import zk_compose as zk
from test_gpu_air import Dev
from test_gpu_boundary_primes_deep_fold4 import GEN as BOUNDARY_GEN, THREE
from test_gpu_deep_args import mirror
from test_gpu_zk import engines  # noqa: F401  (a fixture: one context per modulus)
from test_lookup_emu import chall

pytestmark = pytest.mark.gpu
P_REF = xc.PRIMES[0][0]
KW = dict(row_leaves=True, ext=True, deep_args=True, coset_leaves=True)
GEN = dict(BOUNDARY_GEN)
GEN[P_REF] = 3
SEED, SEED2 = bytes(range(32)), bytes(range(1, 33))
LISTS = {"vm": za.vm, "selectors": za.selectors}
# (list, log_n, log_blowup, t): (6, 2, 1) is the smallest shape with k_t = 24 < n / 2, and a lookup's degree 4 sits at D = B = 4
SHAPES = [("vm", 6, 2, 1, False), ("vm", 7, 3, 2, True), ("selectors", 7, 2, 1, False)]


def gpu_proof(eng, air, args, cols, log_n, lb, t, seed, bits=0, check=True, fill=False, timed=False):
    """-> (result, the device trace after the call)"""
    cols = [list(c) for c in cols]
    if fill:                                                  # the device fills the multiplicity columns over the active rows
        for g_ in args:
            if g_[0] == "lookup":
                cols[g_[3]] = [0] * len(cols[0])
    with Dev(eng) as dev:
        d = dev.upload(np.array(cols, dtype=np.uint64))
        res = eng.dev_air_prove(mirror(air, args), d, len(cols), log_n, lb, t, grind_bits=bits, check=check, zk=seed, fill_multiplicities=fill, timed=timed,
                                **KW)
        after = eng.dev_download(d, len(cols) << log_n).reshape(len(cols), -1)
    return res, [[int(v) for v in c] for c in after]


@functools.lru_cache(maxsize=None)
def reference(oracle, name, log_n, lb, t, p, seed, **kw):
    """statement, restated proof: made once and shared"""
    air, cols, args = LISTS[name](log_n, t, p)
    return air, cols, args, za.prove(oracle, air, args, cols, seed, p, GEN[p], log_n, lb, t, 1, GEN[p], **kw)


def both(eng, oracle, air, args, proof, roots, p, W, log_n, lb, t):
    g = GEN[p]
    return (eng.air_verify(mirror(air, args), proof, roots, W, log_n, lb, t, zk=True, **KW),
            za.verify(oracle, air, args, proof, [bytes(r) for r in roots], p, g, W, log_n, lb, t, 1, g))


@pytest.mark.parametrize("name,log_n,lb,t,fill", SHAPES)
def test_proofs_equal_the_restatement_and_verify(engines, oracle, name, log_n, lb, t, fill):
    p = P_REF
    eng = engines[p]
    air, cols, args, want = reference(oracle, name, log_n, lb, t, p, SEED)
    W, A = len(cols), len(args)
    res, after = gpu_proof(eng, air, args, cols, log_n, lb, t, SEED, fill=fill)
    assert [bytes(r) for r in res["column_roots"]] == want["roots"] and len(want["roots"]) == 3
    assert [v for el in res["ood"] for v in el] == want["ood"]
    assert res["proof"] == want["proof"] and res["top_indices"] == [int(v) for v in want["top"]]
    assert after == want["trace"] and res["seed"] == SEED and SEED not in res["proof"]
    assert res["closes"] == want["closes"] == [True] * A
    assert len(res["proof"]) == eng.air_deep_zk_args_layout(mirror(air, args), W, log_n, lb, t)[1] == za.layout(W, A, want["Dp"], log_n, lb, t)[1]
    assert eng.air_plan_deep_zk_args(mirror(air, args), W, log_n, lb, t) == za.plan(air, args, log_n, t)
    assert both(eng, oracle, air, args, res["proof"], res["column_roots"], p, W, log_n, lb, t) == ((True, ""), (True, ""))


def test_columns_and_tail_above_one_workgroup(engines, oracle):
    """log_n = 11 > PERM_TILE: the scan crosses workgroups and c_a[n_a] sits in the second block.  smi_dev_xargs_columns over the
    randomised trace, then smi_dev_random_fill of stream 6 and smi_dev_zk_args_tail, at an aligned base and one word off"""
    p, g, log_n, t = P_REF, 3, 11, 32
    eng = engines[p]
    n, kt = 1 << log_n, za.k_t(t)
    air, cols, args = xa.scene(n, p, (n, 8, n), seed=log_n + 3, A=3)
    W, A = len(cols), 3
    trace = za.randomised(cols, zk.rng(oracle, SEED, zk.STREAM_ROWS, W * kt, p), t)
    ch = chall(7)
    tail = zk.rng(oracle, SEED, za.STREAM_TAIL, 4 * A * (kt - 1), p)
    want, closes, closing, zero = za.columns(xa.widen(trace, air, p), args, ch, p, g, W, t, tail)
    assert zero is None and n - kt > 1024 and (n - kt + 1) % 4 == 1
    for lead in (0, 1):
        with Dev(eng) as dev:
            d_trace = dev.upload(np.array(trace, dtype=np.uint64))
            d_c = dev.alloc(4 * (4 * A * n + 4)) + 4 * lead
            d_rnd = dev.alloc(4 * 4 * A * (kt - 1))
            eng.dev_args_columns(mirror(air, args), d_trace, W, log_n, ch, d_c)
            eng.dev_random_fill(SEED, za.STREAM_TAIL, d_rnd, 4 * A * (kt - 1))
            got_closing = eng.dev_zk_args_tail(d_c, log_n, kt, A, d_rnd)
            got = eng.dev_download(d_c, 4 * A * n).reshape(4 * A, n)
        assert np.array_equal(got, want), lead
        assert got_closing == closing and [cl == ([1, 0, 0, 0] if arg[0] == "perm" else [0] * 4) for cl, arg in zip(closing, args)] == closes


@pytest.mark.parametrize("name,log_n,lb,t", [("vm", 6, 2, 1), ("selectors", 7, 3, 1)])
def test_dev_air_compose_zk_args_equals_the_restatement(engines, oracle, name, log_n, lb, t):
    """smi_dev_air_compose_zk_xargs alone: the derived AIR's composition plus the 3 A auxiliary quotients over the extension of a
    randomised trace and the restated columns, at strides N from aligned bases (16-byte accesses), at three different odd strides
    and at bases one word off (4-byte accesses); the words between and behind the output columns stay as they were"""
    import air_compose as ac
    import deep_compose as dc
    from test_gpu_ext import _dev_cols
    p, g, tau = P_REF, 3, 1
    eng, h = engines[p], 3
    n, N, kt = 1 << log_n, 1 << (log_n + lb), za.k_t(t)
    air, cols, args = LISTS[name](log_n, t, p)
    W, K, A = len(cols), len(air.constraints), len(args)
    dair = za.derived_air(air, log_n, t, p, tau, oracle.ff_prim_nth_root_g(n, p, g))
    trace = za.randomised(cols, zk.rng(oracle, SEED, zk.STREAM_ROWS, W * kt, p), t)
    wide = xa.widen(trace, dair, p)
    ch = chall(13)
    wch = [int(x) for x in np.random.default_rng(3).integers(1 << 62, (1 << 64) - 1, 4 * (W + K + 3 * A), dtype=np.uint64)]
    c, closes, _closing, zero = za.columns(wide, args, ch, p, g, W, t, zk.rng(oracle, SEED, za.STREAM_TAIL, 4 * A * (kt - 1), p))
    assert zero is None and all(closes)
    lde_wide = np.asarray(ac.lde(oracle, wide, p, g, log_n, lb, tau, h), dtype=np.uint64)
    cl = np.asarray(ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h), dtype=np.uint64)
    want = dc.composition(oracle, dair, trace, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
    want = (want + za.aux_terms(oracle, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W, t, len(wide) - 1)) % np.uint64(p)
    for stride, c_stride, out_stride, lead in ((N, N, N, 0), (N + 1, N + 3, N + 5, 0), (N, N, N, 1), (N + 4, N + 8, N + 4, 0)):
        with Dev(eng) as dev:
            _lt, d_lde = _dev_cols(lde_wide[:W].astype(np.uint32), stride, lead)
            _zt, d_cl = _dev_cols(cl.astype(np.uint32), c_stride, lead)
            ot, d_out = _dev_cols(np.zeros((4, N), dtype=np.uint32), out_stride, lead)
            d_w = dev.upload_u64(wch)
            eng.dev_air_compose_zk_args(mirror(air, args), d_lde, d_cl, W, log_n, lb, t, ch, d_w, d_out, stride=stride, c_stride=c_stride,
                                        out_stride=out_stride)
            eng.sync()
            host = ot.cpu().numpy().view(np.uint32)
        assert np.all(host[:lead] == 0x7fffffff)
        host = host[lead:]
        for e in range(4):
            assert np.all(host[e * out_stride + N:(e + 1) * out_stride] == 0x7fffffff)
        got = np.stack([host[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)
        assert np.array_equal(got, want), (stride, c_stride, out_stride, lead)
    import stark_rs_amd as s
    with Dev(eng) as dev, pytest.raises(s.StarkMiError, match="stride < N"):
        d = dev.alloc(64)
        eng.dev_air_compose_zk_args(mirror(air, args), d, d, W, log_n, lb, t, ch, d, d, c_stride=N - 1)


def test_the_row_bound_of_the_multiplicity_helper(engines):
    p, log_n, t = P_REF, 7, 1
    eng = engines[p]
    n, na = 1 << log_n, (1 << log_n) - za.k_t(t)
    air, cols, args = za.vm(log_n, t, p)
    import stark_rs_amd as s
    missed = [list(c) for c in cols]
    missed[4][na + 1] = 4 * n + 9                             # a tail lookup row that misses; a value only a tail table row holds
    missed[5][na + 2] = 4 * n + 5

    def mult(trace, rows):
        with Dev(eng) as dev:
            d = dev.upload(np.array(trace, dtype=np.uint64))
            d_m = dev.upload(np.full(n, 77, dtype=np.uint64))
            if rows is None:
                eng.dev_args_multiplicities(mirror(air, args), 1, d, 9, log_n, d_m)
            else:
                eng.dev_xargs_multiplicities_rows(mirror(air, args), 1, d, 9, log_n, rows, d_m)
            return [int(v) for v in eng.dev_download(d_m, n)]
    assert mult(cols, n) == mult(cols, None)
    assert mult(missed, na) == cols[6] and not any(cols[6][na:])
    with pytest.raises(s.StarkMiError, match=f"row {na + 1}"):
        mult(missed, None)
    missed[4][3] = 4 * n + 5
    with pytest.raises(s.StarkMiError, match="row 3 "):
        mult(missed, na)


def test_rejections_by_their_sentences(engines, oracle):
    p, name, log_n, lb, t = P_REF, "vm", 6, 2, 1
    eng = engines[p]
    air, cols, args, want = reference(oracle, name, log_n, lb, t, p, SEED)
    W, A, Dp = 9, 3, want["Dp"]
    proof, roots = want["proof"], want["roots"]
    off = za.offsets(W, A, Dp, log_n, lb, t)
    assert off["end"] == len(proof)
    said = lambda pr, rt: both(eng, oracle, air, args, pr, rt, p, W, log_n, lb, t)

    def flipped(at):
        m = bytearray(proof)
        m[at] ^= 1
        return bytes(m)
    cases = {"a salt byte of tree 2": (flipped(off["rec 1"] + 9 + 8 * 4 * 4 * A), za.WORDS["auth"]),
             "an auxiliary value": (flipped(off["rec 1"] + 9 + 8 * 5), za.WORDS["auth"]),
             "a_0": (flipped(off["a0"]), za.FRONT["consistency"]), "a_last": (flipped(off["a0"] + 32 * (A - 1) + 8), za.FRONT["consistency"]),
             "b_0": (flipped(off["b0"]), za.FRONT["consistency"]), "b_last": (flipped(off["b0"] + 32 * (A - 1) + 16), za.FRONT["consistency"]),
             "a salt byte of tree 1": (flipped(off["rec 0"] + 9 + 8 * 4 * W), za.WORDS["auth"]),
             "a salt byte of tree 3": (flipped(off["rec 2"] + 9 + 8 * 4 * (4 * Dp + 4)), za.WORDS["auth"])}
    for what, (bad, sentence) in cases.items():
        got, restated = said(bad, roots)
        assert got == restated == (False, sentence), what
    for kw in (dict(omit_cq=True), dict(no_ea=True)):         # a prover that closes over the wrap; one that composes without E_A
        lazy = reference(oracle, name, log_n, lb, t, p, SEED, **kw)[3]
        got, restated = said(lazy["proof"], lazy["roots"])
        assert got == restated == (False, za.FRONT["consistency"]), kw
    # a lookup miss on the last active row (check=False: the prover does not look): the bit is clear, the verifier refuses
    na = (1 << log_n) - za.k_t(t)
    inside = [list(c) for c in cols]
    inside[4][na - 1] = p - 1
    res, _ = gpu_proof(eng, air, args, inside, log_n, lb, t, SEED, check=False)
    assert res["closes"] == [True, False, True]
    got, restated = said(res["proof"], res["column_roots"])
    assert got == restated == (False, za.FRONT["consistency"])
    import stark_rs_amd as s
    with pytest.raises(s.StarkMiError, match="do not close"):
        gpu_proof(eng, air, args, inside, log_n, lb, t, SEED)
    # a miss on row n_a of the caller's trace is outside the statement: the same proof as without it
    outside = [list(c) for c in cols]
    outside[4][na] = p - 2
    res, _ = gpu_proof(eng, air, args, outside, log_n, lb, t, SEED)
    assert res["proof"] == proof and said(res["proof"], res["column_roots"]) == ((True, ""), (True, ""))


def test_the_variants_refuse_each_others_proofs(engines, oracle):
    p, g, log_n, lb, t = P_REF, 3, 6, 2, 1
    eng = engines[p]
    air, cols, args, want = reference(oracle, "vm", log_n, lb, t, p, SEED)
    m = mirror(air, args)
    with Dev(eng) as dev:                                     # the non-zk coset-leaf list proof of the same trace
        plain = eng.dev_air_prove(m, dev.upload(np.array(want["trace"], dtype=np.uint64)), 9, log_n, lb, t, grind_bits=0, check=False, **KW)
    got, restated = both(eng, oracle, air, args, plain["proof"], plain["column_roots"], p, 9, log_n, lb, t)
    assert got == restated == (False, za.FRONT["record"])
    assert eng.air_verify(m, want["proof"], want["roots"], 9, log_n, lb, t, **KW) == (False, d4.FRONT["record"])
    # the plain zk proof of the list's AIR without the list
    KZ = dict(row_leaves=True, ext=True, deep=True, coset_leaves=True)
    with Dev(eng) as dev:
        zkp = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), 9, log_n, lb, t, grind_bits=0, zk=SEED, **KZ)
    got, restated = both(eng, oracle, air, args, zkp["proof"], list(zkp["column_roots"]) + [bytes(32)], p, 9, log_n, lb, t)
    assert got == restated == (False, za.FRONT["record"])
    assert eng.air_verify(air, want["proof"], want["roots"][:2], 9, log_n, lb, t, zk=True, **KZ) == (False, zk.FRONT["record"])


def test_hiding_shape(engines, oracle):
    """two witnesses of one statement: equal lengths and record structure; two seeds: different roots of all three trees and
    different opened auxiliary values; the same seed: the same bytes"""
    import ext_compose as xc_
    p, log_n, lb, t = P_REF, 7, 2, 2
    eng = engines[p]
    wit = [za.vm(log_n, t, p, seed=s_) for s_ in (7, 8)]
    air, args = wit[0][0], wit[0][2]
    res = [gpu_proof(eng, air, args, w[1], log_n, lb, t, True)[0] for w in wit]
    Dp = za.plan(air, args, log_n, t)[1]
    assert res[0]["seed"] != res[1]["seed"] and len(res[0]["proof"]) == len(res[1]["proof"]) == za.layout(9, 3, Dp, log_n, lb, t)[1]
    assert all(eng.air_verify(mirror(air, args), r["proof"], r["column_roots"], 9, log_n, lb, t, zk=True, **KW) == (True, "") for r in res)

    def tags(pr):
        out, at = [], 0
        while at < len(pr):
            obj = xc_._pop(pr, at)
            assert obj is not None
            out.append((obj[0], len(obj[1])))
            at = obj[2]
        return out
    assert tags(res[0]["proof"]) == tags(res[1]["proof"])
    a, _ = gpu_proof(eng, air, args, wit[0][1], log_n, lb, t, SEED)
    b, _ = gpu_proof(eng, air, args, wit[0][1], log_n, lb, t, SEED2)
    again, _ = gpu_proof(eng, air, args, wit[0][1], log_n, lb, t, SEED)
    assert a["proof"] == again["proof"] and SEED not in a["proof"]
    assert all(bytes(a["column_roots"][k]) != bytes(b["column_roots"][k]) for k in range(3))
    off = za.offsets(9, 3, Dp, log_n, lb, t)
    opened = lambda r: r["proof"][off["rec 1"] + 9:off["rec 1"] + 9 + 8 * 4 * 12]
    assert opened(a) != opened(b) and a["ood"][18:24] != b["ood"][18:24]


@pytest.mark.parametrize("p", THREE)
def test_the_smallest_shape_at_boundary_moduli(engines, oracle, p):
    eng, name, log_n, lb, t = engines[p], "vm", 6, 2, 1
    air, cols, args, want = reference(oracle, name, log_n, lb, t, p, SEED)
    res, after = gpu_proof(eng, air, args, cols, log_n, lb, t, SEED)
    assert res["proof"] == want["proof"] and [bytes(r) for r in res["column_roots"]] == want["roots"] and after == want["trace"]
    assert both(eng, oracle, air, args, res["proof"], res["column_roots"], p, 9, log_n, lb, t) == ((True, ""), (True, ""))
    m = bytearray(res["proof"])
    m[za.offsets(9, 3, want["Dp"], log_n, lb, t)["b0"]] ^= 1
    assert both(eng, oracle, air, args, bytes(m), res["column_roots"], p, 9, log_n, lb, t) == ((False, za.FRONT["consistency"]),) * 2


def test_stage_ms_gets_exactly_ten_values(engines):
    """the library handle with a stage_ms array of eleven doubles, all NaN beforehand: ten finite values >= 0, the eleventh
    untouched, and the bytes of the same call with stage_ms null under the same seed"""
    from stark_rs_amd import _lib, engine
    p, log_n, lb, t = P_REF, 6, 2, 1
    eng = engines[p]
    air, cols, args = za.vm(log_n, t, p)
    a = mirror(air, args).flatten(p)
    xargs = engine.xargs_of(a)
    cfg = _lib.StarkCfg(log_n, lb, 9, 1, 1, 3, t, 1)

    def call(stage):
        roots, ood, top = np.zeros((3, 32), dtype=np.uint8), np.zeros(4096, dtype=np.uint64), np.zeros(t, dtype=np.uint64)
        proof, plen, closes = C.c_void_p(), C.c_size_t(), C.c_uint32()
        with Dev(eng) as dev:
            d = dev.upload(np.array(cols, dtype=np.uint64))
            status = eng.L.smi_dev_air_prove_deep_zk_xargs(eng.h, C.byref(cfg), C.byref(a), C.byref(xargs), C.c_void_p(d), SEED, roots.ctypes.data,
                                                           ood.ctypes.data, C.byref(proof), C.byref(plen), top.ctypes.data, stage, 0, C.byref(closes))
            assert status == 0, (status, eng.L.smi_last_error(eng.h))
            out = C.string_at(proof, plen.value)
            eng.L.smi_free(proof)
        assert closes.value == 7
        return out
    stage = (C.c_double * 11)(*[float("nan")] * 11)
    timed = call(stage)
    got = [float(v) for v in stage]
    print("deep_zk_xargs", got)
    assert all(np.isfinite(v) and v >= 0 for v in got[:10]), got
    assert np.isnan(got[10]), got
    assert len(timed) > 9 and timed == call(None)
    res, _ = gpu_proof(eng, air, args, cols, log_n, lb, t, SEED, timed=True)
    assert list(res["stage_ms"]) == ["random", "lde", "commit", "args", "compose", "segments", "ood", "mask", "fri", "open"]


def test_the_engine_routes_by_the_list(engines):
    """zk with deep_args=True, coset_leaves=True needs a list; the plan's refusals come through with their sentences"""
    import stark_rs_amd as s
    from stark_rs_amd.mirror import Air
    eng = engines[P_REF]
    with pytest.raises(ValueError, match="zk"):
        eng.dev_air_prove(Air(2), 0, 2, 6, 2, 1, zk=SEED, **KW)
    with pytest.raises(ValueError, match="zk"):
        eng.air_verify(Air(2), b"", [bytes(32)] * 3, 2, 6, 2, 1, zk=True, **KW)
    air, cols, args = za.vm(6, 1, P_REF)
    with pytest.raises(s.StarkMiError, match="zk deep argument: k_t = 8 t \\+ 16 = 32 >= n / 2"):
        eng.dev_air_prove(mirror(air, args), 0, 9, 6, 2, 2, zk=SEED, check=False, **KW)
