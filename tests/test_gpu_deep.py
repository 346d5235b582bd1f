"""GPU: out-of-domain sampling (include/stark_mi.h, "Out-of-domain sampling") -- smi_dev_poly_eval_ext, smi_dev_deep_compose,
smi_dev_air_prove_deep / smi_air_verify_deep -- against the restatement over the CPU oracle's primitives
(tests/deep_compose.py).  Every comparison is exact.  `pytest -m gpu`."""
import functools

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import air_rows as ar
import deep_compose as dc
import ext_compose as xc
from test_deep_emu import compose_inputs
from test_deep_host import quartic
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_ext import _dev_cols

pytestmark = pytest.mark.gpu
KW = dict(row_leaves=True, ext=True, deep=True)


# ---------------------------------------------------------------------------------------------- evaluation
@functools.lru_cache(maxsize=None)
def eval_reference(p, g, n_coeffs):
    """four base columns (one of them all p - 1), three points (random z, 5 z, all p - 1) and the values by halving: computed
    once per size and shared by the cases below, which scale the columns"""
    rng = np.random.default_rng(n_coeffs)
    base = rng.integers(0, p, (4, n_coeffs), dtype=np.uint64)
    base[1] = p - 1
    z = [int(v) for v in rng.integers(1, p, 4)]
    pts = [z, dc.scale_q(z, 5, p), [p - 1] * 4]
    return base, pts, [dc.eval_cols(base, pt, p, g) for pt in pts]


def check_eval(eng, p, g, n_coeffs, n_cols):
    """column c = base[c % 4] * (c // 4 + 1): the first four columns are the base columns themselves, so column 1 is all p - 1
    whenever n_cols > 1; a single all-(p - 1) column is sent on its own as well, at the all-(p - 1) point, once and twice.
    Three layouts: contiguous from an aligned base; a stride that is the next multiple of 4 from an aligned base (16-byte loads
    whose last one is cut by n_coeffs); a wider odd stride from an unaligned base (4-byte loads)."""
    import torch
    base, pts, vals = eval_reference(p, g, n_coeffs)
    cols = np.stack([base[c % 4] * np.uint64(c // 4 + 1) % np.uint64(p) for c in range(n_cols)])
    want = lambda ks: [[dc.scale_q(vals[k][c % 4], c // 4 + 1, p) for k in ks] for c in range(n_cols)]
    top = np.full((1, n_coeffs), p - 1, dtype=np.uint64)
    assert np.array_equal(top[0], base[1]) and (n_cols == 1 or np.array_equal(cols[1], top[0]))
    pad4 = (n_coeffs + 3) // 4 * 4
    for stride, lead in ((None, 0), (pad4 if pad4 != n_coeffs else n_coeffs + 4, 0), (n_coeffs + 5, 1)):
        t, d = _dev_cols(cols, stride, lead)
        tt, dt = _dev_cols(top, stride, lead)
        torch.cuda.synchronize()
        for ks in ([0], [0, 1], [2], [2, 2]):
            assert eng.dev_poly_eval_ext(d, n_cols, n_coeffs, [pts[k] for k in ks], stride) == want(ks), (stride, ks)
        for ks in ([2], [2, 2]):                                             # all-(p - 1) coefficients at the all-(p - 1) point
            assert eng.dev_poly_eval_ext(dt, 1, n_coeffs, [pts[k] for k in ks], stride) == [[vals[2][1] for _ in ks]], (stride, ks)
        del t, tt


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("n_cols", [1, 3, 64])
@pytest.mark.parametrize("n_coeffs", [1, 255, 256, 257, (1 << 16) + 1, 1 << 20])
def test_dev_poly_eval_ext_equals_horner(engines, p, g, n_coeffs, n_cols):
    check_eval(engines[p], p, g, n_coeffs, n_cols)
    if n_coeffs <= 257 and n_cols == 1:                                      # the halving against Horner itself, where Python ints reach
        base, pts, vals = eval_reference(p, g, n_coeffs)
        assert vals[0][0] == dc.horner([int(v) for v in base[0]], pts[0], p, g)


def test_dev_poly_eval_ext_refusals(engines):
    import stark_rs_amd as s
    p, g = xc.PRIMES[0]
    eng = engines[p]
    with Dev(eng) as dev:
        d = dev.upload(np.arange(8, dtype=np.uint64))
        for kwargs, word in ((dict(n_cols=1, n_coeffs=8, points=[[p, 0, 0, 0]]), "coordinate"), (dict(n_cols=1, n_coeffs=8, points=[[1, 2, 3, 4]], stride=7), "stride"),
                             (dict(n_cols=0, n_coeffs=8, points=[[1, 2, 3, 4]]), "columns"), (dict(n_cols=1, n_coeffs=0, points=[[1, 2, 3, 4]]), "coefficients")):
            with pytest.raises(s.StarkMiError, match=word):
                eng.dev_poly_eval_ext(d, **kwargs)
        with pytest.raises(ValueError):
            eng.dev_poly_eval_ext(d, 1, 8, [[1, 2, 3, 4]] * 3)
        assert eng.dev_poly_eval_ext(d, 2, 4, [[1, 2, 3, 4]]) == [[dc.horner([0, 1, 2, 3], [1, 2, 3, 4], p, g)], [dc.horner([4, 5, 6, 7], [1, 2, 3, 4], p, g)]]


# ---------------------------------------------------------------------------------------------- the DEEP codeword
def gpu_compose(eng, lde, seg, log_n, lb, z, ood, ch, h, stride=None, lead=0):
    import torch
    W, N = lde.shape
    D = seg.shape[0] // 4
    st = N if stride is None else stride
    tl, dl = _dev_cols(lde, stride, lead)
    ts, ds = _dev_cols(seg, stride, lead)
    out = torch.full((lead + 4 * st,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.dev_deep_compose(dl, ds, W, D, log_n, lb, z, ood, ch, out.data_ptr() + 4 * lead, stride=st, seg_stride=st, out_stride=st, lde_offset=h)
    eng.sync()
    host = out.cpu().numpy().view(np.uint32)
    assert np.all(host[:lead] == 0x5a5a5a5a)
    for e in range(4):                                                       # nothing written between the columns
        assert np.all(host[lead + e * st + N:lead + (e + 1) * st] == 0x5a5a5a5a)
    return np.stack([host[lead + e * st:lead + e * st + N] for e in range(4)]).astype(np.uint64)


def check_compose(eng, oracle, p, g, log_N, combos, h=None):
    """h: the offset of the evaluation domain (default g, what lde_offset=None means); under another h the restatement over
    the default points must differ, so that a kernel which ignored h could not pass"""
    N, h = 1 << log_N, g if h is None else h
    for k, (lb, W, D) in enumerate(combos):
        log_n = log_N - lb
        w, _wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
        x = dc.points(oracle, p, g, log_n, lb, h)
        for kind in ("random", "extreme"):
            lde, seg, z, ood, ch = compose_inputs(p, W, D, N, kind, seed=k)
            want = dc.q_codeword(lde, seg, x, z, ood, ch, w, p, g)
            if h != g:
                assert not np.array_equal(want, dc.q_codeword(lde, seg, dc.points(oracle, p, g, log_n, lb, g), z, ood, ch, w, p, g)), (lb, W, D, kind)
            got = gpu_compose(eng, lde, seg, log_n, lb, z, ood, ch, h)
            assert np.array_equal(got[:, :1 << lb], want[:, :1 << lb]), (lb, W, D, kind, h)   # the first B points: where an index i - B would wrap
            assert np.array_equal(got, want), (lb, W, D, kind, h)
        assert np.array_equal(gpu_compose(eng, lde, seg, log_n, lb, z, ood, ch, h, stride=N + 3, lead=1), want), (lb, W, D, h)   # the 4-byte path


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_N", range(10, 17))
def test_dev_deep_compose_equals_the_restatement(engines, oracle, p, g, log_N):
    check_compose(engines[p], oracle, p, g, log_N, dc.compose_combos(log_N))


def test_dev_deep_compose_refusals(engines):
    import stark_rs_amd as s
    p, g = xc.PRIMES[0]
    eng, log_n, lb, W, D = engines[p], 6, 2, 2, 1
    lde, seg, z, ood, ch = compose_inputs(p, W, D, 1 << (log_n + lb), "random")
    tl, dl = _dev_cols(lde)
    ts, ds = _dev_cols(seg)
    with Dev(eng) as dev:
        d_out = dev.alloc(16 << (log_n + lb))
        with pytest.raises(s.StarkMiError, match="base field"):
            eng.dev_deep_compose(dl, ds, W, D, log_n, lb, [z[0], 0, 0, 0], ood, ch, d_out)
        with pytest.raises(s.StarkMiError, match=">= p"):
            eng.dev_deep_compose(dl, ds, W, D, log_n, lb, z, [p] + ood[1:], ch, d_out)
        with pytest.raises(s.StarkMiError, match="stride"):
            eng.dev_deep_compose(dl, ds, W, D, log_n, lb, z, ood, ch, d_out, stride=(1 << (log_n + lb)) - 1)
        with pytest.raises(s.StarkMiError, match="segments"):
            eng.dev_deep_compose(dl, ds, W, 17, log_n, lb, z, ood + [0] * 64, ch + [0] * 64, d_out)


# ---------------------------------------------------------------------------------------------- the proof
def make_air(name, n, p):
    if name in ("fib", "mixer"):
        return ac.make(name, n, p)
    if name == "mimc":
        return ap.make("mimc", n, p)
    if name == "quartic":
        return quartic(n, p)
    assert name == "wide"
    return ar.wide(12, 3, p, n)


def gpu_proof(eng, air, cols, log_n, lb, t, bits=0, check=True, **kw):
    with Dev(eng) as dev:
        return eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, lb, t, grind_bits=bits, check=check, **KW, **kw)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", range(6, 11))
@pytest.mark.parametrize("name,lb", [("fib", 3), ("mixer", 3), ("mimc", 3), ("wide", 3), ("mimc", 2)])
def test_prove_bytes_equal_the_restatement_and_verify_accepts(engines, oracle, p, g, log_n, name, lb):
    import stark_rs_amd as s
    eng, t = engines[p], 4
    air, cols = make_air(name, 1 << log_n, p)
    W = len(cols)
    _d, D = dc.plan(air)
    assert eng.air_plan_deep(air, W, log_n, lb)[1] == D
    if lb == 2:                                                              # the statement the feature newly proves
        with pytest.raises(s.StarkMiError) as ei:
            with Dev(eng) as dev:
                eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=0)
        assert ei.value.status == -10
    bits = 4 if log_n == 8 else 0
    res = gpu_proof(eng, air, cols, log_n, lb, t, bits)
    want = dc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, bits)
    assert [bytes(r) for r in res["column_roots"]] == want["roots"] and res["column_roots"].shape == (2, 32)
    assert [c for el in res["ood"] for c in el] == want["ood"]
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    assert len(res["proof"]) == eng.air_plan_deep(air, W, log_n, lb, num_colinearity_tests=t)[2]
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **KW)
    assert ok, why
    assert dc.verify(oracle, air, res["proof"], want["roots"], p, g, W, log_n, lb, t, 1, g, bits) == (True, "")
    if bits:
        assert eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=0, **KW)[0]
        assert not eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=32, **KW)[0]


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_a_degree_5_air_in_four_segments(engines, oracle, p, g):
    eng, log_n, lb, t = engines[p], 8, 3, 6
    air, cols = quartic(1 << log_n, p)
    d, D, length = eng.air_plan_deep(air, 1, log_n, lb, num_colinearity_tests=t)
    assert (d, D) == (5, 4)
    res = gpu_proof(eng, air, cols, log_n, lb, t, timed=True)
    assert len(res["proof"]) == length == dc.proof_len(oracle, 1, 4, log_n, lb, t, p, g, g)
    assert list(res["stage_ms"]) == ["lde", "commit", "compose", "segments", "ood", "fri", "open"]
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], 1, log_n, lb, t, **KW)
    assert ok, why
    want = dc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g)
    assert res["proof"] == want["proof"]


def both_reject(eng, oracle, air, proof, roots, p, g, W, log_n, lb, t, reason, bits=0):
    """the library and the restatement reject, the restatement for the reason class `reason`, and the library's sentence
    holds that class's keyword -> the library's sentence"""
    ok, why = eng.air_verify(air, proof, roots, W, log_n, lb, t, grind_bits=bits, **KW)
    ok_o, why_o = dc.verify(oracle, air, proof, [bytes(r) for r in roots], p, g, W, log_n, lb, t, 1, g, bits)
    assert not ok and why and not ok_o, (why, why_o)
    assert why_o == reason, (why, why_o)
    assert dc.keyword(reason) in why, (why, why_o)
    return why


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name", ["mixer", "mimc"])
def test_verify_rejections(engines, oracle, p, g, name):
    import stark_rs_amd as s
    eng, log_n, lb, t = engines[p], 8, 3, 4
    n, log_N = 1 << log_n, log_n + lb
    air, cols = make_air(name, n, p)
    W = len(cols)
    _d, D = dc.plan(air)
    res = gpu_proof(eng, air, cols, log_n, lb, t)
    proof, roots = res["proof"], res["column_roots"]
    args = (p, g, W, log_n, lb, t)
    assert eng.air_verify(air, proof, roots, W, log_n, lb, t, **KW)[0]
    # one trace cell changed: the segments are no longer the composition
    bad_cols = [list(c) for c in cols]
    bad_cols[0][n // 3] = (bad_cols[0][n // 3] + 1) % p
    forged = gpu_proof(eng, air, bad_cols, log_n, lb, t, check=False)
    both_reject(eng, oracle, air, forged["proof"], forged["column_roots"], *args, reason="consistency")
    with pytest.raises(s.StarkMiError):
        gpu_proof(eng, air, bad_cols, log_n, lb, t)                          # check=True names the row instead
    # the sections: record | FRI | rows 1 | paths 1 | rows 2 | paths 2
    m, rec1, rec2, prec = 2 * t, 9 + 8 * W, 9 + 32 * D, 9 + 32 * log_N
    sec2 = len(proof) - m * (rec2 + prec)
    sec1 = sec2 - m * (rec1 + prec)

    def flipped(at):
        b = bytearray(proof)
        b[at] ^= 1
        return bytes(b)
    both_reject(eng, oracle, air, flipped(9 + 8 * 4 + 2), roots, *args, reason="consistency")          # the record: coordinate 0 of the second element
    both_reject(eng, oracle, air, flipped(sec1 + rec1 + 9), roots, *args, reason="auth")                # a trace row
    both_reject(eng, oracle, air, flipped(sec2 + 3 * rec2 + 9 + 8), roots, *args, reason="auth")        # a segment row
    both_reject(eng, oracle, air, flipped(sec1 + m * rec1 + 9 + 40), roots, *args, reason="auth")       # a path of tree 1
    both_reject(eng, oracle, air, flipped(len(proof) - 1), roots, *args, reason="auth")                 # a path of tree 2
    both_reject(eng, oracle, air, flipped(sec1), roots, *args, reason="row")
    both_reject(eng, oracle, air, flipped(sec2 + m * rec2), roots, *args, reason="path")
    both_reject(eng, oracle, air, flipped(1), roots, *args, reason="record")
    for at in (9, 9 + 8 * 7):                                                # a coordinate + p: not canonical
        b = bytearray(proof)
        b[at:at + 8] = xc._u64(int.from_bytes(proof[at:at + 8], "little") + p)
        both_reject(eng, oracle, air, bytes(b), roots, *args, reason="record canonical")
    b = bytearray(proof)                                                     # ... in an opened row: the leaf no longer hashes to the root
    b[sec1 + 9:sec1 + 17] = xc._u64(int.from_bytes(proof[sec1 + 9:sec1 + 17], "little") + p)
    both_reject(eng, oracle, air, bytes(b), roots, *args, reason="auth")
    for keep, reason in ((len(proof) - 1, "length"), (len(proof) - 40, "length"), (sec2, "length"), (sec1 + 7, "length"), (sec1, "length"),
                         (sec1 - 5, "fri: path"), (20, "record"), (5, "record"), (0, "record")):
        both_reject(eng, oracle, air, proof[:keep], roots, *args, reason=reason)
    both_reject(eng, oracle, air, proof + b"\x00", roots, *args, reason="length")
    both_reject(eng, oracle, air, proof, roots[::-1].copy(), *args, reason="consistency")   # swapped roots: other weights, another z
    # crossed over with the proof of smi_dev_air_prove_ext_pow
    with Dev(eng) as dev:
        pow_res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=0)
    both_reject(eng, oracle, air, pow_res["proof"], np.concatenate([pow_res["column_roots"], pow_res["column_roots"]]), *args, reason="record")
    for root in (roots[:1], roots[1:]):                                      # ... and the other way round: no root record leads the proof
        ok, why = eng.air_verify(air, proof, root, W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=0)
        assert not ok and dc.FRI_KEYWORD["root"] in why, why
    # another statement: one coefficient, one boundary value, one periodic value
    other = make_air(name, n, p)[0]
    cf, factors = other._symbolic[0][1]
    other._symbolic[0][1] = (cf + 1, factors)
    both_reject(eng, oracle, other, proof, roots, *args, reason="consistency")
    other = make_air(name, n, p)[0]
    c, r, v = other.boundaries[0]
    other.boundaries[0] = (c, r, (v + 1) % p)
    both_reject(eng, oracle, other, proof, roots, *args, reason="consistency")
    if name == "mimc":
        other = make_air(name, n, p)[0]
        other.periodics[0][5] = (other.periodics[0][5] + 1) % p
        both_reject(eng, oracle, other, proof, roots, *args, reason="consistency")
    both_reject(eng, oracle, air, proof, roots, *args, reason="fri: proof of work", bits=20)


def test_deep_does_not_combine(engines):
    p, g = xc.PRIMES[0]
    eng, log_n = engines[p], 6
    air, cols = ac.make("fib", 1 << log_n, p)
    with Dev(eng) as dev:
        d = dev.upload(np.array(cols, dtype=np.uint64))
        for kw in (dict(row_leaves=True, ext=True, deep=True, folding=4), dict(row_leaves=True, deep=True), dict(deep=True)):
            with pytest.raises(ValueError):
                eng.dev_air_prove(air, d, 2, log_n, 3, 4, **kw)
        for build in (lambda a: a.permutation([0], [1]), lambda a: a.lookup([0], [1], 1), lambda a: a.add_permutation([0], [1])):
            other = ac.make("fib", 1 << log_n, p)[0]
            build(other)
            with pytest.raises(ValueError, match="plain AIR"):
                eng.dev_air_prove(other, d, 2, log_n, 3, 4, **KW)
            with pytest.raises(ValueError, match="plain AIR"):
                eng.air_verify(other, b"", np.zeros((2, 32), dtype=np.uint8), 2, log_n, 3, 4, **KW)
        with pytest.raises(ValueError):
            eng.air_verify(air, b"", np.zeros((2, 32), dtype=np.uint8), 2, log_n, 3, 4, folding=4, **KW)
