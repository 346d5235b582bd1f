"""GPU: transition windows of up to four rows (include/stark_mi.h, "AIR: transition windows") through the C ABI -- the window
composition under base and extension weights, smi_dev_air_check, smi_dev_poly_eval_ext_shifts, smi_dev_deep_compose_window and
the DEEP proofs over row leaves and coset leaves with their verifiers -- against the restatement over the CPU oracle's
primitives (tests/window_compose.py).  Every comparison is exact.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import deep_compose as dc
import deep_fold4_compose as dfc
import ext_compose as xc
import window_compose as wc
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_boundary_primes import u64_set
from test_gpu_ext import _dev_cols, _dev_u64

pytestmark = pytest.mark.gpu
ROWS = dict(row_leaves=True, ext=True, deep=True)
COSETS = dict(row_leaves=True, ext=True, deep=True, coset_leaves=True)


# ---------------------------------------------------------------------------------------------- the composition
def gpu_window_compose(eng, air, lde, wts, log_n, lb, tau, h, ext, stride=None, lead=0):
    import torch
    N = 1 << (log_n + lb)
    st = N if stride is None else stride
    tl, dl = _dev_cols(np.asarray(lde, dtype=np.uint64), stride, lead)
    tw, dw = _dev_u64(wts)
    out = torch.full((4 * st if ext else st,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if ext:
        eng.dev_air_compose_ext(air, dl, len(lde), log_n, lb, dw, out.data_ptr(), stride=st, out_stride=st, trace_offset=tau, lde_offset=h)
    else:
        eng.dev_air_compose(air, dl, len(lde), log_n, lb, dw, out.data_ptr(), stride=st, trace_offset=tau, lde_offset=h)
    eng.sync()
    host = out.cpu().numpy().view(np.uint32)
    if not ext:
        assert np.all(host[N:] == 0x5a5a5a5a)
        return host[:N].astype(np.uint64)
    for e in range(4):
        assert np.all(host[e * st + N:(e + 1) * st] == 0x5a5a5a5a)
    return np.stack([host[e * st:e * st + N] for e in range(4)]).astype(np.uint64)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("lb", [2, 3, 4])
@pytest.mark.parametrize("S", [3, 4])
def test_window_compose_equals_the_restatement(engines, oracle, p, g, S, lb):
    """log_N from log2(S B) up to 12: the halo (S - 1) B is longer than, equal to and shorter than the tile, and wraps at N;
    (W, Q) rotates through {1, 5, 64} x {0, 2} -- the periodic columns of period 2 and n are read at shift S - 1; the tiled
    kernel, and the direct kernel forced by a base one word off 16 bytes and by a stride of N + 3; the first and the last
    (S - 1) B points on their own; column W - 1 holds p - 1 throughout"""
    eng, B, tau = engines[p], 1 << lb, 5
    for log_N in range((S * B - 1).bit_length(), 13):
        log_n = log_N - lb
        N, halo = 1 << log_N, (S - 1) * B
        combos = [(1, 0), (5, 2), (64, 0), (1, 2), (5, 0), (64, 2)]
        for W, Q in (combos if log_N == 8 else [combos[(log_N + lb + S) % 6]]):
            air, cols = wc.synthetic(W, Q, S, 1 if lb == 2 else 2, p, 1 << log_n)
            assert air.window == S and all(c == p - 1 for c in cols[W - 1])
            lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, g)
            for ext in (False, True):
                wts = xc.ext_weights_for(air) if ext else ac.weights_for(air)
                want = (wc.compose_ext if ext else wc.compose)(oracle, air, cols, wts, p, g, log_n, lb, tau, g)
                for stride, lead in ((None, 0), (None, 1), (N + 3, 0)):
                    got = gpu_window_compose(eng, air, lde, wts, log_n, lb, tau, g, ext, stride, lead)
                    where = (S, lb, log_N, W, Q, ext, stride, lead, wc.air_tile(W + Q, B, N, 4 if ext else 1, S))
                    assert np.array_equal(got[..., :halo], want[..., :halo]), where
                    assert np.array_equal(got[..., N - halo:], want[..., N - halo:]), where
                    assert np.array_equal(got, want), where


def test_window_compose_shapes_take_every_tile():
    """the shapes above give every tile size air_tile has, and no tile at all"""
    seen = set()
    for S in (3, 4):
        for lb in (2, 3, 4):
            for log_N in range(((S << lb) - 1).bit_length(), 13):
                combos = [(1, 0), (5, 2), (64, 0), (1, 2), (5, 0), (64, 2)]
                for W, Q in (combos if log_N == 8 else [combos[(log_N + lb + S) % 6]]):
                    for vecs in (1, 4):
                        seen.add(wc.air_tile(W + Q, 1 << lb, 1 << log_N, vecs, S))
    assert seen >= {64, 128, 256, 512, 1024}, seen


def test_dev_air_check_window(engines):
    """a trace that breaks only the window starting at row n - S is refused naming that row; the windows that would start at
    n - S + 1 .. n - 1 are violated by each of these traces and are not checked"""
    p, g = xc.PRIMES[0]
    eng, log_n = engines[p], 8
    n = 1 << log_n
    for name, col in (("fib1", 0), ("sq", 0), ("tap4", 0), ("wide", 2)):
        air, cols = wc.make(name, n, p)
        S = air.window
        assert wc.wrapped_violations(air, p, cols) == list(range(n - S + 1, n))
        bad = [list(c) for c in cols]
        bad[col][n - 1] = (bad[col][n - 1] + 1) % p
        with Dev(eng) as dev:
            assert eng.dev_air_check(air, dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n)[0]
            ok, con, row, why = eng.dev_air_check(air, dev.upload(np.array(bad, dtype=np.uint64)), len(cols), log_n)
        assert not ok and row == n - S and (con, row) == air.first_violation(p, bad), (name, why)
        assert f"rows {n - S} .. {n - 1}" in why


# ---------------------------------------------------------------------------------------------- evaluation at z w^s
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("n_cols", [1, 3, 64])
def test_dev_poly_eval_ext_shifts_equals_horner(engines, oracle, p, g, n_cols):
    import torch
    eng = engines[p]
    w = oracle.ff_prim_nth_root_g(1 << 10, p, g)
    for n_coeffs in (1, 255, 256, 257, 1024, 1025, (1 << 16) + 1):
        rng = np.random.default_rng(n_coeffs + n_cols)
        cols = rng.integers(0, p, (n_cols, n_coeffs), dtype=np.uint64)
        cols[n_cols // 2] = p - 1
        z = [int(v) for v in rng.integers(1, p, 4)]
        pts = wc.shifts_of(z, w, 4, p)
        vals = [dc.eval_cols(cols, pt, p, g) for pt in pts]
        if n_coeffs <= 257:
            assert vals[3][0] == dc.horner([int(v) for v in cols[0]], pts[3], p, g)
        for stride, lead in ((None, 0), (n_coeffs + 5, 1)):              # 16-byte loads; an unaligned base: 4-byte loads
            t, d = _dev_cols(cols, stride, lead)
            torch.cuda.synchronize()
            for S in (1, 2, 3, 4):
                got = eng.dev_poly_eval_ext_shifts(d, n_cols, n_coeffs, z, w, S, stride)
                assert got == [[vals[s][c] for s in range(S)] for c in range(n_cols)], (n_coeffs, stride, S)
                if S <= 2:
                    assert got == eng.dev_poly_eval_ext(d, n_cols, n_coeffs, pts[:S], stride)
            del t


def test_dev_poly_eval_ext_keeps_its_two_points_and_shifts_its_limits(engines):
    import stark_rs_amd as s
    p, g = xc.PRIMES[0]
    eng = engines[p]
    with Dev(eng) as dev:
        d = dev.upload(np.arange(8, dtype=np.uint64))
        pts = (C.c_uint64 * 12)(*([1, 2, 3, 4] * 3))
        out = (C.c_uint64 * 12)()
        assert eng.L.smi_dev_poly_eval_ext(eng.h, C.c_void_p(d), 1, 8, 8, pts, 3, out) == -50   # a third point stays refused
        assert "one or two points" in eng.L.smi_last_error(eng.h).decode()
        for kwargs, word in ((dict(n_shifts=0), "shifts"), (dict(n_shifts=5), "shifts"), (dict(w=p), ">= p"), (dict(z=[p, 0, 0, 0]), "coordinate"),
                             (dict(stride=7), "stride")):
            kw = dict(z=[1, 2, 3, 4], w=3, n_shifts=2)
            kw.update(kwargs)
            with pytest.raises(s.StarkMiError, match=word):
                eng.dev_poly_eval_ext_shifts(d, 1, 8, kw["z"], kw["w"], kw["n_shifts"], kw.get("stride"))


# ---------------------------------------------------------------------------------------------- the DEEP codeword
def codeword_inputs(p, W, D, S, N, extreme, seed=3):
    rng = np.random.default_rng(seed + W + D + S)
    hi, cnt = p - 1, 4 * (S * W + D)
    lde = np.full((W, N), hi, dtype=np.uint64) if extreme else rng.integers(0, p, (W, N), dtype=np.uint64)
    seg = np.full((4 * D, N), hi, dtype=np.uint64) if extreme else rng.integers(0, p, (4 * D, N), dtype=np.uint64)
    z = [hi] * 4 if extreme else [int(v) for v in rng.integers(1, p, 4)]
    ood = [hi] * cnt if extreme else [int(v) for v in rng.integers(0, p, cnt)]
    u = u64_set(p)
    ch = [u[(3 * i + seed) % len(u)] for i in range(cnt)] if extreme else [int(v) for v in rng.integers(1 << 62, (1 << 64) - 1, cnt, dtype=np.uint64)]
    return lde, seg, z, ood, ch


def gpu_codeword(eng, S, lde, seg, log_n, lb, z, ood, ch, h, stride=None, lead=0, old=False):
    import torch
    W, N = lde.shape
    D = seg.shape[0] // 4
    st = N if stride is None else stride
    tl, dl = _dev_cols(lde, stride, lead)
    ts, ds = _dev_cols(seg, stride, lead)
    out = torch.full((lead + 4 * st,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if old:
        eng.dev_deep_compose(dl, ds, W, D, log_n, lb, z, ood, ch, out.data_ptr() + 4 * lead, stride=st, seg_stride=st, out_stride=st, lde_offset=h)
    else:
        eng.dev_deep_compose_window(S, dl, ds, W, D, log_n, lb, z, ood, ch, out.data_ptr() + 4 * lead, stride=st, seg_stride=st, out_stride=st,
                                    lde_offset=h)
    eng.sync()
    host = out.cpu().numpy().view(np.uint32)
    assert np.all(host[:lead] == 0x5a5a5a5a)
    for e in range(4):
        assert np.all(host[lead + e * st + N:lead + (e + 1) * st] == 0x5a5a5a5a)
    return np.stack([host[lead + e * st:lead + e * st + N] for e in range(4)]).astype(np.uint64)


def check_codeword(eng, oracle, p, g, log_N, h=None):
    """smi_dev_deep_compose_window at S in {3, 4} (random and extreme inputs, both load paths) and at S = 2 (against
    smi_dev_deep_compose and dc.q_codeword).  h: the offset of the evaluation domain (default g, what lde_offset=None means);
    under another h the restatement over the default points must differ, so that a kernel which ignored h could not pass"""
    N, h = 1 << log_N, g if h is None else h
    for lb, W, D in dc.compose_combos(log_N):
        log_n = log_N - lb
        w, _wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
        x = dc.points(oracle, p, g, log_n, lb, h)
        x_default = dc.points(oracle, p, g, log_n, lb, g)
        for S in (3, 4):
            for extreme in (False, True):
                lde, seg, z, ood, ch = codeword_inputs(p, W, D, S, N, extreme)
                want = wc.q_codeword(lde, seg, x, z, ood, ch, w, S, p, g)
                if h != g:
                    assert not np.array_equal(want, wc.q_codeword(lde, seg, x_default, z, ood, ch, w, S, p, g)), (lb, W, D, S, extreme)
                assert np.array_equal(gpu_codeword(eng, S, lde, seg, log_n, lb, z, ood, ch, h), want), (lb, W, D, S, extreme, h)
            assert np.array_equal(gpu_codeword(eng, S, lde, seg, log_n, lb, z, ood, ch, h, stride=N + 3, lead=1), want), (lb, W, D, S, h)   # 4-byte path
        lde, seg, z, ood, ch = codeword_inputs(p, W, D, 2, N, False)
        two = gpu_codeword(eng, 2, lde, seg, log_n, lb, z, ood, ch, h)
        assert np.array_equal(two, gpu_codeword(eng, 2, lde, seg, log_n, lb, z, ood, ch, h, old=True))
        assert np.array_equal(two, dc.q_codeword(lde, seg, x, z, ood, ch, w, p, g))
        if h != g:
            assert not np.array_equal(two, dc.q_codeword(lde, seg, x_default, z, ood, ch, w, p, g)), (lb, W, D)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_N", range(6, 13))
def test_dev_deep_compose_window_equals_the_restatement(engines, oracle, p, g, log_N):
    check_codeword(engines[p], oracle, p, g, log_N)


def test_dev_deep_compose_window_refusals(engines):
    import stark_rs_amd as s
    p, g = xc.PRIMES[0]
    eng, log_n, lb, W, D = engines[p], 6, 2, 2, 1
    lde, seg, z, ood, ch = codeword_inputs(p, W, D, 3, 1 << (log_n + lb), False)
    tl, dl = _dev_cols(lde)
    ts, ds = _dev_cols(seg)
    with Dev(eng) as dev:
        d_out = dev.alloc(16 << (log_n + lb))
        for S in (1, 5):
            with pytest.raises(s.StarkMiError, match="window"):
                eng.dev_deep_compose_window(S, dl, ds, W, D, log_n, lb, z, [0] * (4 * (S * W + D)), [0] * (4 * (S * W + D)), d_out)
        with pytest.raises(s.StarkMiError, match="base field"):
            eng.dev_deep_compose_window(3, dl, ds, W, D, log_n, lb, [z[0], 0, 0, 0], ood, ch, d_out)
        with pytest.raises(s.StarkMiError, match=">= p"):
            eng.dev_deep_compose_window(3, dl, ds, W, D, log_n, lb, z, ood[:-1] + [p], ch, d_out)   # the last value of the longer record is read


# ---------------------------------------------------------------------------------------------- the proofs
def gpu_proof(eng, air, cols, log_n, lb, t, kw, bits=0, check=True, **more):
    with Dev(eng) as dev:
        return eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, lb, t, grind_bits=bits, check=check, **kw, **more)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("cosets", [False, True])
@pytest.mark.parametrize("lb", [2, 3])
@pytest.mark.parametrize("log_n", range(6, 11))
@pytest.mark.parametrize("name", ["fib1", "sq", "tap4", "wide"])
def test_prove_bytes_equal_the_restatement_and_verify_accepts(engines, oracle, p, g, name, log_n, lb, cosets):
    eng, t, kw = engines[p], 4, COSETS if cosets else ROWS
    air, cols = wc.make(name, 1 << log_n, p)
    W, S = len(cols), air.window
    d, D = wc.plan(air, log_n)
    assert (S, d, D) == {"fib1": (3, 1, 1), "sq": (3, 2, 2), "tap4": (4, 3, 4), "wide": (4, 2, 2)}[name]
    assert eng.air_plan_deep(air, W, log_n, lb) == (d, D)
    assert not cosets or dfc.folds(log_n, lb, t) >= 1
    bits = 4 if log_n == 8 else 0
    res = gpu_proof(eng, air, cols, log_n, lb, t, kw, bits)
    want = wc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, bits, cosets)
    assert [bytes(r) for r in res["column_roots"]] == want["roots"] and res["column_roots"].shape == (2, 32)
    assert [c for el in res["ood"] for c in el] == want["ood"] and len(res["ood"]) == S * W + D
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    if cosets:
        flat = air.flatten(p)
        cfg = eng._stark_cfg(W, log_n, lb, t, 1, None, True)
        folds, length = C.c_uint64(), C.c_size_t()
        assert eng.L.smi_air_deep_fold4_layout(p, C.byref(cfg), C.byref(flat), C.byref(folds), C.byref(length)) == 0
        assert (folds.value, length.value) == wc.fold4_layout(W, D, S, log_n, lb, t) and length.value == len(res["proof"])
    else:
        assert len(res["proof"]) == eng.air_plan_deep(air, W, log_n, lb, num_colinearity_tests=t)[2] == wc.proof_len(oracle, W, D, S, log_n, lb, t, p, g, g)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **kw)
    assert ok, why
    assert wc.verify(oracle, air, res["proof"], want["roots"], p, g, W, log_n, lb, t, 1, g, bits, cosets) == (True, "")


@pytest.mark.parametrize("cosets", [False, True])
def test_window_field_two_gives_todays_bytes(engines, oracle, cosets):
    """an smi_air with window = 2 written out is the statement of window = 0, byte for byte"""
    p, g = xc.PRIMES[0]
    eng, log_n, lb, t, kw = engines[p], 7, 3, 4, COSETS if cosets else ROWS
    air, cols = ac.make("mixer", 1 << log_n, p)
    flat0, flat2 = air.flatten(p), air.flatten(p)
    assert flat0.window == 0
    flat2.window = 2
    a, b = gpu_proof(eng, flat0, cols, log_n, lb, t, kw, check=False), gpu_proof(eng, flat2, cols, log_n, lb, t, kw, check=False)
    assert a["proof"] == b["proof"] and np.array_equal(a["column_roots"], b["column_roots"])
    want = dfc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g) if cosets else dc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g)
    assert a["proof"] == want["proof"]
    assert eng.air_verify(flat2, a["proof"], a["column_roots"], len(cols), log_n, lb, t, **kw)[0]


def expected(reason, cosets):
    """what wc.verify returns for a reason class: the class itself over row leaves, the sentence over coset leaves"""
    if not cosets:
        return reason
    return dfc.FRONT[reason] if reason in ("consistency", "record") else dfc.WORDS[reason]


def both_reject(eng, oracle, air, proof, roots, p, g, W, log_n, lb, t, cosets, reason=None):
    """the library and the restatement reject for the same class of sentence (`reason`, where the case fixes it)"""
    kw = COSETS if cosets else ROWS
    ok, why = eng.air_verify(air, proof, roots, W, log_n, lb, t, grind_bits=0, **kw)
    ok_o, why_o = wc.verify(oracle, air, proof, [bytes(r) for r in roots], p, g, W, log_n, lb, t, 1, g, 0, cosets)
    assert not ok and why and not ok_o, (why, why_o)
    assert wc.sentence_matches(why_o, why, cosets), (why, why_o)
    if reason is not None:
        assert why_o == expected(reason, cosets), (why, why_o)
    return why


@pytest.mark.parametrize("cosets", [False, True])
@pytest.mark.parametrize("name", ["sq", "tap4", "wide"])
def test_verify_rejections(engines, oracle, name, cosets):
    import stark_rs_amd as s
    p, g = xc.PRIMES[0]
    eng, log_n, lb, t, kw = engines[p], 7, 3, 4, COSETS if cosets else ROWS
    n = 1 << log_n
    air, cols = wc.make(name, n, p)
    W, S = len(cols), air.window
    _d, D = wc.plan(air, log_n)
    res = gpu_proof(eng, air, cols, log_n, lb, t, kw)
    proof, roots = res["proof"], res["column_roots"]
    args = (p, g, W, log_n, lb, t, cosets)
    assert eng.air_verify(air, proof, roots, W, log_n, lb, t, **kw)[0]
    # a flipped value u_{2,0} in the record
    b = bytearray(proof)
    b[9 + 8 * 4 * (2 * W)] ^= 1
    both_reject(eng, oracle, air, bytes(b), roots, *args, reason="consistency")
    # a record of 2 W + D values under this window
    short = xc._elems([int.from_bytes(proof[9 + 8 * i:17 + 8 * i], "little") for i in range(4 * (2 * W + D))])
    both_reject(eng, oracle, air, short + proof[9 + 32 * (S * W + D):], roots, *args, reason="record")
    # the same proof under the statement written with copy columns
    if name in ("sq", "tap4"):
        air2, cols2 = wc.two_row_form(name, n, p)
        assert air2.window == 2 and air2.first_violation(p, cols2) is None
        W2 = len(cols2)
        ok, why = eng.air_verify(air2, proof, roots, W2, log_n, lb, t, grind_bits=0, **kw)
        ok_o, why_o = wc.verify(oracle, air2, proof, [bytes(r) for r in roots], p, g, W2, log_n, lb, t, 1, g, 0, cosets)
        assert not ok and not ok_o and wc.sentence_matches(why_o, why, cosets), (why, why_o)
        same_count = S * W + D == 2 * W2 + wc.plan(air2, log_n)[1]
        assert why_o == expected("consistency" if same_count else "record", cosets)
    # one operand moved from shift 2 to shift 1 (the window stays: another operand keeps the top shift)
    other = wc.make(name, n, p)[0]
    for ci, con in enumerate(other._symbolic):
        hit = [(ti, fi) for ti, (_cf, fs) in enumerate(con) for fi, (kind, _i, _e) in enumerate(fs) if kind == ("row", 2)]
        if hit:
            ti, fi = hit[0]
            kind, i, e = con[ti][1][fi]
            con[ti][1][fi] = (("row", 1), i, e)
            break
    if other.window == S:
        both_reject(eng, oracle, other, proof, roots, *args, reason="consistency")
    else:
        both_reject(eng, oracle, other, proof, roots, *args, reason="record")
    # a trace that breaks the window at row n - S only, proven without the check
    bad = [list(c) for c in cols]
    col = 2 if name == "wide" else 0
    bad[col][n - 1] = (bad[col][n - 1] + 1) % p
    assert air.first_violation(p, bad)[1] == n - S
    forged = gpu_proof(eng, air, bad, log_n, lb, t, kw, check=False)
    both_reject(eng, oracle, air, forged["proof"], forged["column_roots"], *args, reason="consistency")
    with pytest.raises(s.StarkMiError, match=f"rows {n - S}"):
        gpu_proof(eng, air, bad, log_n, lb, t, kw)
    # a flipped opened value of tree 1
    tail = wc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, 0, cosets)["tail_at"]
    b = bytearray(proof)
    b[tail + 9] ^= 1
    both_reject(eng, oracle, air, bytes(b), roots, *args, reason="auth")


def test_every_other_variant_refuses_a_window(engines):
    """the Engine raises before the library is called; the library's own refusals are in tests/test_air_window_host.py"""
    p, g = xc.PRIMES[0]
    eng, log_n = engines[p], 6
    air, cols = wc.make("fib1", 1 << log_n, p)
    with Dev(eng) as dev:
        d = dev.upload(np.array(cols, dtype=np.uint64))
        for kw in (dict(), dict(row_leaves=True), dict(row_leaves=True, ext=True), dict(row_leaves=True, ext=True, grind_bits=0),
                   dict(row_leaves=True, ext=True, folding=4), dict(row_leaves=True, ext=True, deep=True, coset_leaves=True, zk=True)):
            with pytest.raises(ValueError, match="window"):
                eng.dev_air_prove(air, d, 1, log_n, 3, 4, **kw)
            kw = {k: (bool(v) if k == "zk" else v) for k, v in kw.items()}
            with pytest.raises(ValueError, match="window"):
                eng.air_verify(air, b"", np.zeros((2, 32), dtype=np.uint8), 1, log_n, 3, 4, **kw)


def test_the_library_refuses_a_window_in_every_other_variant(engines, monkeypatch):
    """past the Engine's own check: every prover and verifier outside the plain DEEP variants returns SMI_ERR_BAD_ARG with a
    sentence naming the window"""
    import stark_rs_amd as s
    from stark_rs_amd.mirror import Air
    p, g = xc.PRIMES[0]
    eng, log_n, W = engines[p], 6, 3
    monkeypatch.setattr(type(eng), "_check_window", lambda *a, **k: None)
    rng = np.random.default_rng(1)
    cols = rng.integers(0, p, (W, 1 << log_n), dtype=np.uint64)

    def windowed(build):
        air = Air(W).transition({("row", 2, 0): 1, ("row", 1, 0): -1, ("row", 0, 0): -1})
        if build:
            build(air)
        return air
    ext = dict(row_leaves=True, ext=True)
    variants = [(None, dict(), W), (None, dict(row_leaves=True), 1), (None, ext, 1), (None, dict(ext, grind_bits=0), 1), (None, dict(ext, folding=4), 1),
                (lambda a: a.permutation([0], [1]), ext, 2), (lambda a: a.lookup([0], [1], 2), ext, 2), (lambda a: a.add_permutation([0], [1]), ext, 2),
                (lambda a: a.add_permutation([0], [1], left_sel=2), ext, 2), (lambda a: a.add_permutation([0], [1]), dict(ext, deep_args=True), 3),
                (lambda a: a.add_permutation([0], [1]), dict(ext, deep_args=True, coset_leaves=True), 3), (None, dict(COSETS, zk=True), 2),
                (lambda a: a.add_permutation([0], [1]), dict(ext, deep_args=True, coset_leaves=True, zk=True), 3)]
    with Dev(eng) as dev:
        d = dev.upload(cols)
        for i, (build, kw, n_roots) in enumerate(variants):
            air = windowed(build)
            with pytest.raises(s.StarkMiError, match="window") as ei:
                eng.dev_air_prove(air, d, W, log_n, 3, 4, check=False, **kw)
            assert ei.value.status == -50, i
            with pytest.raises(s.StarkMiError, match="window") as ei:
                eng.air_verify(air, b"\x02" + bytes(40), np.zeros((n_roots, 32), dtype=np.uint8), W, log_n, 3, 4, **kw)
            assert ei.value.status == -50, i
