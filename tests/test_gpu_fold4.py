"""GPU: smi_dev_fri_fold4_ext, the fold by 4 over the quartic extension in one launch -- against the two launches of
smi_dev_fri_fold_ext it replaces (alpha, then alpha^2 on the squared domain) and against the Lagrange restatement
(tests/fold4_compose.py).  Every comparison is exact.  `pytest -m gpu`."""
import numpy as np
import pytest

import ext_compose as xc
import fold4_compose as f4
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_ext import _dev_cols, _dev_u64

pytestmark = pytest.mark.gpu
U64_MAX = (1 << 64) - 1
FILL = 0x7fffffff


def gpu_fold4(eng, cw, alpha, offset, omega, stride=None, out_stride=None, lead=0, out_lead=0):
    import torch
    L = cw.shape[1]
    q = L // 4
    out_stride = q if out_stride is None else out_stride
    t_in, d_in = _dev_cols(cw, stride, lead)
    t_al, d_al = _dev_u64(alpha)
    t_out = torch.full((out_lead + 4 * out_stride,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.dev_fri_fold4_ext(d_in, L, L if stride is None else stride, d_al, offset, omega, t_out.data_ptr() + 4 * out_lead, out_stride)
    eng.sync()
    host = t_out.cpu().numpy().view(np.uint32)
    assert np.all(host[:out_lead] == FILL)
    out = host[out_lead:]
    for e in range(4):   # nothing written between the columns
        assert np.all(out[e * out_stride + q:(e + 1) * out_stride] == FILL)
    return np.stack([out[e * out_stride:e * out_stride + q] for e in range(4)]).astype(np.uint64)


def gpu_two_folds(eng, t_in, L, alpha, offset, omega, p, g):
    """the yardstick on the device: smi_dev_fri_fold_ext under alpha over (offset, omega, L), then under alpha^2 (reduced)
    over (offset^2, omega^2, L / 2); t_in: a torch int32 tensor of 4 L words -> a torch tensor of 4 (L / 4) words"""
    import torch
    t_a1, d_a1 = _dev_u64(alpha)
    t_a2, d_a2 = _dev_u64(f4.alpha_squared(alpha, p, g))
    t_mid = torch.empty(4 * (L // 2), dtype=torch.int32, device="cuda")
    t_out = torch.empty(4 * (L // 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.dev_fri_fold_ext(t_in.data_ptr(), L, L, d_a1, offset, omega, t_mid.data_ptr(), L // 2)
    eng.dev_fri_fold_ext(t_mid.data_ptr(), L // 2, L // 2, d_a2, offset * offset % p, omega * omega % p, t_out.data_ptr(), L // 4)
    eng.sync()
    return t_out


def _codeword(p, L, seed):
    rng = np.random.default_rng(seed)
    cw = rng.integers(0, p, (4, L), dtype=np.uint64)
    cw[:, 0] = p - 1
    cw[:, L // 4] = [0, p - 1, 0, p - 1]
    cw[:, L - 1] = p - 1
    return cw


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_fold4_equals_two_launches_of_the_existing_kernel_at_every_length(engines, oracle, p, g):
    eng = engines[p]
    for log_len in range(2, 14):
        L = 1 << log_len
        omega, offset = oracle.ff_prim_nth_root_g(L, p, g), [g, 7, 1][log_len % 3]
        for cw in (_codeword(p, L, log_len), np.full((4, L), p - 1, dtype=np.uint64)):
            for al in ([U64_MAX] * 4, [p, p + 1, U64_MAX - 1, 2 * p - 1], [1 << 63, 12345, p - 1, 1 << 32]):
                t_in, _ = _dev_cols(cw)
                want = gpu_two_folds(eng, t_in, L, al, offset, omega, p, g).cpu().numpy().view(np.uint32).reshape(4, L // 4)
                assert np.array_equal(gpu_fold4(eng, cw, al, offset, omega), want), (log_len, al)


def test_fold4_on_the_second_trip_of_the_grid_stride_loop(engines, oracle):
    """The launcher caps the grid at 2048 workgroups of 256 lanes, four outputs a lane: 2^21 outputs a trip.  len = 2^24 has
    q = 2^22 outputs, so every lane makes a second trip.  The yardstick at this length is the existing kernel alone."""
    import torch
    p, g = xc.PRIMES[1]
    eng, L = engines[p], 1 << 24
    gen = torch.Generator(device="cuda").manual_seed(24)
    t_in = torch.randint(0, p, (4 * L,), dtype=torch.int32, device="cuda", generator=gen)
    t_in[L - 4:L] = p - 1
    omega, al = oracle.ff_prim_nth_root_g(L, p, g), [U64_MAX, p + 1, 12345, U64_MAX - p]
    want = gpu_two_folds(eng, t_in, L, al, g, omega, p, g)
    t_al, d_al = _dev_u64(al)
    t_out = torch.full((4 * (L // 4),), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.dev_fri_fold4_ext(t_in.data_ptr(), L, L, d_al, g, omega, t_out.data_ptr(), L // 4)
    eng.sync()
    assert torch.equal(t_out, want)
    assert bool((want != FILL).any())


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_fold4_equals_the_lagrange_restatement(engines, oracle, p, g):
    eng = engines[p]
    for log_len in range(2, 11):
        L = 1 << log_len
        omega, offset = oracle.ff_prim_nth_root_g(L, p, g), [g, 7, 1][log_len % 3]
        cw = _codeword(p, L, 100 + log_len)
        for al in ([U64_MAX] * 4, [[p, p + 1, U64_MAX - 1, 2 * p - 1], [0, 0, 0, 1], [5, 0, 0, 0]][log_len % 3]):
            assert np.array_equal(gpu_fold4(eng, cw, al, offset, omega), f4.fold4(cw, al, offset, omega, p, g)), (log_len, al)


@pytest.mark.parametrize("case", ["unaligned_in", "unaligned_out", "odd_stride", "odd_out_stride", "wide_strides", "short"])
def test_fold4_access_variants_give_the_same_values(engines, oracle, case):
    p, g = xc.PRIMES[1]
    eng, L = engines[p], (8 if case == "short" else 1 << 12)   # short: q = 2, no 16-byte variant at any alignment
    cw = np.random.default_rng(9).integers(0, p, (4, L), dtype=np.uint64)
    omega, al = oracle.ff_prim_nth_root_g(L, p, g), [U64_MAX, p, 3, U64_MAX - p]
    kw = {"unaligned_in": dict(lead=1), "unaligned_out": dict(out_lead=3), "odd_stride": dict(stride=L + 1),
          "odd_out_stride": dict(out_stride=L // 4 + 3), "wide_strides": dict(stride=L + 64, out_stride=L // 4 + 32), "short": {}}[case]
    want = f4.two_folds(cw, al, g, omega, p, g)
    assert np.array_equal(gpu_fold4(eng, cw, al, g, omega), want)
    assert np.array_equal(gpu_fold4(eng, cw, al, g, omega, **kw), want)


def test_fold4_refusals(engines):
    import stark_rs_amd as s
    p, g = xc.PRIMES[0]
    eng = engines[p]
    BAD_ARG = -50
    with Dev(eng) as dev:
        d = dev.alloc(4 * 64)
        ok = dict(length=16, stride=16, offset=g, omega=5, out_stride=4)
        for bad in [dict(length=2, stride=16), dict(length=12), dict(length=3 << 20, stride=3 << 20, out_stride=3 << 18),
                    dict(length=1 << 28, stride=1 << 28, out_stride=1 << 26), dict(stride=15), dict(out_stride=3)]:
            a = dict(ok, **bad)
            with pytest.raises(s.StarkMiError) as ei:
                eng.dev_fri_fold4_ext(d, a["length"], a["stride"], d, a["offset"], a["omega"], d, a["out_stride"])
            assert ei.value.status == BAD_ARG, bad
        for bad in [dict(offset=p), dict(omega=p), dict(offset=0), dict(omega=0)]:   # the statuses of smi_dev_fri_fold_ext
            a = dict(ok, **bad)
            with pytest.raises(s.StarkMiError) as e4:
                eng.dev_fri_fold4_ext(d, 16, 16, d, a["offset"], a["omega"], d, 4)
            with pytest.raises(s.StarkMiError) as e2:
                eng.dev_fri_fold_ext(d, 16, 16, d, a["offset"], a["omega"], d, 8)
            assert e4.value.status == e2.value.status and e4.value.status != 0, bad
        for null in range(3):
            ptrs = [d, d, d]
            ptrs[null] = 0
            with pytest.raises(s.StarkMiError) as ei:
                eng.dev_fri_fold4_ext(ptrs[0], 16, 16, ptrs[1], g, 5, ptrs[2], 4)
            assert ei.value.status == BAD_ARG
        eng.sync()


# ---------------------------------------------------------------------------------------------- FRI at folding factor 4
def gpu_prove4(eng, cfg, cw, prior=b"", bits=0, stride=None):
    import torch
    t_in, d_in = _dev_cols(cw, stride)
    torch.cuda.synchronize()
    return eng.dev_fri_prove_ext(cfg, d_in, cw.shape[1], stride, transcript=prior, grind_bits=bits, folding=4)


# (log N, E, t, bits, prior): R2 - 1 odd and even, F = 0 .. 5, every prior length, both difficulties
# the three smallest: N = 8 and 16 (F = 0, trees of 2 and 4 coset leaves) and N = 32 (one fold onto a last tree of 2 leaves; a
# layer that is folded has q >= L_last >= 8, so no smaller tree exists)
PROVE4_CASES = [(3, 4, 1, 0, b""), (4, 4, 1, 8, b""), (5, 4, 1, 0, b"\x09" * 5), (6, 4, 1, 0, b""), (6, 8, 5, 8, b"\x05" * 5), (8, 4, 5, 0, b"\x05" * 37), (8, 8, 32, 8, b""), (9, 4, 1, 8, b""), (9, 8, 40, 0, b"\x01" * 5),
                (12, 4, 32, 0, b""), (12, 8, 40, 8, b"\x02" * 37), (13, 4, 5, 8, b"\x03" * 5), (13, 8, 32, 0, b"")]


def test_the_prove_cases_cover_both_parities():
    got = [f4.layout(1 << ln, E, t)[:2] for ln, E, t, _b, _p in PROVE4_CASES]
    assert {(R2 - 1) % 2 for R2, _F in got} == {0, 1} and {F for _R2, F in got} >= {0, 1, 2, 3, 4}, got


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_N,E,t,bits,prior", PROVE4_CASES)
def test_prove_fold4_bytes_equal_the_restatement_and_both_verifiers_accept(engines, oracle, p, g, log_N, E, t, bits, prior):
    eng, N = engines[p], 1 << log_N
    cfg_o, cw, want, want_top, want_nonce = f4.shared_proof(oracle, p, g, log_N, E, t, bits, prior)
    cfg = eng.fri_cfg(int(cfg_o.omega), g, N, E, t)
    got, top, nonce = gpu_prove4(eng, cfg, cw, prior, bits)
    assert (top, nonce) == (want_top, want_nonce)
    assert got == want
    R2, F, last, n = f4.layout(N, E, t)
    assert len(got) == n == eng.fri_fold4_layout(cfg)[2]
    if F >= 1:
        import pow_compose as pc
        assert n < pc.proof_len(N, E, t, R2)
    ok_o, pv_o, used_o, _top, why_o = f4.verify(oracle, cfg_o, got, g, prior, bits)
    ok, pv, used, why = eng.fri_verify_ext(cfg, got, prior, grind_bits=bits, folding=4)
    assert ok_o and ok, (why_o, why)
    assert pv == pv_o and used == used_o == len(got)
    ok, _pv, used, _ = eng.fri_verify_ext(cfg, got + b"\x02trailing", prior, grind_bits=bits, folding=4)
    assert ok and used == len(got)


def test_prove_fold4_from_strided_columns(engines, oracle):
    p, g = xc.PRIMES[0]
    eng, log_N, E, t = engines[p], 9, 4, 5
    cfg_o, cw, want, want_top, _nonce = f4.shared_proof(oracle, p, g, log_N, E, t, 8)
    cfg = eng.fri_cfg(int(cfg_o.omega), g, 1 << log_N, E, t)
    for stride in ((1 << log_N) + 5, (1 << log_N) + 64):
        got, top, _ = gpu_prove4(eng, cfg, cw, b"", 8, stride=stride)
        assert got == want and top == want_top


def _both(eng, oracle, cfg, cfg_o, g, proof, prior, bits):
    ok_o, _pv, _used, _top, why_o = f4.verify(oracle, cfg_o, proof, g, prior, bits)
    ok, _pv, _used, why = eng.fri_verify_ext(cfg, proof, prior, grind_bits=bits, folding=4)
    assert not ok_o and not ok
    assert why == why_o and why
    return why


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_N,E,t,bits", [(8, 8, 5, 0), (9, 4, 5, 8)])
def test_verify_fold4_rejections_give_the_restatement_s_sentence(engines, oracle, p, g, log_N, E, t, bits):
    eng, N = engines[p], 1 << log_N
    cfg_o, cw, proof, _top, nonce = f4.shared_proof(oracle, p, g, log_N, E, t, bits)
    cfg = eng.fri_cfg(int(cfg_o.omega), g, N, E, t)
    assert gpu_prove4(eng, cfg, cw, b"", bits)[0] == proof
    assert eng.fri_verify_ext(cfg, proof, b"", grind_bits=bits, folding=4)[0]
    for name, m, want in f4.mutations(proof, N, E, t, p):
        why = _both(eng, oracle, cfg, cfg_o, g, m, b"", bits)
        assert want is None or why == want, (name, why)
    at = [a for kind, _r, a in f4.objects(N, E, t)[0] if kind == "nonce"][0]
    wrong = bytearray(proof)                                              # a wrong nonce, a wrong transcript, a higher demand
    wrong[at + 9:at + 17] = (nonce + 1).to_bytes(8, "little")
    _both(eng, oracle, cfg, cfg_o, g, bytes(wrong), b"", bits)
    _both(eng, oracle, cfg, cfg_o, g, proof, b"x", bits)
    if bits:
        assert _both(eng, oracle, cfg, cfg_o, g, proof, b"", 24) == "proof of work"
        assert eng.fri_verify_ext(cfg, proof, b"", grind_bits=bits - 3, folding=4)[0]


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_a_crooked_layer_is_rejected_with_the_new_sentence(engines, oracle, p, g):
    """the restated prover with a fold that is off by X^2 in every later layer: honest trees, paths that verify, cosets
    that do not fold to the next layer"""
    log_N, E, t = 8, 4, 3
    N = 1 << log_N
    eng = engines[p]
    cw, omega = f4.low_degree_codeword(oracle, p, g, N, E, g, 5)
    cfg_o, cfg = oracle.fri_cfg(omega, g, N, E, t, p), eng.fri_cfg(omega, g, N, E, t)
    real = f4.fold4
    try:
        def crooked(c, alpha, offset, om, pp, gg):
            out = real(c, alpha, offset, om, pp, gg)
            out[2] = (out[2] + np.uint64(1)) % np.uint64(pp)
            return out
        f4.fold4 = crooked
        proof, _top, _nonce = f4.prove(oracle, cfg_o, cw, g)
    finally:
        f4.fold4 = real
    assert _both(eng, oracle, cfg, cfg_o, g, proof, b"", 0) == f4.FOLD4_MISMATCH


@pytest.mark.parametrize("spoil", range(4))
def test_one_coordinate_of_too_high_degree_is_rejected(engines, oracle, spoil):
    p, g = xc.PRIMES[spoil % 2]
    eng, N, E, t = engines[p], 1 << 9, 4, 5
    cw, omega = f4.low_degree_codeword(oracle, p, g, N, E, g, 11, spoil=spoil)
    cfg_o, cfg = oracle.fri_cfg(omega, g, N, E, t, p), eng.fri_cfg(omega, g, N, E, t)
    proof, _top, _nonce = gpu_prove4(eng, cfg, cw)
    assert _both(eng, oracle, cfg, cfg_o, g, proof, b"", 0) == "last codeword does not correspond to polynomial of low enough degree"


@pytest.mark.parametrize("log_N,E,t", [(6, 8, 5), (8, 8, 5), (9, 4, 5)])
def test_factor_2_and_factor_4_proofs_do_not_cross(engines, oracle, log_N, E, t):
    p, g = xc.PRIMES[1]
    eng, N = engines[p], 1 << log_N
    cfg_o, cw, proof4, _top, _nonce = f4.shared_proof(oracle, p, g, log_N, E, t, 0)
    cfg = eng.fri_cfg(int(cfg_o.omega), g, N, E, t)
    t_in, d_in = _dev_cols(cw)
    proof2, _top2, _n2 = eng.dev_fri_prove_ext(cfg, d_in, N, transcript=b"", grind_bits=0)
    assert eng.fri_verify_ext(cfg, proof2, b"", grind_bits=0)[0] and eng.fri_verify_ext(cfg, proof4, b"", grind_bits=0, folding=4)[0]
    ok, _pv, _used, why = eng.fri_verify_ext(cfg, proof2, b"", grind_bits=0, folding=4)
    assert not ok and why
    assert not f4.verify(oracle, cfg_o, proof2, g)[0]
    ok, _pv, _used, why = eng.fri_verify_ext(cfg, proof4, b"", grind_bits=0)
    assert not ok and why


def test_folding_keyword_refusals(engines):
    import stark_rs_amd as s
    p, g = xc.PRIMES[0]
    eng = engines[p]
    cfg = eng.fri_cfg(5, g, 64, 4, 2)
    for bad in (0, 1, 3, 8, "4"):
        with pytest.raises(s.StarkMiError):
            eng.dev_fri_prove_ext(cfg, 0, 64, folding=bad)
        with pytest.raises(s.StarkMiError):
            eng.fri_verify_ext(cfg, b"", folding=bad)


# ---------------------------------------------------------------------------------------------- the AIR proof over it
import air_compose as ac  # noqa: E402
import air_periodic as ap  # noqa: E402

KW4 = dict(row_leaves=True, ext=True, folding=4)


def _air(name, p, n):
    """K = 0, K > 0, and K > 0 with a periodic column"""
    return {"empty": ac.make, "mixer": ac.make, "fib": ac.make, "mimc": ap.make}[name](name, n, p)


# every AIR at the two smallest sizes, one each (in turn) at the larger ones
AIR4_CASES = [(ln, name) for ln in (8, 9) for name in ("empty", "mixer", "mimc")] + [(10, "mixer"), (11, "mimc"), (12, "empty"), (12, "fib")]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,name", AIR4_CASES)
def test_air_prove_fold4_bytes_equal_the_restatement_and_verify_accepts(engines, oracle, p, g, log_n, name):
    eng, lb, t, bits = engines[p], 3, 4, [0, 8][log_n % 2]
    air, cols = _air(name, p, 1 << log_n)
    W, K = len(cols), len(air.constraints)
    assert (K == 0) == (name == "empty")
    _d, E = eng.air_plan(air, W, log_n, lb)
    with Dev(eng) as dev:
        res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, grind_bits=bits, **KW4)
    root, want, top, _nonce = f4.air_proof(oracle, air, cols, p, g, log_n, lb, t, 1, g, E, bits)
    assert bytes(res["column_roots"][0]) == root
    assert res["top_indices"] == top
    assert res["proof"] == want
    N = 1 << (log_n + lb)
    assert len(want) == f4.layout(N, E, t)[3] + f4.opening4_len(W, K, log_n + lb, t)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **KW4)
    assert ok, why


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_air_verify_fold4_rejections(engines, oracle, p, g):
    import stark_rs_amd as s
    eng, log_n, lb, t, bits = engines[p], 9, 3, 6, 8
    n = 1 << log_n
    air, cols = ac.make("mixer", n, p)
    W, K = len(cols), len(air.constraints)
    kw2 = dict(row_leaves=True, ext=True)
    with Dev(eng) as dev:
        d_trace = dev.upload(np.array(cols, dtype=np.uint64))
        res = eng.dev_air_prove(air, d_trace, W, log_n, lb, t, grind_bits=bits, **KW4)
        res2 = eng.dev_air_prove(air, d_trace, W, log_n, lb, t, grind_bits=bits, **kw2)
        bad_cols = np.array(cols, dtype=np.uint64)
        bad_cols[1, n // 3] = (bad_cols[1, n // 3] + 1) % p                   # a trace that violates one row
        d_bad = dev.upload(bad_cols)
        with pytest.raises(s.StarkMiError):
            eng.dev_air_prove(air, d_bad, W, log_n, lb, t, grind_bits=bits, **KW4)
        forced = eng.dev_air_prove(air, d_bad, W, log_n, lb, t, grind_bits=bits, check=False, **KW4)
    roots, proof = res["column_roots"], res["proof"]
    E = eng.air_plan(air, W, log_n, lb)[1]

    def both(bad, rts=roots, statement=air):
        """the GPU verifier and the restated one on the same bytes: both reject, with the same sentence"""
        ok, why = eng.air_verify(statement, bad, rts, W, log_n, lb, t, grind_bits=bits, **KW4)
        ok_o, why_o = f4.air_verify(oracle, statement, bytes(rts[0]), bad, p, g, log_n, lb, t, 1, g, E, bits)
        assert not ok and not ok_o and why and why == why_o, (why, why_o)
        return why
    assert eng.air_verify(air, proof, roots, W, log_n, lb, t, grind_bits=bits, **KW4) == (True, "")
    assert f4.air_verify(oracle, air, bytes(roots[0]), proof, p, g, log_n, lb, t, 1, g, E, bits) == (True, "")
    assert both(forced["proof"], forced["column_roots"]) == "last codeword does not correspond to polynomial of low enough degree"
    ob = f4.opening4_len(W, K, log_n + lb, t)
    sec = len(proof) - ob
    rec, R, A = 9 + 8 * W, 8, f4.AIR_WORDS
    prec = 9 + 32 * (log_n + lb)
    for name, at, want in [("an opened row", sec + 9 + 3, A["auth"]), ("the row B further", sec + 4 * rec + 9, A["auth"]),
                           ("the last row", sec + (t * R - 1) * rec + 9 + 8, A["auth"]), ("a row's tag", sec + 2 * rec, A["row"]),
                           ("a row's count", sec + 3 * rec + 1, A["row"]), ("a path's tag", sec + t * R * rec + 5 * prec, A["path"]),
                           ("a path's count", sec + t * R * rec + prec + 1, A["path"]), ("a path", sec + t * R * rec + 9 + 40, A["auth"]),
                           ("the last path", len(proof) - 5, A["auth"])]:
        bad = bytearray(proof)
        bad[at] ^= 1
        assert both(bytes(bad)) == want, name
    for bad in (proof[:-1], proof + b"\x00", proof[:sec]):
        assert both(bad) == A["length"]
    bad = bytearray(proof)                                                    # a row value + p: the leaf hashes the raw u64
    v = int.from_bytes(proof[sec + 9:sec + 17], "little") + p
    bad[sec + 9:sec + 17] = v.to_bytes(8, "little")
    assert both(bytes(bad)) == A["auth"]
    bad = bytearray(proof)                                                    # a coset record of layer 0: FRI's own checks
    at = [a for kind, r, a in f4.objects(1 << (log_n + lb), E, t)[0] if kind == "coset"][0]
    bad[at + 9] ^= 1
    assert both(bytes(bad)) == "merkle authentication path verification fails for aa"
    ok, why = eng.air_verify(air, res2["proof"], res2["column_roots"], W, log_n, lb, t, grind_bits=bits, **KW4)
    assert not ok and why                                                     # a proof of _ext_pow is rejected here ...
    ok, why = eng.air_verify(air, proof, roots, W, log_n, lb, t, grind_bits=bits, **kw2)
    assert not ok and why                                                     # ... and the other way round


def test_air_fold4_keyword_refusals(engines):
    import stark_rs_amd as s
    from stark_rs_amd.mirror import Air
    p, g = xc.PRIMES[0]
    eng, log_n, lb = engines[p], 8, 3
    air, cols = ac.make("mixer", 1 << log_n, p)
    W = len(cols)
    with Dev(eng) as dev:
        d_trace = dev.upload(np.array(cols, dtype=np.uint64))
        for kw in (dict(folding=4), dict(folding=4, row_leaves=True), dict(folding=3, row_leaves=True, ext=True), dict(folding=8, row_leaves=True, ext=True)):
            with pytest.raises(s.StarkMiError):
                eng.dev_air_prove(air, d_trace, W, log_n, lb, 4, **kw)
            with pytest.raises(s.StarkMiError):
                eng.air_verify(air, b"", [b"\x00" * 32], W, log_n, lb, 4, **kw)
        perm = Air(W)
        perm.permutation([0], [1])
        with pytest.raises(s.StarkMiError):
            eng.dev_air_prove(perm, d_trace, W, log_n, lb, 4, **KW4)
        # no fold at this shape (t so large that FRI stops after two rounds): refused by prover and verifier with a sentence
        t_big = 1 << (log_n + lb - 3)
        with pytest.raises(s.StarkMiError, match="no fold"):
            eng.dev_air_prove(air, d_trace, W, log_n, lb, t_big, check=False, **KW4)
        with pytest.raises(s.StarkMiError, match="no fold"):
            eng.air_verify(air, b"", [b"\x00" * 32], W, log_n, lb, t_big, **KW4)


def test_air_fold4_at_the_headline_shape(engines):
    """n = 2^22, W = 4, blowup 8, t = 32: no restatement at this size; the verifier accepts, the length is the header's"""
    import torch
    from stark_rs_amd.mirror import Air
    p, g = xc.PRIMES[1]
    eng, W, log_n, lb, t, bits = engines[p], 4, 22, 3, 32, 16
    n, N = 1 << log_n, 1 << (log_n + lb)
    rng = np.random.default_rng(22)
    y = rng.integers(0, p, n, dtype=np.int64)
    xv, yl, xs = 5, y.tolist(), [5]
    for r in range(n - 1):                                                    # column 0 follows x' = x y + 1
        xv = (xv * yl[r] + 1) % p
        xs.append(xv)
    cols = np.stack([np.array(xs, dtype=np.int64), y, rng.integers(0, p, n, dtype=np.int64), rng.integers(0, p, n, dtype=np.int64)])
    air = Air(W)
    air.transition({("next", 0): 1, (("cur", 0), ("cur", 1)): -1, (): -1})
    air.boundary(0, 0, 5).boundary(3, n - 1, int(cols[3][n - 1]))
    _d, E = eng.air_plan(air, W, log_n, lb)
    trace = torch.from_numpy(cols.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    res = eng.dev_air_prove(air, trace.data_ptr(), W, log_n, lb, t, grind_bits=bits, **KW4)
    assert len(res["proof"]) == f4.layout(N, E, t)[3] + f4.opening4_len(W, 1, log_n + lb, t)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **KW4)
    assert ok, why
    assert not eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, row_leaves=True, ext=True)[0]


COMPOSITION = f4.AIR_WORDS["composition"]


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_fold4_verifier_recomputes_the_composition_at_all_four_points(engines, oracle, p, g):
    """An honest proof under another statement with the same W and K: transcript, FRI and every path are the prover's, so
    only the recomputation of the codeword from the opened rows can refuse it -- on the GPU and in the restatement"""
    from test_gpu_air_rows import _mixer_like
    eng, log_n, lb, t, bits = engines[p], 9, 3, 5, 0
    n = 1 << log_n
    mixer, cols = ac.make("mixer", n, p)
    a_last = cols[0][-1]

    def proved(air, trace):
        W = len(trace)
        E = eng.air_plan(air, W, log_n, lb)[1]
        with Dev(eng) as dev:
            res = eng.dev_air_prove(air, dev.upload(np.array(trace, dtype=np.uint64)), W, log_n, lb, t, grind_bits=bits, **KW4)

        def check(statement, **kw):
            got = eng.air_verify(statement, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **KW4)
            want = f4.air_verify(oracle, statement, bytes(res["column_roots"][0]), res["proof"], p, g, log_n, lb, t, 1, g, E, bits)
            assert got == want, (got, want)
            return got
        return res, E, check
    _res, _E, check = proved(mixer, cols)
    assert check(mixer) == (True, "")
    assert check(_mixer_like(n, p, a_last=a_last)) == (True, "")                      # the same statement, rebuilt
    assert check(_mixer_like(n, p, a0=6, a_last=a_last)) == (False, COMPOSITION)      # one boundary value
    assert check(_mixer_like(n, p, b_coef=4, a_last=a_last)) == (False, COMPOSITION)  # one coefficient
    assert check(_mixer_like(n, p, c_next=3, a_last=a_last)) == (False, COMPOSITION)  # one next-row operand
    switch, scols = ap.make("switch", n, p)                                           # one periodic value
    _sres, _sE, scheck = proved(switch, scols)
    assert scheck(switch) == (True, "")
    other, _ = ap.make("switch", n, p)
    other.periodics[0] = [1, 2]
    assert scheck(other) == (False, COMPOSITION)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_a_difference_that_vanishes_at_every_first_point_is_caught_at_the_others(engines, oracle, p, g):
    """The statements differ in the boundary values of column 3 by D(x) = prod_s (x - x_s) over the tests' FIRST coset
    points x_s: the boundary interpolants agree at every x_s, so slot 0 of no test can tell the statements apart, and they
    differ at x_s iota^k.  A verifier that compared slot 0 alone would accept; the restatement restricted to slot 0 does."""
    eng, log_n, lb, t, bits = engines[p], 8, 3, 3, 0
    n, N = 1 << log_n, 1 << (log_n + lb)
    _mixer, cols = ac.make("mixer", n, p)
    rows_pinned = list(range(t + 1))

    def statement(delta):
        air, _ = ac.make("mixer", n, p)
        for r, d in zip(rows_pinned, delta):
            air.boundary(3, r, (cols[3][r] + d) % p)
        return air
    honest = statement([0] * (t + 1))
    W = len(cols)
    E = eng.air_plan(honest, W, log_n, lb)[1]
    with Dev(eng) as dev:
        res = eng.dev_air_prove(honest, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, grind_bits=bits, **KW4)
    roots, proof = res["column_roots"], res["proof"]
    w, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
    xs = [g * pow(wN, s % (N // 4), p) % p for s in res["top_indices"]]
    delta = []
    for r in rows_pinned:                                           # D at the pinned trace points tau w^r, tau = 1
        d = 1
        for x in xs:
            d = d * (pow(w, r, p) - x) % p
        delta.append(d)
    assert all(delta)
    other = statement(delta)
    args = (bytes(roots[0]), proof, p, g, log_n, lb, t, 1, g, E, bits)
    assert eng.air_verify(honest, proof, roots, W, log_n, lb, t, grind_bits=bits, **KW4) == (True, "")
    assert f4.air_verify(oracle, honest, *args) == (True, "")
    assert f4.air_verify(oracle, other, *args, slots=(0,)) == (True, "")             # slot 0 cannot see it ...
    assert f4.air_verify(oracle, other, *args) == (False, COMPOSITION)                # ... the other points do
    assert eng.air_verify(other, proof, roots, W, log_n, lb, t, grind_bits=bits, **KW4) == (False, COMPOSITION)


@pytest.mark.parametrize("name", ["mixer", "empty"])
def test_an_opened_value_plus_p_under_an_honest_tree_gets_the_canonical_sentence(engines, oracle, name):
    """the restated prover commits and opens one column as value + p: every path verifies (the leaf hashes the raw u64), the
    residues are the honest ones, and only the canonical check stands between the proof and acceptance"""
    p, g = xc.PRIMES[0]
    eng, log_n, lb, t, bits = engines[p], 8, 3, 3, 0
    air, cols = ac.make(name, 1 << log_n, p)
    W = len(cols)
    E = eng.air_plan(air, W, log_n, lb)[1]
    for col in (0, W - 1):
        root, proof, _top, _nonce = f4.air_proof(oracle, air, cols, p, g, log_n, lb, t, 1, g, E, bits, plus_p_col=col)
        want = (False, f4.AIR_WORDS["canonical"])
        assert f4.air_verify(oracle, air, root, proof, p, g, log_n, lb, t, 1, g, E, bits) == want
        assert eng.air_verify(air, proof, [root], W, log_n, lb, t, grind_bits=bits, **KW4) == want
