"""GPU: the quartic-extension entry points -- smi_dev_fri_fold_ext, smi_dev_fri_prove_ext / smi_fri_verify_ext,
smi_dev_air_compose_ext, smi_dev_air_prove_ext / smi_air_verify_ext -- against the Python restatement built from the CPU
oracle's primitives (tests/ext_compose.py) and, for the composition, against smi_dev_air_compose coordinate by
coordinate.  Every comparison is exact.  `pytest -m gpu`."""
import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import air_rows as ar
import ext_compose as xc
import transcript_compose as tc
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)

pytestmark = pytest.mark.gpu
U64_MAX = (1 << 64) - 1


def _dev_cols(arr, stride=None, lead=0):
    """(4, L) residues -> a torch int32 buffer with the columns `stride` apart after `lead` words; -> (tensor, pointer)"""
    import torch
    L = arr.shape[1]
    stride = L if stride is None else stride
    host = np.full(lead + arr.shape[0] * stride, 0x7fffffff, dtype=np.uint32)
    for e in range(arr.shape[0]):
        host[lead + e * stride:lead + e * stride + L] = arr[e]
    t = torch.from_numpy(host.view(np.int32)).cuda()
    return t, t.data_ptr() + 4 * lead


def _dev_u64(vals):
    import torch
    t = torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64)).cuda()
    return t, t.data_ptr()


def gpu_fold(eng, cw, alpha, offset, omega, stride=None, out_stride=None, lead=0, out_lead=0):
    import torch
    L = cw.shape[1]
    out_stride = L // 2 if out_stride is None else out_stride
    t_in, d_in = _dev_cols(cw, stride, lead)
    t_al, d_al = _dev_u64(alpha)
    t_out = torch.full((out_lead + 4 * out_stride,), 0x7fffffff, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.dev_fri_fold_ext(d_in, L, L if stride is None else stride, d_al, offset, omega, t_out.data_ptr() + 4 * out_lead, out_stride)
    eng.sync()
    out = t_out.cpu().numpy().view(np.uint32)[out_lead:]
    for e in range(4):   # nothing written between the columns
        assert np.all(out[e * out_stride + L // 2:(e + 1) * out_stride] == 0x7fffffff)
    return np.stack([out[e * out_stride:e * out_stride + L // 2] for e in range(4)]).astype(np.uint64)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_fold_ext_equals_the_restatement_at_every_length(engines, oracle, p, g):
    eng = engines[p]
    for log_len in range(1, 21):
        L = 1 << log_len
        rng = np.random.default_rng(log_len)
        cw = rng.integers(0, p, (4, L), dtype=np.uint64)
        cw[:, 0] = p - 1
        cw[:, L // 2] = [0, p - 1, 0, p - 1]
        omega, offset = oracle.ff_prim_nth_root_g(L, p, g), [g, 7, 1][log_len % 3]
        alphas = [[U64_MAX] * 4, [p, p + 1, U64_MAX - 1, 2 * p - 1], [1 << 63, 12345, p - 1, 1 << 32]]
        for al in alphas[:1 + (log_len <= 12) * 2]:
            assert np.array_equal(gpu_fold(eng, cw, al, offset, omega), xc.fold(cw, al, offset, omega, p, g)), (log_len, al)


@pytest.mark.parametrize("case", ["unaligned_in", "unaligned_out", "odd_stride", "odd_out_stride", "wide_strides"])
def test_fold_ext_without_vector_accesses_equals_the_restatement(engines, oracle, case):
    p, g = xc.PRIMES[1]
    eng, L = engines[p], 1 << 12
    cw = np.random.default_rng(9).integers(0, p, (4, L), dtype=np.uint64)
    omega, al = oracle.ff_prim_nth_root_g(L, p, g), [U64_MAX, p, 3, U64_MAX - p]
    kw = {"unaligned_in": dict(lead=1), "unaligned_out": dict(out_lead=3), "odd_stride": dict(stride=L + 1),
          "odd_out_stride": dict(out_stride=L // 2 + 3), "wide_strides": dict(stride=L + 64, out_stride=L // 2 + 32)}[case]
    assert np.array_equal(gpu_fold(eng, cw, al, g, omega, **kw), xc.fold(cw, al, g, omega, p, g))


def test_fold_ext_refusals(engines):
    import stark_rs_amd as s
    p, g = xc.PRIMES[0]
    eng = engines[p]
    with Dev(eng) as dev:
        d = dev.alloc(4 * 64)
        for bad in [dict(length=12), dict(length=16, stride=8), dict(length=16, out_stride=4)]:
            with pytest.raises(s.StarkMiError):
                eng.dev_fri_fold_ext(d, bad["length"], bad.get("stride", 16), d, g, 5, d, bad.get("out_stride", 8))
    with pytest.raises(s.StarkMiError):   # a square g never gets as far as a context: its 2-power order is not full
        s.Engine(p, 9, 0)                 # (smi_ext_mul / smi_ext_inv refuse it by themselves, tests/test_ext_host.py)


# ---------------------------------------------------------------------------------------------- FRI over F_q
def low_degree_codeword(o, p, g, N, E, offset, seed, spoil=None):
    """four coordinates of degree < N / E on offset * <omega_N>; spoil: a coordinate that gets a random codeword instead"""
    rng = np.random.default_rng(seed)
    omega = o.ff_prim_nth_root_g(N, p, g)
    cw = np.stack([np.asarray(o.fast_coset_ntt(rng.integers(0, p, N // E, dtype=np.uint64), N, omega, offset, p), dtype=np.uint64) for _ in range(4)])
    if spoil is not None:
        cw[spoil] = rng.integers(0, p, N, dtype=np.uint64)
    return cw, omega


def gpu_prove(eng, cfg, cw, prior=b"", stride=None):
    import torch
    t_in, d_in = _dev_cols(cw, stride)
    torch.cuda.synchronize()
    return eng.dev_fri_prove_ext(cfg, d_in, cw.shape[1], stride, transcript=prior)


PROVE_CASES = [(8, 4, 4, b""), (12, 8, 16, b""), (16, 8, 32, b""), (16, 4, 8, b"\x05" * 37)] + \
              [(12, 4, 8, bytes(range(k))) for k in (5, 32, 37)]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_N,E,t,prior", PROVE_CASES)
def test_prove_ext_bytes_equal_the_restatement_and_verify_accepts(engines, oracle, p, g, log_N, E, t, prior):
    eng, N = engines[p], 1 << log_N
    cw, omega = low_degree_codeword(oracle, p, g, N, E, g, log_N)
    cfg_o, cfg = oracle.fri_cfg(omega, g, N, E, t, p), eng.fri_cfg(omega, g, N, E, t)
    want, want_top = xc.prove(oracle, cfg_o, cw, g, prior)
    got, top = gpu_prove(eng, cfg, cw, prior)
    assert top == want_top
    assert got == want
    assert len(got) == xc.proof_len(N, E, t, oracle.fri_num_rounds(cfg_o))
    ok_o, pv_o, used_o, _ = xc.verify(oracle, cfg_o, got, g, prior)
    ok, pv, used, why = eng.fri_verify_ext(cfg, got, prior)
    assert ok_o and ok, why
    assert pv == pv_o and used == used_o == len(got)
    ok, _pv, used, _ = eng.fri_verify_ext(cfg, got + b"\x02trailing", prior)     # objects after the proof are the caller's
    assert ok and used == len(got)


def test_prove_ext_from_strided_columns(engines, oracle):
    p, g = xc.PRIMES[0]
    eng, N, E, t = engines[p], 1 << 10, 4, 8
    cw, omega = low_degree_codeword(oracle, p, g, N, E, 7, 1)
    cfg_o, cfg = oracle.fri_cfg(omega, 7, N, E, t, p), eng.fri_cfg(omega, 7, N, E, t)
    want, _ = xc.prove(oracle, cfg_o, cw, g)
    assert gpu_prove(eng, cfg, cw, stride=N + 5)[0] == want


def _records(proof):
    """-> [(tag, first byte, one byte past the end)] of the proof's objects"""
    out, at = [], 0
    while at < len(proof):
        obj = xc._pop(proof, at)
        out.append((obj[0], at, obj[2]))
        at = obj[2]
    return out


def _both_reject(eng, oracle, cfg, cfg_o, g, proof, prior=b""):
    ok_o = xc.verify(oracle, cfg_o, proof, g, prior)[0]
    ok, _pv, _used, why = eng.fri_verify_ext(cfg, proof, prior)
    assert not ok_o and not ok and why
    return why


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_verify_ext_rejections(engines, oracle, p, g):
    eng, N, E, t, prior = engines[p], 1 << 10, 4, 6, b"prefix"
    cw, omega = low_degree_codeword(oracle, p, g, N, E, g, 4)
    cfg_o, cfg = oracle.fri_cfg(omega, g, N, E, t, p), eng.fri_cfg(omega, g, N, E, t)
    proof, _ = gpu_prove(eng, cfg, cw, prior)
    assert eng.fri_verify_ext(cfg, proof, prior)[0] and xc.verify(oracle, cfg_o, proof, g, prior)[0]
    recs = _records(proof)
    R = oracle.fri_num_rounds(cfg_o)
    kinds = {"first root": recs[0], "last root": recs[R - 1], "last codeword": recs[R], "first triple": recs[R + 1],
             "last layer triple": [r for r in recs if r[0] == 2][-1], "first path": [r for r in recs if r[0] == 3][0],
             "last path": recs[-1]}
    for name, (tag, a, b) in kinds.items():
        for at in ({a + 1, a + 9, b - 1} if tag else {a + 1, b - 1}):    # payload bytes, the low byte of a value among them
            bad = bytearray(proof)
            bad[at] ^= 0x01
            _both_reject(eng, oracle, cfg, cfg_o, g, bytes(bad), prior)
        bad = bytearray(proof)                                            # the tag, and for counted records the count
        bad[a] ^= 0x02
        _both_reject(eng, oracle, cfg, cfg_o, g, bytes(bad), prior)
    for name in ("last codeword", "first triple"):                        # a coordinate + p: the same residue, not canonical
        _tag, a, _b = kinds[name]
        for k in (0, 3, 5):
            bad = bytearray(proof)
            v = int.from_bytes(proof[a + 9 + 8 * k:a + 17 + 8 * k], "little")
            bad[a + 9 + 8 * k:a + 17 + 8 * k] = (v + p).to_bytes(8, "little")
            assert "canonical" in _both_reject(eng, oracle, cfg, cfg_o, g, bytes(bad), prior)
    for cut in (1, 31, 32, 33, len(proof) // 2, len(proof) - 40):
        _both_reject(eng, oracle, cfg, cfg_o, g, proof[:len(proof) - cut], prior)
    _both_reject(eng, oracle, cfg, cfg_o, g, b"", prior)
    for wrong in (b"", b"prefiy", b"prefix\x00"):
        _both_reject(eng, oracle, cfg, cfg_o, g, proof, wrong)
    other = eng.fri_cfg(omega, g, N, E * 2, t)                            # a tighter degree bound than the codeword's
    assert not eng.fri_verify_ext(other, proof, prior)[0]


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_base_and_extension_proofs_do_not_cross(engines, oracle, p, g):
    eng, N, E, t = engines[p], 1 << 10, 4, 6
    cw, omega = low_degree_codeword(oracle, p, g, N, E, g, 5)
    cfg_o, cfg = oracle.fri_cfg(omega, g, N, E, t, p), eng.fri_cfg(omega, g, N, E, t)
    with Dev(eng) as dev:
        base, _ = eng.dev_fri_prove(cfg, dev.upload(cw[0]), N, transcript=b"tr")
    assert eng.fri_verify(cfg, base, transcript=b"tr")[0]
    _both_reject(eng, oracle, cfg, cfg_o, g, base, b"tr")
    ext, _ = gpu_prove(eng, cfg, cw, b"tr")
    assert eng.fri_verify_ext(cfg, ext, b"tr")[0]
    assert not eng.fri_verify(cfg, ext, transcript=b"tr")[0]
    assert not tc.verify(oracle, cfg_o, ext, b"tr")[0]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("spoil", [0, 3])
def test_one_coordinate_of_high_degree_is_rejected(engines, oracle, p, g, spoil):
    """coordinates of low degree but one: a verifier that checks one coordinate (or three) accepts this"""
    eng, N, E, t = engines[p], 1 << 10, 4, 6
    cw, omega = low_degree_codeword(oracle, p, g, N, E, g, 6, spoil=spoil)
    cfg_o, cfg = oracle.fri_cfg(omega, g, N, E, t, p), eng.fri_cfg(omega, g, N, E, t)
    proof, _ = gpu_prove(eng, cfg, cw)
    assert proof == xc.prove(oracle, cfg_o, cw, g)[0]                      # the prover does not judge: same bytes
    assert "degree" in _both_reject(eng, oracle, cfg, cfg_o, g, proof)


# ---------------------------------------------------------------------------------------------- the composition
def gpu_compose_pair(eng, dev, air, cols, ch, log_n, lb, tau, h):
    """-> (four coordinate columns of smi_dev_air_compose_ext, four codewords of smi_dev_air_compose under weights e)"""
    W, N = len(cols), 1 << (log_n + lb)
    d_trace = dev.upload(np.array(cols, dtype=np.uint64))
    d_lde, d_out4, d_out = dev.alloc(4 * W * N), dev.alloc(16 * N), dev.alloc(4 * N)
    eng.dev_lde(d_trace, W, log_n, lb, d_lde, trace_offset=tau, lde_offset=h)
    eng.dev_air_compose_ext(air, d_lde, W, log_n, lb, dev.upload_u64(ch), d_out4, trace_offset=tau, lde_offset=h)
    got = eng.dev_download(d_out4, 4 * N).reshape(4, N)
    want = []
    for e in range(4):
        eng.dev_air_compose(air, d_lde, W, log_n, lb, dev.upload_u64(xc.weight_vector(ch, e)), d_out, trace_offset=tau, lde_offset=h)
        want.append(eng.dev_download(d_out, N))
    return got, want


def _airs(p, n):
    yield "fib", ac.make("fib", n, p)
    yield "mixer", ac.make("mixer", n, p)
    yield "empty", ac.make("empty", n, p)
    yield "mimc", ap.make("mimc", n, p)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_compose_ext_coordinate_e_is_compose_under_weights_e(engines, p, g):
    """2^16 rows x blowup 8 = 2^19 points, T = 1024 and four points per thread"""
    eng, log_n, lb = engines[p], 16, 3
    for name, (air, cols) in _airs(p, 1 << log_n):
        ch = xc.ext_weights_for(air)
        ch[0], ch[5] = U64_MAX, p
        with Dev(eng) as dev:
            got, want = gpu_compose_pair(eng, dev, air, cols, ch, log_n, lb, 1, g)
        for e in range(4):
            assert np.array_equal(got[e], want[e]), (name, e)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_compose_ext_wide_rows(engines, p, g):
    """W = 64 at 2^16 rows x blowup 8 = 2^19 points: the smallest tile, one point per thread, several inversion batches"""
    eng, log_n, lb = engines[p], 16, 3
    air, cols = ar.wide(64, 20, p, 1 << log_n)
    ch = xc.ext_weights_for(air)
    with Dev(eng) as dev:
        got, want = gpu_compose_pair(eng, dev, air, cols, ch, log_n, lb, 5, 7)
    for e in range(4):
        assert np.array_equal(got[e], want[e]), e


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_compose_ext_two_points_per_thread(engines, p, g):
    """W = 20 at blowup 8: twenty tile rows fit a tile of 512 points and no larger one -- air_compose_ext_kernel<2>"""
    eng, log_n, lb = engines[p], 13, 3
    air, cols = ar.wide(20, 8, p, 1 << log_n)
    ch = xc.ext_weights_for(air)
    with Dev(eng) as dev:
        got, want = gpu_compose_pair(eng, dev, air, cols, ch, log_n, lb, 1, g)
    for e in range(4):
        assert np.array_equal(got[e], want[e]), e


@pytest.mark.parametrize("case", ["no_tile_fits", "odd_stride", "unaligned_base"])
def test_compose_ext_without_tiles(engines, case):
    import torch
    p, g = xc.PRIMES[0]
    eng = engines[p]
    if case == "no_tile_fits":
        log_n, lb = 6, 8
        air, cols = ac.synthetic(64, 32, p, 1 << log_n)
    else:
        log_n, lb = 10, 3
        air, cols = ac.make("wide4", 1 << log_n, p)
    W, N = len(cols), 1 << (log_n + lb)
    ch = xc.ext_weights_for(air)
    with Dev(eng) as dev:
        d_trace, d_lde = dev.upload(np.array(cols, dtype=np.uint64)), dev.alloc(4 * W * N)
        eng.dev_lde(d_trace, W, log_n, lb, d_lde)
        lde = eng.dev_download(d_lde, W * N).astype(np.uint32).reshape(W, N)
    stride, lead = (N + 1, 0) if case == "odd_stride" else (N, 1 if case == "unaligned_base" else 0)
    t_lde, d_lde = _dev_cols(lde, stride, lead)
    out_stride = N + 3
    t_out = torch.zeros(4 * out_stride, dtype=torch.int32, device="cuda")
    t_one = torch.zeros(N, dtype=torch.int32, device="cuda")
    t_w, d_w = _dev_u64(ch)
    torch.cuda.synchronize()
    eng.dev_air_compose_ext(air, d_lde, W, log_n, lb, d_w, t_out.data_ptr(), stride=stride, out_stride=out_stride)
    eng.sync()
    got = t_out.cpu().numpy().view(np.uint32)
    for e in range(4):
        t_we, d_we = _dev_u64(xc.weight_vector(ch, e))
        torch.cuda.synchronize()
        eng.dev_air_compose(air, d_lde, W, log_n, lb, d_we, t_one.data_ptr(), stride=stride)
        eng.sync()
        assert np.array_equal(got[e * out_stride:e * out_stride + N], t_one.cpu().numpy().view(np.uint32)), e


def test_compose_ext_headline_shape_equals_the_mirror_at_sampled_points(engines):
    """n = 2^22, W = 4, B = 8 on 469762049: 4096 sampled points against mirror.Air.compose_at under each weight vector"""
    import torch
    p, g = xc.PRIMES[1]
    eng, log_n, lb, W = engines[p], 22, 3, 4
    n, N, B = 1 << log_n, 1 << (log_n + lb), 1 << lb
    air, _ = ac.make("mixer", 64, p)
    air.boundaries = [(c, (n - 1 if r == 63 else r), v) for (c, r, v) in air.boundaries]
    ch = xc.ext_weights_for(air)
    rng = np.random.default_rng(22)
    dev = torch.device("cuda:0")
    trace = torch.from_numpy(rng.integers(0, p, (W, n), dtype=np.int64).astype(np.int32)).to(dev)
    lde, out = torch.empty((W, N), dtype=torch.int32, device=dev), torch.empty((4, N), dtype=torch.int32, device=dev)
    t_w, d_w = _dev_u64(ch)
    torch.cuda.synchronize()
    eng.dev_lde(trace.data_ptr(), W, log_n, lb, lde.data_ptr())
    eng.dev_air_compose_ext(air, lde.data_ptr(), W, log_n, lb, d_w, out.data_ptr())
    eng.sync()
    idx = np.unique(np.concatenate([rng.integers(0, N, 4200), [0, 1, B - 1, B, N // 2, N - B - 1, N - B, N - 1]]))
    assert len(idx) >= 4096                                  # distinct points
    ti = torch.from_numpy(idx).to(dev)
    cur = lde[:, ti].cpu().numpy().view(np.uint32)
    nxt = lde[:, (ti + B) % N].cpu().numpy().view(np.uint32)
    got = out[:, ti].cpu().numpy().view(np.uint32)
    wN = pow(g, (p - 1) // N, p)
    for e in range(4):
        we = xc.weight_vector(ch, e)
        for q, i in enumerate(idx):
            want = air.compose_at(p, log_n, lb, 1, g, wN, int(i), [int(v) for v in cur[:, q]], [int(v) for v in nxt[:, q]], we)
            assert int(got[e, q]) == want, (e, int(i))


# ---------------------------------------------------------------------------------------------- the AIR proof
def restated_air_proof(o, air, cols, p, g, log_n, lb, t, tau, h, E):
    """-> (row root, proof bytes, top) of smi_dev_air_prove_ext from the oracle's primitives"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K = len(cols), len(air.constraints)
    lde = ac.lde(o, cols, p, g, log_n, lb, tau, h)
    nodes = o.merkle_new(ar.row_leaves(o, lde))
    root = bytes(nodes[-1])
    tr, ch = xc.air_transcript(o, W, K, root)
    if log_n <= 8:      # the polynomial route proper; beyond it the same polynomials through the oracle's fast transforms
        cw = [ap.route(o, air, cols, xc.weight_vector(ch, e), p, g, log_n, lb, tau, h)[0] for e in range(4)]
    else:
        cw = [ap.fast_route(o, air, cols, xc.weight_vector(ch, e), p, g, log_n, lb, tau, h) for e in range(4)]
    cw = np.stack([np.asarray(c, dtype=np.uint64) for c in cw])
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    fri, top = xc.prove(o, cfg_o, cw, g, tr)
    return root, fri + ar.openings_bytes(o, lde, top, N, B, K > 0, nodes), top


def _air_cases(p, n):
    yield "fib", ac.make("fib", n, p)
    yield "mixer", ac.make("mixer", n, p)
    yield "mimc", ap.make("mimc", n, p)
    yield "wide", ar.wide(12, 5, p, n)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", range(8, 13))
def test_air_prove_ext_bytes_equal_the_restatement_and_verify_accepts(engines, oracle, p, g, log_n):
    eng, lb, t = engines[p], 3, 4
    for name, (air, cols) in _air_cases(p, 1 << log_n):
        W = len(cols)
        _d, E = eng.air_plan(air, W, log_n, lb)
        with Dev(eng) as dev:
            res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, row_leaves=True, ext=True)
        root, want, top = restated_air_proof(oracle, air, cols, p, g, log_n, lb, t, 1, g, E)
        assert bytes(res["column_roots"][0]) == root, name
        assert res["top_indices"] == top, name
        assert res["proof"] == want, name
        ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True)
        assert ok, (name, why)
        ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, row_leaves=True)
        assert not ok and why, name                   # the rows verifier rejects an ext proof


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_air_verify_ext_rejections(engines, p, g):
    eng, log_n, lb, t = engines[p], 9, 3, 8
    n = 1 << log_n
    air, cols = ac.make("mixer", n, p)
    W = len(cols)
    kw = dict(row_leaves=True, ext=True)
    with Dev(eng) as dev:
        res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, **kw)
        rows = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, row_leaves=True)
        bad_cols = [list(c) for c in cols]
        bad_cols[1][n // 3] = (bad_cols[1][n // 3] + 1) % p                 # one cell of the trace changed
        cheat = eng.dev_air_prove(air, dev.upload(np.array(bad_cols, dtype=np.uint64)), W, log_n, lb, t, check=False, **kw)
    roots, proof = res["column_roots"], res["proof"]
    assert eng.air_verify(air, proof, roots, W, log_n, lb, t, **kw)[0]
    ok, why = eng.air_verify(air, cheat["proof"], cheat["column_roots"], W, log_n, lb, t, **kw)
    assert not ok and why
    ok, why = eng.air_verify(air, rows["proof"], rows["column_roots"], W, log_n, lb, t, **kw)
    assert not ok and why                                                   # a prove_rows proof
    assert eng.air_verify(air, rows["proof"], rows["column_roots"], W, log_n, lb, t, row_leaves=True)[0]
    # an honest proof under an AIR that differs in one boundary value / one coefficient
    other, _ = ac.make("mixer", n, p)
    c, r, v = other.boundaries[0]
    other.boundaries[0] = (c, r, (v + 1) % p)
    assert not eng.air_verify(other, proof, roots, W, log_n, lb, t, **kw)[0]
    other, _ = ac.make("mixer", n, p)
    cf, factors = other._symbolic[1][-1]
    other._symbolic[1][-1] = (cf + 1, factors)
    assert not eng.air_verify(other, proof, roots, W, log_n, lb, t, **kw)[0]
    # ... and in one periodic value
    pair, pcols = ap.make("mimc", n, p)
    with Dev(eng) as dev:
        pres = eng.dev_air_prove(pair, dev.upload(np.array(pcols, dtype=np.uint64)), len(pcols), log_n, lb, t, **kw)
    assert eng.air_verify(pair, pres["proof"], pres["column_roots"], len(pcols), log_n, lb, t, **kw)[0]
    pair.periodics[0][3] = (pair.periodics[0][3] + 1) % p
    ok, why = eng.air_verify(pair, pres["proof"], pres["column_roots"], len(pcols), log_n, lb, t, **kw)
    assert not ok and "composition" in why
    # a flipped byte in the opening section, a truncated proof, another root
    bad = bytearray(proof)
    bad[-5] ^= 1
    assert not eng.air_verify(air, bytes(bad), roots, W, log_n, lb, t, **kw)[0]
    assert not eng.air_verify(air, proof[:-1], roots, W, log_n, lb, t, **kw)[0]
    assert not eng.air_verify(air, proof, [bytes(32)], W, log_n, lb, t, **kw)[0]
    import stark_rs_amd as s
    with pytest.raises(s.StarkMiError, match="row_leaves"):
        eng.air_verify(air, proof, roots, W, log_n, lb, t, ext=True)


def test_air_prove_ext_headline_shape_is_accepted(engines):
    """2^22 x 4, B = 8, t = 32 on the second prime: accepted, and the proof has the expected length"""
    import torch
    p, g = xc.PRIMES[1]
    eng, log_n, lb, t, W = engines[p], 22, 3, 32, 4
    n, N = 1 << log_n, 1 << (log_n + lb)
    # the mixer's columns a, b, c by a device scan would be a test of its own: a satisfiable AIR of this length whose trace
    # numpy builds quickly is the wide one (x' = x y + const) with K = 1 on four columns
    rng = np.random.default_rng(1)
    y = rng.integers(0, p, n, dtype=np.int64)
    xv, yl, xs = 5, y.tolist(), [5]
    for r in range(n - 1):
        xv = (xv * yl[r] + 1) % p
        xs.append(xv)
    x = np.array(xs, dtype=np.int64)
    cols = np.stack([x, y, rng.integers(0, p, n, dtype=np.int64), rng.integers(0, p, n, dtype=np.int64)])
    from stark_rs_amd.mirror import Air
    air = Air(W)
    air.transition({("next", 0): 1, (("cur", 0), ("cur", 1)): -1, (): -1})
    air.boundary(0, 0, 5).boundary(3, n - 1, int(cols[3][n - 1]))
    _d, E = eng.air_plan(air, W, log_n, lb)
    trace = torch.from_numpy(cols.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    res = eng.dev_air_prove(air, trace.data_ptr(), W, log_n, lb, t, row_leaves=True, ext=True, timed=True)
    cfg = eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t)
    R = eng.fri_num_rounds(cfg)
    assert len(res["proof"]) == xc.proof_len(N, E, t, R) + ar.opening_len(W, 1, log_n + lb, t)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True)
    assert ok, why
    print("stage_ms", res["stage_ms"])
