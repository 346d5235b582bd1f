"""GPU: the AIR entry points (smi_dev_air_compose / _check / _prove, smi_air_verify) against the oracle's polynomial
route, the CPU emulator, the Python mirror and the op-for-op oracle composition of Fri::prove with a caller's
transcript.  Every comparison is exact.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import transcript_compose as tc

pytestmark = pytest.mark.gpu

COMPOSITION = "air openings: the composition of the opened rows is not the codeword value"
# smi_stark_verify reads an AIR proof at expansion factor 8 where the prover ran FRI at 4: the last codeword (checked
# before any query) has twice the degree that bound allows
STARK_VERIFY_REASON = "last codeword does not correspond to polynomial of low enough degree"


@pytest.fixture(scope="module")
def engines():
    import stark_rs_amd as s
    es = {p: s.Engine(p, g, 0) for p, g in ac.PRIMES}
    yield es
    for e in es.values():
        e.close()


class Dev:
    """device buffers of one test, freed on exit"""

    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def alloc(self, nbytes):
        self.ptrs.append(self.eng.dev_alloc(nbytes))
        return self.ptrs[-1]

    def upload(self, values):
        v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64)).reshape(-1)
        d = self.alloc(4 * v.size)
        self.eng.dev_upload(v, d)
        return d

    def upload_u64(self, values):
        """raw u64 words (the unreduced weights) through a torch tensor: dev_upload narrows to residues"""
        import torch
        self.keep = getattr(self, "keep", []) + [torch.from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).cuda()]
        torch.cuda.synchronize()
        return self.keep[-1].data_ptr()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.sync()
        for d in self.ptrs:
            self.eng.dev_free(d)


def gpu_compose(eng, dev, air, cols, wts, log_n, lb, tau, h):
    """trace columns -> smi_dev_lde -> smi_dev_air_compose; -> (codeword, device pointer of the extended columns)"""
    W, N = len(cols), 1 << (log_n + lb)
    d_trace = dev.upload(np.array(cols, dtype=np.uint64))
    d_lde, d_out = dev.alloc(4 * W * N), dev.alloc(4 * N)
    eng.dev_lde(d_trace, W, log_n, lb, d_lde, trace_offset=tau, lde_offset=h)
    eng.dev_air_compose(air, d_lde, W, log_n, lb, dev.upload_u64(wts), d_out, trace_offset=tau, lde_offset=h)
    return eng.dev_download(d_out, N), d_lde


@pytest.mark.parametrize("name", ["mixer", "fib", "wide4", "empty"])
@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("lb,tau,h", [(3, 1, None), (4, 5, 7)])
def test_compose_equals_the_polynomial_route(engines, oracle, name, p, g, lb, tau, h):
    eng, log_n = engines[p], 10
    h = g if h is None else h
    air, cols = ac.make(name, 1 << log_n, p)
    wts = ac.weights_for(air)
    want, _ = ac.codeword_poly_route(oracle, air, cols, wts, p, g, log_n, lb, tau, h)
    with Dev(eng) as dev:
        got, _ = gpu_compose(eng, dev, air, cols, wts, log_n, lb, tau, h)
    assert np.array_equal(got, np.asarray(want, dtype=np.uint64))


def _emu():
    from stark_rs_amd import _lib
    L = C.CDLL(_lib.EMU_PATH)
    L.emu_air_compose.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.c_void_p, C.c_int]
    return L


@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("shape", ["w4", "w64"])
def test_compose_equals_the_emulator(engines, p, g, shape):
    from stark_rs_amd import _lib
    eng, log_n, lb = engines[p], 16, 3
    n, N = 1 << log_n, 1 << (log_n + lb)
    if shape == "w4":
        air, _ = ac.make("wide4", 64, p)          # the constraints; the columns are random (no division by a zerofier here)
        cols = [[int(x) for x in np.random.default_rng(5).integers(0, p, n)] for _ in range(4)]
    else:
        air, cols = ac.synthetic(64, 32, p, n)
    W = len(cols)
    wts = ac.weights_for(air)
    with Dev(eng) as dev:
        got, d_lde = gpu_compose(eng, dev, air, cols, wts, log_n, lb, 1, g)
        lde = eng.dev_download(d_lde, W * N).astype(np.uint32)
    out, w = np.zeros(N, dtype=np.uint32), np.array(wts, dtype=np.uint64)
    cfg, a = _lib.StarkCfg(log_n, lb, W, 0, 1, g, 0, 1), air.flatten(p)
    assert _emu().emu_air_compose(p, g, C.byref(cfg), C.byref(a), lde.ctypes.data, N, w.ctypes.data, out.ctypes.data, 0) == 0
    assert np.array_equal(got, out.astype(np.uint64))


@pytest.mark.parametrize("case", ["no_tile_fits", "odd_stride", "unaligned_base"])
def test_compose_without_tiles_equals_the_emulator(engines, case):
    """the kernel smi_dev_air_compose takes when no tile of all columns fits in LDS (W = 64 at blowup 256), when the
    stride is not a multiple of 4, or when the columns are not 16-byte aligned"""
    import torch
    from stark_rs_amd import _lib
    p, g = ac.PRIMES[0]
    eng = engines[p]
    if case == "no_tile_fits":
        log_n, lb = 6, 8
        air, cols = ac.synthetic(64, 32, p, 1 << log_n)
    else:
        log_n, lb = 10, 3
        air, cols = ac.make("wide4", 1 << log_n, p)
    W, N = len(cols), 1 << (log_n + lb)
    wts = ac.weights_for(air)
    with Dev(eng) as dev:
        d_trace, d_lde = dev.upload(np.array(cols, dtype=np.uint64)), dev.alloc(4 * W * N)
        eng.dev_lde(d_trace, W, log_n, lb, d_lde)
        lde = eng.dev_download(d_lde, W * N).astype(np.uint32).reshape(W, N)
    stride, lead = (N + 1, 0) if case == "odd_stride" else (N, 1 if case == "unaligned_base" else 0)
    host = np.zeros(lead + W * stride, dtype=np.uint32)
    for c in range(W):
        host[lead + c * stride:lead + c * stride + N] = lde[c]
    t_lde = torch.from_numpy(host.view(np.int32)).cuda()
    t_w = torch.from_numpy(np.array(wts, dtype=np.uint64).view(np.int64)).cuda()
    t_out = torch.zeros(N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.dev_air_compose(air, t_lde.data_ptr() + 4 * lead, W, log_n, lb, t_w.data_ptr(), t_out.data_ptr(), stride=stride)
    eng.sync()
    got = t_out.cpu().numpy().view(np.uint32)
    want, w = np.zeros(N, dtype=np.uint32), np.array(wts, dtype=np.uint64)
    cfg, a, flat = _lib.StarkCfg(log_n, lb, W, 0, 1, g, 0, 1), air.flatten(p), np.ascontiguousarray(lde)
    assert _emu().emu_air_compose(p, g, C.byref(cfg), C.byref(a), flat.ctypes.data, N, w.ctypes.data, want.ctypes.data, 0) == 0
    assert np.array_equal(got, want)


def test_compose_headline_shape_equals_the_mirror_at_sampled_points(engines, oracle):
    """n = 2^22, W = 4, B = 8 on 469762049: 4096 sample indices, the operands gathered on the device from the
    smi_dev_lde output at those indices and B further on -- nothing of size N crosses to the host"""
    import torch
    p, g = ac.PRIMES[1]
    eng, log_n, lb, W = engines[p], 22, 3, 4
    n, N, B, T = 1 << log_n, 1 << (log_n + lb), 1 << lb, 1024
    air, _ = ac.make("mixer", 64, p)
    air.boundaries = [(c, (n - 1 if r == 63 else r), v) for (c, r, v) in air.boundaries]
    wts = ac.weights_for(air)
    rng = np.random.default_rng(22)
    dev = torch.device("cuda:0")
    trace = torch.from_numpy(rng.integers(0, p, (W, n), dtype=np.int64).astype(np.int32)).to(dev)
    lde, out = torch.empty((W, N), dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    w32 = torch.from_numpy(np.array(wts, dtype=np.uint64).view(np.int64)).to(dev)
    torch.cuda.synchronize()
    eng.dev_lde(trace.data_ptr(), W, log_n, lb, lde.data_ptr())
    eng.dev_air_compose(air, lde.data_ptr(), W, log_n, lb, w32.data_ptr(), out.data_ptr())
    eng.sync()
    fixed = [0, N - 1, T - 1, T, 5 * T - 1, 5 * T, N - T - 1, N - T] + list(range(N - B, N))
    idx = sorted(set(fixed + [int(x) for x in rng.integers(0, N, 4096 - len(fixed))]))
    ti = torch.tensor(idx, dtype=torch.int64, device=dev)
    cur, nxt, got = lde[:, ti].cpu().numpy(), lde[:, (ti + B) % N].cpu().numpy(), out[ti].cpu().numpy()
    _, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
    for j, i in enumerate(idx):
        want = air.compose_at(p, log_n, lb, 1, g, wN, i, [int(v) for v in cur[:, j]], [int(v) for v in nxt[:, j]], wts)
        assert int(got[j]) == want, i


def _prove(eng, dev, air, cols, log_n, lb, t, check=True):
    d_trace = dev.upload(np.array(cols, dtype=np.uint64))
    return eng.dev_air_prove(air, d_trace, len(cols), log_n, lb, t, check=check, timed=True)


def _split(res, W, K, log_N, t):
    R = 4 if K else 2
    ob = t * R * (9 + 8 * W) + t * W * R * (9 + 32 * log_N)
    return res["proof"][:len(res["proof"]) - ob], res["proof"][len(res["proof"]) - ob:]


@pytest.mark.parametrize("name", ["mixer", "wide4"])
@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_prove_bytes_equal_the_oracle_composition(engines, oracle, name, p, g):
    o, eng, log_n, lb, t = oracle, engines[p], 10, 3, 8
    N, B = 1 << (log_n + lb), 1 << lb
    air, cols = ac.make(name, 1 << log_n, p)
    W, K = air.n_cols, len(air.constraints)
    d, E = eng.air_plan(air, W, log_n, lb)
    assert (d, E) == (3, 4)
    with Dev(eng) as dev:
        res = _prove(eng, dev, air, cols, log_n, lb, t)
    lde = ac.lde(o, cols, p, g, log_n, lb, 1, g)
    roots = [o.merkle_commit(o.leaf_hashes(col)) for col in lde]
    assert [bytes(r) for r in res["column_roots"]] == roots
    prior, wts = ac.transcript(o, air, roots)
    assert len(prior) == 32 * W + 8 * K
    codeword, _ = ac.codeword_poly_route(o, air, cols, wts, p, g, log_n, lb, 1, g)
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    ocfg = o.fri_cfg(wN, g, N, E, t, p)
    want_fri, top = tc.prove(o, ocfg, codeword, prior)
    fri, opened = _split(res, W, K, log_n + lb, t)
    assert res["top_indices"] == [int(x) for x in top]
    assert fri == want_fri
    assert opened == ac.openings_bytes(o, lde, top, N, B, True)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t)
    assert ok, why
    ecfg = eng.fri_cfg(wN, g, N, E, t)
    ok, _pv, why, used = eng.fri_verify(ecfg, res["proof"], transcript=prior, want_consumed=True)
    assert ok and used == len(fri), why


def test_rejections(engines, oracle):
    o = oracle
    p, g = ac.PRIMES[0]
    eng, log_n, lb, t = engines[p], 10, 3, 8
    n, N = 1 << log_n, 1 << (log_n + lb)
    mixer, cols = ac.make("mixer", n, p)
    wide4, _ = ac.make("wide4", n, p)
    W, K = 4, 3
    with Dev(eng) as dev:
        res = _prove(eng, dev, mixer, cols, log_n, lb, t)
    proof, roots = res["proof"], res["column_roots"]
    verify = lambda air, pr, rt: eng.air_verify(air, pr, rt, W, log_n, lb, t)
    assert verify(mixer, proof, roots) == (True, "")
    fri, opened = _split(res, W, K, log_n + lb, t)
    rec = 9 + 8 * W

    def flipped(at):
        b = bytearray(proof)
        b[at] ^= 1
        return bytes(b)
    # a flipped opened value: this row (record 0 of test 0), then a next row (record 2)
    assert verify(mixer, flipped(len(fri) + 9), roots) == (False, "air openings: authentication path does not verify")
    assert verify(mixer, flipped(len(fri) + 2 * rec + 9 + 8), roots) == (False, "air openings: authentication path does not verify")
    # the value AND its leaf cannot both be forged: a flipped path digest is the same verdict
    assert verify(mixer, flipped(len(proof) - 1), roots) == (False, "air openings: authentication path does not verify")
    swapped = np.array(roots)[[1, 0, 2, 3]]
    # other roots, another transcript: other challenges and other sampled indices than the prover's
    assert verify(mixer, proof, swapped) == (False, "colinearity check failure")
    assert verify(mixer, proof[:-1], roots) == (False, "air openings: wrong length")
    assert verify(mixer, proof[:len(fri) + 2 * rec], roots) == (False, "air openings: wrong length")
    # K = 4: a 160-byte transcript where the prover had 152 bytes
    assert verify(wide4, proof, roots) == (False, "colinearity check failure")
    got = eng.stark_verify(proof, roots, W, log_n, lb, t, open_columns=True)
    print("stark_verify on an AIR proof:", got)
    assert got == (False, STARK_VERIFY_REASON)
    # a trace with one cell changed
    bad = [list(c) for c in cols]
    bad[1][500] = (bad[1][500] + 1) % p
    want = mixer.first_violation(p, bad)
    with Dev(eng) as dev:
        d_trace = dev.upload(np.array(bad, dtype=np.uint64))
        okc, con, row, sentence = eng.dev_air_check(mixer, d_trace, W, log_n)
        assert (okc, con, row) == (False,) + want
        assert f"rows {want[1]} and {want[1] + 1}" in sentence
        import stark_rs_amd as s
        with pytest.raises(s.StarkMiError, match=f"rows {want[1]} and {want[1] + 1}"):
            eng.dev_air_prove(mixer, d_trace, W, log_n, lb, t)
        res_bad = eng.dev_air_prove(mixer, d_trace, W, log_n, lb, t, check=False)
        okc, *_ = eng.dev_air_check(mixer, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n)
        assert okc
    # the prover folds honestly, so every layer is colinear; what the folding ends in is not of low degree
    got = verify(mixer, res_bad["proof"], res_bad["column_roots"])
    print("proof from a violating trace:", got)
    assert got == (False, "last codeword does not correspond to polynomial of low enough degree")
    fri_bad, _ = _split(res_bad, W, K, log_n + lb, t)
    prior, _ = ac.transcript(o, mixer, [bytes(r) for r in res_bad["column_roots"]])
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    assert tc.verify(o, o.fri_cfg(wN, g, N, 4, t, p), fri_bad, prior)[0] is False
    # a wrong boundary value comes before any transition violation
    bad[0][0] = (bad[0][0] + 1) % p
    with Dev(eng) as dev:
        okc, con, row, sentence = eng.dev_air_check(mixer, dev.upload(np.array(bad, dtype=np.uint64)), W, log_n)
    assert (okc, con, row) == (False, 0, 0) and "boundary point 0" in sentence
    with pytest.raises(Exception, match="row_leaves"):
        from stark_rs_amd import _lib
        cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, g, t, 1)
        a = mixer.flatten(p)
        eng._ck(eng.L.smi_air_verify(eng.h, C.byref(cfg), C.byref(a), np.array(roots).ctypes.data, proof, len(proof), C.byref(C.c_int())))


def _mixer_like(n, p, a0=5, b_coef=3, last_c_col=2, c_next=2, a_last=None):
    """the mixer AIR of tests/air_compose.py with one thing changed: same W, same K, same transcript"""
    from stark_rs_amd.mirror import Air
    air = Air(4)
    air.transition({("next", 0): 1, (("cur", 0), ("cur", 1)): -1, ("cur", 2): -1})
    air.transition({("next", 1): 1, (("cur", 0, 2), ("cur", 2)): -1, ("cur", 1): -b_coef})
    air.transition({("next", c_next): 1, ("cur", 2): -1, (): -1})
    air.boundary(0, 0, a0).boundary(1, 0, 11).boundary(2, 0, 0).boundary(last_c_col, n - 1, (n - 1) % p).boundary(0, n - 1, a_last)
    return air


@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_verifier_recomputes_the_composition(engines, p, g):
    """An honest mixer proof under another statement with the same W and K: the transcript, FRI and every path are
    the prover's, so only the recomputation of the codeword from the opened rows can refuse it -- and it does, for a
    boundary value, a boundary point's column, a coefficient and a next-row operand."""
    eng, log_n, lb, t = engines[p], 10, 3, 8
    n = 1 << log_n
    mixer, cols = ac.make("mixer", n, p)
    a_last = cols[0][-1]
    with Dev(eng) as dev:
        res = _prove(eng, dev, mixer, cols, log_n, lb, t)
    verify = lambda air: eng.air_verify(air, res["proof"], res["column_roots"], 4, log_n, lb, t)
    assert verify(mixer) == (True, "")
    assert verify(_mixer_like(n, p, a_last=a_last)) == (True, "")                     # the same statement, rebuilt
    assert verify(_mixer_like(n, p, a0=6, a_last=a_last)) == (False, COMPOSITION)     # a[0] = 6
    assert verify(_mixer_like(n, p, a_last=(a_last + 1) % p)) == (False, COMPOSITION)  # a[n-1] off by one
    assert verify(_mixer_like(n, p, b_coef=4, a_last=a_last)) == (False, COMPOSITION)  # b' = a^2 c + 4 b
    assert verify(_mixer_like(n, p, last_c_col=3, a_last=a_last)) == (False, COMPOSITION)   # c[n-1] = n-1 claimed of column 3
    assert verify(_mixer_like(n, p, c_next=3, a_last=a_last)) == (False, COMPOSITION)  # d' = c + 1: differs in a next-row operand only


def test_prove_and_verify_at_2_20(engines, oracle):
    o = oracle
    p, g = ac.PRIMES[1]
    eng, log_n, lb, t = engines[p], 20, 3, 32
    N = 1 << (log_n + lb)
    air, cols = ac.make("mixer", 1 << log_n, p)
    with Dev(eng) as dev:
        res = _prove(eng, dev, air, cols, log_n, lb, t)
    print("stage_ms", res["stage_ms"])
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], 4, log_n, lb, t)
    assert ok, why
    fri, _ = _split(res, 4, 3, log_n + lb, t)
    prior, _ = ac.transcript(o, air, [bytes(r) for r in res["column_roots"]])
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    okv, _pv, used = tc.verify(o, o.fri_cfg(wN, g, N, 4, t, p), fri, prior)
    assert okv and used == len(fri)
