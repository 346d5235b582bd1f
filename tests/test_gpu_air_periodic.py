"""GPU: periodic columns of the AIR through smi_dev_air_compose / _check / _prove and smi_air_verify, against the
oracle's polynomial route on the augmented AIR (tests/air_periodic.py), the CPU emulator, the Python mirror and the
op-for-op oracle composition of Fri::prove with the caller's transcript.  Every comparison is exact.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import transcript_compose as tc
from test_gpu_air import COMPOSITION, Dev, _emu, _prove, _split, engines, gpu_compose  # noqa: F401  (engines is a fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ap.NAMES)
@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("lb,tau,h", ap.CASES)
def test_compose_equals_the_augmented_polynomial_route(engines, oracle, name, p, g, lb, tau, h):
    eng, log_n = engines[p], 10
    h = g if h is None else h
    air, cols = ap.make(name, 1 << log_n, p)
    wts = ac.weights_for(air)
    want, _ = ap.route(oracle, air, cols, wts, p, g, log_n, lb, tau, h)
    with Dev(eng) as dev:
        got, _ = gpu_compose(eng, dev, air, cols, wts, log_n, lb, tau, h)
    assert np.array_equal(got, np.asarray(want, dtype=np.uint64))


def _emu_compose(air, lde, wts, p, g, log_n, lb):
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    out, w = np.zeros(N, dtype=np.uint32), np.array(wts, dtype=np.uint64)
    cfg, a, flat = _lib.StarkCfg(log_n, lb, len(lde), 0, 1, g, 0, 1), air.flatten(p), np.ascontiguousarray(lde)
    assert _emu().emu_air_compose(p, g, C.byref(cfg), C.byref(a), flat.ctypes.data, N, w.ctypes.data, out.ctypes.data, 0) == 0
    return out


@pytest.mark.parametrize("p,g", ac.PRIMES)
@pytest.mark.parametrize("W,Q,K", [(4, 2, 4), (56, 8, 24)])
def test_compose_equals_the_emulator(engines, p, g, W, Q, K):
    """2^16 rows x blowup 8: W + Q = 6 tile rows (T = 1024, four points per thread) and 64 (T = 128, one)"""
    eng, log_n, lb = engines[p], 16, 3
    N = 1 << (log_n + lb)
    air, cols = ap.synthetic(W, Q, K, p, 1 << log_n)
    wts = ac.weights_for(air)
    with Dev(eng) as dev:
        got, d_lde = gpu_compose(eng, dev, air, cols, wts, log_n, lb, 1, g)
        lde = eng.dev_download(d_lde, W * N).astype(np.uint32).reshape(W, N)
    assert np.array_equal(got, _emu_compose(air, lde, wts, p, g, log_n, lb).astype(np.uint64))


@pytest.mark.parametrize("case", ["no_tile_fits", "odd_stride", "unaligned_base"])
def test_compose_without_tiles_equals_the_emulator(engines, case):
    """the three ways into the kernel without tiles, which reads the periodic tables from memory modulo their length"""
    import torch
    p, g = ac.PRIMES[0]
    eng = engines[p]
    if case == "no_tile_fits":
        log_n, lb = 6, 8
        air, cols = ap.synthetic(56, 8, 24, p, 1 << log_n)
    else:
        log_n, lb = 10, 3
        air, cols = ap.make("public", 1 << log_n, p)
        sw, _ = ap.make("switch", 1 << log_n, p)
        j = air.periodic(sw.periodics[0])
        air.transition({("next", 3): 1, (("per", j), ("cur", 3)): -1, (("per_next", j), ("cur", 0), ("cur", 1)): -1})
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
    assert np.array_equal(got, _emu_compose(air, lde, wts, p, g, log_n, lb))


def test_compose_headline_shape_equals_the_augmented_air_and_the_mirror(engines, oracle):
    """n = 2^22, W = 4, B = 8 on 469762049 with Q = 4 (periods 64, 64, 2, n).  The whole codeword against
    smi_dev_air_compose of the augmented AIR (W = 8, weight 0 on the last four): tables read modulo their length against
    committed-style extended columns.  4096 sampled points against mirror.Air.compose_at, whose periodic operands come
    from the oracle's fast LDE of the tiled columns -- nothing of the library under test"""
    import torch
    o = oracle
    p, g = ac.PRIMES[1]
    eng, log_n, lb, W, Q = engines[p], 22, 3, 4, 4
    n, N, B, T = 1 << log_n, 1 << (log_n + lb), 1 << lb, 1024
    air = ap.lanes([64, 64, 2, n], p)
    wts = ac.weights_for(air)
    rng = np.random.default_rng(22)
    cols = rng.integers(0, p, (W, n), dtype=np.int64)
    tiled = np.stack([np.resize(np.array(v, dtype=np.int64), n) for v in air.periodics])
    aug = air.with_periodic_as_trace()
    awts = wts[:W] + [0] * Q + wts[W:]
    dev = torch.device("cuda:0")
    trace = torch.from_numpy(np.concatenate([cols, tiled]).astype(np.int32)).to(dev)
    lde = torch.empty((W + Q, N), dtype=torch.int32, device=dev)
    out, out_aug = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    w32 = torch.from_numpy(np.array(wts, dtype=np.uint64).view(np.int64)).to(dev)
    aw32 = torch.from_numpy(np.array(awts, dtype=np.uint64).view(np.int64)).to(dev)
    torch.cuda.synchronize()
    eng.dev_lde(trace.data_ptr(), W + Q, log_n, lb, lde.data_ptr())
    eng.dev_air_compose(air, lde.data_ptr(), W, log_n, lb, w32.data_ptr(), out.data_ptr())
    eng.dev_air_compose(aug, lde.data_ptr(), W + Q, log_n, lb, aw32.data_ptr(), out_aug.data_ptr())
    eng.sync()
    assert torch.equal(out, out_aug)
    fixed = [0, N - 1, T - 1, T, 5 * T - 1, 5 * T, N - T - 1, N - T] + list(range(N - B, N)) + [64 * B - 1, 64 * B, 2 * B - 1, 2 * B]
    idx = sorted(set(fixed + [int(x) for x in rng.integers(0, N, 4096 - len(fixed))]))
    ti = torch.tensor(idx, dtype=torch.int64, device=dev)
    cur, nxt, got = lde[:W, ti].cpu().numpy(), lde[:W, (ti + B) % N].cpu().numpy(), out[ti].cpu().numpy()
    del lde, out_aug, trace
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    at, at_next = np.array(idx), (np.array(idx) + B) % N
    pc, pn = [], []
    for j in range(Q):
        ext = o.fast_coset_ntt(o.fast_intt(tiled[j].astype(np.uint64), w, 1, p), N, wN, g, p)
        pc.append(ext[at])
        pn.append(ext[at_next])
    for k, i in enumerate(idx):
        want = air.compose_at(p, log_n, lb, 1, g, wN, i, [int(v) for v in cur[:, k]], [int(v) for v in nxt[:, k]], wts,
                              per_cur=[int(c[k]) for c in pc], per_nxt=[int(c[k]) for c in pn])
        assert int(got[k]) == want, i


@pytest.mark.parametrize("name", ap.NAMES)
@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_check_with_periodic_columns(engines, name, p, g):
    eng, log_n = engines[p], 10
    n = 1 << log_n
    air, cols = ap.make(name, n, p)
    nb = len(air.boundaries)
    bad = [list(c) for c in cols]
    bad[0][500] = (bad[0][500] + 1) % p
    want = air.first_violation(p, bad)
    other, _ = ap.make(name, n, p)
    other.periodics[0][0] += 1
    want_other = other.first_violation(p, cols)
    assert want is not None and want[0] >= nb and want_other is not None and want_other[0] >= nb
    with Dev(eng) as dev:
        d_good, d_bad = dev.upload(np.array(cols, dtype=np.uint64)), dev.upload(np.array(bad, dtype=np.uint64))
        assert eng.dev_air_check(air, d_good, len(cols), log_n) == (True, None, None, "")
        okc, con, row, sentence = eng.dev_air_check(air, d_bad, len(cols), log_n)
        assert (okc, con, row) == (False,) + want
        assert sentence == f"air_check: transition constraint {want[0] - nb} is violated on rows {want[1]} and {want[1] + 1}"
        okc, con, row, sentence = eng.dev_air_check(other, d_good, len(cols), log_n)
        assert (okc, con, row) == (False,) + want_other
        assert f"rows {want_other[1]} and {want_other[1] + 1}" in sentence


@pytest.mark.parametrize("name,log_n", [("mimc", 10), ("mimc", 16), ("switch", 10), ("public", 10)])
@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_prove_bytes_equal_the_oracle_composition(engines, oracle, name, log_n, p, g):
    """The column roots are the oracle's; the FRI part is byte for byte what the oracle's Fri::prove writes for the
    route's codeword after the 32 W + 8 K-byte transcript; the total length is the documented layout for W columns:
    nothing about the periodic columns is in the proof.  At 2^16 rows the route is air_periodic.fast_route (the schoolbook
    products of codeword_poly_route do not reach that length; the CPU tests pin the one to the other)."""
    o, eng, lb, t = oracle, engines[p], 3, 8
    N, B = 1 << (log_n + lb), 1 << lb
    air, cols = ap.make(name, 1 << log_n, p)
    W, K = air.n_cols, len(air.constraints)
    assert eng.air_plan(air, W, log_n, lb) == (3, 4)
    with Dev(eng) as dev:
        res = _prove(eng, dev, air, cols, log_n, lb, t, check=True)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t)
    assert ok, why
    lde = ac.lde(o, cols, p, g, log_n, lb, 1, g)
    roots = [o.merkle_commit(o.leaf_hashes(col)) for col in lde]
    assert [bytes(r) for r in res["column_roots"]] == roots
    prior, wts = ac.transcript(o, air, roots)
    assert len(prior) == 32 * W + 8 * K
    if log_n <= 10:
        codeword, _ = ap.route(o, air, cols, wts, p, g, log_n, lb, 1, g)
    else:
        codeword = ap.fast_route(o, air, cols, wts, p, g, log_n, lb, 1, g)
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    want_fri, top = tc.prove(o, o.fri_cfg(wN, g, N, 4, t, p), codeword, prior)
    fri, opened = _split(res, W, K, log_n + lb, t)
    assert len(res["proof"]) == len(want_fri) + t * 4 * (9 + 8 * W) + t * W * 4 * (9 + 32 * (log_n + lb))
    assert res["top_indices"] == [int(x) for x in top]
    assert fri == want_fri
    assert opened == ac.openings_bytes(o, lde, top, N, B, True)


def _mimc_like(n, p, change=None):
    air, cols = ap.make("mimc", n, p)
    if change == "value":
        air.periodics[0][17] = (air.periodics[0][17] + 1) % p
    elif change == "half":
        air.periodics[0] = air.periodics[0][:32]
    elif change == "next":
        from stark_rs_amd.mirror import Air
        moved = Air(1)
        k = moved.periodic(air.periodics[0])
        moved.transition({("next", 0): 1, ("cur", 0, 3): -1, (("cur", 0, 2), ("per_next", k)): -3, (("cur", 0), ("per", k, 2)): -3, ("per", k, 3): -1})
        moved.boundaries = list(air.boundaries)
        air = moved
    return air, cols


@pytest.mark.parametrize("p,g", ac.PRIMES)
def test_verifier_recomputes_the_periodic_operands(engines, p, g):
    """An honest proof under a statement that differs in one thing about a periodic column: W, K, the transcript, FRI
    and every path are the prover's, so only the recomputation of the codeword from the opened rows and the
    statement's own periodic values can refuse it"""
    import stark_rs_amd as s
    eng, log_n, lb, t = engines[p], 10, 3, 8
    n = 1 << log_n
    mimc, cols = _mimc_like(n, p)
    with Dev(eng) as dev:
        res = _prove(eng, dev, mimc, cols, log_n, lb, t)
    verify = lambda air, r=res, W=1: eng.air_verify(air, r["proof"], r["column_roots"], W, log_n, lb, t)
    assert verify(mimc) == (True, "")
    assert verify(_mimc_like(n, p)[0]) == (True, "")                         # the same statement, rebuilt
    assert verify(_mimc_like(n, p, "value")[0]) == (False, COMPOSITION)      # one round constant changed
    assert verify(_mimc_like(n, p, "next")[0]) == (False, COMPOSITION)       # one periodic operand moved to the next row
    assert verify(_mimc_like(n, p, "half")[0]) == (False, COMPOSITION)       # period 64 replaced by its first 32 values
    # switch: the selector's value, its row, and the respelling [1, 0] -> [1, 0, 1, 0], which is the same statement
    switch, scols = ap.make("switch", n, p)
    with Dev(eng) as dev:
        sres = _prove(eng, dev, switch, scols, log_n, lb, t)
    sverify = lambda air: verify(air, sres, 2)
    assert sverify(switch) == (True, "")
    respelt, _ = ap.make("switch", n, p)
    respelt.periodics[0] = respelt.periodics[0] * 2
    assert respelt.flatten(p)._keep[8][0] == 2
    assert sverify(respelt) == (True, "")
    flipped, _ = ap.make("switch", n, p)
    flipped.periodics[0] = [0, 1]
    assert sverify(flipped) == (False, COMPOSITION)
    changed, _ = ap.make("switch", n, p)
    changed.periodics[0] = [1, 2]
    assert sverify(changed) == (False, COMPOSITION)
    # a trace with one cell changed
    bad = [list(c) for c in cols]
    bad[0][500] = (bad[0][500] + 1) % p
    want = mimc.first_violation(p, bad)
    with Dev(eng) as dev:
        d_trace = dev.upload(np.array(bad, dtype=np.uint64))
        with pytest.raises(s.StarkMiError, match=f"rows {want[1]} and {want[1] + 1}"):
            eng.dev_air_prove(mimc, d_trace, 1, log_n, lb, t)
        res_bad = eng.dev_air_prove(mimc, d_trace, 1, log_n, lb, t, check=False)
    got = verify(mimc, res_bad)
    print("proof from a violating trace:", got)
    assert got[0] is False
