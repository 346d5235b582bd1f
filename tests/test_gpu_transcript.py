"""GPU: smi_fri_*_fs -- Fri::commit / Fri::prove / Fri::verify continuing the caller's FiatShamir (src/fri.rs:105-110,
250-255, 313-318) -- against the oracle composition of tests/transcript_compose.py, byte for byte.  The priors cover
both device paths: a transcript of whole 32-byte chunks (phase 0: the fused Fiat-Shamir sites and the fused tail run
as for a fresh transcript, from another seed) and any other length (phase != 0: a phase-aware single-lane round after
every tree, no fused tail).  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import transcript_compose as tc
from test_transcript_host import REF_CASES, _prior, low_degree_case, ref_case

pytestmark = pytest.mark.gpu

P, G = 998244353, 3
P2, G2 = 469762049, 3
PRIORS = [0, 8, 31, 32, 33, 64, 100, 4099]


@pytest.fixture(scope="module")
def eng():
    import stark_rs_amd as s
    e = s.Engine(P, G, 0)
    yield e
    e.close()


def _cfg(eng, ocfg):
    return eng.fri_cfg(int(ocfg.omega), int(ocfg.offset), int(ocfg.domain_length), int(ocfg.expansion_factor),
                       int(ocfg.num_colinearity_tests))


def _cases(o):
    return [ref_case(o, *c) for c in REF_CASES] + [low_degree_case(o, 12), low_degree_case(o, 14, 4, 24, 7)]


def test_prove_with_prior_is_the_composition(eng, oracle):
    o = oracle
    for ocfg, cw in _cases(o):
        cfg = _cfg(eng, ocfg)
        for n in PRIORS:
            prior = _prior(n)
            want, want_top = tc.prove(o, ocfg, cw, prior)
            got, top = eng.fri_prove(cfg, cw, prior)
            assert got == want and top == want_top, (int(ocfg.domain_length), n)


@pytest.mark.parametrize("prior_len", [64, 37])
def test_prove_with_prior_large_codeword(eng, oracle, prior_len):
    """2^21: the four-leaves-per-lane kernel with LEAF_FOLD, the chunk kernel, and (prior 64) its Fiat-Shamir epilogue
    and the fused tail; (prior 37) the same trees with the phase-aware round after each."""
    o = oracle
    ocfg, cw = low_degree_case(o, 21, 8, 16, 3, seed=21)
    prior = _prior(prior_len)
    want, want_top = tc.prove(o, ocfg, cw, prior)
    got, top = eng.fri_prove(_cfg(eng, ocfg), cw, prior)
    assert got == want and top == want_top


def test_prove_2_23_on_p2_with_prior_is_accepted_by_the_composition(oracle):
    import stark_rs_amd as s
    o = oracle
    e2 = s.Engine(P2, G2, 0)
    try:
        ocfg, cw = low_degree_case(o, 23, 8, 32, 3, seed=23, p=P2)
        prior = _prior(37)
        proof, top = e2.fri_prove(_cfg(e2, ocfg), cw, prior)
        ok, pv, used = tc.verify(o, ocfg, proof, prior)
        assert ok and used == len(proof)
        assert [i for i, _ in pv[::2]] == [x % (len(cw) // 2) for x in top]
        assert all(cw[i] == v for i, v in pv)
        assert not tc.verify(o, ocfg, proof)[0]
    finally:
        e2.close()


def test_empty_prior_is_the_fresh_entry_point(eng, oracle):
    o = oracle
    ocfg, cw = low_degree_case(o, 12)
    cfg = _cfg(eng, ocfg)
    want, want_top = eng.fri_prove(cfg, cw)
    c = np.ascontiguousarray(cw, dtype=np.uint64)
    proof, plen = C.c_void_p(), C.c_size_t()
    top = np.zeros(int(cfg.num_colinearity_tests), dtype=np.uint64)
    assert eng.L.smi_fri_prove_fs(eng.h, C.byref(cfg), None, 0, c.ctypes.data, len(c), C.byref(proof), C.byref(plen), top.ctypes.data) == 0
    got = C.string_at(proof, plen.value)
    eng.L.smi_free(proof)
    assert got == want and [int(v) for v in top] == want_top
    # a NULL transcript with a length is a bad argument
    assert eng.L.smi_fri_prove_fs(eng.h, C.byref(cfg), None, 5, c.ctypes.data, len(c), C.byref(proof), C.byref(plen), top.ctypes.data) == -50


@pytest.mark.parametrize("prior_len", [0, 32, 33, 100])
def test_commit_with_prior_is_the_composition(eng, oracle, prior_len):
    o = oracle
    for ocfg, cw in _cases(o)[2:]:
        prior = _prior(prior_len)
        stream, _cws, _trees, wroots, walphas = tc.commit(o, ocfg, cw, prior)
        roots, alphas, last = eng.fri_commit(_cfg(eng, ocfg), cw, prior)
        assert [bytes(r) for r in roots] == wroots and alphas == walphas
        assert tc._elems(last) == stream[33 * len(wroots):]


@pytest.mark.parametrize("prior_len", [32, 37])
def test_device_codeword_with_prior(eng, oracle, prior_len):
    o = oracle
    ocfg, cw = low_degree_case(o, 14)
    prior = _prior(prior_len)
    d = eng.dev_alloc(len(cw) * 4)
    try:
        eng.dev_upload(cw, d)
        got, top = eng.dev_fri_prove(_cfg(eng, ocfg), d, len(cw), prior)
    finally:
        eng.dev_free(d)
    want, want_top = tc.prove(o, ocfg, cw, prior)
    assert got == want and top == want_top


@pytest.mark.parametrize("prior_len", [8, 32, 33, 4099])
def test_verify_with_prior(eng, oracle, prior_len):
    o = oracle
    for ocfg, cw in (_cases(o)[1], _cases(o)[4]):
        cfg = _cfg(eng, ocfg)
        prior = _prior(prior_len)
        proof, _top = eng.fri_prove(cfg, cw, prior)
        ok_w, pv_w, used_w = tc.verify(o, ocfg, proof, prior)
        assert ok_w and used_w == len(proof)
        ok, pv, why, consumed = eng.fri_verify(cfg, proof, prior, want_consumed=True)
        assert ok, why
        assert pv == pv_w and consumed == len(proof)
        # the wrong transcript: none, or one byte flipped
        assert not eng.fri_verify(cfg, proof)[0]
        bad = bytearray(prior)
        bad[len(bad) // 2] ^= 1
        ok_b, _pv, _why, used_b = eng.fri_verify(cfg, proof, bytes(bad), want_consumed=True)
        assert not ok_b and used_b == 0
        # a caller's stream that goes on after Fri::verify's objects
        more = proof + tc._elems([1, 2, 3])
        ok_m, _pv, _why, consumed_m = eng.fri_verify(cfg, more, prior, want_consumed=True)
        assert ok_m and consumed_m == len(proof)


def test_mirror_continues_a_non_empty_fiat_shamir(oracle):
    import stark_rs_amd.mirror as m
    o = oracle
    f = m.FiniteField(P)
    n, exp, t, offset, coeffs = REF_CASES[3]
    ocfg, cw = ref_case(o, n, exp, t, offset, coeffs)
    fri = m.Fri.new(f.prim_nth_root(n), f.new_element(offset), n, exp, t)
    codeword = [f.new_element(int(v)) for v in cw]
    prior = _prior(45)
    caller_objs = tc._elems([7, 8])                    # the caller's own object ahead of FRI's
    # prove
    wfs = tc.fiat_shamir(o, prior)
    want, want_top = tc.prove(o, ocfg, cw, fs=wfs)
    stream = m.ProofStream.deserialize(caller_objs, f)
    fs = m.FiatShamir.new()
    fs.absorb(prior)
    top = fri.prove(list(codeword), fs, stream)
    assert stream.serialize() == caller_objs + want and top == want_top
    assert bytes(fs.transcript) == prior + b"".join(want[33 * k + 1:33 * k + 33] for k in range(fri.num_rounds()))
    # commit
    stream2, _cws, _trees, wroots, _alphas = tc.commit(o, ocfg, cw, prior)
    s2, fs2 = m.ProofStream.new(), m.FiatShamir.new()
    fs2.absorb(prior)
    cws = fri.commit(list(codeword), s2, fs2)
    assert s2.serialize() == stream2 and bytes(fs2.transcript) == prior + b"".join(wroots)
    assert [fe.value for fe in cws[0]] == [int(v) for v in cw]
    # verify, after the caller has popped its own object
    vstream = m.ProofStream.deserialize(caller_objs + want, f)
    vstream.pop()
    vfs = m.FiatShamir.new()
    vfs.absorb(prior)
    pv = []
    assert fri.verify(vstream, vfs, pv)
    assert [(i, v.value) for i, v in pv] == tc.verify(o, ocfg, want, prior)[1]
    assert bytes(vfs.transcript) == bytes(fs.transcript)


def _mgpu_rank(rank, world, port, prior_len, q):
    import os
    import torch.distributed as dist
    import stark_rs_amd as s
    from stark_rs_amd.mgpu import MultiGpu
    from oracle import oracle as o
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    o.build()
    eng = s.Engine(P, G, 0)
    ocfg, cw = low_degree_case(o, 14, 8, 16, 3, seed=5)
    prior = _prior(prior_len)
    cfg = _cfg(eng, ocfg)
    from stark_rs_amd.mgpu import HipMem, HostCollectives
    coll = HostCollectives(rank, world, HipMem())
    mg = MultiGpu(eng, rank, world, host=coll, min_block=1 << 10)
    blk = len(cw) // world
    d = eng.dev_alloc(blk * 4)
    eng.dev_upload(cw[rank * blk:(rank + 1) * blk], d)
    got, top = mg.fri_prove(cfg, d, blk, prior)
    want, want_top = eng.fri_prove(cfg, cw, prior)
    ok = got == want and top == want_top and got == tc.prove(o, ocfg, cw, prior)[0]
    mg.close()
    eng.dev_free(d)
    eng.close()
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_mgpu_two_ranks_on_one_card_with_prior(oracle):
    """smi_mgpu_fri_prove_fs over 2 ranks on this card (smi_mgpu_create_with, gloo shim), a 37-byte prior: the
    single-GPU proof and the composition's on every rank."""
    import torch.multiprocessing as mp
    from test_mgpu_gloo import _free_port
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mgpu_rank, args=(r, world, port, 37, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(300)
        assert pr.exitcode == 0
    got = sorted(q.get(timeout=5) for _ in range(world))
    assert got == [(r, True) for r in range(world)], got
