"""CPU: FRI continuing a caller's Fiat-Shamir transcript (src/fri.rs:105-110, 250-255, 313-318 take the caller's
`&mut FiatShamir`; every challenge hashes the whole transcript, src/fiat_shamir.rs:15-25).

  * the oracle composition of tests/transcript_compose.py against the oracle's own Fri::prove / Fri::commit
    (empty prior), so that it can be trusted as the checker with a non-empty one;
  * the shared hash code (csrc/hash_core.h fs_seed / fs_absorb_root_phase / fs_challenge_phase, through the
    emulator) against oracle.FiatShamir for priors of every phase;
  * the multi-GPU round loop (csrc/mgpu_loop.h) continuing a prior over gloo, against the composition."""
import ctypes as C

import numpy as np
import pytest

import transcript_compose as tc
from test_mgpu_gloo import _free_port

P, G = 998244353, 3
u32p = C.POINTER(C.c_uint32)

REF_CASES = [                                   # the reference's four FRI tests (n, expansion, t, offset, coeffs)
    (32, 4, 2, 3, [5]),                         # fri.rs:533-563
    (64, 4, 3, 7, [5, 3]),                      # fri.rs:566-601
    (128, 4, 4, 13, [1, 3, 2]),                 # fri.rs:604-646
    (256, 8, 5, 17, [1, 2, 5, 3, 7, 4, 1, 2]),  # fri.rs:649-693
]


def _prior(n, seed=1):
    return np.random.default_rng(seed + 7919 * n).integers(0, 256, n, dtype=np.uint8).tobytes()


def ref_case(o, n, exp, t, offset, coeffs):
    omega = o.ff_prim_nth_root(n)
    dom = [o.ff_mul(offset, o.ff_exp(omega, i)) for i in range(n)]
    return o.fri_cfg(omega, offset, n, exp, t), np.asarray(o.poly_eval_domain(coeffs, dom), dtype=np.uint64)


def low_degree_case(o, logn, exp=8, t=16, offset=3, seed=99, p=P):
    n = 1 << logn
    omega = o.ff_prim_nth_root(n) if p == P else o.ff_prim_nth_root_g(n, p, 3)
    coeffs = o.splitmix64(seed, n // exp) % np.uint64(p)
    return o.fri_cfg(omega, offset, n, exp, t, p), o.fast_coset_ntt(coeffs, n, omega, offset, p)


# ------------------------------------------------------------------ the composition itself
@pytest.mark.parametrize("case", range(len(REF_CASES)))
def test_composition_with_empty_prior_is_the_oracle_prove(oracle, case):
    o = oracle
    cfg, cw = ref_case(o, *REF_CASES[case])
    want, want_top = o.fri_prove(cfg, cw)
    got, top = tc.prove(o, cfg, cw)
    assert got == want and top == want_top
    roots, alphas, last = o.fri_commit_trace(cfg, cw)
    stream, _cws, _trees, groots, galphas = tc.commit(o, cfg, cw)
    assert groots == [bytes(r) for r in roots] and galphas == alphas
    assert stream.endswith(tc._elems(last))
    ok, pv, used = tc.verify(o, cfg, want)
    assert ok and used == len(want)
    assert (ok, pv) == o.fri_verify(cfg, want, want_values=True)


@pytest.mark.parametrize("logn", [10, 11, 12, 13, 14])
def test_composition_larger_domains(oracle, logn):
    o = oracle
    cfg, cw = low_degree_case(o, logn)
    want, want_top = o.fri_prove(cfg, cw)
    got, top = tc.prove(o, cfg, cw)
    assert got == want and top == want_top
    roots, alphas, _last = o.fri_commit_trace(cfg, cw)
    _s, _c, _t, groots, galphas = tc.commit(o, cfg, cw)
    assert groots == [bytes(r) for r in roots] and galphas == alphas


def test_composition_verify_with_prior_accepts_its_own_proof_only_under_that_prior(oracle):
    o = oracle
    cfg, cw = low_degree_case(o, 10)
    prior = _prior(37)
    proof, _top = tc.prove(o, cfg, cw, prior)
    assert tc.verify(o, cfg, proof, prior)[0]
    assert not tc.verify(o, cfg, proof)[0]
    assert proof != tc.prove(o, cfg, cw)[0]


# ------------------------------------------------------------------ seed state and phase (hash_core.h)
def _emu():
    import stark_rs_amd as s
    s.build()
    from stark_rs_amd._lib import EMU_PATH
    L = C.CDLL(EMU_PATH)
    L.emu_fs_seed.argtypes = [C.c_char_p, C.c_size_t, u32p, u32p]
    L.emu_fs_seed.restype = None
    L.emu_fs_absorb_root_phase.argtypes = [u32p, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint64)]
    L.emu_fs_absorb_root_phase.restype = None
    L.emu_fs_challenge_phase.argtypes = [u32p, C.c_uint32]
    L.emu_fs_challenge_phase.restype = C.c_uint64
    return L


@pytest.mark.parametrize("P_len", list(range(97)) + [4096, 4097, 4101, 4127])
def test_seed_phase_and_challenges_equal_the_whole_transcript_hash(oracle, P_len):
    o, L = oracle, _emu()
    prior = _prior(P_len, 3)
    words, phase = (C.c_uint32 * 16)(), C.c_uint32()
    L.emu_fs_seed(prior, P_len, words, C.byref(phase))
    assert phase.value == P_len % 32
    fs = tc.fiat_shamir(o, prior)
    assert L.emu_fs_challenge_phase(words, phase.value) == fs.challenge()
    rng = np.random.default_rng(P_len)
    for _ in range(24):
        root = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        alpha = C.c_uint64()
        L.emu_fs_absorb_root_phase(words, phase.value, root, C.byref(alpha))
        fs.absorb(root)
        want = fs.challenge()
        assert alpha.value == want
        assert L.emu_fs_challenge_phase(words, phase.value) == want


def test_empty_seed_is_the_initial_state(oracle):
    L = _emu()
    words, phase = (C.c_uint32 * 16)(), C.c_uint32(99)
    L.emu_fs_seed(None, 0, words, C.byref(phase))
    primes = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53]   # src/hash.rs:10-12, paired lanes
    assert phase.value == 0 and list(words) == [q * 0x00010001 for q in primes]


# ------------------------------------------------------------------ multi-GPU loop (emulator, gloo)
def _mgpu_emu():
    import stark_rs_amd as s
    from stark_rs_amd.mgpu import CollOps
    from stark_rs_amd._lib import FriCfg
    s.build()
    from stark_rs_amd._lib import EMU_PATH
    L = C.CDLL(EMU_PATH)
    sz, vp, i32 = C.c_size_t, C.c_void_p, C.c_int
    L.emu_mgpu_fri_prove_fs.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(CollOps), i32, i32, C.POINTER(FriCfg), C.c_char_p, sz, u32p,
                                        sz, sz, vp, sz, C.POINTER(sz), vp]
    L.emu_mgpu_fri_commit_fs.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(CollOps), i32, i32, C.POINTER(FriCfg), C.c_char_p, sz,
                                         u32p, sz, sz, vp, vp, vp, C.POINTER(sz)]
    return L


def _mgpu_worker(rank, world, port, logn, exp, t, offset, min_block, prior_len, q):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from stark_rs_amd.mgpu import HostCollectives, HostMem
    from stark_rs_amd._lib import FriCfg
    from oracle import oracle as o
    o.build()
    L, coll = _mgpu_emu(), HostCollectives(rank, world, HostMem())
    ocfg, cw = low_degree_case(o, logn, exp, t, offset, seed=78)
    prior = _prior(prior_len, 5)
    n, blk = 1 << logn, (1 << logn) // world
    block = np.ascontiguousarray(cw[rank * blk:(rank + 1) * blk].astype(np.uint32))
    cfg = FriCfg(ocfg.omega, offset, n, exp, t)
    proof, plen, top = (C.c_uint8 * (1 << 22))(), C.c_size_t(), (C.c_uint64 * (t + 1))()
    rc = L.emu_mgpu_fri_prove_fs(P, G, C.byref(coll.ops), rank, world, C.byref(cfg), prior, len(prior), block.ctypes.data_as(u32p), blk,
                                 min_block, proof, len(proof), C.byref(plen), top)
    R = o.fri_num_rounds(ocfg)
    roots, alphas, last, ll = (C.c_uint8 * (32 * R))(), (C.c_uint64 * R)(), np.zeros(n, dtype=np.uint64), C.c_size_t()
    rc2 = L.emu_mgpu_fri_commit_fs(P, G, C.byref(coll.ops), rank, world, C.byref(cfg), prior, len(prior), block.ctypes.data_as(u32p),
                                   blk, min_block, roots, alphas, last.ctypes.data, C.byref(ll))
    ok = rc == 0 and rc2 == 0 and not coll.errors
    if ok:
        want, want_top = tc.prove(o, ocfg, cw, prior)
        _s, _c, _t, wroots, walphas = tc.commit(o, ocfg, cw, prior)
        ok = bytes(proof[:plen.value]) == want and list(top)[:t] == want_top
        ok = ok and bytes(roots) == b"".join(wroots) and list(alphas)[:R - 1] == walphas
        ok = ok and list(last[:ll.value]) == tc._pop(_s, 33 * R)[1]
    q.put((rank, bool(ok), rc, rc2, coll.errors))
    dist.destroy_process_group()


def _run(world, args):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mgpu_worker, args=(r, world, port) + args + (q,)) for r in range(world)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(300)
        assert pr.exitcode == 0
    got = sorted(q.get(timeout=5) for _ in range(world))
    assert [g[0] for g in got] == list(range(world))
    assert all(g[1] for g in got), got


@pytest.mark.parametrize("prior_len", [0, 64, 37])
@pytest.mark.parametrize("world,logn,exp,t,offset,min_block", [
    (2, 10, 4, 4, 3, 64),       # sharded rounds (Fiat-Shamir after the gathered top levels), then replicated
    (4, 11, 8, 8, 7, 32),       # four ranks; with prior 0 / 64 the replicated rounds run the loop's tail branch
])
def test_native_loop_continues_the_transcript_on_every_rank(oracle, world, logn, exp, t, offset, min_block, prior_len):
    _run(world, (logn, exp, t, offset, min_block, prior_len))
