"""GPU: out-of-domain sampling with an argument list (include/stark_mi.h, "Out-of-domain sampling with an argument list") --
smi_dev_deep_compose_args, smi_dev_air_prove_deep_xargs / smi_air_verify_deep_xargs -- against the restatement over the CPU
oracle's primitives (tests/deep_args_compose.py).  Every comparison is exact.  `pytest -m gpu`."""
import functools

import numpy as np
import pytest

import air_compose as ac
import deep_args_compose as da
import deep_compose as dc
import ext_compose as xc
import xargs_compose as xa
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_boundary_primes import u64_set
from test_gpu_deep import gpu_compose
from test_gpu_ext import _dev_cols

pytestmark = pytest.mark.gpu
KW = dict(row_leaves=True, ext=True, deep_args=True)
SHAPES = [(1, 1, 1), (3, 2, 2), (9, 8, 4), (64, 8, 16)]
FILL = 0x5a5a5a5a


# ---------------------------------------------------------------------------------------------- the DEEP codeword
def gpu_compose_args(eng, lde, cl, seg, log_n, lb, z, ood, ch, h, odd=False):
    """odd: four different odd strides from bases one word into their buffers -- the 4-byte path.  The words before, between and
    behind the output columns must stay as they were."""
    import torch
    lde, cl, seg = (np.asarray(a, dtype=np.uint64) for a in (lde, cl, seg))
    W, N = lde.shape
    lead = 1 if odd else 0
    st = [N + 1, N + 3, N + 5, N + 7] if odd else [N] * 4
    tl, dl = _dev_cols(lde, st[0], lead)
    tc, dcl = _dev_cols(cl, st[1], lead)
    ts, ds = _dev_cols(seg, st[2], lead)
    out = torch.full((lead + 4 * st[3] + 4,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.dev_deep_compose_args(dl, dcl, ds, W, cl.shape[0] // 4, seg.shape[0] // 4, log_n, lb, z, ood, ch, out.data_ptr() + 4 * lead, stride=st[0],
                              c_stride=st[1], seg_stride=st[2], out_stride=st[3], lde_offset=h)
    eng.sync()
    host = out.cpu().numpy().view(np.uint32)
    assert np.all(host[:lead] == FILL) and np.all(host[lead + 3 * st[3] + N:] == FILL)
    for e in range(3):
        assert np.all(host[lead + e * st[3] + N:lead + (e + 1) * st[3]] == FILL)
    del tl, tc, ts
    return np.stack([host[lead + e * st[3]:lead + e * st[3] + N] for e in range(4)]).astype(np.uint64)


def check_compose(eng, oracle, p, g, log_N, shapes, challenge_sets=("random", "u64"), h=None):
    """h: the offset of the evaluation domain (default g, what lde_offset=None means); under another h the restatement over
    the default points must differ, so that a kernel which ignored h could not pass"""
    N, h = 1 << log_N, g if h is None else h
    for k, (W, A, D) in enumerate(shapes):
        lb = 2 if log_N < 5 else 2 + k % 3
        log_n = log_N - lb
        w, _wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
        x = dc.points(oracle, p, g, log_n, lb, h)
        for cs in challenge_sets:
            u = {"u64": u64_set(p), "max": [(1 << 64) - 1], "pm1": [p - 1]}.get(cs)
            lde, cl, seg, z, ood, ch = da.compose_inputs(p, W, A, D, N, "random" if cs == "random" else "extreme", seed=k + log_N, u=u)
            want = da.q_codeword(lde, cl, seg, x, z, ood, ch, w, p, g)
            if h != g:
                assert not np.array_equal(want, da.q_codeword(lde, cl, seg, dc.points(oracle, p, g, log_n, lb, g), z, ood, ch, w, p, g)), (W, A, D, cs)
            for odd in (False, True):
                assert np.array_equal(gpu_compose_args(eng, lde, cl, seg, log_n, lb, z, ood, ch, h, odd=odd), want), (log_N, W, A, D, cs, odd, h)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_N", [3, 4, 10, 11, 16])
def test_dev_deep_compose_args_equals_the_restatement(engines, oracle, p, g, log_N):
    """below one lane group, one lane group, exactly one workgroup, the first shape with two workgroups, many workgroups"""
    check_compose(engines[p], oracle, p, g, log_N, SHAPES)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_with_every_delta_zero_the_kernel_is_dev_deep_compose(engines, p, g):
    eng = engines[p]
    for log_N, (W, A, D) in ((4, (1, 1, 1)), (11, (3, 2, 2)), (12, (9, 8, 4))):
        lb, N = 2, 1 << log_N
        lde, cl, seg, z, ood, ch = da.compose_inputs(p, W, A, D, N, "random", seed=log_N)
        for i in range(4 * 2 * W, 4 * (2 * W + 2 * A)):
            ch[i] = 0 if i % 2 else p
        plain = lambda v: v[:8 * W] + v[4 * (2 * W + 2 * A):]
        got = gpu_compose_args(eng, lde, cl, seg, log_N - lb, lb, z, ood, ch, g)
        assert np.array_equal(got, gpu_compose(eng, lde, seg, log_N - lb, lb, z, plain(ood), plain(ch), g)), (W, A, D)


def test_the_grid_stride_loop_on_the_device(engines, oracle):
    """N = 2^22 at (W, A, D) = (1, 1, 1): 4096 workgroups' worth of points under the cap of 8 workgroups a compute unit, so the
    lanes of a 256-CU part take two trips; pointwise against the restatement's q_at"""
    import torch
    p, g = xc.PRIMES[1]
    eng, log_N, lb = engines[p], 22, 3
    N, log_n = 1 << log_N, log_N - lb
    lde, cl, seg, z, ood, ch = da.compose_inputs(p, 1, 1, 1, N, "random", seed=22)
    got = gpu_compose_args(eng, lde, cl, seg, log_n, lb, z, ood, ch, g)
    grid = min(N // 1024, 8 * torch.cuda.get_device_properties(0).multi_processor_count)
    edge = grid * 1024
    rng = np.random.default_rng(5)
    idx = sorted(set(list(range(16)) + list(range(N - 16, N)) + [i % N for i in range(edge - 16, edge + 16)] + [int(i) for i in rng.integers(0, N, 2048)]))
    w, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
    for i in idx:
        want = da.q_at(lde[:, i], cl[:, i], seg[:, i], g * pow(wN, i, p) % p, z, ood, ch, w, p, g)
        assert [int(v) for v in got[:, i]] == want, i


def test_dev_deep_compose_args_refusals(engines):
    import stark_rs_amd as s
    p, g = xc.PRIMES[0]
    eng, log_n, lb, W, A, D = engines[p], 6, 2, 2, 1, 1
    N = 1 << (log_n + lb)
    lde, cl, seg, z, ood, ch = da.compose_inputs(p, W, A, D, N, "random")
    tl, dl = _dev_cols(lde)
    tc, dcl = _dev_cols(cl)
    ts, ds = _dev_cols(seg)
    with Dev(eng) as dev:
        d_out = dev.alloc(16 * N)
        with pytest.raises(s.StarkMiError, match="base field"):
            eng.dev_deep_compose_args(dl, dcl, ds, W, A, D, log_n, lb, [z[0], 0, 0, 0], ood, ch, d_out)
        with pytest.raises(s.StarkMiError, match=">= p"):
            eng.dev_deep_compose_args(dl, dcl, ds, W, A, D, log_n, lb, z, [p] + ood[1:], ch, d_out)
        with pytest.raises(s.StarkMiError, match="stride"):
            eng.dev_deep_compose_args(dl, dcl, ds, W, A, D, log_n, lb, z, ood, ch, d_out, c_stride=N - 1)
        with pytest.raises(s.StarkMiError, match="auxiliary"):
            eng.dev_deep_compose_args(dl, dcl, ds, W, 9, D, log_n, lb, z, ood + [0] * 64, ch + [0] * 64, d_out)
        with pytest.raises(ValueError):
            eng.dev_deep_compose_args(dl, dcl, ds, W, A, D, log_n, lb, z, ood[:-1], ch, d_out)


# ---------------------------------------------------------------------------------------------- the proof
@functools.lru_cache(maxsize=None)
def statement(name, log_n, p):
    """-> (air, cols, args) of one of the four lists; built once per size and modulus"""
    n = 1 << log_n
    if name in ("perm", "lookup"):
        return da.small_lists(n, p)[name]
    return da.readme_lists(n, p)[name]


def mirror(air, args):
    import copy
    return xa.mirror_air(copy.deepcopy(air), args)


def gpu_proof(eng, air, args, cols, log_n, lb, t, bits=0, check=True, fill=False, **kw):
    cols = [list(c) for c in cols]
    if fill:                                                                # the device fills the multiplicity columns
        for g_ in args:
            if g_[0] == "lookup":
                cols[g_[3]] = [0] * len(cols[0])
    with Dev(eng) as dev:
        return eng.dev_air_prove(mirror(air, args), dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, lb, t, grind_bits=bits, check=check,
                                 fill_multiplicities=fill, **KW, **kw)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("bits", [0, 8])
@pytest.mark.parametrize("lb", [2, 3])
@pytest.mark.parametrize("log_n", [3, 6, 10])
@pytest.mark.parametrize("name", ["perm", "lookup", "nine", "selectors"])
def test_prove_bytes_equal_the_restatement_and_verify_accepts(engines, oracle, p, g, name, log_n, lb, bits):
    """At (log_n, lb) = (3, 2) with t = 4 FRI has one round and no fold: there is no layer-0 triple, and the verifier rejects
    with that sentence, as smi_air_verify_deep does at such a shape; the prover's bytes are compared all the same."""
    eng, t = engines[p], 4
    air, cols, args = statement(name, log_n, p)
    W, A = len(cols), len(args)
    fill = name in ("lookup", "nine")
    res = gpu_proof(eng, air, args, cols, log_n, lb, t, bits, fill=fill)
    want = da.prove(oracle, air, args, cols, p, g, log_n, lb, t, 1, g, bits)
    _d, D = da.plan(air, args)
    assert eng.air_plan_deep_args(mirror(air, args), W, log_n, lb)[1] == D
    assert [bytes(r) for r in res["column_roots"]] == want["roots"] and res["column_roots"].shape == (3, 32)
    assert [c for el in res["ood"] for c in el] == want["ood"] and len(res["ood"]) == 2 * W + 2 * A + D
    assert res["closes"] == want["closes"] == [True] * A
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    assert len(res["proof"]) == eng.air_plan_deep_args(mirror(air, args), W, log_n, lb, num_colinearity_tests=t)[2]
    ok, why = eng.air_verify(mirror(air, args), res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **KW)
    ok_o, why_o = da.verify(oracle, air, args, res["proof"], want["roots"], p, g, W, log_n, lb, t, 1, g, bits)
    if (log_n, lb) == (3, 2):
        assert not ok and not ok_o and why_o == "no layer" and da.KEYWORD["no layer"] in why, (why, why_o)
    else:
        assert ok and ok_o, (why, why_o)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_a_lookup_list_at_log_blowup_2(engines, oracle, p, g):
    import stark_rs_amd as s
    eng, log_n, lb, t = engines[p], 6, 2, 4
    air, cols, args = statement("nine", log_n, p)
    with pytest.raises(s.StarkMiError) as ei:
        with Dev(eng) as dev:
            eng.dev_air_prove(mirror(air, args), dev.upload(np.array(cols, dtype=np.uint64)), 9, log_n, lb, t, row_leaves=True, ext=True, grind_bits=0)
    assert ei.value.status == -10
    res = gpu_proof(eng, air, args, cols, log_n, lb, t, timed=True)
    assert list(res["stage_ms"]) == ["lde", "commit", "args", "compose", "segments", "ood", "fri", "open"]
    ok, why = eng.air_verify(mirror(air, args), res["proof"], res["column_roots"], 9, log_n, lb, t, **KW)
    assert ok, why
    # the same list through mirror.Air's switch to the superset form: the same bytes
    sup = mirror(air, args)
    sup.xargs_always = True
    with Dev(eng) as dev:
        again = eng.dev_air_prove(sup, dev.upload(np.array(cols, dtype=np.uint64)), 9, log_n, lb, t, grind_bits=0, **KW)
    assert again["proof"] == res["proof"]


def gpu_composition(eng, air, args, ref, W, log_n, lb):
    """H as the device composes it (smi_dev_air_compose_xargs) from the committed columns under the transcript's challenges"""
    import torch
    from test_gpu_ext import _dev_u64
    N = 1 << (log_n + lb)
    tl, dl = _dev_cols(np.array(ref["lde"]))
    tc, dcl = _dev_cols(np.array(ref["cl"]))
    tw, dw = _dev_u64(ref["wch"])
    out = torch.zeros(4 * N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    listed = mirror(air, args)
    listed.xargs_always = True                                               # the superset form: the entry point the prover's H comes from
    eng.dev_air_compose_args(listed, dl, dcl, W, log_n, lb, ref["ch"], dw, out.data_ptr())
    eng.sync()
    return out.cpu().numpy().view(np.uint32).astype(np.uint64).reshape(4, N)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_the_degrees_of_q_and_of_the_composition(engines, oracle, p, g):
    """Independent of the restated codewords: Q as the device composes it from the prover's own record, interpolated through
    the oracle, has no coefficient from n up -- for an honest trace, and for a lookup that does not close as well: every
    committed column is a polynomial of degree < n and the record holds its true values, so Q cannot show the defect.  It shows
    in the composition: the device's H has no coefficient from D n up for the honest trace and some for the other one, whose
    segments are therefore not H, and the verifier rejects it on the consistency check."""
    eng, log_n, lb, t = engines[p], 6, 2, 4
    n = 1 << log_n
    _w, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
    air, cols, args = statement("lookup", log_n, p)
    _d, D = da.plan(air, args)
    broken = [list(c) for c in cols]
    broken[2][broken[2].index(max(broken[2]))] -= 1
    for trace, honest in ((cols, True), (broken, False)):
        res = gpu_proof(eng, air, args, trace, log_n, lb, t, check=False)
        assert res["closes"] == [honest]
        ref = da.prove(oracle, air, args, trace, p, g, log_n, lb, t, 1, g, honest=honest)
        assert [bytes(r) for r in res["column_roots"]] == ref["roots"]     # the committed columns are the restatement's
        ood = [c for el in res["ood"] for c in el]
        Q = gpu_compose_args(eng, np.array(ref["lde"]), np.array(ref["cl"]), ref["seg"], log_n, lb, ref["z"], ood, ref["gammas"], g)
        assert not any(np.asarray(oracle.fast_intt(Q[e], wN, g, p))[n:].any() for e in range(4)), honest
        H = gpu_composition(eng, air, args, ref, 3, log_n, lb)
        high = any(np.asarray(oracle.fast_intt(H[e], wN, g, p))[D * n:].any() for e in range(4))
        assert high != honest, honest
        ok, why = eng.air_verify(mirror(air, args), res["proof"], res["column_roots"], 3, log_n, lb, t, **KW)
        assert ok == honest and (honest or da.KEYWORD["consistency"] in why), why
        assert da.verify(oracle, air, args, res["proof"], ref["roots"], p, g, 3, log_n, lb, t, 1, g) == ((True, "") if honest else (False, "consistency"))


def both_reject(eng, oracle, air, args, proof, roots, p, g, W, log_n, lb, t, reason, bits=0):
    ok, why = eng.air_verify(mirror(air, args), proof, roots, W, log_n, lb, t, grind_bits=bits, **KW)
    ok_o, why_o = da.verify(oracle, air, args, proof, [bytes(r) for r in roots], p, g, W, log_n, lb, t, 1, g, bits)
    assert not ok and why and not ok_o, (why, why_o)
    assert why_o == reason, (why, why_o)
    assert da.keyword(reason) in why, (why, why_o)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_verify_rejections(engines, oracle, p, g):
    eng, log_n, lb, t = engines[p], 6, 2, 4
    air, cols, args = xa.scene(1 << log_n, p, (4, 8, 2), A=3)
    W, A, log_N = len(cols), len(args), log_n + lb
    _d, D = da.plan(air, args)
    res = gpu_proof(eng, air, args, cols, log_n, lb, t)
    proof, roots = res["proof"], res["column_roots"]
    a = (p, g, W, log_n, lb, t)
    assert eng.air_verify(mirror(air, args), proof, roots, W, log_n, lb, t, **KW)[0]

    def flipped(at):
        b = bytearray(proof)
        b[at] ^= 1
        return bytes(b)
    both_reject(eng, oracle, air, args, flipped(1), roots, *a, reason="record")
    b = bytearray(proof)
    b[9:17] = xc._u64(int.from_bytes(proof[9:17], "little") + p)
    both_reject(eng, oracle, air, args, bytes(b), roots, *a, reason="record canonical")
    for i in (2 * W, 2 * W + A, 2 * W + 2 * A):                               # one a_a, one b_a, one s_j
        both_reject(eng, oracle, air, args, flipped(9 + 32 * i + 8), roots, *a, reason="consistency")
    m, prec = 2 * t, 9 + 32 * log_N
    widths = (W, 4 * A, 4 * D)
    lens = [m * (9 + 8 * wd) + m * prec for wd in widths]
    start = len(proof) - sum(lens)
    for v, wd in enumerate(widths):                                          # a value, a path, a width, a path's tag -- in each section
        both_reject(eng, oracle, air, args, flipped(start + 9), roots, *a, reason="auth")
        both_reject(eng, oracle, air, args, flipped(start + m * (9 + 8 * wd) + 9 + 40), roots, *a, reason="auth")
        both_reject(eng, oracle, air, args, flipped(start + 1), roots, *a, reason="row")
        both_reject(eng, oracle, air, args, flipped(start + m * (9 + 8 * wd)), roots, *a, reason="path")
        start += lens[v]
    both_reject(eng, oracle, air, args, proof[:-1], roots, *a, reason="length")
    both_reject(eng, oracle, air, args, proof + b"\x00", roots, *a, reason="length")
    both_reject(eng, oracle, air, [args[2], args[1], args[0]], proof, roots, *a, reason="consistency")   # the list in another order
    both_reject(eng, oracle, air, [args[0][:4], args[1], args[2]], proof, roots, *a, reason="consistency")   # one selector removed
    both_reject(eng, oracle, air, args, proof, roots, *a, reason="fri: proof of work", bits=20)
    # crossed over with the two neighbouring variants
    with Dev(eng) as dev:
        plain = eng.dev_air_prove(mirror(air, args), dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, 3, t, row_leaves=True, ext=True, grind_bits=0)
    a3 = (p, g, W, log_n, 3, t)
    both_reject(eng, oracle, air, args, plain["proof"], np.concatenate([plain["column_roots"], plain["column_roots"][:1]]), *a3, reason="record")
    ok, why = eng.air_verify(mirror(air, args), proof, roots[:2], W, log_n, 3, t, row_leaves=True, ext=True, grind_bits=0)
    assert not ok and why
    bare = mirror(air, [])
    with Dev(eng) as dev:
        deep = eng.dev_air_prove(bare, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=0, deep=True)
    both_reject(eng, oracle, air, args, deep["proof"], np.concatenate([deep["column_roots"], deep["column_roots"][:1]]), *a, reason="record")
    ok, why = eng.air_verify(bare, proof, roots[:2], W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=0, deep=True)
    assert not ok and dc.KEYWORD["record"] in why, why


def test_engine_refusals(engines):
    p, g = xc.PRIMES[0]
    eng, log_n = engines[p], 6
    air, cols, args = statement("perm", log_n, p)
    listed = mirror(air, args)
    with Dev(eng) as dev:
        d = dev.upload(np.array(cols, dtype=np.uint64))
        with pytest.raises(ValueError, match="argument list"):
            eng.dev_air_prove(air, d, 2, log_n, 3, 4, **KW)                   # a plain AIR
        for kw in (dict(KW, deep=True), dict(KW, folding=4), dict(row_leaves=True, deep_args=True), dict(deep_args=True), dict(ext=True, deep_args=True)):
            with pytest.raises(ValueError):
                eng.dev_air_prove(listed, d, 2, log_n, 3, 4, **kw)
            with pytest.raises(ValueError):
                eng.air_verify(listed, b"", np.zeros((3, 32), dtype=np.uint8), 2, log_n, 3, 4, **kw)
        with pytest.raises(ValueError, match="no lookup"):
            eng.dev_air_prove(listed, d, 2, log_n, 3, 4, fill_multiplicities=True, **KW)
        with pytest.raises(ValueError, match="plain AIR"):                   # deep=True keeps refusing a list
            eng.dev_air_prove(listed, d, 2, log_n, 3, 4, row_leaves=True, ext=True, deep=True)
