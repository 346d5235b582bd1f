"""GPU: the zero-knowledge building blocks (include/stark_mi.h, "Zero-knowledge DEEP proofs") --
smi_dev_random_fill and smi_dev_zk_segments against the CPU emulator of their lane bodies and the restatement over the oracle's
hash (tests/zk_compose.py), on the 16-byte and the 4-byte paths, at the reference modulus and the boundary moduli of
tests/test_gpu_boundary_primes.py.  Every comparison is exact.  `pytest -m gpu`."""
import numpy as np
import pytest

import zk_compose as zk
from test_gpu_boundary_primes import GEN as BOUNDARY_GEN, THREE
from test_gpu_ext import _dev_cols
from test_zk_emu import COUNTS, P_REF, SEED, SPLITS, emu, emu_fill, emu_split, split_case  # noqa: F401  (emu is a fixture)

pytestmark = pytest.mark.gpu
FILL = 0x5a5a5a5a
PRIMES = [P_REF] + THREE
GEN = dict(BOUNDARY_GEN)
GEN[P_REF] = 3


@pytest.fixture(scope="module")
def engines():
    """one context per modulus, made on first use, closed at the end of the module"""
    import stark_rs_amd as s

    class Lazy(dict):
        def __missing__(self, p):
            self[p] = s.Engine(p, GEN[p], 0)
            return self[p]
    es = Lazy()
    yield es
    for e in es.values():
        e.close()


def gpu_fill(eng, seed, stream, count, lead=0):
    """count residues `lead` words into a device buffer; the words around them must stay as they were"""
    import torch
    buf = torch.full((lead + count + 9,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.dev_random_fill(seed, stream, buf.data_ptr() + 4 * lead, count)
    eng.sync()
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[:lead] == FILL).all() and (host[lead + count:] == FILL).all()
    return [int(v) for v in host[lead:lead + count]]


def gpu_split(eng, hc, h_len, log_n, ks, Dp, rho, lead=0, pad=0):
    import torch
    n = 1 << log_n
    hs, os_ = h_len + pad, n + pad
    th, dh = _dev_cols(np.asarray(hc, dtype=np.uint64), hs, lead)
    tr = torch.from_numpy(np.asarray(rho, dtype=np.uint32).view(np.int32).copy()).cuda() if len(rho) else None
    out = torch.full((lead + 4 * Dp * os_,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.dev_zk_segments(dh, h_len, log_n, ks, Dp, tr.data_ptr() if tr is not None else None, out.data_ptr() + 4 * lead, h_stride=hs, out_stride=os_)
    eng.sync()
    host = out.cpu().numpy().view(np.uint32)
    body = host[lead:].reshape(4 * Dp, os_)
    assert (host[:lead] == FILL).all() and (body[:, n:] == FILL).all(), "a word outside the n coefficients of a column was written"
    del th, tr
    return [[int(v) for v in row[:n]] for row in body]


@pytest.mark.parametrize("p", PRIMES)
def test_random_fill_equals_the_emulator_and_the_hash(engines, oracle, emu, p):
    eng = engines[p]
    for count in COUNTS + [2048, 2049, (1 << 16) + 5]:          # one lane, one workgroup and its edge, many workgroups
        want = emu_fill(emu, p, SEED, 3, count)
        if count <= 1025:
            assert want == zk.rng(oracle, SEED, 3, count, p)
        for lead in (0, 4, 1, 2, 3):                             # 16-byte stores, then the 4-byte path from every misalignment
            assert gpu_fill(eng, SEED, 3, count, lead) == want, (count, lead)
    assert gpu_fill(eng, SEED, 4, 64) != gpu_fill(eng, SEED, 3, 64)
    assert gpu_fill(eng, bytes(32), (1 << 64) - 1, 9) == zk.rng(oracle, bytes(32), (1 << 64) - 1, 9, p)
    assert gpu_fill(eng, SEED, 3, 0) == []


def test_random_fill_refusals(engines):
    import stark_rs_amd as s
    eng = engines[P_REF]
    with pytest.raises(ValueError):
        eng.dev_random_fill(b"short", 0, 0, 0)
    with pytest.raises(s.StarkMiError):
        eng.dev_random_fill(SEED, 0, None, 4)


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("log_n,t,D,h_len", SPLITS + [(12, 2, 2, None)])
def test_zk_segments_equal_the_emulator_and_the_split(engines, emu, p, log_n, t, D, h_len):
    eng = engines[p]
    n, ks, L, h_len, Dp, hc, rho = split_case(log_n, t, D, h_len, p)
    if log_n == 12:
        hc[:, ::7] = p - 1                                       # the largest residue under the subtraction
        rho[::3] = p - 1
    want = emu_split(emu, p, hc, h_len, log_n, ks, Dp, rho)
    if log_n <= 8:
        assert want == zk.split(hc, h_len, log_n, ks, Dp, rho, p)
    for lead, pad in ((0, 0), (0, 4), (1, 0), (0, 3), (2, 5)):   # two 16-byte layouts, three 4-byte ones
        assert gpu_split(eng, hc, h_len, log_n, ks, Dp, rho, lead, pad) == want, (lead, pad)


def test_zk_segments_refusals(engines):
    import stark_rs_amd as s
    eng = engines[P_REF]
    n, ks, L, h_len, Dp, hc, rho = split_case(6, 1, 2, None, P_REF)
    t, d = _dev_cols(np.asarray(hc, dtype=np.uint64))
    for kw, word in ((dict(n_segments=Dp - 1), "do not hold"), (dict(k_s=32), "k_s"), (dict(n_segments=15), "segments"), (dict(log_n=1), "log_n")):
        args = dict(h_len=h_len, log_n=6, k_s=ks, n_segments=Dp)
        args.update(kw)
        with pytest.raises(s.StarkMiError, match=word):
            eng.dev_zk_segments(d, args["h_len"], args["log_n"], args["k_s"], args["n_segments"], d, d)
    with pytest.raises(s.StarkMiError, match="stride"):
        eng.dev_zk_segments(d, h_len, 6, ks, Dp, d, d, out_stride=n - 1)
    del t
