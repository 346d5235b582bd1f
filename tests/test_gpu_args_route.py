"""GPU: the plain argument list on the operand list's kernels (xargs_block_kernel, air_xargs_compose_kernel) at the shapes where
that route could differ from a list of its own: an AIR WITH periodic columns, whose tables the kernels are handed and must not
read, two rows, and the smallest blowup the plan accepts.  Against the restatement (tests/args_compose.py) and the emulator;
every comparison is exact.  The column build at two rows, on the 4-byte path too, is tests/test_gpu_args.py's already (its
LOG_NS starts at 1).  `pytest -m gpu`."""
import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import args_compose as agc
import ext_compose as xc
import perm_compose as pm
from test_args_emu import SPECS, case, emu, emu_compose  # noqa: F401  (emu is a fixture)
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_args import KW, TAU, U64_MAX
from test_gpu_ext import _dev_cols
from test_lookup_emu import chall

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_prove_args_over_an_air_with_periodic_columns(engines, oracle, p, g):
    """the mixer of tests/air_periodic.py: one periodic column of period n, the largest the AIR accepts, and one of period 1,
    beside the list [perm m = 1, lookup m = 1] over columns of its own.  Bytes and roots are the restatement's."""
    log_n, lb, t, bits = 3, 3, 4, 8
    eng, n = engines[p], 1 << log_n
    air, cols = ap.make("public", n, p)
    assert [len(v) for v in air.periodics] == [n, 1]
    W0 = len(cols)
    more, args = agc.pool(n, p, 9, [("perm", 1), ("lookup", 1)], first=W0)
    air.n_cols = W0 + len(more)
    agc.mirror_air(air, args)
    cols = [list(c) for c in cols] + more
    W = len(cols)
    d, E = eng.air_plan(air, W, log_n, lb)
    assert (d, E) == (agc.plan(air, args, lb)[0], agc.plan(air, args, lb)[2])
    with Dev(eng) as dev:
        res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, grind_bits=bits, **KW)
    want = agc.prove(oracle, air, args, cols, p, g, log_n, lb, t, TAU, g, E, bits)
    assert res["closes"] == want["closes"] == [True, True]
    assert res["column_roots"].tobytes() == want["roots"]
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **KW)
    assert ok, why


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name,log_n,lb", [("PL", 1, 3), ("P", 1, 2), ("P", 4, 2)])
def test_compose_args_at_two_rows_and_at_the_smallest_blowup(engines, oracle, emu, p, g, name, log_n, lb):
    """n = 2 is below one lane's four rows; log_blowup = 2 is the smallest the plan accepts for permutations alone, 3 with a
    lookup: B = 4 points a row, so the next row of a lane's four points is the lane's neighbour"""
    eng, h = engines[p], g
    n, N = 1 << log_n, 1 << (log_n + lb)
    air, cols, args = case(n, p, SPECS[name])
    W, K, A = len(cols), len(air.constraints), len(args)
    assert eng.air_plan(air, W, log_n, lb)[1] == agc.plan(air, args, lb)[2] == 4
    ch = chall(21)
    c, closes, zero = agc.columns(cols, args, ch, p, g)
    assert zero is None and all(closes)
    lde = np.array(ac.lde(oracle, cols, p, g, log_n, lb, TAU, h), dtype=np.uint64)
    cl = np.array(ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, TAU, h), dtype=np.uint64)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 2 * A), dtype=np.uint64)]
    want = pm.main_codeword(oracle, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, TAU, h)
    want = (want + agc.aux_terms(oracle, lde, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, TAU, h)) % np.uint64(p)
    assert np.array_equal(emu_compose(emu, air, lde, cl, ch, wch, p, g, log_n, lb, TAU, h), want)
    # aligned (16-byte accesses); every stride odd and the bases off 16 bytes (4-byte accesses)
    for stride, c_stride, out_stride, lead in ((N, N, N, 0), (N + 1, N + 3, N + 5, 1)):
        with Dev(eng) as dev:
            lt, d_lde = _dev_cols(lde.astype(np.uint32), stride, lead)
            zt, d_cl = _dev_cols(cl.astype(np.uint32), c_stride, lead)
            ot, d_out = _dev_cols(np.zeros((4, N), dtype=np.uint32), out_stride, lead)
            d_w = dev.upload_u64(wch)
            eng.dev_air_compose_args(air, d_lde, d_cl, W, log_n, lb, ch, d_w, d_out, stride=stride, c_stride=c_stride, out_stride=out_stride, lde_offset=h)
            eng.sync()
            host = ot.cpu().numpy().view(np.uint32)[lead:]
        got = np.stack([host[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)
        assert np.array_equal(got, want), (stride, lead)
        for e in range(4):
            assert np.all(host[e * out_stride + N:(e + 1) * out_stride] == 0x7fffffff)

