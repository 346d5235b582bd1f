"""GPU: transition windows of up to four rows at the boundary moduli of tests/test_gpu_boundary_primes.py (THREE: one per range
bound of the lazy reductions) -- the window composition under the unreduced u64 weights with random operands and with every
operand p - 1, smi_dev_poly_eval_ext_shifts, smi_dev_deep_compose_window, the window smi_dev_air_check and one proof over row
leaves and one over coset leaves with their verifiers -- against the restatement (tests/window_compose.py).  Every comparison
is exact.  `pytest -m gpu`."""
import numpy as np
import pytest

import air_compose as ac
import deep_compose as dc
import deep_fold4_compose as dfc
import window_compose as wc
from test_gpu_air import Dev
from test_gpu_air_window import COSETS, ROWS, both_reject, check_codeword, gpu_proof, gpu_window_compose
from test_gpu_boundary_primes import GEN, THREE, _weights, engines, u64_set  # noqa: F401  (engines is a fixture)
from test_gpu_ext import _dev_cols

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- the composition
@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("lb", [2, 4])
@pytest.mark.parametrize("S", [3, 4])
def test_window_compose_at_boundary_moduli(engines, oracle, p, S, lb):
    """N = 2^8: five and 64 columns beside two periodic ones (tiles of 256 and 128 points with a halo of (S - 1) B), degree 2
    where the blowup holds its segments; random operands and every operand p - 1; the unreduced weights of the u64 set; base
    and extension weights; the tiled kernel and the direct one (a stride of N + 3); the first and the last halo on their own"""
    eng, g, B, tau, log_N = engines[p], GEN[p], 1 << lb, 5, 8
    log_n, N, halo = log_N - lb, 1 << log_N, (S - 1) * (1 << lb)
    assert set(_weights(p, 9)) == set(u64_set(p))
    for W, Q in ((5, 2), (64, 2)):
        for extreme in (False, True):
            air, cols = wc.synthetic(W, Q, S, 1 if lb == 2 else 2, p, 1 << log_n, extreme=extreme)
            K = len(air.constraints)
            assert air.window == S and all(c == p - 1 for c in cols[W - 1]) and (not extreme or all(v == p - 1 for c in cols for v in c))
            lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, g)
            for ext in (False, True):
                wts = _weights(p, 4 * (W + K), 1) if ext else _weights(p, W + K)
                want = (wc.compose_ext if ext else wc.compose)(oracle, air, cols, wts, p, g, log_n, lb, tau, g)
                assert want.any()
                for stride in (None, N + 3):
                    got = gpu_window_compose(eng, air, lde, wts, log_n, lb, tau, g, ext, stride)
                    where = (S, lb, W, Q, extreme, ext, stride, wc.air_tile(W + Q, B, N, 4 if ext else 1, S))
                    assert np.array_equal(got[..., :halo], want[..., :halo]), where
                    assert np.array_equal(got[..., N - halo:], want[..., N - halo:]), where
                    assert np.array_equal(got, want), where


# ---------------------------------------------------------------------------------------------- evaluation at z w^s
@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("n_coeffs,n_cols", [(1, 3), (257, 64), ((1 << 16) + 1, 3)])
def test_dev_poly_eval_ext_shifts_at_boundary_moduli(engines, oracle, p, n_coeffs, n_cols):
    """one column all p - 1; z random and all p - 1; 16-byte loads, and 4-byte loads from an unaligned base"""
    import torch
    eng, g = engines[p], GEN[p]
    w = oracle.ff_prim_nth_root_g(1 << 10, p, g)
    rng = np.random.default_rng(n_coeffs + n_cols)
    cols = rng.integers(0, p, (n_cols, n_coeffs), dtype=np.uint64)
    cols[n_cols // 2] = p - 1
    for z in ([int(v) for v in rng.integers(1, p, 4)], [p - 1] * 4):
        pts = wc.shifts_of(z, w, 4, p)
        vals = [dc.eval_cols(cols, pt, p, g) for pt in pts]
        for stride, lead in ((None, 0), (n_coeffs + 5, 1)):
            t, d = _dev_cols(cols, stride, lead)
            torch.cuda.synchronize()
            for S in (3, 4):
                got = eng.dev_poly_eval_ext_shifts(d, n_cols, n_coeffs, z, w, S, stride)
                assert got == [[vals[s][c] for s in range(S)] for c in range(n_cols)], (n_coeffs, z, stride, S)
            del t


# ---------------------------------------------------------------------------------------------- the DEEP codeword
@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("log_N", [6, 10])
def test_dev_deep_compose_window_at_boundary_moduli(engines, oracle, p, log_N):
    """the combinations of dc.compose_combos, S in {3, 4} (and 2 beside the two-row kernel), random operands and every operand
    p - 1 under challenges of the u64 set, 16-byte and 4-byte loads"""
    check_codeword(engines[p], oracle, p, GEN[p], log_N)


# ---------------------------------------------------------------------------------------------- the check on the trace
@pytest.mark.parametrize("p", THREE)
def test_dev_air_check_window_at_boundary_moduli(engines, p):
    eng, log_n = engines[p], 8
    n = 1 << log_n
    for name, col in (("sq", 0), ("wide", 2)):
        air, cols = wc.make(name, n, p)
        S = air.window
        assert wc.wrapped_violations(air, p, cols) == list(range(n - S + 1, n))
        bad = [list(c) for c in cols]
        bad[col][n - 1] = (bad[col][n - 1] + 1) % p
        with Dev(eng) as dev:
            assert eng.dev_air_check(air, dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n)[0], name
            ok, con, row, why = eng.dev_air_check(air, dev.upload(np.array(bad, dtype=np.uint64)), len(cols), log_n)
        assert not ok and row == n - S and (con, row) == air.first_violation(p, bad), (name, why)
        assert f"rows {n - S} .. {n - 1}" in why


# ---------------------------------------------------------------------------------------------- the proofs
@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("name,cosets", [("tap4", False), ("wide", True)])
def test_window_proofs_at_boundary_moduli(engines, oracle, p, name, cosets):
    eng, g, log_n, lb, t, kw = engines[p], GEN[p], 5, 3, 4, COSETS if cosets else ROWS
    assert dfc.folds(log_n, lb, t) >= 1
    air, cols = wc.make(name, 1 << log_n, p)
    W, S = len(cols), air.window
    res = gpu_proof(eng, air, cols, log_n, lb, t, kw)
    want = wc.prove(oracle, air, cols, p, g, log_n, lb, t, 1, g, 0, cosets)
    assert [bytes(r) for r in res["column_roots"]] == want["roots"]
    assert [c for el in res["ood"] for c in el] == want["ood"] and len(res["ood"]) == S * W + wc.plan(air, log_n)[1]
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=0, **kw)
    assert ok, why
    assert wc.verify(oracle, air, res["proof"], want["roots"], p, g, W, log_n, lb, t, 1, g, 0, cosets) == (True, "")
    b = bytearray(res["proof"])
    b[9 + 8 * 4 * (2 * W)] ^= 1                                              # u_{2,0} in the record
    both_reject(eng, oracle, air, bytes(b), res["column_roots"], p, g, W, log_n, lb, t, cosets, reason="consistency")
