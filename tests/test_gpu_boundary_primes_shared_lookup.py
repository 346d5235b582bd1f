"""Shared-table lookups at the moduli of tests/test_gpu_boundary_primes.py with the edge operands of
tests/test_gpu_boundary_primes_xargs.py.  The fold of csrc/xargs_core.h adds plain-times-Montgomery products of its own --
Nn f_j and S_j P in xshared_fold, Nn f_T and (M S_b) P in xshared_lane_deltas and xshared_compose_point -- and takes any
residue as a selector cell.  Operands on the bounds:
  "pm1"   every tuple cell and every table cell p - 1 (all J n tuples hit table row 0, whose multiplicity is J n);
  "wide"  the trace selectors of the tuples overwritten by the edge set {0, 1, p - 1, p - 2, (p - 1) / 2, (p + 1) / 2} tiled
          (such a list need not close: the column and the quotients are what is compared);
under the four challenge sets (random, the unreduced u64 set around 0, p, 2^32 and 2^64, all 2^64 - 1, all p - 1) and
unreduced u64 weights.  References: tests/shared_lookup_compose.py, which takes (p, g): row by row up to 2^5 rows, by the
multiplied-out recurrences at 2^10 and 2^11 rows, where the emulator's column is the one compared word for word.  Every
comparison is exact.  The J n >= p refusal is met at the smallest modulus, 12289 = 3 * 2^12 + 1, with 2^12 rows.
Without a GPU the lane code runs in the CPU emulator; `pytest -m gpu` for the kernels.
No case is left out for a prime's two-adicity: the largest domain is 2^11 rows, the compositions run on 2^5 rows at blowup 8
and on 2^6 rows at blowup 4 and 8, and the smallest two-adicity of the table is 12 -- 0 cases."""
import copy

import numpy as np
import pytest

import deep_compose as dc
import perm_compose as pm
import shared_lookup_compose as sl
import xargs_compose as xg
import zk_args_compose as za
from test_gpu_boundary_primes import ADICITY, ALL, GEN, engines  # noqa: F401  (engines is a fixture)
from test_gpu_boundary_primes_args import CH_NAMES, challenge_sets, weights
from test_shared_lookup_emu import compose_inputs, emu, emu_columns, emu_compose, emu_mult, scene  # noqa: F401  (emu is a fixture)

EDGES = ["pm1", "wide"]
SMALL_LOGS, LARGE_LOGS = [2, 5], [10, 11]
COMPOSE = [(5, 3, 3, 2), (6, 2, 2, 1), (6, 3, 4, 2)]                      # (log_n, log_blowup, J, m); the last two also under zk
assert min(ADICITY.values()) >= max(log_n + lb for log_n, lb, _J, _m in COMPOSE) and min(ADICITY.values()) >= 12


def edge_tile(p, count, shift=0):
    tile = [0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    return [tile[(r + shift) % 6] for r in range(count)]


_edge = {}


def bscene(log_n, p, J, m, edge, extra=False):
    """-> (air, cols, args): test_shared_lookup_emu.scene with trace selectors on every tuple, then the edge"""
    key = (log_n, p, J, m, edge, extra)
    if key not in _edge:
        air, cols, args = scene(log_n, p, J, m, "trace", extra=extra)
        n, W = 1 << log_n, air.n_cols - (4 if extra else 0)
        assert J * n < p
        cols = [list(c) for c in cols]
        shared = args[0]
        if edge == "pm1":
            air = copy.copy(air)
            air.periodics = [[p - 1] * len(v) if j == 0 else list(v) for j, v in enumerate(air.periodics)]
            for c in [c for t in shared[1] for c in t] + [c for c in shared[2] if not isinstance(c, tuple)]:
                cols[c] = [p - 1] * n
            M, missing = sl.multiplicities(xg.widen(cols, air, p), shared, air.n_cols)
            assert missing is None and M[0] == sum(sum(cols[s]) for s in shared[4]) and not any(M[1:])
            cols[shared[3]] = M
        else:
            for k, s in enumerate(sorted(set(shared[4]))):
                cols[s] = edge_tile(p, n, k)
        _edge[key] = (air, cols, args)
    return _edge[key]


def column_cases(p, logs):
    """-> [(log_n, J, m, edge, index of the challenge set, challenges)]: every size x edge under each of the four sets; J and m
    move on from case to case so that every J and every width meets every set at every prime"""
    out = []
    for log_n in logs:
        for ei, edge in enumerate(EDGES):
            for ci, ch in enumerate(challenge_sets(p, 100 * log_n + ei)):
                k = log_n + ei + ci + ALL.index(p)
                out.append((log_n, 2 + k % 3, [1, 2, 8][(k // 3) % 3], edge, ci, ch))
    return out


def check_columns(c, closes, log_n, p, J, m, edge, ci, ch):
    g, what = GEN[p], (log_n, J, m, edge, CH_NAMES[ci])
    air, cols, args = bscene(log_n, p, J, m, edge)
    wide = xg.widen(cols, air, p)
    if log_n <= 5:
        want, want_closes, zero = sl.columns(wide, args, ch, p, g, air.n_cols)
        assert zero is None, what
        assert c.shape == want.shape and np.array_equal(c, want) and closes == want_closes, what
    holds = sl.recurrences_hold(c, wide, args, ch, p, g, air.n_cols)
    assert holds == [(True, closes[0])], what
    assert edge == "wide" or closes == [True], what


# ---------------------------------------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("p", ALL)
def test_emu_columns_and_multiplicities_at_the_bounds(emu, p):
    g = GEN[p]
    for log_n, J, m, edge, ci, ch in column_cases(p, SMALL_LOGS) + column_cases(p, LARGE_LOGS)[ALL.index(p) % 4::4]:
        air, cols, args = bscene(log_n, p, J, m, edge)
        st, c, closes, _ = emu_columns(emu, air, cols, args, ch, p, g)
        assert st == 0, (log_n, J, m, edge, ci)
        check_columns(c, closes, log_n, p, J, m, edge, ci, ch)
        if edge == "pm1" and ci == 0:
            st, M, _ = emu_mult(emu, air, cols, args, 0, p, g, 0)
            assert st == 0 and M == cols[air.n_cols - 1] and M[0] > 0


def composition_case(oracle, p, log_n, lb, J, m, edge, ci, zk):
    """-> (air, args, W, lde, cl, ch, wch, want): the composition of the restatement under challenge set ci and u64 weights"""
    g, tau, t = GEN[p], 1, 1
    air, cols, args = bscene(log_n, p, J, m, edge, extra=True)
    ch = challenge_sets(p, 7 * log_n + J)[ci]
    dair = za.derived_air(air, log_n, t, p, tau, oracle.ff_prim_nth_root_g(1 << log_n, p, g)) if zk else None
    W, K, ch, wch, lde_wide, cl = compose_inputs(oracle, air, cols, args, p, g, log_n, lb, tau, g, 3 if zk else 2, dair, ch=ch,
                                                 weights=lambda count: weights(p, count, ci), closed=False)
    if zk:
        want = dc.composition(oracle, dair, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, g)
        want = (want + sl.zk_aux_terms(oracle, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, g, W, t, len(lde_wide) - 1)) % np.uint64(p)
    else:
        want = pm.main_codeword(oracle, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, g)
        want = (want + sl.aux_terms(oracle, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, g, W)) % np.uint64(p)
    return air, args, W, lde_wide[:W], cl, ch, wch, want


def compose_cases(p):
    """-> [(log_n, lb, J, m, edge, ci, zk)]: every shape x edge x launch, the challenge set moving on from case to case"""
    out = []
    for si, (log_n, lb, J, m) in enumerate(COMPOSE):
        for ei, edge in enumerate(EDGES):
            for zk in ([False, True] if log_n >= 6 else [False]):
                out.append((log_n, lb, J, m, edge, (si + ei + zk + ALL.index(p)) % 4, zk))
    return out


@pytest.mark.parametrize("p", ALL)
def test_emu_compositions_at_the_bounds(oracle, emu, p):
    for log_n, lb, J, m, edge, ci, zk in compose_cases(p):
        air, args, W, lde, cl, ch, wch, want = composition_case(oracle, p, log_n, lb, J, m, edge, ci, zk)
        got = emu_compose(emu, air, args, lde, cl, ch, wch, p, GEN[p], log_n, lb, 1, GEN[p], t=1 if zk else None)
        assert np.array_equal(got, want), (log_n, lb, J, m, edge, CH_NAMES[ci], zk)


# ---------------------------------------------------------------------------------------------- on the card
@pytest.mark.gpu
@pytest.mark.parametrize("p", ALL)
def test_dev_columns_and_multiplicities_at_the_bounds(engines, emu, p):
    from test_gpu_shared_lookup import gpu_columns, gpu_mult
    g, eng = GEN[p], engines[p]
    for log_n, J, m, edge, ci, ch in column_cases(p, SMALL_LOGS) + column_cases(p, LARGE_LOGS)[ALL.index(p) % 4::4]:
        air, cols, args = bscene(log_n, p, J, m, edge)
        n = 1 << log_n
        c, closes = gpu_columns(eng, air, cols, args, ch)
        check_columns(c, closes, log_n, p, J, m, edge, ci, ch)
        st, ce, _closes, _ = emu_columns(emu, air, cols, args, ch, p, g)
        assert st == 0 and np.array_equal(c, ce), (log_n, J, m, edge, ci)
        c4, closes4 = gpu_columns(eng, air, cols, args, ch, c_stride=n + 1 + 3 * (ci % 2), lead=ci % 2)   # the 4-byte path
        assert np.array_equal(c4, c) and closes4 == closes
        if edge == "pm1" and ci == 0:
            assert gpu_mult(eng, air, cols, args, 0) == cols[air.n_cols - 1]


@pytest.mark.gpu
@pytest.mark.parametrize("p", ALL)
def test_dev_compositions_at_the_bounds(engines, oracle, p):
    from test_gpu_shared_lookup import gpu_compose, paths
    eng = engines[p]
    for k, (log_n, lb, J, m, edge, ci, zk) in enumerate(compose_cases(p)):
        air, args, W, lde, cl, ch, wch, want = composition_case(oracle, p, log_n, lb, J, m, edge, ci, zk)
        N = 1 << (log_n + lb)
        for stride, c_stride, out_stride, lead in (paths(N)[0], paths(N)[1 + k % 2]):
            got = gpu_compose(eng, air, args, lde, cl, ch, wch, log_n, lb, GEN[p], stride, c_stride, out_stride, lead, t=1 if zk else None)
            assert np.array_equal(got, want), (log_n, lb, J, m, edge, CH_NAMES[ci], zk, stride, lead)


@pytest.mark.gpu
def test_multiplicities_that_could_wrap_are_refused(engines):
    """12289 = 3 * 2^12 + 1 with 2^12 rows: J = 4 gives J n = 16384 >= p and is refused by every entry point that reads the list,
    before any launch; the context stays usable, and 2^11 rows take J = 4 (J = 3 at 2^12 rows, 12288 < p: the emulator's test)"""
    import stark_rs_amd as s
    from test_gpu_shared_lookup import gpu_columns, gpu_mult
    p = 12289
    g, eng = GEN[p], engines[p]
    air, cols, args = sl.scene(1 << 12, p, 4, 1, periodic=False, seed=1)
    for call in (lambda: gpu_columns(eng, air, cols, args, challenge_sets(p, 1)[0]), lambda: gpu_mult(eng, air, cols, args, 0)):
        with pytest.raises(s.StarkMiError) as ei:
            call()
        assert ei.value.status == -50 and "argument 0: J n >= p" in str(ei.value)
    air, cols, args = sl.scene(1 << 11, p, 4, 1, periodic=False, seed=1)   # J n = 8192 < p
    ch = challenge_sets(p, 1)[0]
    assert gpu_mult(eng, air, cols, args, 0) == cols[air.n_cols - 1]
    c, closes = gpu_columns(eng, air, cols, args, ch)
    assert closes == [True] and sl.recurrences_hold(c, xg.widen(cols, air, p), args, ch, p, g, air.n_cols) == [(True, True)]
