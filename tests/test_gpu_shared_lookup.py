"""GPU: shared-table lookups (include/stark_mi.h, "Shared-table lookups") -- the shared instantiations of the column build, the
count launch of the multiplicity helper and both auxiliary-quotient launches, the four list provers and their verifiers --
against the Python restatement (tests/shared_lookup_compose.py: the shared column as the sum of J single-lookup columns,
the quotients with the denominators multiplied out) and the CPU emulator.  Every comparison is exact, at both project primes.

log_n 1, 2, 5, 10, 11: below one lane, one lane, a few lanes, exactly one workgroup of 1024 rows, the first size with two.
The zero-knowledge composition needs k_t = 8 t + 16 < n / 2: its cases are log_n 6 and 7.  The row-leaves prover needs
E = B / D >= 4: J = 2 runs at log_blowup 4 and J = 4, whose D is 8, at log_blowup 5 (2^5 rows there)."""
import numpy as np
import pytest

import air_compose as ac
import args_compose as agc
import deep_compose as dc
import ext_compose as xc
import perm_compose as pm
import shared_lookup_compose as sl
import xargs_compose as xg
import zk_args_compose as za
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_ext import _dev_cols
from test_lookup_emu import chall
from test_shared_lookup_emu import (COLUMN_CASES, COMPOSE_CASES, compose_inputs, emu, emu_columns, emu_compose, emu_mult, scene, with_args,  # noqa: F401
                                    zero_cases)

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
ROWS = dict(row_leaves=True, ext=True)
DEEP = dict(row_leaves=True, ext=True, deep_args=True)
FOLD4 = dict(row_leaves=True, ext=True, deep_args=True, coset_leaves=True)


def gpu_columns(eng, air, cols, args, ch, c_stride=None, lead=0):
    """-> (c (4 A, n) uint64, closes); the words in front of c, between its columns and behind the last stay untouched"""
    cols = np.asarray(cols, dtype=np.uint64)
    n_cols, n = cols.shape
    A = len(args)
    c_stride = n if c_stride is None else c_stride
    with Dev(eng) as dev:
        d_trace = dev.upload(cols)
        ct, d_c = _dev_cols(np.full((4 * A, n), 0x7ffffffe, dtype=np.uint32), c_stride, lead)
        closes = eng.dev_args_columns(with_args(air, args), d_trace, n_cols, n.bit_length() - 1, ch, d_c, c_stride)
        eng.sync()
        whole = ct.cpu().numpy().view(np.uint32)
    assert np.all(whole[:lead] == 0x7fffffff)
    host = whole[lead:]
    for e in range(4 * A):
        assert np.all(host[e * c_stride + n:(e + 1) * c_stride] == 0x7fffffff)
    return np.stack([host[e * c_stride:e * c_stride + n] for e in range(4 * A)]).astype(np.uint64), closes


def gpu_mult(eng, air, cols, args, a, rows=None):
    """-> M as a list; guard words on either side of d_mult stay untouched"""
    cols = np.asarray(cols, dtype=np.uint64)
    n_cols, n = cols.shape
    with Dev(eng) as dev:
        d_trace = dev.upload(cols)
        mt, d_m = _dev_cols(np.full((1, n), 0x7ffffffe, dtype=np.uint32), n + 3, 1)
        try:
            if rows is None:
                eng.dev_args_multiplicities(with_args(air, args), a, d_trace, n_cols, n.bit_length() - 1, d_m)
            else:
                eng.dev_xargs_multiplicities_rows(with_args(air, args), a, d_trace, n_cols, n.bit_length() - 1, rows, d_m)
        finally:
            eng.sync()
            whole = mt.cpu().numpy().view(np.uint32)
            assert whole[0] == 0x7fffffff and np.all(whole[1 + n:] == 0x7fffffff)
    return [int(v) for v in whole[1:1 + n]]


# ---------------------------------------------------------------------------------------------- columns and multiplicities
@pytest.mark.parametrize("log_n,J,m,sels,periodic", COLUMN_CASES)
def test_dev_columns_and_multiplicities_equal_the_restatement_and_the_emulator(engines, emu, log_n, J, m, sels, periodic):
    p, g = xc.PRIMES[(log_n + J) % 2]
    eng, n = engines[p], 1 << log_n
    air, cols, args = scene(log_n, p, J, m, sels, periodic)
    W = air.n_cols
    ch = chall(log_n + J)
    wide = xg.widen(cols, air, p)
    c, closes = gpu_columns(eng, air, cols, args, ch)
    assert closes == [True]
    st, ce, _closes, _key = emu_columns(emu, air, cols, args, ch, p, g)
    assert st == 0 and np.array_equal(c, ce)
    assert sl.recurrences_hold(c, wide, args, ch, p, g, W) == [(True, True)]
    if log_n <= 5:
        want, want_closes, zero = sl.columns(wide, args, ch, p, g, W)
        assert zero is None and want_closes == [True] and np.array_equal(c, want)
    c4, got = gpu_columns(eng, air, cols, args, ch, c_stride=n + 1)      # the 4-byte path: an odd stride, then a base off 16 bytes
    assert np.array_equal(c4, c) and got == [True]
    c4, got = gpu_columns(eng, air, cols, args, ch, c_stride=n + 4, lead=1)
    assert np.array_equal(c4, c) and got == [True]
    blank = [list(col) for col in cols]
    blank[W - 1] = [7] * n                                               # the helper does not read mult_col
    M, missing = sl.multiplicities(wide, args[0], W)
    assert missing is None
    assert gpu_mult(eng, air, blank, args, 0) == M == cols[W - 1] == emu_mult(emu, air, cols, args, 0, p, g, 0)[1]


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_two_tuples_of_a_row_and_the_rows_of_a_wave_hit_one_table_row(engines, p, g):
    """tuple 1 reads tuple 0's table row on every even row; the first 64 rows of tuple 0 -- one wave -- all read table row 0,
    which collects at least 96 counts; the row bound leaves out the lookups and the table rows from `rows` on"""
    log_n = 10
    air, cols, args = scene(log_n, p, 2, 2)
    W = air.n_cols
    assert cols[W - 1][0] >= 96 and sum(cols[W - 1]) == 2 << log_n
    assert gpu_mult(engines[p], air, cols, args, 0) == cols[W - 1]
    air, cols, args = scene(log_n, p, 2, 2, rows=900)
    assert not any(cols[W - 1][900:]) and sum(cols[W - 1]) == 2 * 900
    assert gpu_mult(engines[p], air, cols, args, 0, rows=900) == cols[W - 1]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("J,log_n", [(2, 5), (4, 5), (3, 11)])
def test_the_shared_column_is_the_sum_of_the_devices_single_columns(engines, p, g, J, log_n):
    """on the device: the J single lookups as a list of J arguments over a trace with J multiplicity columns that hold the
    shares -- their columns add up to the shared column, coordinate by coordinate"""
    from stark_rs_amd.mirror import Air
    m, n = 2, 1 << log_n
    air, cols, args = scene(log_n, p, J, m, "mixed")
    W = air.n_cols
    ch = chall(9)
    c, closes = gpu_columns(engines[p], air, cols, args, ch)
    assert closes == [True]
    Ms, _ = sl.shares(xg.widen(cols, air, p), args[0], W)
    split = Air(W + J)
    split.periodics = air.periodics
    singles = [one[:3] + (W + j,) + one[4:] for j, one in enumerate(sl.singles(args[0]))]
    cs, closes = gpu_columns(engines[p], split, [list(col) for col in cols] + Ms, singles, ch)
    assert closes == [True] * J
    total = np.zeros((4, n), dtype=np.uint64)
    for j in range(J):
        total = (total + cs[4 * j:4 * j + 4]) % np.uint64(p)
    assert np.array_equal(total, c)


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,J", [(2, 2), (5, 4)])
def test_zero_denominators_are_named_by_row_argument_side_and_the_next_call_succeeds(engines, p, g, log_n, J):
    import stark_rs_amd as s
    n, eng = 1 << log_n, engines[p]
    air, cols, args = scene(log_n, p, J, 1, periodic=False, extra=True)
    args = [args[1], args[0], args[2]]                                   # the shared lookup in the middle: a = 1
    W = air.n_cols
    good = sl.columns(xg.widen(cols, air, p), args, chall(4), p, g, W)[0]
    seen = set()
    for ch, (row, a, side) in zero_cases(air, cols, args, W, n, p, g):
        what = "g_R" if args[a][0] == "perm" else "f_T" if side == (J if a == 1 else 1) else f"f_{side} (tuple {side})" if a == 1 else "f_L"
        with pytest.raises(s.StarkMiError) as ei:
            gpu_columns(eng, air, cols, args, ch)
        assert ei.value.status == -1 and f"argument {a}: {what} is zero in row {row}: no inverse" in str(ei.value), (str(ei.value), row, a, side)
        seen.add((a, side))
        c, closes = gpu_columns(eng, air, cols, args, chall(4))          # the context stays usable
        assert all(closes) and np.array_equal(c, good)
    assert {(1, side) for side in range(J + 1)} <= seen


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_a_missing_tuple_is_named_by_row_and_tuple_and_an_unselected_one_is_not(engines, p, g):
    import stark_rs_amd as s
    eng = engines[p]
    air, cols, args = scene(5, p, 3, 2, "trace")
    W = air.n_cols
    arg = args[0]
    sel1, sel2 = cols[arg[4][1]], cols[arg[4][2]]
    on, on2 = [r for r in range(32) if sel1[r]], [r for r in range(32) if sel2[r]]
    assert cols[arg[1][1][0]][sel1.index(0)] >= p - 3                    # an unselected cell holds a value outside the table
    assert gpu_mult(eng, air, cols, args, 0) == cols[W - 1]
    bad = [list(c) for c in cols]
    for j, r in ((2, on2[-1]), (1, on[1]), (2, on[1]), (1, on[2])):
        bad[arg[1][j][0]][r] = p - 2
    _M, first = sl.multiplicities(xg.widen(bad, air, p), arg, W)
    assert first == (on[1], 1)
    with pytest.raises(s.StarkMiError) as ei:
        gpu_mult(eng, air, bad, args, 0)
    assert ei.value.status == -56 and f"argument 0: tuple 1 of row {on[1]}, which its selector selects, is in no selected table row" in str(ei.value)
    assert gpu_mult(eng, air, cols, args, 0) == cols[W - 1]


# ---------------------------------------------------------------------------------------------- the compositions
def gpu_compose(eng, air, args, lde, cl, ch, wch, log_n, lb, h, stride, c_stride, out_stride, lead, t=None):
    N = 1 << (log_n + lb)
    with Dev(eng) as dev:
        _lt, d_lde = _dev_cols(lde.astype(np.uint32), stride, lead)
        _zt, d_cl = _dev_cols(cl.astype(np.uint32), c_stride, lead)
        ot, d_out = _dev_cols(np.zeros((4, N), dtype=np.uint32), out_stride, lead)
        d_w = dev.upload_u64(wch)
        if t is None:
            eng.dev_air_compose_args(with_args(air, args), d_lde, d_cl, len(lde), log_n, lb, ch, d_w, d_out, stride=stride, c_stride=c_stride,
                                     out_stride=out_stride, lde_offset=h)
        else:
            eng.dev_air_compose_zk_args(with_args(air, args), d_lde, d_cl, len(lde), log_n, lb, t, ch, d_w, d_out, stride=stride, c_stride=c_stride,
                                        out_stride=out_stride)
        eng.sync()
        host = ot.cpu().numpy().view(np.uint32)
    assert np.all(host[:lead] == 0x7fffffff)
    host = host[lead:]
    for e in range(4):
        assert np.all(host[e * out_stride + N:(e + 1) * out_stride] == 0x7fffffff)
    return np.stack([host[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)


def paths(N):
    """aligned (16-byte accesses); every stride odd; bases off 16 bytes"""
    return ((N, N, N, 0), (N + 1, N + 3, N + 5, 0), (N + 4, N + 4, N + 4, 1))


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,lb,J,m,sels", COMPOSE_CASES)
def test_dev_air_compose_xargs_equals_the_restatement_and_the_emulator(engines, oracle, emu, p, g, log_n, lb, J, m, sels):
    eng, h, tau = engines[p], g, 1
    N = 1 << (log_n + lb)
    air, cols, args = scene(log_n, p, J, m, sels, extra=True)
    W, K, ch, wch, lde_wide, cl = compose_inputs(oracle, air, cols, args, p, g, log_n, lb, tau, h, 2)
    want = pm.main_codeword(oracle, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
    want = (want + sl.aux_terms(oracle, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W)) % np.uint64(p)
    assert np.array_equal(emu_compose(emu, air, args, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, tau, h), want)
    for stride, c_stride, out_stride, lead in paths(N):
        got = gpu_compose(eng, air, args, lde_wide[:W], cl, ch, wch, log_n, lb, h, stride, c_stride, out_stride, lead)
        assert np.array_equal(got, want), (stride, lead)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,lb,J,m,sels", [(6, 2, 2, 1, "mixed"), (6, 3, 4, 2, "mixed"), (7, 3, 3, 8, "trace"), (7, 2, 2, 2, "periodic")])
def test_dev_air_compose_zk_xargs_equals_the_restatement_and_the_emulator(engines, oracle, emu, p, g, log_n, lb, J, m, sels):
    eng, h, tau, t = engines[p], g, 1, 1
    N = 1 << (log_n + lb)
    air, cols, args = scene(log_n, p, J, m, sels, extra=True)
    dair = za.derived_air(air, log_n, t, p, tau, oracle.ff_prim_nth_root_g(1 << log_n, p, g))
    W, K, ch, wch, lde_wide, cl = compose_inputs(oracle, air, cols, args, p, g, log_n, lb, tau, h, 3, dair)
    want = dc.composition(oracle, dair, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
    want = (want + sl.zk_aux_terms(oracle, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W, t, len(lde_wide) - 1)) % np.uint64(p)
    assert np.array_equal(emu_compose(emu, air, args, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, tau, h, t=t), want)
    for stride, c_stride, out_stride, lead in paths(N):
        got = gpu_compose(eng, air, args, lde_wide[:W], cl, ch, wch, log_n, lb, h, stride, c_stride, out_stride, lead, t=t)
        assert np.array_equal(got, want), (stride, lead)


def test_compose_on_every_trip_of_the_grid_equals_the_restatement_at_sampled_points(engines):
    """air_xargs_compose_shared_kernel on at least four trips of its grid (tests/test_gpu_perm.py, looping_check: the shape is
    the smallest N with four trips, asserted there; >= 4096 sampled points, the edges of every trip among them).  A shared
    lookup of three tuples with a periodic member, a trace selector and a periodic selector beside a permutation; the periodic
    operands at the sampled points come from their definition (mirror.Air.periodic_at)"""
    from test_gpu_perm import LB, TAU, looping_check
    p, g = xc.PRIMES[1]
    eng = engines[p]
    args = [("lookups", [[0, 1], [2, ("per", 1)], [4, 5]], [("per", 0), 3], 7, [None, 6, ("per", 2)], None), ("perm", [0], [2])]
    rng = np.random.default_rng(3)
    held = {}

    def state(air):
        for P in (2, 8, 4):
            air.periodic([int(v) for v in rng.integers(0, p, P)])
        held["air"] = sl.mirror_air(air, args)

    def restated(idx, lde_at, c_at, c_next, ch, w, wN, log_n):
        air = held["air"]
        wn = pow(wN, 1 << LB, p)
        per_at = np.array([air.periodic_at(p, log_n, TAU, wn, g * pow(wN, int(i), p) % p) for i in idx], dtype=np.uint64).T
        return sl.aux_terms_at(idx, np.concatenate([lde_at, per_at]), c_at, c_next, args, ch, w, p, g, wN, log_n, TAU, g, 8)

    looping_check(eng, p, 8, 4 * len(args), 29, state,
                  lambda air, d_lde, d_c, n_cols, log_n, ch, d_w, d_out: eng.dev_air_compose_args(air, d_lde, d_c, n_cols, log_n, LB, ch, d_w, d_out),
                  restated)


# ---------------------------------------------------------------------------------------------- whole proofs
PROVERS = {"xargs": ROWS, "deep_xargs": DEEP, "deep_xargs_fold4": FOLD4, "deep_zk_xargs": FOLD4}


def shape_of(prover, J):
    """(log_n, log_blowup, t): the smallest shapes of tests/test_gpu_xargs.py, test_gpu_deep_args.py and test_gpu_zk_args.py that
    the degree J + 2 (J + 3 under zk) fits"""
    if prover == "xargs":
        return (5, 4 if J < 4 else 5, 4)
    if prover == "deep_zk_xargs":
        return (6, 2 if J < 3 else 3, 1)
    return (6, 2 if J < 4 else 3, 4)


def statement(prover, J, p, extra):
    log_n, lb, t = shape_of(prover, J)
    rows = (1 << log_n) - za.k_t(t) if prover == "deep_zk_xargs" else None
    return scene(log_n, p, J, 2, "mixed", extra=extra, rows=rows)


def prove(eng, prover, air, args, cols, fill=True, check=True, bits=0):
    log_n, lb, t = shape_of(prover, max(len(g_[1]) if sl.is_shared(g_) else 1 for g_ in args))
    cols = [list(c) for c in cols]
    if fill:                                                             # the device fills every multiplicity column
        for g_ in args:
            if g_[0] != "perm":
                cols[g_[3]] = [0] * len(cols[0])
    kw = dict(PROVERS[prover], zk=SEED) if prover == "deep_zk_xargs" else PROVERS[prover]
    with Dev(eng) as dev:
        return eng.dev_air_prove(with_args(air, args), dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, lb, t, grind_bits=bits, check=check,
                                 fill_multiplicities=fill, **kw)


def verify(eng, prover, air, args, res, J, bits=0):
    log_n, lb, t = shape_of(prover, J)
    kw = dict(PROVERS[prover], zk=True) if prover == "deep_zk_xargs" else PROVERS[prover]
    return eng.air_verify(with_args(air, args), res["proof"], res["column_roots"], air.n_cols, log_n, lb, t, grind_bits=bits, **kw)


def layout_len(eng, prover, air, args, J):
    log_n, lb, t = shape_of(prover, J)
    W, A, f = air.n_cols, len(args), with_args(air, args)
    if prover == "xargs":
        N, (_d, E) = 1 << (log_n + lb), eng.air_plan(f, W, log_n, lb)
        g = dict(xc.PRIMES)[eng.p]
        return agc.proof_len(N, E, t, eng.fri_num_rounds(eng.fri_cfg(pow(g, (eng.p - 1) // N, eng.p), g, N, E, t)), W, A)
    if prover == "deep_xargs":
        return eng.air_plan_deep_args(f, W, log_n, lb, num_colinearity_tests=t)[2]
    if prover == "deep_xargs_fold4":
        return eng.air_deep_args_fold4_layout(f, W, log_n, lb, t)[1]
    return eng.air_deep_zk_args_layout(f, W, log_n, lb, t)[1]


@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("J", [2, 4])
@pytest.mark.parametrize("prover", list(PROVERS))
def test_the_four_list_provers(engines, prover, J, extra):
    """a shared lookup alone, and in a list with a permutation and a single lookup: the device fills the multiplicities (over
    the active rows under zk), the proof verifies, its length is the layout function's, closes is set"""
    p, g = xc.PRIMES[(J // 2 + extra) % 2]
    eng = engines[p]
    air, cols, args = statement(prover, J, p, extra)
    res = prove(eng, prover, air, args, cols)
    assert res["closes"] == [True] * len(args)
    assert len(res["proof"]) == layout_len(eng, prover, air, args, J)
    ok, why = verify(eng, prover, air, args, res, J)
    assert ok, why
    handed = prove(eng, prover, air, args, cols, fill=False)             # the caller's own multiplicities: the same statement
    assert handed["closes"] == res["closes"] and (prover == "deep_zk_xargs" or handed["proof"] == res["proof"])


@pytest.mark.parametrize("J", [2, 4])
@pytest.mark.parametrize("prover", list(PROVERS))
def test_the_verifiers_reject_another_list_and_a_corrupted_multiplicity(engines, prover, J):
    import stark_rs_amd as s
    p, g = xc.PRIMES[J // 2 % 2]
    eng = engines[p]
    air, cols, args = statement(prover, J, p, True)
    res = prove(eng, prover, air, args, cols, fill=False)
    ok, why = verify(eng, prover, air, args, res, J)
    assert ok, why
    shared = args[0]
    changed = [list(t) for t in shared[1]]
    changed[J - 1][1] = shared[1][0][1]                                  # one operand of the last tuple
    dropped = [None if j == 1 else x for j, x in enumerate(shared[4])]   # "mixed": tuple 1 has a trace selector
    assert shared[4][1] is not None
    others = {"J - 1 tuples": [sl.fewer(shared, J - 1)] + args[1:],
              "one changed operand": [("lookups", changed) + shared[2:]] + args[1:],
              "one dropped selector": [shared[:4] + (dropped, shared[5])] + args[1:],
              "the J single lookups": sl.singles(shared) + args[1:]}
    for name, other in others.items():
        try:
            ok, why = verify(eng, prover, air, other, res, J)
        except s.StarkMiError as e:                                      # a list this shape cannot carry is refused outright
            ok, why = False, str(e)
        assert not ok and why, name
    bad = [list(c) for c in cols]
    bad[shared[3]][3] = (bad[shared[3]][3] + 1) % p
    with pytest.raises(s.StarkMiError, match=r"the arguments \[0\] do not close"):
        prove(eng, prover, air, args, bad, fill=False)
    res = prove(eng, prover, air, args, bad, fill=False, check=False)
    assert res["closes"] == [False, True, True]
    ok, why = verify(eng, prover, air, args, res, J)
    assert not ok and why
