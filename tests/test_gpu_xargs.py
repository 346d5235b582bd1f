"""GPU: the argument list with selectors and periodic members (include/stark_mi.h) -- smi_dev_xargs_multiplicities,
smi_dev_xargs_columns, smi_dev_air_compose_xargs, smi_dev_air_prove_xargs / smi_air_verify_xargs through Engine's routing --
against the restatement (tests/xargs_compose.py), the CPU emulator of the kernels, and, for a list without selectors or
periodic members, the entry points of "Argument list".  Every comparison is exact.  `pytest -m gpu`.

A closing permutation with 0 / 1 selectors selects as many rows on one side as on the other (the selected tuples are equal
as multisets); the lists here select DIFFERENT rows on the two sides."""
import copy

import numpy as np
import pytest

import air_compose as ac
import args_compose as agc
import ext_compose as xc
import perm_compose as pm
import pow_compose as pc
import xargs_compose as xg
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_ext import _dev_cols
from test_lookup_emu import chall
from test_xargs_emu import PERIODS, emu, emu_columns, emu_compose, emu_mult, scene  # noqa: F401  (emu is a fixture)

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
LB, TAU = 3, 1
KW = dict(row_leaves=True, ext=True)
W = xg.W_SCENE


def with_args(air, args, always=False):
    """a copy of air (its periodic columns and constraints) carrying args"""
    a = copy.copy(air)
    a.args, a.xargs_always = [], always
    return xg.mirror_air(a, args)


def gpu_columns(eng, air, cols, args, ch, c_stride=None, lead=0, always=False):
    """-> (c (4 A, n) uint64, closes); the words in front of c, between its columns and behind the last stay untouched"""
    cols = np.asarray(cols, dtype=np.uint64)
    n_cols, n = cols.shape
    A = len(args)
    c_stride = n if c_stride is None else c_stride
    with Dev(eng) as dev:
        d_trace = dev.upload(cols)
        ct, d_c = _dev_cols(np.full((4 * A, n), 0x7ffffffe, dtype=np.uint32), c_stride, lead)
        closes = eng.dev_args_columns(with_args(air, args, always), d_trace, n_cols, n.bit_length() - 1, ch, d_c, c_stride)
        eng.sync()
        whole = ct.cpu().numpy().view(np.uint32)
    assert np.all(whole[:lead] == 0x7fffffff)
    host = whole[lead:]
    for e in range(4 * A):
        assert np.all(host[e * c_stride + n:(e + 1) * c_stride] == 0x7fffffff)
    return np.stack([host[e * c_stride:e * c_stride + n] for e in range(4 * A)]).astype(np.uint64), closes


def gpu_mult(eng, air, cols, args, a):
    """-> M as a list; guard words on either side of d_mult stay untouched"""
    cols = np.asarray(cols, dtype=np.uint64)
    n_cols, n = cols.shape
    with Dev(eng) as dev:
        d_trace = dev.upload(cols)
        mt, d_m = _dev_cols(np.full((1, n), 0x7ffffffe, dtype=np.uint32), n + 3, 1)
        try:
            eng.dev_args_multiplicities(with_args(air, args), a, d_trace, n_cols, n.bit_length() - 1, d_m)
        finally:
            eng.sync()
            whole = mt.cpu().numpy().view(np.uint32)
            assert whole[0] == 0x7fffffff and np.all(whole[1 + n:] == 0x7fffffff)
    return [int(v) for v in whole[1:1 + n]]


# ---------------------------------------------------------------------------------------------- columns and multiplicities
@pytest.mark.parametrize("log_n,A,kind", [(1, 8, "in-lane"), (2, 8, "in-lane"), (2, 8, "public"), (5, 8, "in-lane"), (5, 8, "lane-edge"), (5, 8, "lanes"),
                                          (5, 3, "public"), (5, 8, "mixed"), (11, 3, "in-lane"), (11, 3, "public")])
def test_dev_columns_and_multiplicities_equal_the_restatement_and_the_emulator(engines, emu, log_n, A, kind):
    p, g = xc.PRIMES[log_n % 2]
    eng, n = engines[p], 1 << log_n
    air, cols, args = scene(log_n, p, kind, A=A)
    ch = chall(log_n)
    wide = xg.widen(cols, air, p)
    want, closes, zero = xg.columns(wide, args, ch, p, g, W)
    assert zero is None and all(closes)
    c, got = gpu_columns(eng, air, cols, args, ch)
    assert got == [True] * A and np.array_equal(c, want)
    st, ce, _closes, _key = emu_columns(emu, air, cols, args, ch, p, g)
    assert st == 0 and np.array_equal(c, ce)
    c4, got = gpu_columns(eng, air, cols, args, ch, c_stride=n + 1)      # the 4-byte path: an odd stride, then a base off 16 bytes
    assert np.array_equal(c4, c) and all(got)
    c4, got = gpu_columns(eng, air, cols, args, ch, c_stride=n + 4, lead=1)
    assert np.array_equal(c4, c) and all(got)
    blank = [list(col) for col in cols]
    for arg in args:
        if arg[0] == "lookup":
            blank[arg[3]] = [7] * n                                      # the helper does not read mult_col
    for a, arg in enumerate(args):
        if arg[0] == "lookup":
            assert gpu_mult(eng, air, blank, args, a) == cols[arg[3]] == emu_mult(emu, air, cols, args, a, p, g, 0)[1], a


@pytest.mark.parametrize("edge", ["sel0", "sel1", "pm1"])
def test_dev_columns_on_edge_cells(engines, edge):
    log_n = 5
    p, g = xc.PRIMES[1]
    air, cols, args = scene(log_n, p, "mixed", edge)
    ch = chall(20 + log_n)
    want, closes, zero = xg.columns(xg.widen(cols, air, p), args, ch, p, g, W)
    assert zero is None and all(closes)
    c, got = gpu_columns(engines[p], air, cols, args, ch)
    assert all(got) and np.array_equal(c, want)


def big_scene(n, p, seed):
    """numpy: 2^19 rows.  per 0: a public table of 256 values, per 1: a public selector of period 8.
      0  lookup [c0] in [per 0], mult c2, sel c1        1  perm [c3] sel c4 ~ [c5] sel c6        2  perm [c3] ~ [c7]
      3  lookup [c0] in [c8], mult c9, sel per 1, table_sel per 1   (c8 = per 0 written out)
    -> (air, cols, args, the widened trace)"""
    from stark_rs_amd.mirror import Air
    rng = np.random.default_rng(seed)
    table = rng.permutation(256).astype(np.uint64)
    s1 = np.array([1, 0, 1, 1, 0, 0, 1, 0], dtype=np.uint64)
    air = Air(10)
    j0, j1 = air.periodic([int(v) for v in table]), air.periodic([int(v) for v in s1])
    rows = np.arange(n)
    good = rows[:256][s1[rows[:256] % 8] == 1]                           # table rows of the first period that per 1 selects
    pick = good[rng.integers(0, len(good), n)]
    c0, c1 = table[pick], rng.integers(0, 2, n).astype(np.uint64)
    c2 = np.bincount(pick[c1 == 1], minlength=n).astype(np.uint64)       # the lowest row with a value is in the first period
    c3, c4 = rng.integers(0, p, n).astype(np.uint64), rng.integers(0, 2, n).astype(np.uint64)
    k = int(c4.sum())
    right = np.sort(rng.permutation(n)[:k])
    c5, c6 = rng.integers(0, p, n).astype(np.uint64), np.zeros(n, dtype=np.uint64)
    c5[right], c6[right] = c3[c4 == 1][rng.permutation(k)], 1
    c7, c8 = c3[rng.permutation(n)], table[rows % 256]
    c9 = np.bincount(pick[s1[rows % 8] == 1], minlength=n).astype(np.uint64)
    args = [("lookup", [0], [("per", j0)], 2, 1, None), ("perm", [3], [5], 4, 6), ("perm", [3], [7]), ("lookup", [0], [8], 9, ("per", j1), ("per", j1))]
    cols = np.stack([c0, c1, c2, c3, c4, c5, c6, c7, c8, c9])
    return air, cols, args, np.concatenate([cols, table[rows % 256][None, :], s1[rows % 8][None, :]])


def test_dev_columns_large_by_the_recurrences(engines):
    """2^19 rows: 512 workgroup aggregates per argument, so the reused scan launch goes twice round its loop behind
    xargs_block_kernel.  Every column satisfies its recurrence and closes; the helper's counts are the trace's; with one
    selector cell changed only the arguments that read it drop their bit"""
    log_n = 19
    p, g = xc.PRIMES[log_n % 2]
    n = 1 << log_n
    air, cols, args, wide = big_scene(n, p, log_n)
    ch = chall(log_n)
    c, closes = gpu_columns(engines[p], air, cols, args, ch)
    assert closes == [True] * 4
    assert xg.recurrences_hold(c, wide, args, ch, p, g, 10) == [(True, True)] * 4
    blank = cols.copy()
    blank[2] = blank[9] = 3
    assert np.array_equal(np.array(gpu_mult(engines[p], air, blank, args, 0), dtype=np.uint64), cols[2])
    assert np.array_equal(np.array(gpu_mult(engines[p], air, blank, args, 3), dtype=np.uint64), cols[9])
    bad, bad_wide = cols.copy(), wide.copy()
    at = n - 7
    bad[1][at] = bad_wide[1][at] = 1 - bad[1][at]                        # a selector of argument 0 alone
    c, closes = gpu_columns(engines[p], air, bad, args, ch)
    assert closes == [False, True, True, True]
    assert xg.recurrences_hold(c, bad_wide, args, ch, p, g, 10) == [(True, False), (True, True), (True, True), (True, True)]


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_zero_denominators_and_missing_rows_are_named_and_the_next_call_succeeds(engines, p, g):
    import stark_rs_amd as s
    log_n = 5
    n, eng = 1 << log_n, engines[p]
    air, cols, args = scene(log_n, p, "mixed")
    wide = xg.widen(cols, air, p)
    good = xg.columns(wide, args, chall(4), p, g, W)[0]
    sides = {(0, 1): "f_T", (0, 0): "f_L", (1, 1): "g_R"}
    cases = [(xg.norm(args[0], W)[2], 0), (xg.norm(args[0], W)[2], n - 1), (xg.norm(args[2], W)[1], 3), ([10], cols[7].index(1))]
    for side_cols, row in cases:
        ch = pm.gamma_for_zero(wide, side_cols, chall(4), row, p, g)
        key = xg.columns(wide, args, ch, p, g, W)[2]
        assert key is not None
        a, side = (key & 15) >> 1, key & 1
        with pytest.raises(s.StarkMiError) as ei:
            gpu_columns(eng, air, cols, args, ch)
        assert ei.value.status == -1 and "no inverse" in str(ei.value)
        assert f"argument {a}: {sides[(args[a][0] == 'perm', side)]} is zero in row {key >> 4}:" in str(ei.value), (str(ei.value), key)
        c, closes = gpu_columns(eng, air, cols, args, chall(4))          # the context stays usable
        assert all(closes) and np.array_equal(c, good)
    # the helper: values outside the table in unselected rows are not missed; in selected rows the smallest is named
    on = [r for r in range(n) if cols[6][r]]
    bad = [list(c) for c in cols]
    for r in on[1:3]:
        bad[14][r] = p - 2
    want, first = xg.multiplicities(xg.widen(bad, air, p), args[0], W)
    assert first == on[1]
    with pytest.raises(s.StarkMiError) as ei:
        gpu_mult(eng, air, bad, args, 0)
    assert ei.value.status == -56 and f"argument 0: the tuple of selected row {on[1]} is in no selected table row" in str(ei.value)
    assert gpu_mult(eng, air, cols, args, 0) == cols[8]
    with pytest.raises(s.StarkMiError) as ei:                            # a permutation has no multiplicities
        gpu_mult(eng, air, cols, args, 1)
    assert ei.value.status == -50 and "argument 1 is a permutation" in str(ei.value)
    with Dev(eng) as dev:                                                # ("per", Q) is variable 2 W + Q: periodic column 0 at the NEXT row
        d = dev.alloc(4 * W * n)
        with pytest.raises(s.StarkMiError) as ei:
            eng.dev_args_columns(with_args(air, [("perm", [("per", 3)], [1])]), d, W, log_n, chall(1), d)
        assert ei.value.status == -50 and "argument 0: a_var is a next-row variable" in str(ei.value)


# ---------------------------------------------------------------------------------------------- the composition
def gpu_compose(eng, air, args, lde, cl, ch, wch, log_n, h, stride, c_stride, out_stride, lead, always=False):
    N = 1 << (log_n + LB)
    with Dev(eng) as dev:
        lt, d_lde = _dev_cols(lde.astype(np.uint32), stride, lead)
        zt, d_cl = _dev_cols(cl.astype(np.uint32), c_stride, lead)
        ot, d_out = _dev_cols(np.zeros((4, N), dtype=np.uint32), out_stride, lead)
        d_w = dev.upload_u64(wch)
        eng.dev_air_compose_args(with_args(air, args, always), d_lde, d_cl, len(lde), log_n, LB, ch, d_w, d_out, stride=stride, c_stride=c_stride,
                                 out_stride=out_stride, lde_offset=h)
        eng.sync()
        host = ot.cpu().numpy().view(np.uint32)[lead:]
    for e in range(4):
        assert np.all(host[e * out_stride + N:(e + 1) * out_stride] == 0x7fffffff)
    return np.stack([host[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n,kind,A", [(3, "in-lane", 8), (4, "lane-edge", 3), (5, "mixed", 8), (6, "public", 3), (7, "lanes", 3)])
def test_dev_air_compose_xargs_equals_the_restatement_and_the_emulator(engines, oracle, emu, p, g, log_n, kind, A):
    eng, h = engines[p], g
    N = 1 << (log_n + LB)
    air, cols, args = scene(log_n, p, kind, A=A)
    K = len(air.constraints)
    ch = chall(21)
    wide = xg.widen(cols, air, p)
    c, closes, zero = xg.columns(wide, args, ch, p, g, W)
    assert zero is None and all(closes)
    lde_wide = np.array(ac.lde(oracle, wide, p, g, log_n, LB, TAU, h), dtype=np.uint64)
    lde = lde_wide[:W]
    cl = np.array(ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, LB, TAU, h), dtype=np.uint64)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 2 * A), dtype=np.uint64)]
    want = pm.main_codeword(oracle, air, cols, wch[:4 * (W + K)], p, g, log_n, LB, TAU, h)
    want = (want + xg.aux_terms(oracle, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, LB, TAU, h, W)) % np.uint64(p)
    assert np.array_equal(emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, LB, TAU, h), want)
    # aligned (16-byte accesses); every stride odd; bases off 16 bytes
    for stride, c_stride, out_stride, lead in ((N, N, N, 0), (N + 1, N + 3, N + 5, 0), (N + 4, N + 4, N + 4, 1)):
        got = gpu_compose(eng, air, args, lde, cl, ch, wch, log_n, h, stride, c_stride, out_stride, lead)
        assert np.array_equal(got, want), (stride, lead)


def test_compose_xargs_on_every_trip_of_the_grid_equals_the_restatement_at_sampled_points(engines):
    """air_xargs_compose_kernel on at least four trips of its grid (tests/test_gpu_perm.py, looping_check: the shape is the
    smallest N with four trips, asserted there; >= 4096 sampled points, the edges of every trip among them).  The list has
    periodic members of period 2 and 8, whose tables of 16 and 64 entries are far shorter than a trip, a periodic selector
    and a trace selector; the periodic operands at the sampled points come from their definition (mirror.Air.periodic_at)"""
    from test_gpu_perm import looping_check
    p, g = xc.PRIMES[1]
    eng = engines[p]
    args = [("lookup", [4], [("per", 0)], 6, 5, None), ("perm", [0, ("per", 1)], [2, 3], ("per", 2), 1), ("lookup", [0, 1], [("per", 1), ("per", 0)], 7)]
    rng = np.random.default_rng(3)
    held = {}

    def state(air):
        for P in (2, 8, 4):
            air.periodic([int(v) for v in rng.integers(0, p, P)])
        held["air"] = xg.mirror_air(air, args)

    def restated(idx, lde_at, c_at, c_next, ch, w, wN, log_n):
        air = held["air"]
        wn = pow(wN, 1 << LB, p)
        per_at = np.array([air.periodic_at(p, log_n, TAU, wn, g * pow(wN, int(i), p) % p) for i in idx], dtype=np.uint64).T
        return xg.aux_terms_at(idx, np.concatenate([lde_at, per_at]), c_at, c_next, args, ch, w, p, g, wN, log_n, TAU, g, 8)

    looping_check(eng, p, 8, 4 * len(args), 23, state,
                  lambda air, d_lde, d_c, n_cols, log_n, ch, d_w, d_out: eng.dev_air_compose_args(air, d_lde, d_c, n_cols, log_n, LB, ch, d_w, d_out),
                  restated)


# ---------------------------------------------------------------------------------------------- whole proofs
def gpu_prove(eng, air, cols, log_n, t, bits, **kw):
    with Dev(eng) as dev:
        return eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, LB, t, grind_bits=bits, **KW, **kw)


@pytest.mark.parametrize("name", ["LPL", "EIGHT"])
def test_a_plain_list_gives_every_byte_of_the_argument_list(engines, oracle, name):
    """the anchor: no selector, no periodic member -> the proof, the roots, the columns and the codeword of the old entry points"""
    from test_args_emu import SPECS, case
    log_n, t, bits = 6, 4, 8
    p, g = xc.PRIMES[name == "EIGHT"]
    eng, N = engines[p], 1 << (log_n + LB)
    air, cols, args = case(1 << log_n, p, SPECS[name])
    n_cols, K, A = len(cols), len(air.constraints), len(args)
    new = with_args(air, args, always=True)
    assert air.flatten(p).xargs is None and new.flatten(p).args is None
    assert eng.air_plan(air, n_cols, log_n, LB) == eng.air_plan(new, n_cols, log_n, LB)
    a, b = gpu_prove(eng, air, cols, log_n, t, bits), gpu_prove(eng, new, cols, log_n, t, bits, timed=True)
    assert a["closes"] == b["closes"] == [True] * A
    assert a["proof"] == b["proof"] and a["column_roots"].tobytes() == b["column_roots"].tobytes() and a["top_indices"] == b["top_indices"]
    assert list(b["stage_ms"]) == ["lde", "commit", "args", "compose", "fri", "open"]
    for air_v, res in ((air, b), (new, a)):
        ok, why = eng.air_verify(air_v, res["proof"], res["column_roots"], n_cols, log_n, LB, t, grind_bits=bits, **KW)
        assert ok, why
    a_look = next(a for a, arg in enumerate(args) if arg[0] == "lookup")   # Engine.dev_args_multiplicities on a plain list: the old helper
    assert gpu_mult(eng, air, cols, args, a_look) == [int(v) for v in cols[args[a_look][3]]]
    ch = chall(5)
    c_old, _ = gpu_columns(eng, air, cols, args, ch)
    c_new, _ = gpu_columns(eng, air, cols, args, ch, always=True)
    assert np.array_equal(c_old, c_new)
    lde = np.array(ac.lde(oracle, cols, p, g, log_n, LB, TAU, g), dtype=np.uint64)
    cl = np.array(ac.lde(oracle, [[int(v) for v in c_old[e]] for e in range(4 * A)], p, g, log_n, LB, TAU, g), dtype=np.uint64)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (n_cols + K + 2 * A), dtype=np.uint64)]
    cw = [gpu_compose(eng, air, args, lde, cl, ch, wch, log_n, g, N, N, N, 0, always) for always in (False, True)]
    assert np.array_equal(cw[0], cw[1])


@pytest.mark.parametrize("bits", [0, 8])
@pytest.mark.parametrize("log_n,A", [(5, 8), (6, 3)])
def test_prove_xargs_bytes_equal_the_restatement_and_verify_agrees(engines, oracle, log_n, A, bits):
    t = 4
    p, g = xc.PRIMES[bits % 3 % 2]
    eng, n, N = engines[p], 1 << log_n, 1 << (log_n + LB)
    base, cols, args = scene(log_n, p, "mixed", A=A)
    air = with_args(base, args)
    d, E = eng.air_plan(air, W, log_n, LB)
    assert (d, E) == (xg.plan(air, args, LB)[0], xg.plan(air, args, LB)[2])
    res = gpu_prove(eng, air, cols, log_n, t, bits, timed=True)
    want = xg.prove(oracle, air, args, cols, p, g, log_n, LB, t, TAU, g, E, bits)
    assert want["closes"] == res["closes"] == [True] * A
    assert res["column_roots"].tobytes() == want["roots"]
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    assert list(res["stage_ms"]) == ["lde", "commit", "args", "compose", "fri", "open"]
    R = eng.fri_num_rounds(eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t))
    assert len(res["proof"]) == agc.proof_len(N, E, t, R, W, A)          # the byte counts of "Argument list"
    at = pc.nonce_offset(N, R)
    assert int.from_bytes(res["proof"][at + 9:at + 17], "little") == want["nonce"]
    blank = [list(c) for c in cols]                                      # the helper once per lookup argument: the same bytes
    for arg in args:
        if arg[0] == "lookup":
            blank[arg[3]] = [0] * n
    filled = gpu_prove(eng, air, blank, log_n, t, bits, fill_multiplicities=True)
    assert filled["proof"] == res["proof"] and filled["column_roots"].tobytes() == want["roots"]
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert ok, why
    assert xg.verify(oracle, air, args, want["roots"], want["proof"], p, g, log_n, LB, t, TAU, g, E, bits) == (True, "")


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_verify_xargs_rejections_agree_with_the_restatement(engines, oracle, p, g):
    import stark_rs_amd as s
    eng, log_n, t, bits = engines[p], 5, 4, 8
    n = 1 << log_n
    base, cols, args = scene(log_n, p, "mixed")
    air = with_args(base, args)
    _d, E = eng.air_plan(air, W, log_n, LB)
    # an unselected row of argument 0 holds a value outside the table, and the proof verifies
    row = cols[6].index(0)
    assert cols[14][row] not in base.periodics[0]
    res = gpu_prove(eng, air, cols, log_n, t, bits)
    proof, roots = res["proof"], res["column_roots"].tobytes()
    ok, why = eng.air_verify(air, proof, res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert ok, why

    def both(args_v, bad_proof, want_class, name):
        ok_r, cls = xg.verify(oracle, with_args(base, args_v), args_v, roots, bad_proof, p, g, log_n, LB, t, TAU, g, E, bits)
        assert not ok_r and cls == want_class, (name, cls)
        ok, why = eng.air_verify(with_args(base, args_v), bad_proof, [roots[:32], roots[32:]], W, log_n, LB, t, grind_bits=bits, **KW)
        assert not ok and agc.reason_class(why) == cls, (name, why)

    swap = lambda a, g_: args[:a] + [g_] + args[a + 1:]
    lists = {"a selector removed": swap(0, ("lookup", [14], [("per", 0)], 8)),
             "a selector moved to the other side": swap(0, ("lookup", [14], [("per", 0)], 8, None, 6)),
             "a table selector removed": swap(5, ("lookup", [0], [12], 13)),
             "a periodic selector made a trace selector": swap(2, ("lookup", [0, 5], [("per", 0), ("per", 1)], 9, 6, None)),
             "a periodic member replaced by a trace column": swap(0, ("lookup", [14], [12], 8, 6, None))}
    s1 = len(proof) - agc.opening_len(W, len(args), log_n + LB, t)
    for name, args_v in lists.items():
        assert xg.plan(with_args(base, args_v), args_v, LB)[2] == E      # the same FRI: the rejection is the composition's
        both(args_v, proof, "composition", name)
        for at, cls in ((s1 + 3 * (9 + 8 * W) + 9 + 8 * (W - 1), "path"), (s1 // 2, "fri")):   # two tampered proofs per list
            bad = bytearray(proof)
            bad[at] ^= 1
            both(args_v, bytes(bad), cls, name)
    # with that row's selector set the lookup does not close: proved with its bit down, and rejected
    bad = [list(c) for c in cols]
    bad[6][row] = 1
    with pytest.raises(s.StarkMiError, match=r"the arguments \[0, 3\] do not close"):
        gpu_prove(eng, air, bad, log_n, t, bits)
    res = gpu_prove(eng, air, bad, log_n, t, bits, check=False)
    want = xg.prove(oracle, air, args, bad, p, g, log_n, LB, t, TAU, g, E, bits, honest=False)
    assert res["closes"] == want["closes"] == [a not in (0, 3) for a in range(len(args))]
    assert res["proof"] == want["proof"] and res["column_roots"].tobytes() == want["roots"]
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert not ok and why
    assert not xg.verify(oracle, air, args, want["roots"], want["proof"], p, g, log_n, LB, t, TAU, g, E, bits)[0]
