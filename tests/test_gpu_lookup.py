"""GPU: the lookup argument (include/stark_mi.h, "Lookup argument") -- smi_dev_lookup_multiplicities, smi_dev_lookup_column,
smi_dev_air_compose_lookup, smi_dev_air_prove_lookup / smi_air_verify_lookup -- against the restatement over the CPU oracle's
primitives (tests/lookup_compose.py) and the CPU emulator of the kernels.  Every comparison is exact.  `pytest -m gpu`."""
import numpy as np
import pytest

import air_compose as ac
import ext_compose as xc
import lookup_compose as lc
import perm_compose as pm
import pow_compose as pc
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_ext import _dev_cols
from test_lookup_emu import chall, emu, emu_column, emu_mult, fib_case, plan_DE, rejection_list, shaped  # noqa: F401  (emu is a fixture)

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
LB, TAU = 3, 1
KW = dict(row_leaves=True, ext=True)


def lookup_air(n_cols, lookup, table, mult_col):
    from stark_rs_amd.mirror import Air
    return Air(n_cols).lookup(lookup, table, mult_col)


def gpu_mult(eng, cols, lookup, table, mult_col):
    """-> M as a list; the device buffer has a sentinel word on either side"""
    import torch
    cols = np.asarray(cols, dtype=np.uint64)
    W, n = cols.shape
    with Dev(eng) as dev:
        d_trace = dev.upload(cols)
        mt = torch.full((n + 8,), 0x7ffffffe, dtype=torch.int32).cuda()
        try:
            eng.dev_lookup_multiplicities(lookup_air(W, lookup, table, mult_col), d_trace, W, n.bit_length() - 1, mt.data_ptr() + 16)
        finally:
            eng.sync()
            host = mt.cpu().numpy().view(np.uint32)
            gpu_mult.last = [int(v) for v in host[4:4 + n]]
    assert np.all(host[:4] == 0x7ffffffe) and np.all(host[4 + n:] == 0x7ffffffe)
    return gpu_mult.last


def gpu_column(eng, cols, lookup, table, mult_col, ch, s_stride=None, lead=0):
    """-> (s (4, n) uint64, closes); lead: words in front of s, so that its base is not 16-byte aligned"""
    cols = np.asarray(cols, dtype=np.uint64)
    W, n = cols.shape
    s_stride = n if s_stride is None else s_stride
    with Dev(eng) as dev:
        d_trace = dev.upload(cols)
        st, d_s = _dev_cols(np.full((4, n), 0x7ffffffe, dtype=np.uint32), s_stride, lead)
        closes = eng.dev_lookup_column(lookup_air(W, lookup, table, mult_col), d_trace, W, n.bit_length() - 1, ch, d_s, s_stride)
        eng.sync()
        host = st.cpu().numpy().view(np.uint32)[lead:]
    for e in range(4):   # the sentinel words between the coordinate columns stay untouched
        assert np.all(host[e * s_stride + n:(e + 1) * s_stride] == 0x7fffffff)
    return np.stack([host[e * s_stride:e * s_stride + n] for e in range(4)]).astype(np.uint64), closes


# ---------------------------------------------------------------------------------------------- the helper and the column
@pytest.mark.parametrize("log_n", range(1, 14))
def test_dev_multiplicities_and_column_equal_the_restatement_and_the_emulator(engines, emu, log_n):
    """log_n 1 and 2 are below one lane's four rows, 10 is exactly one workgroup of the column build, 11 the first with two"""
    p, g = xc.PRIMES[log_n % 2]
    n = 1 << log_n
    for kind in ("m2", "dups", "one", ["m1", "m8", "overlap"][log_n % 3]):
        cols, lookup, table, mult_col = shaped(kind, n, p, log_n)
        blank = [list(c) for c in cols]
        blank[mult_col] = [0x5a5a5a5] * n
        M = gpu_mult(engines[p], blank, lookup, table, mult_col)
        assert M == cols[mult_col], kind
        assert emu_mult(emu, blank, lookup, table, mult_col, p, g)[1] == M, kind
        ch = chall(log_n)
        want, closes, zero = lc.column(cols, lookup, table, mult_col, ch, p, g)
        assert zero is None and closes
        s, got = gpu_column(engines[p], cols, lookup, table, mult_col, ch)
        assert np.array_equal(s, want), kind
        assert got is True, kind
        st, se, _c, _z = emu_column(emu, cols, lookup, table, mult_col, ch, p, g)
        assert st == 0 and np.array_equal(s, se), kind
    # the 4-byte path: a stride that is no multiple of 4, then a base that is one word off 16 bytes
    s, got = gpu_column(engines[p], cols, lookup, table, mult_col, ch, s_stride=n + 1)
    assert np.array_equal(s, want) and got
    s, got = gpu_column(engines[p], cols, lookup, table, mult_col, ch, s_stride=n + 4, lead=1)
    assert np.array_equal(s, want) and got


def test_dev_lookup_large_by_the_recurrence(engines):
    """2^19 rows is the smallest trace whose workgroup sums (512) take lookup_scan_kernel round its loop twice: s[0] = 0 and
    (s[r+1] - s[r]) f_L f_T = f_T - M f_L determine s, and it closes; with one multiplicity off by one the recurrence still
    holds and the sum does not close.  All 2^19 lookups hitting one table row is the contention case of the count launch."""
    log_n = 19
    p, g = xc.PRIMES[log_n % 2]
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    tab = np.stack([rng.permutation(n).astype(np.uint64), rng.integers(0, p, n, dtype=np.uint64)])
    pick = rng.integers(0, n, n)
    M = np.bincount(pick, minlength=n).astype(np.uint64)
    cols = np.stack([tab[0][pick], tab[1][pick], tab[0], tab[1], np.zeros(n, dtype=np.uint64)])
    lookup, table, mult_col = [0, 1], [2, 3], 4
    got_M = gpu_mult(engines[p], cols, lookup, table, mult_col)
    assert np.array_equal(np.array(got_M, dtype=np.uint64), M)           # the table tuples are distinct: a plain count
    cols[mult_col] = M
    ch = chall(log_n)
    s, closes = gpu_column(engines[p], cols, lookup, table, mult_col, ch)
    assert closes
    assert lc.recurrence_holds(s, cols, lookup, table, mult_col, ch, p, g) == (True, True)
    cols[mult_col][n - 7] += np.uint64(1)
    s, closes = gpu_column(engines[p], cols, lookup, table, mult_col, ch)
    assert not closes
    assert lc.recurrence_holds(s, cols, lookup, table, mult_col, ch, p, g) == (True, False)
    cols[0], cols[1] = tab[0][n // 3], tab[1][n // 3]                    # every lookup is table row n / 3
    got_M = gpu_mult(engines[p], cols, lookup, table, mult_col)
    assert got_M[n // 3] == n and sum(got_M) == n


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("where", ["first", "last", "inside", "two"])
def test_a_missing_lookup_names_the_smallest_row_and_the_next_call_succeeds(engines, p, g, where):
    import stark_rs_amd as s
    n = 1 << 11
    cols, lookup, table, mult_col = lc.shaped("range", n, p, 8)
    rows = {"first": [0], "last": [n - 1], "inside": [6], "two": [n // 2 + 1, 5]}[where]
    bad = [list(c) for c in cols]
    for r in rows:
        bad[lookup[0]][r] = lc.absent_value(cols, table)
    want_M, missing = lc.multiplicities(bad, lookup, table)
    assert missing == min(rows)
    with pytest.raises(s.StarkMiError) as ei:
        gpu_mult(engines[p], bad, lookup, table, mult_col)
    assert ei.value.status == -56 and f"the tuple of row {min(rows)} is in no table row" in str(ei.value)
    assert gpu_mult.last == want_M                                       # the others are counted
    assert gpu_mult(engines[p], cols, lookup, table, mult_col) == cols[mult_col]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("side", ["f_L", "f_T"])
@pytest.mark.parametrize("where", ["first", "last", "inside", "two"])
def test_a_zero_denominator_is_no_inverse_and_the_next_call_succeeds(engines, p, g, side, where):
    import stark_rs_amd as s
    n = 1 << 11
    cols, lookup, table, mult_col = lc.shaped("range", n, p, 8)
    idx = lookup if side == "f_L" else table
    rows = {"first": [0], "last": [n - 1], "inside": [6], "two": [n // 2 + 1, 5]}[where]
    cols[idx[0]][rows[0]] = lc.absent_value(cols, table)
    for r in rows[1:]:
        for c in idx:
            cols[c][r] = cols[c][rows[0]]
    ch = lc.gamma_for_zero(cols, idx, chall(4), rows[0], p, g)
    assert lc.column(cols, lookup, table, mult_col, ch, p, g) == (None, None, (min(rows), side))
    with pytest.raises(s.StarkMiError) as ei:
        gpu_column(engines[p], cols, lookup, table, mult_col, ch)
    assert ei.value.status == -1 and "no inverse" in str(ei.value) and f"{side} is zero in row {min(rows)}:" in str(ei.value)
    s_, _closes = gpu_column(engines[p], cols, lookup, table, mult_col, chall(4))
    assert np.array_equal(s_, lc.column(cols, lookup, table, mult_col, chall(4), p, g)[0])


def test_argument_checks(engines):
    import stark_rs_amd as s
    from stark_rs_amd.mirror import Air
    p, _g = xc.PRIMES[0]
    eng = engines[p]
    with Dev(eng) as dev:
        d = dev.alloc(4 * 5 * 16)
        for lookup, table, mult, log_n, text in (([], [], 4, 2, "width must be in 1 .. SMI_LOOKUP_MAX_WIDTH (8)"),
                                                 ([0], [5], 4, 2, "table_col must be < n_cols"), ([5], [0], 4, 2, "lookup_col must be < n_cols"),
                                                 ([0], [1], 1, 2, "mult_col must be none of the tuple columns"), ([0], [1], 4, 0, "log_n must be in 1 .. 27")):
            with pytest.raises(s.StarkMiError) as ei:
                eng.dev_lookup_column(lookup_air(5, lookup, table, mult), d, 5, log_n, chall(1), d)
            assert ei.value.status == -50 and text in str(ei.value)
            with pytest.raises(s.StarkMiError) as ei:
                eng.dev_lookup_multiplicities(lookup_air(5, lookup, table, mult), d, 5, log_n, d)
            assert ei.value.status == -50 and text in str(ei.value)
        with pytest.raises(s.StarkMiError, match="s_stride < n"):
            eng.dev_lookup_column(lookup_air(5, [0], [1], 4), d, 5, 2, chall(1), d, s_stride=3)
        with pytest.raises(ValueError, match="no lookup"):
            eng.dev_lookup_column(Air(3), d, 3, 4, chall(1), d)
        air = lookup_air(5, [0], [1], 4)
        for kw in (dict(), dict(row_leaves=True), dict(ext=True)):
            with pytest.raises(ValueError, match="row_leaves=True, ext=True"):
                eng.dev_air_prove(air, d, 5, 4, LB, 2, **kw)
            with pytest.raises(ValueError, match="row_leaves=True, ext=True"):
                eng.air_verify(air, b"", [bytes(32), bytes(32)], 5, 4, LB, 2, **kw)
        with pytest.raises(s.StarkMiError) as ei:                        # log_blowup = 2: E < 4
            eng.dev_air_prove(air, d, 5, 4, 2, 2, check=False, **KW)
        assert ei.value.status == -10


# ---------------------------------------------------------------------------------------------- the composition
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", range(3, 9))
def test_dev_air_compose_lookup_equals_the_restatement(engines, oracle, p, g, log_n):
    eng, h = engines[p], g
    n, N = 1 << log_n, 1 << (log_n + LB)
    air, cols = fib_case(n, p)
    W, K = len(cols), len(air.constraints)
    lookup, table, mult_col = air.lookup_arg
    ch = chall(21)
    s, closes, zero = lc.column(cols, lookup, table, mult_col, ch, p, g)
    assert zero is None and closes
    lde = np.array(ac.lde(oracle, cols, p, g, log_n, LB, TAU, h), dtype=np.uint64)
    sl = np.array(ac.lde(oracle, [[int(v) for v in s[e]] for e in range(4)], p, g, log_n, LB, TAU, h), dtype=np.uint64)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 2), dtype=np.uint64)]
    want = pm.main_codeword(oracle, air, cols, wch[:4 * (W + K)], p, g, log_n, LB, TAU, h)
    want = (want + lc.aux_terms(oracle, lde, sl, lookup, table, mult_col, ch, wch[4 * (W + K):4 * (W + K) + 4], wch[4 * (W + K) + 4:], p, g, log_n, LB, TAU,
                                h)) % np.uint64(p)
    # aligned (16-byte accesses); every stride odd; bases off 16 bytes
    for stride, s_stride, out_stride, lead in ((N, N, N, 0), (N + 1, N + 3, N + 5, 0), (N + 4, N + 4, N + 4, 1)):
        with Dev(eng) as dev:
            lt, d_lde = _dev_cols(lde.astype(np.uint32), stride, lead)
            zt, d_sl = _dev_cols(sl.astype(np.uint32), s_stride, lead)
            ot, d_out = _dev_cols(np.zeros((4, N), dtype=np.uint32), out_stride, lead)
            d_w = dev.upload_u64(wch)
            eng.dev_air_compose_lookup(air, d_lde, d_sl, W, log_n, LB, ch, d_w, d_out, stride=stride, s_stride=s_stride, out_stride=out_stride,
                                       lde_offset=h)
            eng.sync()
            host = ot.cpu().numpy().view(np.uint32)[lead:]
        got = np.stack([host[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)
        assert np.array_equal(got, want), (stride, lead)
        for e in range(4):
            assert np.all(host[e * out_stride + N:(e + 1) * out_stride] == 0x7fffffff)


def test_compose_lookup_on_every_trip_of_the_grid_equals_the_restatement_at_sampled_points(engines):
    """air_lookup_compose_kernel on four trips of its grid (tests/test_gpu_perm.py, looping_check): width 2, against
    lc.aux_terms_at"""
    from test_gpu_perm import looping_check
    p, g = xc.PRIMES[1]
    eng = engines[p]
    looping_check(eng, p, 5, 4, 21, lambda air: air.lookup([0, 1], [2, 3], 4),
                  lambda air, d_lde, d_s, W, log_n, ch, d_w, d_out: eng.dev_air_compose_lookup(air, d_lde, d_s, W, log_n, LB, ch, d_w, d_out),
                  lambda idx, lde_at, s_at, s_next, ch, w, wN, log_n: lc.aux_terms_at(idx, lde_at, s_at, s_next, [0, 1], [2, 3], 4, ch, w[:4], w[4:8], p, g,
                                                                                      wN, log_n, TAU, g))


# ---------------------------------------------------------------------------------------------- whole proofs
def gpu_prove(eng, air, cols, log_n, t, bits, **kw):
    with Dev(eng) as dev:
        return eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, LB, t, grind_bits=bits, **KW, **kw)


@pytest.mark.parametrize("log_n,t,bits", [(4, 4, 0), (10, 8, 8)])
def test_prove_lookup_bytes_equal_the_restatement_and_verify_agrees(engines, oracle, log_n, t, bits):
    """a Fibonacci main AIR plus a range lookup; fill_multiplicities=True gives the same bytes as filling by the restatement"""
    p, g = xc.PRIMES[log_n % 2]
    eng, n, N = engines[p], 1 << log_n, 1 << (log_n + LB)
    air, cols = fib_case(n, p)
    W, K = len(cols), len(air.constraints)
    lookup, table, mult_col = air.lookup_arg
    d, E = eng.air_plan(air, W, log_n, LB)
    assert (d, E) == (3, plan_DE(air, LB)[1])
    res = gpu_prove(eng, air, cols, log_n, t, bits, timed=True)
    want = lc.prove(oracle, air, lookup, table, mult_col, cols, p, g, log_n, LB, t, TAU, g, E, bits)
    assert want["closes"] and res["closes"]
    assert res["column_roots"].tobytes() == want["roots"]
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    R = eng.fri_num_rounds(eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t))
    assert len(res["proof"]) == pm.proof_len(N, E, t, R, W)              # the formula in the header
    at = pc.nonce_offset(N, R)
    assert int.from_bytes(res["proof"][at + 9:at + 17], "little") == want["nonce"]
    assert list(res["stage_ms"]) == ["lde", "commit", "lookup", "compose", "fri", "open"]
    blank = [list(c) for c in cols]
    blank[mult_col] = [0] * n
    filled = gpu_prove(eng, air, blank, log_n, t, bits, fill_multiplicities=True)
    assert filled["proof"] == res["proof"] and filled["column_roots"].tobytes() == want["roots"]
    assert lc.verify(oracle, air, lookup, table, mult_col, want["roots"], want["proof"], p, g, log_n, LB, t, TAU, g, E, bits) == (True, "")
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert ok, why


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_verify_lookup_rejections_agree_with_the_restatement(engines, oracle, p, g):
    eng, log_n, t, bits = engines[p], 5, 4, 8
    air, cols = fib_case(1 << log_n, p)
    W = len(cols)
    _d, E = eng.air_plan(air, W, log_n, LB)
    res = gpu_prove(eng, air, cols, log_n, t, bits)
    proof, roots = res["proof"], res["column_roots"].tobytes()
    for name, air_v, bad_proof, bad_roots, want_class in rejection_list(oracle, air, cols, p, g, log_n, LB, t, bits, proof, roots):
        lv, tv, mv = air_v.lookup_arg                                    # the restated verdict first, then the library's
        ok_r, cls = lc.verify(oracle, air_v, lv, tv, mv, bad_roots, bad_proof, p, g, log_n, LB, t, TAU, g, E, bits)
        assert not ok_r and cls == want_class, (name, cls)
        ok, why = eng.air_verify(air_v, bad_proof, [bad_roots[:32], bad_roots[32:]], W, log_n, LB, t, grind_bits=bits, **KW)
        assert not ok and why, name
        assert lc.reason_class(why) == cls, (name, why, cls)
    # the other way round: an honest lookup proof offered to smi_air_verify_perm over the same columns
    air_l, air_p, tcols = lc.perm_twin(1 << log_n, p)
    twin = gpu_prove(eng, air_l, tcols, log_n, t, bits)
    assert twin["closes"] and eng.air_verify(air_l, twin["proof"], twin["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)[0]
    ok, why = eng.air_verify(air_p, twin["proof"], twin["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert not ok and pm.reason_class(why) == "composition", why


@pytest.mark.parametrize("spoil", ["multiplicity", "absent"])
def test_a_trace_that_does_not_close_is_proved_and_rejected(engines, oracle, spoil):
    import stark_rs_amd as s
    p, g = xc.PRIMES[len(spoil) % 2]
    eng, log_n, t, bits = engines[p], 6, 4, 0
    air, cols = fib_case(1 << log_n, p, spoil=spoil)
    W = len(cols)
    lookup, table, mult_col = air.lookup_arg
    _d, E = eng.air_plan(air, W, log_n, LB)
    with pytest.raises(s.StarkMiError, match="does not close"):
        gpu_prove(eng, air, cols, log_n, t, bits)
    res = gpu_prove(eng, air, cols, log_n, t, bits, check=False)
    want = lc.prove(oracle, air, lookup, table, mult_col, cols, p, g, log_n, LB, t, TAU, g, E, bits, honest=False)
    assert not want["closes"] and not res["closes"]
    assert res["proof"] == want["proof"] and res["column_roots"].tobytes() == want["roots"]
    ok_r, cls = lc.verify(oracle, air, lookup, table, mult_col, want["roots"], want["proof"], p, g, log_n, LB, t, TAU, g, E, bits)
    assert not ok_r
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert not ok and lc.reason_class(why) == cls, (why, cls)
    if spoil == "absent":                                                # the helper refuses what the prover proves
        with pytest.raises(s.StarkMiError) as ei:
            gpu_prove(eng, air, cols, log_n, t, bits, fill_multiplicities=True)
        assert ei.value.status == -56
