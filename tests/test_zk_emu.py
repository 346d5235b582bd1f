"""CPU: the zero-knowledge building blocks.  The kernels' own lane bodies (csrc/zk_core.h) run by the emulator library with the
kernels' lanes and aligned loads (csrc/emu_zk.cpp) against the restatement over the oracle's hash (tests/zk_compose.py); the
derived AIR that the library builds against the mirror's, and under the trace checker; the plan's numbers and refusals through
libstarkmi.so (host only: no context, no GPU)."""
import ctypes as C
import math

import numpy as np
import pytest

import zk_compose as zk

P_REF, G_REF = 998244353, 3
SEED = bytes(range(32))
COUNTS = [1, 3, 4, 1023, 1024, 1025]
# (log_n, t, D, h_len or None for D n): D' = 2, D' = 3, D n a multiple of L or not, the last coefficient of H in any residue;
# then the limits: D' = 14 (the largest grid.y) with a full last segment and with one coefficient in it, and t = 32 (k_s = 129,
# more masked coefficients at a column's end than a wavefront has lanes) at D' = 5 and with the last segment three short of full
SPLITS = [(6, 1, 1, None), (6, 1, 2, None), (7, 2, 2, None), (7, 1, 2, 2 * 123), (6, 2, 1, 57), (8, 2, 4, None),
          (6, 2, 14, 14 * (64 - 9)), (6, 2, 14, 13 * (64 - 9) + 1), (10, 32, 4, None), (10, 32, 2, 2 * 895 - 3)]
# case -> (D', h_len mod L), written out
SPLIT_DP = dict(zip(SPLITS, [(2, 5), (3, 10), (3, 18), (2, 0), (2, 2), (5, 36), (14, 0), (14, 1), (5, 516), (2, 892)]))


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.emu_random_fill.argtypes = [u64, C.c_char_p, u64, vp, u64]
    L.emu_zk_segments.argtypes = [u64, vp, u64, u64, u32, u32, u32, vp, vp, u64]
    L.emu_zk_derived_air.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), vp, vp, vp, vp, vp, vp, vp, vp]
    L.emu_air_check.argtypes = [u64, C.POINTER(_lib.Air), u32, u32, vp, C.POINTER(C.c_int), C.POINTER(u32), C.POINTER(u64)]
    return L


def emu_fill(emu, p, seed, stream, count, lead=0):
    """count residues written `lead` words into a buffer; the words around them must stay untouched"""
    buf = np.full(lead + count + 3, 0xFFFFFFFF, dtype=np.uint32)
    assert emu.emu_random_fill(p, seed, stream, buf.ctypes.data + 4 * lead, count) == 0
    assert (buf[:lead] == 0xFFFFFFFF).all() and (buf[lead + count:] == 0xFFFFFFFF).all()
    return [int(v) for v in buf[lead:lead + count]]


# ---------------------------------------------------------------------------------------------- statements
def fib_statement(log_n, t, p):
    """Fibonacci over the first n - k_t rows, the claim on the last real row; the tail rows hold whatever the caller left"""
    from stark_rs_amd.mirror import Air
    n = 1 << log_n
    real = n - zk.k_t(t)
    a, b = [1], [1]
    for _ in range(n - 1):
        a.append(b[-1])
        b.append((a[-2] + b[-1]) % p)
    air = Air(2)
    air.transition({("next", 0): 1, ("cur", 1): -1})
    air.transition({("next", 1): 1, ("cur", 0): -1, ("cur", 1): -1})
    air.boundary(0, 0, 1).boundary(1, 0, 1).boundary(0, real - 1, a[real - 1])
    return air, [a, b]


def cubic_statement(log_n, t, p):
    """a' = a^3 + pi with round constants of period 8, b' = b + a: degree 3 with a periodic column"""
    from stark_rs_amd.mirror import Air
    n = 1 << log_n
    real = n - zk.k_t(t)
    rc = [(7 * i * i + 3) % p for i in range(8)]
    a, b = [2], [0]
    for r in range(n - 1):
        a.append((pow(a[-1], 3, p) + rc[r % 8]) % p)
        b.append((b[-1] + a[-2]) % p)
    air = Air(2)
    j = air.periodic(rc)
    air.transition({("next", 0): 1, ("cur", 0, 3): -1, ("per", j): -1})
    air.transition({("next", 1): 1, ("cur", 1): -1, ("cur", 0): -1})
    air.boundary(0, 0, 2).boundary(1, 0, 0).boundary(1, real - 1, b[real - 1])
    return air, [a, b]


STATEMENTS = {"fib": fib_statement, "cubic": cubic_statement}
SHAPES = [(6, 1), (7, 2), (8, 1), (8, 2)]          # (log_n, t): k_t = 16, 24 < n / 2


def wide_statement(log_n, t, p, W=5):
    """W >= 3 columns and two periodic columns, k4 of period 4 and k8 of period 8: a' = a^2 + k4, b' = b + k8' a with k8 read
    at the next row, c_i' = c_i + c_(i-1) c_(i-2) for every further column.  Degree 2, so the derived AIR has degree 3: D = 2,
    D' = 3.  A claim on every column in row 0 and on the last column in the last real row."""
    from stark_rs_amd.mirror import Air
    assert W >= 3
    n = 1 << log_n
    real = n - zk.k_t(t)
    k4, k8 = [(5 * i + 1) % p for i in range(4)], [(3 * i * i + 2) % p for i in range(8)]
    cols = [[c + 1] for c in range(W)]
    for r in range(n - 1):
        cur = [c[-1] for c in cols]
        nxt = [(cur[0] * cur[0] + k4[r % 4]) % p, (cur[1] + k8[(r + 1) % 8] * cur[0]) % p]
        nxt += [(cur[i] + cur[i - 1] * cur[i - 2]) % p for i in range(2, W)]
        for c, v in zip(cols, nxt):
            c.append(v)
    air = Air(W)
    j4, j8 = air.periodic(k4), air.periodic(k8)
    air.transition({("next", 0): 1, ("cur", 0, 2): -1, ("per", j4): -1})
    air.transition({("next", 1): 1, ("cur", 1): -1, (("per_next", j8), ("cur", 0)): -1})
    for i in range(2, W):
        air.transition({("next", i): 1, ("cur", i): -1, (("cur", i - 1), ("cur", i - 2)): -1})
    for c in range(W):
        air.boundary(c, 0, c + 1)
    air.boundary(W - 1, real - 1, cols[W - 1][real - 1])
    return air, cols


def quintic_statement(log_n, t, p):
    """one column, a' = a^5 + k with k a periodic column of period 1: the derived AIR has degree 6, D = 8 (log_blowup >= 3),
    D' = 9 or, where n is small against k_s, 10"""
    from stark_rs_amd.mirror import Air
    n = 1 << log_n
    real = n - zk.k_t(t)
    a = [3]
    for _ in range(n - 1):
        a.append((pow(a[-1], 5, p) + 11) % p)
    air = Air(1)
    j = air.periodic([11])
    air.transition({("next", 0): 1, ("cur", 0, 5): -1, ("per", j): -1})
    air.boundary(0, 0, 3).boundary(0, real - 1, a[real - 1])
    return air, [a]


# the statements past two columns: name -> (log_n, t, p, W) -> (air, cols); the tests above STATEMENTS hard-code W = 2
MORE_STATEMENTS = {"wide": wide_statement, "quintic": lambda log_n, t, p, W=1: quintic_statement(log_n, t, p)}
# (statement, log_n, log_blowup, t, W, (d, D', k_t, k_s)): two periods with a next-row read, the widest leaf, D' = 9 and 10
MORE_SHAPES = [("wide", 7, 2, 2, 5, (3, 3, 24, 9)), ("wide", 6, 2, 1, 63, (3, 3, 16, 5)), ("quintic", 6, 3, 1, 1, (6, 9, 16, 5)),
               ("quintic", 6, 3, 2, 1, (6, 10, 24, 9))]


def statement(name, log_n, t, p, W=2):
    """any statement of this module by name"""
    return STATEMENTS[name](log_n, t, p) if name in STATEMENTS else MORE_STATEMENTS[name](log_n, t, p, W)


def w_of(oracle, log_n, p, g):
    return oracle.ff_prim_nth_root_g(1 << log_n, p, g)


# ---------------------------------------------------------------------------------------------- random residues
@pytest.mark.parametrize("count", COUNTS)
def test_random_fill_equals_the_hash_in_counter_mode(oracle, emu, count):
    for p, stream in ((P_REF, 0), (469762049, 1), (P_REF, (1 << 64) - 1)):
        want = zk.rng(oracle, SEED, stream, count, p)
        for lead in (0, 1, 2, 3):
            assert emu_fill(emu, p, SEED, stream, count, lead) == want, (p, stream, lead)


def test_random_fill_streams_and_seeds_differ(oracle, emu):
    a = emu_fill(emu, P_REF, SEED, 1, 64)
    assert a != emu_fill(emu, P_REF, SEED, 2, 64) and a != emu_fill(emu, P_REF, bytes(32), 1, 64)
    assert a == emu_fill(emu, P_REF, SEED, 1, 64) and a[:17] == emu_fill(emu, P_REF, SEED, 1, 17)


def test_random_fill_passes_a_chi_square_test(emu):
    """2^16 outputs in 64 equal bins of [0, p).  The bound is the 1 - 10^-6 quantile of chi-square with 63 degrees of freedom
    by Wilson and Hilferty's cube approximation (accurate to well under 1 % at 63 degrees): a uniform source exceeds it once
    in a million seeds, and the seed is fixed, so the test cannot flake.  The bias of the reduction mod p (< 2^-34 an element)
    moves a bin's expectation by less than 2^-18 of a count."""
    count, bins, df = 1 << 16, 64, 63
    z = 4.7534                                            # the standard normal's 1 - 10^-6 quantile
    bound = df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3
    vals = np.array(emu_fill(emu, P_REF, SEED, 7, count), dtype=np.uint64)
    assert int(vals.max()) < P_REF
    hist = np.bincount((vals * np.uint64(bins) // np.uint64(P_REF)).astype(np.int64), minlength=bins)
    edges = [-(-P_REF * b // bins) for b in range(bins + 1)]       # bin b holds the residues in [edges[b], edges[b + 1])
    chi2 = sum((int(hist[b]) - count * (edges[b + 1] - edges[b]) / P_REF) ** 2 / (count * (edges[b + 1] - edges[b]) / P_REF) for b in range(bins))
    print("chi-square", chi2, "bound", bound)
    assert 120 < bound < 135 and chi2 < bound


# ---------------------------------------------------------------------------------------------- masked segments
def split_case(log_n, t, D, h_len, p, seed=5):
    n, ks = 1 << log_n, zk.k_s(t)
    L = n - ks
    h_len = D * n if h_len is None else h_len
    Dp = max(1, -(-h_len // L))
    rng = np.random.default_rng(seed + log_n + 10 * D)
    hc = rng.integers(0, p, (4, h_len), dtype=np.uint64)
    rho = rng.integers(0, p, 4 * (Dp - 1) * ks, dtype=np.uint64)
    return n, ks, L, h_len, Dp, hc, rho


def emu_split(emu, p, hc, h_len, log_n, ks, Dp, rho, lead=0, pad=0):
    """lead: words before every base (lead % 4 != 0: the 4-byte path's alignment); pad: extra stride on both sides"""
    n = 1 << log_n
    hs, os_ = h_len + pad, n + pad
    src = np.zeros(lead + 4 * hs, dtype=np.uint32)
    for e in range(4):
        src[lead + e * hs:lead + e * hs + h_len] = hc[e]
    r = np.ascontiguousarray(np.asarray(rho, dtype=np.uint32))
    out = np.full(lead + 4 * Dp * os_, 0xFFFFFFFF, dtype=np.uint32)
    st = emu.emu_zk_segments(p, src.ctypes.data + 4 * lead, hs, h_len, log_n, ks, Dp, r.ctypes.data if len(r) else None, out.ctypes.data + 4 * lead, os_)
    assert st == 0, st
    body = out[lead:].reshape(4 * Dp, os_)
    assert (body[:, n:] == 0xFFFFFFFF).all() and (out[:lead] == 0xFFFFFFFF).all(), "a word outside the n coefficients of a column was written"
    return [[int(v) for v in row[:n]] for row in body]


@pytest.mark.parametrize("p,g", [(P_REF, G_REF), (469762049, 3)])
@pytest.mark.parametrize("log_n,t,D,h_len", SPLITS)
def test_zk_segments_equal_the_restated_split(emu, p, g, log_n, t, D, h_len):
    n, ks, L, h_len, Dp, hc, rho = split_case(log_n, t, D, h_len, p)
    want = zk.split(hc, h_len, log_n, ks, Dp, rho, p)
    assert len(want) == 4 * Dp and all(len(c) == n for c in want)
    for lead, pad in ((0, 0), (1, 0), (0, 3), (2, 5), (4, 4)):
        assert emu_split(emu, p, hc, h_len, log_n, ks, Dp, rho, lead, pad) == want, (lead, pad)


@pytest.mark.parametrize("log_n,t,D,h_len", SPLITS)
def test_zk_segments_recombine_to_the_composition(emu, log_n, t, D, h_len):
    """sum_j x^(j L) H~_j(x) = H(x) at 8 random points of F_q; every column has n coefficients, so degree < n"""
    import deep_compose as dc
    p, g = P_REF, G_REF
    n, ks, L, h_len, Dp, hc, rho = split_case(log_n, t, D, h_len, p)
    assert (Dp, h_len % L) == SPLIT_DP[(log_n, t, D, None if h_len == D * n else h_len)] and Dp in (2, 3, 5, 14)
    got = emu_split(emu, p, hc, h_len, log_n, ks, Dp, rho)
    rng = np.random.default_rng(99)
    for _ in range(8):
        x = [int(v) for v in rng.integers(0, p, 4)]
        want = dc.horner([[int(hc[e][i]) for e in range(4)] for i in range(h_len)], x, p, g)
        assert zk.recombined_at(got, log_n, ks, x, p, g) == want
    for j in range(Dp):                                       # the masks sit where the section says and nowhere else
        for e in range(4):
            tail = got[4 * j + e][L:]
            assert tail == ([int(v) for v in rho[(4 * j + e) * ks:(4 * j + e + 1) * ks]] if j < Dp - 1 else [0] * ks)


def test_zk_segments_refusals(emu):
    p = P_REF
    n, ks, L, h_len, Dp, hc, rho = split_case(6, 1, 2, None, p)
    src, r, out = np.zeros(4 * h_len, dtype=np.uint32), np.zeros(len(rho), dtype=np.uint32), np.zeros(4 * Dp * n, dtype=np.uint32)
    call = lambda hs, hl, ln, k, d, os_: emu.emu_zk_segments(p, src.ctypes.data, hs, hl, ln, k, d, r.ctypes.data, out.ctypes.data, os_)
    assert call(h_len, h_len, 6, ks, Dp, n) == 0
    assert call(h_len, h_len, 6, ks, Dp - 1, n) == -50          # h_len > D' L: H does not fit
    assert call(h_len - 1, h_len, 6, ks, Dp, n) == -50
    assert call(h_len, h_len, 6, ks, Dp, n - 1) == -50
    assert call(h_len, h_len, 6, 32, Dp, n) == -50 and call(h_len, h_len, 6, 0, Dp, n) == -50
    assert call(h_len, h_len, 6, ks, 15, n) == -50 and call(h_len, h_len, 1, ks, Dp, n) == -50


# ---------------------------------------------------------------------------------------------- the derived AIR
def emu_derived(emu, air, W, log_n, t, p, g, tau=1, lb=2):
    from stark_rs_amd import _lib
    a = air.flatten(p)
    cfg = _lib.StarkCfg(log_n, lb, W, 1, tau, g, t, 1)
    head = np.zeros(6, dtype=np.uint64)
    none = None
    assert emu.emu_zk_derived_air(p, g, C.byref(cfg), C.byref(a), head.ctypes.data, none, none, none, none, none, none, none) == 0
    K, nt, nf, nb, Q, npv = [int(v) for v in head]
    arrs = [np.zeros(K + 1, dtype=np.uint32), np.zeros(nt, dtype=np.uint64), np.zeros(nt + 1, dtype=np.uint32), np.zeros(nf, dtype=np.uint32),
            np.zeros(nf, dtype=np.uint32), np.zeros(Q, dtype=np.uint32), np.zeros(npv, dtype=np.uint64)]
    assert emu.emu_zk_derived_air(p, g, C.byref(cfg), C.byref(a), head.ctypes.data, *[x.ctypes.data for x in arrs]) == 0
    return (K, nt, nf, nb, Q), [[int(v) for v in x] for x in arrs]


def emu_check(emu, air, cols, p, log_n):
    a = air.flatten(p)
    tr = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    ok, con, row = C.c_int(), C.c_uint32(), C.c_uint64()
    assert emu.emu_air_check(p, C.byref(a), len(cols), log_n, tr.ctypes.data, C.byref(ok), C.byref(con), C.byref(row)) == 0
    return (True, None, None) if ok.value else (False, con.value, row.value)


@pytest.mark.parametrize("name", sorted(STATEMENTS))
@pytest.mark.parametrize("log_n,t", SHAPES)
def test_the_library_derives_the_mirrors_air(oracle, emu, name, log_n, t):
    p, g = P_REF, G_REF
    air, _cols = STATEMENTS[name](log_n, t, p)
    for tau in (1, 5):
        want = zk.derived_air(air, log_n, t, p, tau, w_of(oracle, log_n, p, g)).flatten(p)
        head, arrs = emu_derived(emu, air, 2, log_n, t, p, g, tau)
        assert head == (want.n_constraints, want.n_terms, want.n_factors, want.n_boundary, want.n_periodic)
        assert arrs == [[int(v) for v in k] for k in (want._keep[0], want._keep[1], want._keep[2], want._keep[3], want._keep[4], want._keep[8], want._keep[9])]


@pytest.mark.parametrize("log_n,t", SHAPES)
def test_the_exemption_column_vanishes_exactly_on_the_exempt_rows(oracle, emu, log_n, t):
    """the library's column (the sliding product of csrc/zk_core.h), not the restatement's"""
    p, g, n = P_REF, G_REF, 1 << log_n
    air, _cols = fib_statement(log_n, t, p)
    for tau in (1, 5):
        _head, arrs = emu_derived(emu, air, 2, log_n, t, p, g, tau)
        col = arrs[6][-n:]
        assert col == zk.exemption_column(n, t, p, tau, w_of(oracle, log_n, p, g))
        assert [r for r in range(n) if col[r] == 0] == list(range(n - zk.k_t(t) - 1, n - 1))
        # its interpolant is E itself: degree k_t, so the coefficients above k_t are zero and the leading one is 1
        coef = [int(v) for v in oracle.fast_intt(np.array(col, dtype=np.uint64), w_of(oracle, log_n, p, g), tau, p)]
        assert coef[zk.k_t(t)] == 1 and not any(coef[zk.k_t(t) + 1:])


@pytest.mark.parametrize("name", sorted(STATEMENTS))
@pytest.mark.parametrize("log_n,t", SHAPES)
def test_the_derived_air_holds_on_garbage_tails_and_names_a_violation(oracle, emu, name, log_n, t):
    p, g, n = P_REF, G_REF, 1 << log_n
    kt = zk.k_t(t)
    air, cols = STATEMENTS[name](log_n, t, p)
    derived = zk.derived_air(air, log_n, t, p, 1, w_of(oracle, log_n, p, g))
    tail = zk.rng(oracle, SEED, 1, 2 * kt, p)
    masked = zk.randomised(cols, tail, t)
    assert [c[-kt:] for c in masked] == [tail[:kt], tail[kt:]] and [c[:n - kt] for c in masked] == [c[:n - kt] for c in cols]
    assert emu_check(emu, derived, masked, p, log_n) == (True, None, None)
    ok, con, row = emu_check(emu, air, masked, p, log_n)          # the caller's own AIR does not hold on the masked trace
    assert not ok and row == n - kt - 1
    bad = [list(c) for c in masked]
    k = {"fib": 1, "cubic": 0}[name]                              # the column without a boundary point there; constraint k sets it
    bad[k][n - kt - 1] = (bad[k][n - kt - 1] + 1) % p             # the last real row: transition n - k_t - 2 -> n - k_t - 1 breaks
    ok, con, row = emu_check(emu, derived, bad, p, log_n)
    assert (ok, con, row) == (False, len(air.boundaries) + k, n - kt - 2)
    bad = [list(c) for c in masked]
    bad[0][n - kt] = (bad[0][n - kt] + 1) % p                     # a randomiser row: exempt
    assert emu_check(emu, derived, bad, p, log_n) == (True, None, None)


@pytest.mark.parametrize("name,log_n,lb,t,W,numbers", MORE_SHAPES)
def test_the_library_derives_the_mirrors_air_past_two_columns(oracle, emu, name, log_n, lb, t, W, numbers):
    """next-row periodic variables 2 W + Q + j move up by one when the exemption column takes index Q, and its n values stand
    behind the caller's periods (4 + 8, or 1) in the value table"""
    p, g, n = P_REF, G_REF, 1 << log_n
    air, cols = statement(name, log_n, t, p, W)
    assert len(cols) == W == air.n_cols and air.degree + 1 == numbers[0]
    if name == "wide":
        Q = len(air.periodics)
        assert Q == 2 and any(v == 2 * W + Q + 1 for con in air.constraints for _cf, f in con for v, _e in f), "no next-row read of k8"
    for tau in (1, 5):
        want = zk.derived_air(air, log_n, t, p, tau, w_of(oracle, log_n, p, g)).flatten(p)
        head, arrs = emu_derived(emu, air, W, log_n, t, p, g, tau, lb)
        assert head == (want.n_constraints, want.n_terms, want.n_factors, want.n_boundary, want.n_periodic)
        assert arrs == [[int(v) for v in k] for k in (want._keep[0], want._keep[1], want._keep[2], want._keep[3], want._keep[4], want._keep[8], want._keep[9])]
        assert arrs[6][-n:] == zk.exemption_column(n, t, p, tau, w_of(oracle, log_n, p, g))
        assert arrs[6][:-n] == [x % p for v in air.periodics for x in v]
        if name == "wide":                                        # k8 at the next row: variable 2 W + (Q + 1) + 1 of the derived AIR
            assert 2 * W + 3 + 1 in arrs[3] and 2 * W + 2 + 1 not in arrs[3]


@pytest.mark.parametrize("name,log_n,lb,t,W,numbers", MORE_SHAPES)
def test_the_derived_air_past_two_columns_holds_and_names_a_violation(oracle, emu, name, log_n, lb, t, W, numbers):
    p, g, n = P_REF, G_REF, 1 << log_n
    kt = zk.k_t(t)
    air, cols = statement(name, log_n, t, p, W)
    derived = zk.derived_air(air, log_n, t, p, 1, w_of(oracle, log_n, p, g))
    tail = zk.rng(oracle, SEED, 1, W * kt, p)
    masked = zk.randomised(cols, tail, t)
    assert [c[-kt:] for c in masked] == [tail[c * kt:(c + 1) * kt] for c in range(W)] and [c[:n - kt] for c in masked] == [c[:n - kt] for c in cols]
    assert emu_check(emu, derived, masked, p, log_n) == (True, None, None)
    ok, con, row = emu_check(emu, air, masked, p, log_n)          # the caller's own AIR does not hold on the masked trace
    assert not ok and row == n - kt - 1
    nb = len(air.boundaries)
    bad = [list(c) for c in masked]
    bad[0][n - kt - 1] = (bad[0][n - kt - 1] + 1) % p             # the last real row: transition n - k_t - 2 -> n - k_t - 1 breaks
    if name == "wide":                                            # column 0 has no boundary point there; constraint 0 sets it
        assert emu_check(emu, derived, bad, p, log_n) == (False, nb + 0, n - kt - 2)
    else:                                                         # the only column has one: it is named first, then the transition
        assert emu_check(emu, derived, bad, p, log_n) == (False, nb - 1, n - kt - 1)
        moved = zk.derived_air(air, log_n, t, p, 1, w_of(oracle, log_n, p, g))
        moved.boundaries[-1] = (0, n - kt - 1, bad[0][n - kt - 1])
        assert emu_check(emu, moved, bad, p, log_n) == (False, nb + 0, n - kt - 2)
    bad = [list(c) for c in masked]
    bad[W - 1][n - kt] = (bad[W - 1][n - kt] + 1) % p             # a randomiser row: exempt
    assert emu_check(emu, derived, bad, p, log_n) == (True, None, None)
    bad = [list(c) for c in masked]
    bad[W - 1][n - 1] = (bad[W - 1][n - 1] + 1) % p               # the last row: only the wrap-around follows it, which no AIR checks
    assert emu_check(emu, derived, bad, p, log_n) == (True, None, None)


# ---------------------------------------------------------------------------------------------- the plan
def lib_plan(air, W, log_n, lb, t, p=P_REF, g=G_REF):
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, g, t, 1)
    return s.engine.air_plan_deep_zk(p, air.flatten(p), cfg)


@pytest.mark.parametrize("name", sorted(STATEMENTS))
@pytest.mark.parametrize("log_n,t", SHAPES)
@pytest.mark.parametrize("lb", [2, 3])
def test_plan_numbers(name, log_n, t, lb):
    air, _cols = STATEMENTS[name](log_n, t, P_REF)
    want = zk.plan(air, log_n, t)
    assert lib_plan(air, 2, log_n, lb, t) == want
    assert want[2] in (16, 24) and want[3] in (5, 9) and want[1] == {"fib": 2, "cubic": 5}[name] and 4 * want[1] + 5 <= 64


@pytest.mark.parametrize("name,log_n,lb,t,W,numbers", MORE_SHAPES + [("wide", 7, 2, 2, 4, (3, 3, 24, 9)), ("wide", 8, 3, 5, 3, (3, 3, 48, 21))])
def test_plan_numbers_past_two_columns(name, log_n, lb, t, W, numbers):
    """the numbers are written out in MORE_SHAPES, not computed: D' = 10 and a leaf of 64 values among them"""
    air, _cols = statement(name, log_n, t, P_REF, W)
    assert lib_plan(air, W, log_n, lb, t) == zk.plan(air, log_n, t) == numbers
    assert lib_layout(air, W, log_n, lb, t) == zk.layout(W, numbers[1], log_n, lb, t)
    assert W + 1 <= 64 and 4 * numbers[1] + 5 <= 64


def test_plan_refusals():
    from stark_rs_amd import StarkMiError
    from stark_rs_amd.mirror import Air
    p = P_REF

    def refused(air, W, log_n, lb, t, words):
        with pytest.raises(StarkMiError) as e:
            lib_plan(air, W, log_n, lb, t)
        assert e.value.status == -50 and words in str(e.value), str(e.value)
    air, _ = fib_statement(6, 1, p)
    bare = Air(2)
    bare._symbolic = list(air._symbolic)
    refused(bare, 2, 5, 2, 1, "zk deep: k_t = 8 t + 8 = 16 >= n / 2")
    refused(air, 2, 6, 2, 3, "zk deep: k_t = 8 t + 8 = 32 >= n / 2")
    late = Air(2)
    late._symbolic, late.boundaries = list(air._symbolic), list(air.boundaries) + [(1, 48, 3)]
    refused(late, 2, 6, 2, 1, "zk deep: boundary point 3 lies on row 48 >= n - k_t = 48, a randomiser row")
    late.boundaries[-1] = (1, 47, 3)
    assert lib_plan(late, 2, 6, 2, 1)[2:] == (16, 5)
    cubic, _ = cubic_statement(6, 1, p)
    refused(cubic, 2, 6, 1, 1, "deep: D > 2^log_blowup")          # the derived AIR has degree 4: D = 4 > B = 2
    wide = Air(64)
    wide.transition({("next", 0): 1, ("cur", 0): -1})
    refused(wide, 64, 8, 2, 1, "zk deep: W + 1 > 64")
    deep = Air(1)
    deep.transition({("next", 0): 1, ("cur", 0, 9): -1})          # degree 10 with the factor: D = 16 > D' bound
    refused(deep, 1, 8, 4, 1, "zk deep: 4 D' + 5 = 73 > 64")
    full = Air(8)                                                 # a term of SMI_AIR_MAX_TERM_FACTORS factors has no room for one more
    full.transition({("next", 0): 1, tuple(("cur", c) for c in range(8)): -1})
    refused(full, 8, 8, 4, 1, "air: more than SMI_AIR_MAX_TERM_FACTORS (8) factors in a term")


def test_the_entry_points_are_declared_everywhere():
    import os
    import re
    import stark_rs_amd
    from stark_rs_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stark_mi.h")).read()
    rust = open(os.path.join(root, "bindings", "stark_mi.rs")).read()
    assert "Zero-knowledge DEEP proofs" in header
    stark_rs_amd.build()
    names = ["smi_air_plan_deep_zk", "smi_dev_random_fill", "smi_dev_zk_segments", "smi_air_deep_zk_layout", "smi_dev_air_prove_deep_zk", "smi_air_verify_deep_zk"]
    for name in names:
        assert re.search(r"\bint %s\(" % name, header), name
        assert "pub fn %s(" % name in rust, name
        assert getattr(_lib.lib(), name).argtypes is not None, name
    assert set(names) <= set(stark_rs_amd.declared_symbols())


# ---------------------------------------------------------------------------------------------- the proof, restated
PROOF_SHAPES = [("fib", 6, 2, 1), ("fib", 6, 3, 1), ("fib", 7, 2, 2), ("fib", 8, 3, 2), ("cubic", 6, 2, 1), ("cubic", 7, 3, 2), ("cubic", 8, 2, 1)]


def lib_layout(air, W, log_n, lb, t, p=P_REF, g=G_REF):
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    return s.engine.air_deep_zk_layout(p, air.flatten(p), _lib.StarkCfg(log_n, lb, W, 1, 1, g, t, 1))


@pytest.mark.parametrize("name,log_n,lb,t", PROOF_SHAPES)
def test_the_proof_length_equals_the_layout_and_the_restated_verifier_accepts(oracle, name, log_n, lb, t):
    p, g = P_REF, G_REF
    air, cols = STATEMENTS[name](log_n, t, p)
    res = zk.prove(oracle, air, cols, SEED, p, g, log_n, lb, t, 1, g)
    folds, nbytes = lib_layout(air, 2, log_n, lb, t)
    assert (folds, nbytes) == zk.layout(2, res["Dp"], log_n, lb, t) and len(res["proof"]) == nbytes and folds >= 1
    assert res["Dp"] == zk.plan(air, log_n, t)[1]
    assert zk.verify(oracle, air, res["proof"], res["roots"], p, g, 2, log_n, lb, t, 1, g) == (True, "")
    off = zk.offsets(2, res["Dp"], log_n, lb, t)
    assert off["end"] == nbytes
    for at, why in ((off["s0"], zk.FRONT["consistency"]), (off["rec 0"] + 9 + 64, zk.WORDS["auth"]), (off["rec 1"] + 9 + 32 * 4 * res["Dp"], zk.WORDS["auth"]),
                    (off["path 1"] + 9, zk.WORDS["auth"]), (1, zk.FRONT["record"])):
        m = bytearray(res["proof"])
        m[at] ^= 1
        assert zk.verify(oracle, air, bytes(m), res["roots"], p, g, 2, log_n, lb, t, 1, g) == (False, why), at
    other = zk.prove(oracle, air, cols, bytes(32), p, g, log_n, lb, t, 1, g)
    assert other["roots"][0] != res["roots"][0] and len(other["proof"]) == nbytes and other["trace"] != res["trace"]


@pytest.mark.parametrize("name,log_n,lb,t,W,numbers", MORE_SHAPES)
def test_the_restated_prover_and_verifier_agree_past_two_columns(oracle, name, log_n, lb, t, W, numbers):
    p, g = P_REF, G_REF
    air, cols = statement(name, log_n, t, p, W)
    res = zk.prove(oracle, air, cols, SEED, p, g, log_n, lb, t, 1, g)
    assert res["Dp"] == numbers[1] and d4_folds(log_n, lb, t) == 2
    assert (2, len(res["proof"])) == zk.layout(W, res["Dp"], log_n, lb, t) == lib_layout(air, W, log_n, lb, t)
    assert zk.verify(oracle, air, res["proof"], res["roots"], p, g, W, log_n, lb, t, 1, g) == (True, "")
    off = zk.offsets(W, res["Dp"], log_n, lb, t)
    assert off["end"] == len(res["proof"])
    for at, why in ((off["s0"] + 32 * (res["Dp"] - 1), zk.FRONT["consistency"]), (off["rec 0"] + 9 + 32 * (W - 1), zk.WORDS["auth"]),
                    (off["rec 1"] + 9 + 32 * (4 * res["Dp"] - 1), zk.WORDS["auth"])):
        m = bytearray(res["proof"])
        m[at] ^= 1
        assert zk.verify(oracle, air, bytes(m), res["roots"], p, g, W, log_n, lb, t, 1, g) == (False, why), at


def d4_folds(log_n, lb, t):
    import deep_fold4_compose as d4
    return d4.folds(log_n, lb, t)


def test_the_restated_verifier_on_dishonest_commitments(oracle):
    """commit_as of zk.prove: a column committed as value + p keeps every path and only the canonical check refuses it -- unless
    it is a salt, which the verifier does not look at; a column committed with two coset points exchanged keeps every path
    and every value canonical, and only the masked DEEP quotient refuses it"""
    p, g, log_n, lb, t, W = P_REF, G_REF, 7, 2, 2, 5
    air, cols = wide_statement(log_n, t, p, W)
    Dp = zk.plan(air, log_n, t)[1]
    said = lambda commit_as: zk.verify(oracle, air, *[zk.prove(oracle, air, cols, SEED, p, g, log_n, lb, t, 1, g, commit_as=commit_as)[k] for k in ("proof", "roots")],
                                       p, g, W, log_n, lb, t, 1, g)
    assert said(None) == (True, "")
    assert said(zk.plus_p(0, W, p)) == (True, "") and said(zk.plus_p(1, 4 * Dp + 4, p)) == (True, "")        # the two salts
    for group, col in ((0, 0), (0, W - 1), (1, 0), (1, 4 * Dp - 1), (1, 4 * Dp), (1, 4 * Dp + 3)):            # trace, segments, R
        assert said(zk.plus_p(group, col, p)) == (False, zk.WORDS["canonical"]), (group, col)
    for group, col in ((0, 1), (1, 0), (1, 4 * Dp + 1)):
        assert said(zk.swapped(group, col)) == (False, zk.WORDS["quotient"]), (group, col)


def test_layout_refusals():
    from stark_rs_amd import StarkMiError
    from stark_rs_amd.mirror import Air
    air, _ = fib_statement(6, 1, P_REF)
    bare = Air(2)
    bare._symbolic = list(air._symbolic)
    for a, log_n, lb, t, words in ((bare, 5, 2, 1, "zk deep: k_t = 8 t + 8 = 16 >= n / 2"), (air, 6, 2, 2, "zk deep: boundary point 2 lies on row 47"),
                                   (cubic_statement(6, 1, P_REF)[0], 6, 1, 1, "deep: D > 2^log_blowup")):
        with pytest.raises(StarkMiError) as e:
            lib_layout(a, 2, log_n, lb, t)
        assert e.value.status == -50 and words in str(e.value), str(e.value)
