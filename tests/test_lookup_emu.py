"""CPU: the lookup argument's kernels' own lane code (csrc/lookup_core.h), run by the emulator library with the kernels' lane
batching and block split, against the Python restatement (tests/lookup_compose.py).  Every comparison is exact.

The library's prover and verifier need a GPU context; what runs here of a whole proof is the restated prover with the
emulator's column and the emulator's composition held against the column and the codeword it commits to, and the restated
verifier over the rejection list.  tests/test_gpu_lookup.py holds the library's bytes and verdicts against the same."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import ext_compose as xc
import lookup_compose as lc
import perm_compose as pm
import pow_compose as pc

U64_MAX = (1 << 64) - 1
NO_INVERSE, LOOKUP_MISSING = -1, -56


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp = C.c_void_p
    L.emu_lookup_multiplicities.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.AirLookup), vp, C.c_uint32, C.c_uint32, vp, C.c_int,
                                            C.POINTER(C.c_uint64)]
    L.emu_lookup_column.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.AirLookup), vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64,
                                    C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.emu_air_compose_lookup.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.POINTER(_lib.AirLookup), vp, C.c_uint64,
                                         vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_int, C.c_uint32]
    return L


def make_lookup(lookup, table, mult_col):
    from stark_rs_amd import _lib
    la, ta = np.array(lookup, dtype=np.uint32), np.array(table, dtype=np.uint32)
    out = _lib.AirLookup(len(la), mult_col, la.ctypes.data_as(_lib.u32p), ta.ctypes.data_as(_lib.u32p))
    out._keep = (la, ta)
    return out


def emu_mult(emu, cols, lookup, table, mult_col, p, g, order=0):
    """-> (status, M as a list, missing row)"""
    cols = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    W, n = cols.shape
    mult = np.full(n + 2, 0xdeadbeef, dtype=np.uint32)
    missing = C.c_uint64(0)
    st = emu.emu_lookup_multiplicities(p, g, C.byref(make_lookup(lookup, table, mult_col)), cols.ctypes.data, W, n.bit_length() - 1, mult.ctypes.data, order,
                                       C.byref(missing))
    assert mult[n] == 0xdeadbeef and mult[n + 1] == 0xdeadbeef
    return st, [int(v) for v in mult[:n]], missing.value


def emu_column(emu, cols, lookup, table, mult_col, ch, p, g, s_stride=None):
    """-> (status, s (4, n) uint64, closes, zero_at = 2 row + (1 if f_T))"""
    cols = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    W, n = cols.shape
    s_stride = n if s_stride is None else s_stride
    s = np.full(4 * s_stride, 0xdeadbeef, dtype=np.uint32)
    cha = np.array(ch, dtype=np.uint64)
    closes, zero = C.c_int(-1), C.c_uint64(0)
    st = emu.emu_lookup_column(p, g, C.byref(make_lookup(lookup, table, mult_col)), cols.ctypes.data, W, n.bit_length() - 1, cha.ctypes.data, s.ctypes.data,
                               s_stride, C.byref(closes), C.byref(zero))
    for e in range(4):   # nothing written between the columns
        assert np.all(s[e * s_stride + n:(e + 1) * s_stride] == 0xdeadbeef)
    return st, np.stack([s[e * s_stride:e * s_stride + n] for e in range(4)]).astype(np.uint64), closes.value, zero.value


def chall(seed):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(1 << 62, U64_MAX, 8, dtype=np.uint64)]


SHAPES = ["m1", "m2", "m8", "dups", "one", "overlap"]


def shaped(kind, n, p, seed):
    """m1 / m2 / m8: a shuffled range of that width; the other shapes at m = 2"""
    if kind[0] == "m":
        return lc.shaped("range", n, p, seed, m=int(kind[1:]))
    return lc.shaped(kind, n, p, seed)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("kind", SHAPES)
@pytest.mark.parametrize("log_n", range(1, 14))
def test_emu_multiplicities_and_column_equal_the_restatement(emu, p, g, log_n, kind):
    n = 1 << log_n
    cols, lookup, table, mult_col = shaped(kind, n, p, log_n)
    want_M = cols[mult_col]
    blank = [list(c) for c in cols]
    blank[mult_col] = [0x5a5a5a5] * n                                    # the helper does not read the column it fills
    for order in range(3):                                               # lane by lane in three fixed orders: the same bytes
        st, M, missing = emu_mult(emu, blank, lookup, table, mult_col, p, g, order)
        assert st == 0 and missing == U64_MAX and M == want_M, order
    if kind == "one":
        assert want_M[n // 3] == n
    ch = chall(log_n)
    want, closes, zero = lc.column(cols, lookup, table, mult_col, ch, p, g)
    assert zero is None and closes
    st, s, got_closes, _ = emu_column(emu, cols, lookup, table, mult_col, ch, p, g, s_stride=n + (log_n % 3))
    assert st == 0
    assert np.array_equal(s, want)
    assert got_closes == 1
    if log_n == 7:
        assert lc.recurrence_holds(s, cols, lookup, table, mult_col, ch, p, g) == (True, True)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", [3, 11])
@pytest.mark.parametrize("where", ["first", "last", "inside", "two"])
def test_a_missing_lookup_names_the_smallest_row_and_the_next_call_succeeds(emu, p, g, log_n, where):
    n = 1 << log_n
    cols, lookup, table, mult_col = lc.shaped("range", n, p, 8)
    rows = {"first": [0], "last": [n - 1], "inside": [6], "two": [n // 2 + 1, 5]}[where]
    bad = [list(c) for c in cols]
    for r in rows:
        bad[lookup[0]][r] = lc.absent_value(cols, table)
    want_M, missing = lc.multiplicities(bad, lookup, table)
    assert missing == min(rows)
    for order in range(3):
        st, M, got = emu_mult(emu, bad, lookup, table, mult_col, p, g, order)
        assert st == LOOKUP_MISSING and got == min(rows) and M == want_M   # the others are counted
    st, M, got = emu_mult(emu, cols, lookup, table, mult_col, p, g)
    assert st == 0 and got == U64_MAX and M == cols[mult_col]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", [3, 11])
@pytest.mark.parametrize("side", ["f_L", "f_T"])
@pytest.mark.parametrize("where", ["first", "last", "inside", "two"])
def test_a_zero_denominator_is_no_inverse_naming_the_smallest_row_and_the_side(emu, p, g, log_n, side, where):
    n = 1 << log_n
    cols, lookup, table, mult_col = lc.shaped("range", n, p, 8)
    idx = lookup if side == "f_L" else table
    rows = {"first": [0], "last": [n - 1], "inside": [6], "two": [n // 2 + 1, 5]}[where]
    cols[idx[0]][rows[0]] = lc.absent_value(cols, table)   # a tuple no other row holds on either side: one zero denominator
    for r in rows[1:]:                         # the same tuple in both rows: one gamma makes both denominators zero
        for c in idx:
            cols[c][r] = cols[c][rows[0]]
    ch = lc.gamma_for_zero(cols, idx, chall(4), rows[0], p, g)
    assert lc.column(cols, lookup, table, mult_col, ch, p, g) == (None, None, (min(rows), side))
    st, _s, _closes, zero = emu_column(emu, cols, lookup, table, mult_col, ch, p, g)
    assert st == NO_INVERSE and zero == 2 * min(rows) + (side == "f_T")
    st, s, _closes, _ = emu_column(emu, cols, lookup, table, mult_col, chall(4), p, g)       # the next call succeeds
    assert st == 0 and np.array_equal(s, lc.column(cols, lookup, table, mult_col, chall(4), p, g)[0])


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("kind", ["multiplicity", "absent"])
@pytest.mark.parametrize("log_n", [2, 6, 11])
def test_the_sum_does_not_close_on_a_wrong_multiplicity_or_an_absent_value(emu, p, g, log_n, kind):
    n = 1 << log_n
    cols, lookup, table, mult_col = lc.non_closing(kind, n, p)
    ch = chall(3)
    want, closes, zero = lc.column(cols, lookup, table, mult_col, ch, p, g)
    assert zero is None and not closes
    st, s, got_closes, _ = emu_column(emu, cols, lookup, table, mult_col, ch, p, g)
    assert st == 0 and got_closes == 0
    assert np.array_equal(s, want)


# ---------------------------------------------------------------------------------------------- the composition
def emu_compose(emu, air, cols_lde, sl, ch, wch, p, g, log_n, lb, tau, h, stride=None, s_stride=None, out_stride=None, force_direct=0, grid=0):
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    W = len(cols_lde)
    stride, s_stride, out_stride = (N if v is None else v for v in (stride, s_stride, out_stride))
    a = air.flatten(p)
    cfg = _lib.StarkCfg(log_n, lb, W, 1, tau, h, 0, 1)
    lde = np.zeros(W * stride, dtype=np.uint32)
    for c in range(W):
        lde[c * stride:c * stride + N] = cols_lde[c]
    sb = np.zeros(4 * s_stride, dtype=np.uint32)
    for e in range(4):
        sb[e * s_stride:e * s_stride + N] = sl[e]
    out = np.full(4 * out_stride, 0xdeadbeef, dtype=np.uint32)
    cha, wa = np.array(ch, dtype=np.uint64), np.array(wch, dtype=np.uint64)
    st = emu.emu_air_compose_lookup(p, g, C.byref(cfg), C.byref(a), C.byref(a.lookup), lde.ctypes.data, stride, sb.ctypes.data, s_stride, cha.ctypes.data,
                                    wa.ctypes.data, out.ctypes.data, out_stride, force_direct, grid)
    assert st == 0
    for e in range(4):
        assert np.all(out[e * out_stride + N:(e + 1) * out_stride] == 0xdeadbeef)
    return np.stack([out[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)


def degree_below(o, cw, bound, p, g, log_N, h):
    """every coordinate of cw, interpolated on the coset, has degree < bound"""
    wN = o.ff_prim_nth_root_g(1 << log_N, p, g)
    return all(not np.any(np.asarray(o.fast_intt(np.asarray(cw[e], dtype=np.uint64), wN, h, p))[bound:]) for e in range(4))


def plan_DE(air, lb):
    d, D = max(air.degree, 3), 1
    while D < d - 1:
        D *= 2
    return D, (1 << lb) // D


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name", ["empty", "fib", "mixer"])
def test_emu_air_compose_lookup_equals_the_restatement(oracle, emu, p, g, name):
    log_n, lb, tau, h = 7, 3, 1, g
    n, N = 1 << log_n, 1 << (log_n + lb)
    for spoil in (None, "multiplicity", "absent"):
        air, cols = ac.make(name, n, p)
        air, cols = lc.with_range_lookup(air, cols, p, spoil=spoil)
        W, K = len(cols), len(air.constraints)
        lookup, table, mult_col = air.lookup_arg
        ch = chall(11)
        s, closes, zero = lc.column(cols, lookup, table, mult_col, ch, p, g)
        assert zero is None and closes == (spoil is None)
        lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
        sl = ac.lde(oracle, [[int(v) for v in s[e]] for e in range(4)], p, g, log_n, lb, tau, h)
        wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 2), dtype=np.uint64)]
        want = pm.main_codeword(oracle, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
        want = (want + lc.aux_terms(oracle, lde, sl, lookup, table, mult_col, ch, wch[4 * (W + K):4 * (W + K) + 4], wch[4 * (W + K) + 4:], p, g, log_n, lb,
                                    tau, h)) % np.uint64(p)
        got = emu_compose(emu, air, lde, sl, ch, wch, p, g, log_n, lb, tau, h)
        assert np.array_equal(got, want), (name, spoil)
        D, _E = plan_DE(air, lb)
        assert degree_below(oracle, got, D * n, p, g, log_n + lb, h) == (spoil is None)
        if spoil is None:   # the shapes of the 4-byte path and a grid that makes every lane loop
            assert np.array_equal(emu_compose(emu, air, lde, sl, ch, wch, p, g, log_n, lb, tau, h, stride=N + 1, s_stride=N + 3, out_stride=N + 5), want)
            assert np.array_equal(emu_compose(emu, air, lde, sl, ch, wch, p, g, log_n, lb, tau, h, force_direct=1, grid=1), want)


# ---------------------------------------------------------------------------------------------- whole proofs, restated
def fib_case(n, p, spoil=None):
    air, cols = ac.make("fib", n, p)
    return lc.with_range_lookup(air, cols, p, spoil=spoil)


@pytest.mark.parametrize("bits", [0, 8])
@pytest.mark.parametrize("lb", [3, 4])
@pytest.mark.parametrize("log_n", range(3, 7))
def test_restated_proofs_commit_to_the_emulators_column_and_codeword(oracle, emu, log_n, lb, bits):
    p, g = xc.PRIMES[(log_n + lb) % 2]
    n, N, t, tau, h = 1 << log_n, 1 << (log_n + lb), 4, 1, g
    air, cols = fib_case(n, p)
    W, K = len(cols), len(air.constraints)
    lookup, table, mult_col = air.lookup_arg
    _D, E = plan_DE(air, lb)
    want = lc.prove(oracle, air, lookup, table, mult_col, cols, p, g, log_n, lb, t, tau, h, E, bits)
    assert want["closes"]
    st, s, closes, _ = emu_column(emu, cols, lookup, table, mult_col, want["ch"], p, g)
    assert st == 0 and closes == 1 and np.array_equal(s, want["s"])
    lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
    sl = ac.lde(oracle, [[int(v) for v in s[e]] for e in range(4)], p, g, log_n, lb, tau, h)
    assert np.array_equal(emu_compose(emu, air, lde, sl, want["ch"], want["wch"], p, g, log_n, lb, tau, h), want["cw"])
    _, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
    R = oracle.fri_num_rounds(oracle.fri_cfg(wN, h, N, E, t, p))
    assert len(want["proof"]) == pm.proof_len(N, E, t, R, W)             # the formula in the header
    assert lc.verify(oracle, air, lookup, table, mult_col, want["roots"], want["proof"], p, g, log_n, lb, t, tau, h, E, bits) == (True, "")


def offsets(W, log_N, t, plen):
    """byte offsets inside a proof: (section 1, its paths, section 2, its paths)"""
    s1 = plen - pm.opening_len(W, log_N, t)
    p1 = s1 + 4 * t * (9 + 8 * W)
    s2 = p1 + 4 * t * (9 + 32 * log_N)
    p2 = s2 + 4 * t * (9 + 32)
    return s1, p1, s2, p2


def rejection_list(oracle, air, cols, p, g, log_n, lb, t, bits, proof, roots):
    """-> [(name, air to verify under, proof, roots, class or None)]: every entry must be rejected"""
    from stark_rs_amd.mirror import Air
    n, log_N, tau, h = 1 << log_n, log_n + lb, 1, g
    W = len(cols)
    lookup, table, mult_col = air.lookup_arg
    _D, E = plan_DE(air, lb)
    s1, p1, s2, p2 = offsets(W, log_N, t, len(proof))
    rec1, prec = 9 + 8 * W, 9 + 32 * log_N
    out = []
    flips = [("row tag 1", s1 + 2 * rec1, "record"), ("a value of M", s1 + 3 * rec1 + 9 + 8 * mult_col, "path"),
             ("path tag 1", p1 + prec, "record"), ("path digest 1", p1 + 5 * prec + 9 + 40, "path"),
             ("row tag 2", s2 + 41, "record"), ("a value of s", s2 + 6 * 41 + 9 + 16, "path"),
             ("path tag 2", p2 + 3 * prec, "record"), ("path digest 2", p2 + 7 * prec + 9 + 3, "path")]
    for name, at, cls in flips:
        bad = bytearray(proof)
        bad[at] ^= 1
        out.append((name, air, bytes(bad), roots, cls))
    tam = lc.prove(oracle, air, lookup, table, mult_col, cols, p, g, log_n, lb, t, tau, h, E, bits, s_plus_p=3)
    out.append(("non-canonical s coordinate", air, tam["proof"], tam["roots"], "canonical"))
    out.append(("section 2 cut short", air, proof[:-1], roots, "length"))
    out.append(("section 2 missing", air, proof[:s2], roots, "length"))
    out.append(("section 1 cut short", air, proof[:p1 - 1], roots, "length"))
    out.append(("cut inside FRI", air, proof[:s1 // 2], roots, "fri"))
    out.append(("swapped roots", air, proof, roots[32:] + roots[:32], "fri"))
    # an honest permutation proof over the columns of a lookup that holds as well: same W, same E, same transcript
    air_l, air_p, tcols = lc.perm_twin(n, p)
    assert len(tcols) == W and plan_DE(air_l, lb)[1] == E
    pproof = pm.prove(oracle, air_p, air_p.perm[0], air_p.perm[1], tcols, p, g, log_n, lb, t, tau, h, E, bits)
    assert pproof["closes"]
    out.append(("a permutation proof", air_l, pproof["proof"], pproof["roots"], "composition"))
    other = Air(W)
    other._symbolic, other.boundaries = air._symbolic, air.boundaries
    other.lookup(table, table, mult_col)
    out.append(("a proof under another lookup", other, proof, roots, "composition"))
    return out


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_restated_verifier_rejects_the_list(oracle, p, g):
    log_n, lb, t, bits, tau, h = 5, 3, 4, 8, 1, g
    air, cols = fib_case(1 << log_n, p)
    lookup, table, mult_col = air.lookup_arg
    _D, E = plan_DE(air, lb)
    res = lc.prove(oracle, air, lookup, table, mult_col, cols, p, g, log_n, lb, t, tau, h, E, bits)
    for name, air_v, bad_proof, bad_roots, cls in rejection_list(oracle, air, cols, p, g, log_n, lb, t, bits, res["proof"], res["roots"]):
        lv, tv, mv = air_v.lookup_arg
        assert lc.verify(oracle, air_v, lv, tv, mv, bad_roots, bad_proof, p, g, log_n, lb, t, tau, h, E, bits) == (False, cls), name
    # and the other way round: an honest lookup proof offered to the permutation argument's restated verifier
    air_l, air_p, tcols = lc.perm_twin(1 << log_n, p)
    lk = air_l.lookup_arg
    twin = lc.prove(oracle, air_l, lk[0], lk[1], lk[2], tcols, p, g, log_n, lb, t, tau, h, E, bits)
    assert twin["closes"] and lc.verify(oracle, air_l, lk[0], lk[1], lk[2], twin["roots"], twin["proof"], p, g, log_n, lb, t, tau, h, E, bits) == (True, "")
    assert pm.verify(oracle, air_p, air_p.perm[0], air_p.perm[1], twin["roots"], twin["proof"], p, g, log_n, lb, t, tau, h, E, bits) == (False, "composition")
    for spoil in ("multiplicity", "absent"):   # a trace that does not close is proved and rejected
        air_b, cols_b = fib_case(1 << log_n, p, spoil=spoil)
        bad = lc.prove(oracle, air_b, lookup, table, mult_col, cols_b, p, g, log_n, lb, t, tau, h, E, bits, honest=False)
        assert not bad["closes"]
        assert not lc.verify(oracle, air_b, lookup, table, mult_col, bad["roots"], bad["proof"], p, g, log_n, lb, t, tau, h, E, bits)[0], spoil
