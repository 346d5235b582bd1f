"""The argument list with selectors and periodic members at the moduli of tests/test_gpu_boundary_primes.py, with selector
cells OUTSIDE {0, 1}: csrc/xargs_core.h adds arithmetic of its own to args_core.h's -- xargs_select forms 1 + S (f - 1) with
to_mont(S) once per row, xlookup_lane_deltas and xlookup_compose_point form S_a f_T - (M S_b) f_L with plain-times-Montgomery
products, xlookup_weights forms M S_b -- and the kernels take any residue as a selector cell.  Operands on the bounds: the
edge values as selector cells (trace selectors and the public one), every free cell p - 1, constant selectors p - 1 and 1
beside tuples whose every Montgomery coordinate is p - 1, and the unreduced u64 challenges and weights a transcript can
hand over.
References: tests/xargs_compose.py, which takes (p, g).  Its `columns` inverts row by row in Python ints: it is the reference
up to 2^5 rows.  At 2^10 and 2^11 rows one argument's column (a different one from prime to prime) is restated in full and
every column is held to `recurrences_hold` -- the recurrences with the denominators multiplied out, vectorised, which with a
first value and no zero denominator determine the column -- and to the restated denominators being non-zero.  Every
comparison is exact.  Without a GPU the kernels' lane code runs in the CPU emulator; `pytest -m gpu` for the kernels and the
verifier.
No GPU case is left out for a prime's two-adicity: the largest domain is 2^11 rows, or 2^7 rows at blowup 8 -- 0 cases."""
import copy

import numpy as np
import pytest

import air_compose as ac
import args_compose as agc
import ext_compose as xc
import perm_compose as pm
import xargs_compose as xg
from test_gpu_boundary_primes import ADICITY, ALL, GEN, KINDS, LARGE, THREE, U64, engines, operands, u64_set  # noqa: F401  (engines is a fixture)
from test_gpu_boundary_primes_args import CH_NAMES, LB, R, TAU, bound_case, challenge_sets, weights
from test_xargs_emu import emu, emu_columns, emu_compose, emu_mult, periods_of, scene as xscene  # noqa: F401  (emu is a fixture)

W = xg.W_SCENE
A = 8
CPU_LOGS = [1, 2, 5, 11]
GPU_LOGS = [1, 2, 10, 11]                       # below one lane's four rows (twice), exactly one workgroup, the first with two
RESTATED_UP_TO = 5                              # xg.columns row by row; above: one column in full, all by their recurrences
EDGES = [None, "sel0", "sel1", "pm1", "wide"]
SHAPES = {0: "a trace selector", 2: "a periodic selector", 5: "a table selector"}   # arguments of xg.scene, for the helper


def same(got, want):
    """the comparison of every GPU test of this module: shape and every word"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.array_equal(got, want))


def edge_tile(p, count, shift=0):
    tile = [0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    return [tile[(r + shift) % 6] for r in range(count)]


_wide = {}


def bscene(log_n, p, kind, edge):
    """xg.scene as tests/test_xargs_emu.py seeds it -> (air, cols, args).  "wide": the random scene with the trace selectors,
    columns 6 and 7, overwritten by the edge set {0, 1, p - 1, p - 2, (p - 1) / 2, (p + 1) / 2} tiled and the public selector
    per 2 holding the same values (all six where its period is 8 or more).  The arguments of such a scene need not close"""
    if edge != "wide":
        return xscene(log_n, p, kind, edge)
    key = (log_n, p, kind)
    if key not in _wide:
        air, cols, args = xscene(log_n, p, kind, None)
        n = 1 << log_n
        assert 4 * n + 7 < p
        air = copy.copy(air)
        air.periodics = [list(v) for v in air.periodics]
        air.periodics[2] = edge_tile(p, len(air.periodics[2]), 2)
        cols = [list(c) for c in cols]
        cols[6], cols[7] = edge_tile(p, n), edge_tile(p, n, 1)
        _wide[key] = (air, cols, args)
    return _wide[key]


def kinds_at(log_n):
    return ["in-lane", "public"] + (["mixed"] if log_n in (5, 10) else [])


def column_cases(p, log_n, every_set=True):
    """-> [(period kind, edge, index of the challenge set, challenges)]: every kind x edge under each of the four challenge
    sets.  every_set=False, for the sizes at which the row-by-row restatement is the slow part of a test without a GPU: every
    kind x edge under one of the four sets, the wide selectors under two; from kind to kind, edge to edge and size to size the
    set moves on, so that every edge and every kind still meets all four"""
    out = []
    for ki, kind in enumerate(kinds_at(log_n)):
        for ei, edge in enumerate(EDGES):
            c = (ki + ei + log_n) % 4
            for ci in (range(4) if every_set else (c, (c + 2) % 4) if edge == "wide" else (c,)):
                out.append((kind, edge, ci, challenge_sets(p, 100 * log_n + ei)[ci]))
    return out


def zero_free(wide, args, ch, p, g):
    """no zero denominator, from the tuple values alone (numpy): f_L and f_T of a lookup, g_R of a permutation"""
    w = np.asarray(wide, dtype=np.uint64)
    for arg in args:
        perm, ai, bi, _mc, _sa, sb = xg.norm(arg, W)
        fl, fr = pm.tuples_vec(w, ai, ch, p, g), pm.tuples_vec(w, bi, ch, p, g)
        for f in ([xg._g_vec(fr, xg._sel_vec(w, sb, p), p)] if perm else [fl, fr]):
            if np.any(~np.any(f, axis=0)):
                return False
    return True


_restated = {}


def restated_columns(log_n, p, kind, edge, ci, ch):
    key = (log_n, p, kind, edge, ci)
    if key not in _restated:
        air, cols, args = bscene(log_n, p, kind, edge)
        _restated[key] = xg.columns(xg.widen(cols, air, p), args, ch, p, GEN[p], W)
    return _restated[key]


def check_columns(c, closes, log_n, p, kind, edge, ci, ch, in_full=None):
    """the columns c (4 A, n) and the closes flags of a kernel or of the emulator against the restatement"""
    g, what = GEN[p], (log_n, kind, edge, CH_NAMES[ci])
    air, cols, args = bscene(log_n, p, kind, edge)
    wide = xg.widen(cols, air, p)
    if log_n <= RESTATED_UP_TO:
        want, want_closes, zero = restated_columns(log_n, p, kind, edge, ci, ch)
        assert zero is None, what
        assert same(c, want) and closes == want_closes, what
    else:
        assert zero_free(wide, args, ch, p, g), what
        want_closes = closes
        if in_full is not None:
            col, closes_a, zero = xg.column(wide, args[in_full], ch, p, g, W)
            assert zero is None and same(c[4 * in_full:4 * in_full + 4], col) and closes[in_full] == closes_a, (what, in_full)
    assert xg.recurrences_hold(c, wide, args, ch, p, g, W) == [(True, bool(cl)) for cl in want_closes], what
    assert edge == "wide" or all(closes), what


def in_full_at(p, log_n):
    """the argument restated in full at a size above RESTATED_UP_TO: another one from prime to prime and size to size"""
    return (ALL.index(p) + log_n) % A


# ---------------------------------------------------------------------------------------------- without a GPU: columns, helper
@pytest.mark.parametrize("log_n", CPU_LOGS)
@pytest.mark.parametrize("p", ALL)
def test_emu_xargs_columns_equal_the_restatement(emu, p, log_n):
    """up to 2^5 rows against xg.columns, one challenge set per kind and edge (column_cases); at 2^11 rows every challenge set,
    by the recurrences, and at the three range-bound primes one column in full (the GPU test restates one at every prime)"""
    g, n = GEN[p], 1 << log_n
    cases = column_cases(p, log_n, every_set=log_n > RESTATED_UP_TO)
    full = [case[:3] for case in cases if case[:2] == ("public", "wide")][0]
    for k, (kind, edge, ci, ch) in enumerate(cases):
        air, cols, args = bscene(log_n, p, kind, edge)
        st, c, closes, _key = emu_columns(emu, air, cols, args, ch, p, g, c_stride=n + (log_n + k) % 3)
        assert st == 0, (kind, edge, CH_NAMES[ci])
        check_columns(c, closes, log_n, p, kind, edge, ci, ch, in_full=in_full_at(p, log_n) if (kind, edge, ci) == full and p in THREE else None)


def test_the_wide_selectors_are_outside_0_and_1_on_either_kind_of_selector():
    for p in ALL:
        for log_n, kind in ((5, "mixed"), (11, "public")):
            air, cols, args = bscene(log_n, p, kind, "wide")
            cells = {0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2}
            assert set(cols[6]) == set(cols[7]) == set(air.periodics[2]) == cells and cols[6] != cols[7]
            sels = [s for arg in args for s in xg.norm(arg, W)[4:] if s is not None]
            assert {6, 7, W + 2} <= set(sels)                                # trace selectors and the public one are all in use


@pytest.mark.parametrize("log_n", [2, 11])
@pytest.mark.parametrize("p", THREE)
def test_emu_xargs_multiplicities_equal_the_dictionary(emu, p, log_n):
    """the helper counts rows: 0 / 1 selectors.  One argument of each shape, on random cells and with the free cells p - 1"""
    g = GEN[p]
    for edge in (None, "pm1"):
        air, cols, args = bscene(log_n, p, "mixed", edge)
        assert args[0][4] == 6 and args[2][4] == ("per", 2) and args[5][5] == ("per", 2)
        wide = xg.widen(cols, air, p)
        for a in SHAPES:
            want, missing = xg.multiplicities(wide, args[a], W)
            assert missing is None and want == cols[args[a][3]]
            for order in (0, 1):
                st, M, _ = emu_mult(emu, air, cols, args, a, p, g, order)
                assert st == 0 and M == want, (edge, SHAPES[a], order)


# ---------------------------------------------------------------------------------------------- without a GPU: the composition
_composed = {}


def composition(o, p, log_n, edge):
    """-> (air, args, extended trace (W, N), extended columns (4 A, N), ch, wch, main + aux (4, N)) of the mixed scene (edge
    None) or the wide-selectors scene, as test_dev_air_compose_xargs_equals_the_restatement_and_the_emulator builds it, under
    challenges and weights of the u64 set"""
    key = (p, log_n, edge)
    if key not in _composed:
        g = GEN[p]
        air, cols, args = bscene(log_n, p, "mixed", edge)
        K = len(air.constraints)
        ch = u64_set(p)[1:9]
        wch = weights(p, 4 * (W + K + 2 * A), 1)
        wide = xg.widen(cols, air, p)
        c, closes, zero = xg.columns(wide, args, ch, p, g, W)
        assert zero is None and (edge == "wide" or all(closes))
        lde_wide = np.asarray(ac.lde(o, wide, p, g, log_n, LB, TAU, g), dtype=np.uint64)
        cl = np.asarray(ac.lde(o, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, LB, TAU, g), dtype=np.uint64)
        want = pm.main_codeword(o, air, cols, wch[:4 * (W + K)], p, g, log_n, LB, TAU, g)
        want = (want + xg.aux_terms(o, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, LB, TAU, g, W)) % np.uint64(p)
        _composed[key] = (air, args, lde_wide[:W], cl, ch, wch, want)
    return _composed[key]


@pytest.mark.parametrize("edge", [None, "wide"])
@pytest.mark.parametrize("p", ALL)
def test_emu_air_compose_xargs_under_unreduced_weights_equals_the_restatement(oracle, emu, p, edge):
    """2^6 rows, blowup 8 (2^9 points: within the two-adicity of 12289): the 16-byte layout, the odd strides of the 4-byte
    path, and a grid of one workgroup that makes every lane loop"""
    g, log_n = GEN[p], 6
    N = 1 << (log_n + LB)
    air, args, lde, cl, ch, wch, want = composition(oracle, p, log_n, edge)
    assert same(emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, LB, TAU, g), want)
    assert same(emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, LB, TAU, g, stride=N + 1, c_stride=N + 3, out_stride=N + 5), want)
    assert same(emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, LB, TAU, g, force_direct=1, grid=1), want)


# ---------------------------------------------------------------------------------------------- selector products at the bound
XBOUND = [(aux_kind, S) for aux_kind in ("top", "steps") for S in ("p - 1", "1")]


def xbound_case(p, N, aux_kind, S):
    """test_gpu_boundary_primes_args.bound_case (constant columns, gamma chosen so that every MONTGOMERY coordinate of
    f_L = f_R (= f_T) is p - 1, the auxiliary columns at "top" or at "steps") with a constant selector column, column 5, on both
    sides of a permutation and of a lookup whose multiplicity column is the constant p - 1.  What each case pushes to its
    largest value in csrc/xargs_core.h:
      S = p - 1   xlookup_compose_point's mont_mul(sa, ft.c[e]), S_a f_T: both operands p - 1, the product (p - 1)^2; and
                  xlookup_weights' M S_b = mont_mul(to_mont(p - 1), p - 1): both cells p - 1.  xargs_select gets f - 1 with
                  coordinates 1 .. 3 at p - 1 beside to_mont(p - 1); its g = 2 - f is then an ordinary element.
      S = 1       M S_b = p - 1, so mont_mul(mult, fl.c[e]), (M S_b) f_L, has both operands p - 1; xargs_select must return
                  g = f with every coordinate p - 1 (1 + 1 (f - 1) through fp_sub, mont_mul by R mod p and fp_add), and
                  args_perm_point's z(w x) * g_R and z(x) * g_L are ext_mul_prepared sums of exactly 4 (p - 1)^2 again.
    -> (air without arguments, lde (6, N), aux (8, N), arguments, ch)"""
    from stark_rs_amd.mirror import Air
    _air, lde, aux, _args, ch = bound_case("args", p, N, aux_kind)
    s = {"p - 1": p - 1, "1": 1}[S]
    lde = np.concatenate([lde, np.full((1, N), s, dtype=np.uint64)])
    args = [("perm", [0, 1], [2, 3], 5, 5), ("lookup", [0, 1], [2, 3], 4, 5, 5)]
    return Air(6), lde, aux, args, ch


def xbound_operands(p, lde, args, ch):
    """on Python ints -> (Montgomery coordinates of f_L, of f_R = f_T, S, M S_b, g_L of the permutation)"""
    g = GEN[p]
    v = [int(c[0]) for c in lde]
    alpha, gamma = pm.alpha_gamma(ch, p)
    apow = pm.alpha_powers(alpha, 2, p, g)
    fl, fr = (pm.tuple_value(v, idx, apow, gamma, p) for idx in (args[0][1], args[0][2]))
    S = v[5]
    gl = xc.add(xg.ONE, xc.scale(xc.sub(fl, xg.ONE, p), S, p), p)
    return [c * R % p for c in fl], [c * R % p for c in fr], S, v[4] * S % p, [c * R % p for c in gl]


@pytest.mark.parametrize("p", LARGE)
def test_the_targeted_operands_of_the_selector_products_are_p_minus_one(p):
    for aux_kind, S in XBOUND:
        _air, lde, aux, args, ch = xbound_case(p, 1 << (4 + LB), aux_kind, S)
        assert all(len(set(int(x) for x in col)) == 1 for col in lde)           # constant columns
        fl_m, fr_m, s, ms, gl_m = xbound_operands(p, lde, args, ch)
        assert fl_m == fr_m == [p - 1] * 4 and int(lde[4][0]) == p - 1
        if S == "p - 1":
            assert s == p - 1 and s * fr_m[0] == (p - 1) ** 2 and ms == 1       # S_a f_T; M S_b from two cells at p - 1
        else:
            assert s == 1 and ms == p - 1 and ms * fl_m[0] == (p - 1) ** 2      # (M S_b) f_L
            assert gl_m == [p - 1] * 4 and sum((p - 1) * c for c in gl_m) == 4 * (p - 1) ** 2
        assert int(aux.max()) == p - 1


_main = {}


def xpointwise(air, lde, aux, args, ch, wch, p, log_n, S):
    """main + aux for inputs that extend nothing: mirror.Air.compose_at under each weight vector plus xg.aux_terms_at"""
    g = GEN[p]
    Wc, N, B = len(lde), lde.shape[1], 1 << LB
    wN = pow(g, (p - 1) // N, p)
    key = (p, N, S, tuple(wch[:4 * Wc]))
    if key not in _main:                                                    # the main part knows nothing of the auxiliary columns
        main = np.zeros((4, N), dtype=np.uint64)
        for e in range(4):
            we = xc.weight_vector(wch[:4 * Wc], e)
            for i in range(N):
                main[e, i] = air.compose_at(p, log_n, LB, TAU, g, wN, i, [int(x) for x in lde[:, i]], [int(x) for x in lde[:, (i + B) % N]], we)
        _main[key] = main
    aux_part = xg.aux_terms_at(np.arange(N), lde, aux, np.roll(aux, -B, axis=1), args, ch, wch[4 * Wc:], p, g, wN, log_n, TAU, g, Wc)
    return (_main[key] + aux_part) % np.uint64(p)


def xbound_weights(p, count, shift):
    return weights(p, count, shift) if shift else [p - 1] * count


@pytest.mark.parametrize("aux_kind,S", XBOUND)
@pytest.mark.parametrize("p", LARGE)
def test_emu_compose_xargs_with_the_selector_products_at_their_bound(emu, p, aux_kind, S):
    g, log_n = GEN[p], 4
    air, lde, aux, args, ch = xbound_case(p, 1 << (log_n + LB), aux_kind, S)
    for shift in (0, 3):
        wch = xbound_weights(p, 4 * (len(lde) + 2 * len(args)), shift)
        want = xpointwise(air, lde, aux, args, ch, wch, p, log_n, S)
        assert same(emu_compose(emu, air, args, lde, aux, ch, wch, p, g, log_n, LB, TAU, g), want), shift


def test_the_comparison_of_the_gpu_tests_fails_on_one_flipped_word():
    """host arrays only: one word of the expected array flipped, one bit, at either end and in the middle"""
    want = np.arange(32 * 64, dtype=np.uint64).reshape(32, 64)
    assert same(want.copy(), want) and same(want.astype(np.uint32), want)
    for at in ((0, 0), (17, 31), (31, 63)):
        bad = want.copy()
        bad[at] ^= np.uint64(1)
        assert not same(want, bad), at
    assert not same(want[:, :63], want) and not same(want[:31], want) and not same(want.reshape(-1), want)


# ---------------------------------------------------------------------------------------------- on the GPU
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("log_n", GPU_LOGS)
@pytest.mark.parametrize("p", LARGE)
def test_dev_xargs_columns_equal_the_restatement(engines, p, log_n):
    """smi_dev_xargs_columns; then the last case with a stride that is no multiple of 4 and with a base one word off 16 bytes
    (the helper checks the words in front of, between and behind the columns)"""
    from test_gpu_xargs import gpu_columns
    eng, n = engines[p], 1 << log_n
    full = [case[:3] for case in column_cases(p, log_n) if case[:2] == ("public", "wide")][0]
    for kind, edge, ci, ch in column_cases(p, log_n):
        air, cols, args = bscene(log_n, p, kind, edge)
        c, closes = gpu_columns(eng, air, cols, args, ch)
        check_columns(c, closes, log_n, p, kind, edge, ci, ch, in_full=in_full_at(p, log_n) if (kind, edge, ci) == full else None)
    assert edge == "wide"
    for kw in (dict(c_stride=n + 1), dict(c_stride=n + 4, lead=1)):
        c4, got = gpu_columns(eng, air, cols, args, ch, **kw)
        assert same(c4, c) and got == closes, kw


@gpu
@pytest.mark.parametrize("log_n", [2, 11])
@pytest.mark.parametrize("p", THREE)
def test_dev_xargs_multiplicities_equal_the_dictionary(engines, p, log_n):
    from test_gpu_xargs import gpu_mult
    eng, n = engines[p], 1 << log_n
    for edge in (None, "pm1"):
        air, cols, args = bscene(log_n, p, "mixed", edge)
        wide = xg.widen(cols, air, p)
        blank = [list(col) for col in cols]
        for arg in args:
            if arg[0] == "lookup":
                blank[arg[3]] = [7] * n                                      # the helper does not read mult_col
        for a in SHAPES:
            want, missing = xg.multiplicities(wide, args[a], W)
            assert missing is None
            assert gpu_mult(eng, air, blank, args, a) == want, (edge, SHAPES[a])


@gpu
@pytest.mark.parametrize("edge", [None, "wide"])
@pytest.mark.parametrize("p", LARGE)
def test_dev_air_compose_xargs_under_unreduced_weights_equals_the_restatement(engines, oracle, p, edge):
    """2^7 rows, blowup 8: aligned (16-byte accesses), every stride odd, bases off 16 bytes"""
    from test_gpu_xargs import gpu_compose
    eng, g, log_n = engines[p], GEN[p], 7
    N = 1 << (log_n + LB)
    air, args, lde, cl, ch, wch, want = composition(oracle, p, log_n, edge)
    for stride, c_stride, out_stride, lead in ((N, N, N, 0), (N + 1, N + 3, N + 5, 0), (N + 4, N + 4, N + 4, 1)):
        got = gpu_compose(eng, air, args, lde, cl, ch, wch, log_n, g, stride, c_stride, out_stride, lead)
        assert same(got, want), (stride, lead)


@gpu
@pytest.mark.parametrize("aux_kind,S", XBOUND)
@pytest.mark.parametrize("p", LARGE)
def test_dev_air_compose_xargs_with_the_selector_products_at_their_bound(engines, p, aux_kind, S):
    from test_gpu_xargs import gpu_compose
    eng, g, log_n = engines[p], GEN[p], 7
    N = 1 << (log_n + LB)
    air, lde, aux, args, ch = xbound_case(p, N, aux_kind, S)
    for shift in (0, 3):
        wch = xbound_weights(p, 4 * (len(lde) + 2 * len(args)), shift)
        want = xpointwise(air, lde, aux, args, ch, wch, p, log_n, S)
        assert same(gpu_compose(eng, air, args, lde, aux, ch, wch, log_n, g, N, N, N, 0), want), shift
        assert same(gpu_compose(eng, air, args, lde, aux, ch, wch, log_n, g, N + 1, N + 3, N + 5, 0), want), (shift, "4-byte path")


@gpu
@pytest.mark.parametrize("bits", [0, 8])
@pytest.mark.parametrize("p", THREE)
def test_prove_xargs_bytes_equal_the_restatement_and_the_verifier_agrees(engines, oracle, p, bits):
    """the mixed scene at 2^5 rows, A = 8, blowup 8, t = 4: smi_dev_air_prove_xargs against xg.prove, smi_air_verify_xargs
    accepts, and a flipped bit in an opened auxiliary value and in root_2 get the verdict of xg.verify"""
    from test_gpu_xargs import KW, gpu_prove, with_args
    eng, g, log_n, t = engines[p], GEN[p], 5, 4
    base, cols, args = bscene(log_n, p, "mixed", None)
    air = with_args(base, args)
    d, E = eng.air_plan(air, W, log_n, LB)
    assert (d, E) == (xg.plan(air, args, LB)[0], xg.plan(air, args, LB)[2])
    res = gpu_prove(eng, air, cols, log_n, t, bits)
    want = xg.prove(oracle, air, args, cols, p, g, log_n, LB, t, TAU, g, E, bits)
    assert want["closes"] == res["closes"] == [True] * A
    assert res["column_roots"].tobytes() == want["roots"]
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    assert xg.verify(oracle, air, args, want["roots"], want["proof"], p, g, log_n, LB, t, TAU, g, E, bits) == (True, "")
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert ok, why
    proof, roots = res["proof"], want["roots"]
    aux_width = 4 * A
    rec2, prec = 9 + 8 * aux_width, 9 + 32 * (log_n + LB)
    s2 = len(proof) - 4 * t * (rec2 + prec)                               # the second section: 4 t rows, then 4 t paths
    bad = bytearray(proof)
    bad[s2 + 6 * rec2 + 9 + 8 * (aux_width - 2)] ^= 1                     # a coordinate of the auxiliary columns in row 6
    wrong = bytearray(roots)
    wrong[40] ^= 1                                                        # root_2
    for name, bad_proof, bad_roots, cls in (("an auxiliary value", bytes(bad), roots, "path"), ("root_2", proof, bytes(wrong), "fri")):
        assert xg.verify(oracle, air, args, bad_roots, bad_proof, p, g, log_n, LB, t, TAU, g, E, bits) == (False, cls), name
        ok, why = eng.air_verify(air, bad_proof, [bad_roots[:32], bad_roots[32:]], W, log_n, LB, t, grind_bits=bits, **KW)
        assert not ok and agc.reason_class(why) == cls, (name, why, cls)
