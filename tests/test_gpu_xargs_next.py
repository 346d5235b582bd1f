"""GPU: next-row operands in argument lists (include/stark_mi.h, "Argument list: next-row operands") -- the NEXT instantiations
of xargs_block_kernel, air_xargs_compose_kernel, xargs_insert_kernel / xargs_count_kernel and their shared siblings, the
row-leaf, DEEP and coset-leaf provers and their verifiers -- against the restatement over the widened trace T | rot(T)
(tests/xargs_next_compose.py), the CPU emulator of the kernels, and the existing GPU path run on the widened trace with the
plain list.  Every comparison is exact.  `pytest -m gpu`."""
import copy

import numpy as np
import pytest

import air_compose as ac
import args_compose as agc
import deep_args_compose as da
import deep_fold4_compose as d4
import ext_compose as xc
import perm_compose as pm
import shared_lookup_compose as sl
import xargs_compose as xg
import xargs_next_compose as xn
from test_gpu_air import Dev
from test_gpu_boundary_primes import GEN, THREE
from test_gpu_ext import _dev_cols
from test_lookup_emu import chall
from test_xargs_next_emu import emu, emu_columns, emu_compose, emu_mult, scene  # noqa: F401  (emu is a fixture)

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
TAU = 1
W = xn.W_SCENE
GENS = {**GEN, **dict(xc.PRIMES)}
ROWS = dict(row_leaves=True, ext=True)
DEEP = dict(row_leaves=True, ext=True, deep_args=True)
COSETS = dict(row_leaves=True, ext=True, deep_args=True, coset_leaves=True)


@pytest.fixture(scope="module")
def engines():
    """one context per modulus, made on first use, closed at the end of the module"""
    import stark_rs_amd as s

    class Lazy(dict):
        def __missing__(self, p):
            self[p] = s.Engine(p, GENS[p], 0)
            return self[p]
    es = Lazy()
    yield es
    for e in es.values():
        e.close()


def gpu_columns(eng, air, cols, args, ch, c_stride=None, lead=0, t_lead=0):
    """-> (c (4 A, n) uint64, closes).  lead: words in front of c (a base off 16 bytes); t_lead: the same for the trace.  The
    words in front of c, between its columns and behind the last stay untouched"""
    import torch
    cols = np.asarray(cols, dtype=np.uint64)
    n_cols, n = cols.shape
    A = len(args)
    c_stride = n if c_stride is None else c_stride
    tt = torch.from_numpy(np.concatenate([np.zeros(t_lead, dtype=np.int32), cols.astype(np.uint32).view(np.int32).reshape(-1)])).cuda()
    ct, d_c = _dev_cols(np.full((4 * A, n), 0x7ffffffe, dtype=np.uint32), c_stride, lead)
    torch.cuda.synchronize()
    closes = eng.dev_args_columns(xn.mirror(air, args), tt.data_ptr() + 4 * t_lead, n_cols, n.bit_length() - 1, ch, d_c, c_stride)
    eng.sync()
    whole = ct.cpu().numpy().view(np.uint32)
    assert np.all(whole[:lead] == 0x7fffffff)
    host = whole[lead:]
    for e in range(4 * A):
        assert np.all(host[e * c_stride + n:(e + 1) * c_stride] == 0x7fffffff)
    return np.stack([host[e * c_stride:e * c_stride + n] for e in range(4 * A)]).astype(np.uint64), closes


def gpu_mult(eng, air, cols, args, a):
    """-> M as a list; guard words on either side of d_mult stay untouched.  args None: air carries its list already"""
    cols = np.asarray(cols, dtype=np.uint64)
    n_cols, n = cols.shape
    with Dev(eng) as dev:
        d_trace = dev.upload(cols)
        mt, d_m = _dev_cols(np.full((1, n), 0x7ffffffe, dtype=np.uint32), n + 3, 1)
        try:
            eng.dev_args_multiplicities(air if args is None else xn.mirror(air, args), a, d_trace, n_cols, n.bit_length() - 1, d_m)
        finally:
            eng.sync()
            whole = mt.cpu().numpy().view(np.uint32)
            assert whole[0] == 0x7fffffff and np.all(whole[1 + n:] == 0x7fffffff)
    return [int(v) for v in whole[1:1 + n]]


def widened(air, cols, args, p):
    """the plain list over the real trace T | rot(T) | the rotated periodic columns -> (air of that width, cols2, args2)"""
    cols2, args2 = xn.widened_trace(cols, air, args, p)
    wide_air = copy.copy(air)
    wide_air.n_cols = len(cols2)
    assert not xn.has_next(args2)
    return wide_air, cols2, args2


# ---------------------------------------------------------------------------------------------- columns and multiplicities
PROJECT = [q for q, _g in xc.PRIMES]
COLUMN_CASES = ([(p, log_n, P) for p in PROJECT + THREE for log_n, P in [(1, 2), (2, 1), (2, 4), (5, 1), (5, 2), (5, 8), (5, 32)]] +
                [(p, 11, P) for p in PROJECT + THREE[:1] for P in (2, 8)])   # two workgroups: the project primes and the largest boundary modulus


@pytest.mark.parametrize("p,log_n,P", COLUMN_CASES)
def test_dev_columns_and_multiplicities_three_ways(engines, emu, p, log_n, P):
    """the restatement (row by row up to 2^5 rows, by the multiplied-out recurrences above), the emulator, and word for word
    the existing launch over the widened trace with the plain list; aligned buffers, an odd stride, bases off 16 bytes.
    At log_n = 11 row 1023 reads its successor from the other workgroup and row 2047 wraps to row 0; c0 holds p - 1 at the rows
    0, 3, 4 and n - 1."""
    g = GENS[p]
    eng, n = engines[p], 1 << log_n
    air, cols, args = scene(log_n, p, P, shared=log_n < 11)
    A, ch = len(args), chall(log_n)
    c, got = gpu_columns(eng, air, cols, args, ch)
    assert got == [True] * A
    st, ce, _closes, _key = emu_columns(emu, air, cols, args, ch, p, g)
    assert st == 0 and np.array_equal(c, ce)
    if log_n <= 5:
        want, closes, zero = xn.columns(cols, air, args, ch, p, g)
        assert zero is None and all(closes) and np.array_equal(c, want)
    else:
        _air2, args2 = xn.restate(air, args, cols, p)
        assert xg.recurrences_hold(c, np.array(xn.widen(cols, air, p), dtype=np.uint64), args2, ch, p, g, W) == [(True, True)] * A
    wide_air, cols2, args2 = widened(air, cols, args, p)
    cw, got = gpu_columns(eng, wide_air, cols2, args2, ch)
    assert got == [True] * A and np.array_equal(cw, c)
    for c_stride, lead, t_lead in ((n + 1, 0, 0), (n + 4, 1, 0), (n, 0, 1)):      # the 4-byte path: an odd stride, c off 16 bytes, the trace off 16 bytes
        c4, got = gpu_columns(eng, air, cols, args, ch, c_stride=c_stride, lead=lead, t_lead=t_lead)
        assert np.array_equal(c4, c) and all(got), (c_stride, lead, t_lead)
    blank = [list(col) for col in cols]
    for arg in args:
        if arg[0] != "perm":
            blank[arg[3]] = [7] * n                                             # the helper does not read mult_col
    blank2 = [list(col) for col in blank] + cols2[W:]
    for a, arg in enumerate(args):
        if arg[0] != "perm":
            M = gpu_mult(eng, air, blank, args, a)
            assert M == cols[arg[3]] == emu_mult(emu, air, cols, args, a, p, g, 0)[1], a
            assert M == gpu_mult(eng, wide_air, blank2, args2, a), a


def test_zero_denominators_and_missing_rows_name_the_same_row_argument_and_side(engines):
    import stark_rs_amd as s
    p, g = xc.PRIMES[1]
    log_n = 5
    n, eng = 1 << log_n, engines[p]
    air, cols, args = scene(log_n, p, 8, shared=False)
    air2, args2 = xn.restate(air, args, cols, p)
    wide = xg.widen(cols, air2, p)
    good = xn.columns(cols, air, args, chall(4), p, g)[0]
    sides = {(False, 0): "f_L", (False, 1): "f_T", (True, 1): "g_R"}
    for a, side, row in ((1, 1, n - 1), (2, 2, 0), (3, 2, next(r for r in range(n) if wide[xg.norm(args2[3], W)[5]][r]))):
        ch = pm.gamma_for_zero(wide, xg.norm(args2[a], W)[side], chall(4), row, p, g)
        key = xg.columns(wide, args2, ch, p, g, W)[2]
        assert key is not None
        ka, ks = (key & 15) >> 1, key & 1
        with pytest.raises(s.StarkMiError) as ei:
            gpu_columns(eng, air, cols, args, ch)
        assert ei.value.status == -1 and f"argument {ka}: {sides[(args[ka][0] == 'perm', ks)]} is zero in row {key >> 4}:" in str(ei.value), (str(ei.value), key)
        c, closes = gpu_columns(eng, air, cols, args, chall(4))                 # the context stays usable
        assert all(closes) and np.array_equal(c, good)
    for at, named in ((7, 6), (0, n - 1)):                                      # next(c1) at row r is c1[r + 1]; row n - 1 reads row 0
        bad = [list(c) for c in cols]
        bad[1][at] = p - 2
        assert xn.multiplicities(bad, air, args[1], p)[1] == named
        with pytest.raises(s.StarkMiError) as ei:
            gpu_mult(eng, air, bad, args, 1)
        assert ei.value.status == -56 and f"argument 1: the tuple of selected row {named} is in no selected table row" in str(ei.value)
    air, cols, args = scene(log_n, p, 8)
    bad = [list(c) for c in cols]
    bad[1][3] = p - 2
    with pytest.raises(s.StarkMiError) as ei:
        gpu_mult(eng, air, bad, args, 4)
    assert ei.value.status == -56 and "argument 4: tuple 0 of row 2," in str(ei.value)
    with Dev(eng) as dev:                                                       # the helper over a row bound takes this-row operands only
        d = dev.upload(np.array(cols, dtype=np.uint64))
        d_m = dev.alloc(4 * n)
        with pytest.raises(s.StarkMiError) as ei:
            eng.dev_xargs_multiplicities_rows(xn.mirror(air, args), 1, d, W, log_n, n - 8, d_m)
        assert ei.value.status == -50 and "xargs_multiplicities_rows: argument 0: b_var is a next-row operand" in str(ei.value)
        d8 = dev.upload(np.zeros((W, 256), dtype=np.uint64))
        with pytest.raises(s.StarkMiError) as ei:                               # and so does the zero-knowledge prover, in its plan
            eng.dev_air_prove(xn.mirror(air, args), d8, W, 8, 3, 2, zk=bytes(32), **COSETS)
        assert ei.value.status == -50 and "zk deep argument: argument 0: b_var is a next-row operand" in str(ei.value)


# ---------------------------------------------------------------------------------------------- the composition
def gpu_compose(eng, air, args, lde, cl, ch, wch, log_n, lb, h, stride, c_stride, out_stride, lead):
    N = 1 << (log_n + lb)
    with Dev(eng) as dev:
        lt, d_lde = _dev_cols(lde.astype(np.uint32), stride, lead)
        zt, d_cl = _dev_cols(cl.astype(np.uint32), c_stride, lead)
        ot, d_out = _dev_cols(np.zeros((4, N), dtype=np.uint32), out_stride, lead)
        d_w = dev.upload_u64(wch)
        eng.dev_air_compose_args(xn.mirror(air, args), d_lde, d_cl, len(lde), log_n, lb, ch, d_w, d_out, stride=stride, c_stride=c_stride,
                                 out_stride=out_stride, lde_offset=h)
        eng.sync()
        host = ot.cpu().numpy().view(np.uint32)[lead:]
    for e in range(4):
        assert np.all(host[e * out_stride + N:(e + 1) * out_stride] == 0x7fffffff)
    return np.stack([host[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)


@pytest.mark.parametrize("p", [q for q, _g in xc.PRIMES] + THREE[:1])
@pytest.mark.parametrize("log_n,lb,P", [(3, 2, 2), (5, 3, 8), (7, 2, 1 << 20)])
def test_dev_air_compose_xargs_equals_the_restatement_and_the_emulator(engines, oracle, emu, p, log_n, lb, P):
    g = GENS[p]
    eng, h = engines[p], g
    N = 1 << (log_n + lb)
    air, cols, args = scene(log_n, p, P)
    A, ch = len(args), chall(21)
    c, closes, zero = xn.columns(cols, air, args, ch, p, g)
    assert zero is None and all(closes)
    lde = np.array(ac.lde(oracle, cols, p, g, log_n, lb, TAU, h), dtype=np.uint64)
    cl = np.array(ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, TAU, h), dtype=np.uint64)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + 2 * A), dtype=np.uint64)]
    want = pm.main_codeword(oracle, air, cols, wch[:4 * W], p, g, log_n, lb, TAU, h)
    want = (want + xn.aux_terms(oracle, cols, air, args, cl, ch, wch[4 * W:], p, g, log_n, lb, TAU, h)) % np.uint64(p)
    assert np.array_equal(emu_compose(emu, air, args, lde, cl, ch, wch, p, g, log_n, lb, TAU, h), want)
    # aligned (16-byte accesses); every stride odd; bases off 16 bytes
    for stride, c_stride, out_stride, lead in ((N, N, N, 0), (N + 1, N + 3, N + 5, 0), (N + 4, N + 4, N + 4, 1)):
        got = gpu_compose(eng, air, args, lde, cl, ch, wch, log_n, lb, h, stride, c_stride, out_stride, lead)
        assert np.array_equal(got, want), (stride, lead)


def test_compose_next_row_operands_on_every_trip_of_the_grid_at_sampled_points(engines):
    """air_xargs_compose_kernel's NEXT instantiation on at least four trips of its grid (tests/test_gpu_perm.py, looping_check):
    next-row trace members and a next-row periodic member and selector, whose tables of 16 and 64 entries are far shorter than
    a trip.  A next-row trace operand at point i is the extended column at (i + B) mod N, gathered from the same seeded
    inputs; a next-row periodic operand comes from its definition at w x (mirror.Air.periodic_at)"""
    from test_gpu_perm import LB, gathered, looping_check, looping_inputs
    import torch
    p, g = xc.PRIMES[1]
    eng, seed = engines[p], 29
    args = [("lookup", [("next", 4)], [("next", ("per", 0))], 6, 5, None), ("perm", [0, ("per", 1)], [("next", 0), 3], ("next", ("per", 2)), ("next", 1)),
            ("lookup", [0, ("next", 1)], [("per", 1), ("per", 0)], 7)]
    rng = np.random.default_rng(3)
    held = {}

    def state(air):
        for P in (2, 8, 4):
            air.periodic([int(v) for v in rng.integers(0, p, P)])
        held["air"] = sl.mirror_air(air, args)

    def restated(idx, lde_at, c_at, c_next, ch, w, wN, log_n):
        air = held["air"]
        N, B = 1 << (log_n + LB), 1 << LB
        wn = pow(wN, B, p)
        lde = looping_inputs(p, 8, 4 * len(args), log_n, seed)[1]              # the same seeded residues: what the launch read B further
        nxt_at = gathered(lde, torch.from_numpy((idx + B) % N).cuda())
        del lde
        per_at = np.array([air.periodic_at(p, log_n, TAU, wn, g * pow(wN, int(i), p) % p) for i in idx], dtype=np.uint64).T
        per_nx = np.array([air.periodic_at(p, log_n, TAU, wn, g * pow(wN, int(i) + B, p) % p) for i in idx], dtype=np.uint64).T
        wide = np.concatenate([lde_at, per_at, nxt_at, per_nx])                   # the widened trace at the points: T | per | rot(T) | rot(per)
        f = lambda c: (("per", 3 + 8 + c[1][1]) if isinstance(c[1], tuple) else ("per", 3 + c[1])) if xn.is_next(c) else c
        return xg.aux_terms_at(idx, wide, c_at, c_next, [xn._map_arg(a, f) for a in args], ch, w, p, g, wN, log_n, TAU, g, 8)

    looping_check(eng, p, 8, 4 * len(args), seed, state,
                  lambda air, d_lde, d_c, n_cols, log_n, ch, d_w, d_out: eng.dev_air_compose_args(air, d_lde, d_c, n_cols, log_n, LB, ch, d_w, d_out),
                  restated)


# ---------------------------------------------------------------------------------------------- whole proofs
def gpu_prove(eng, air, args, cols, log_n, lb, t, bits=0, check=True, fill=False, **kw):
    cols = [list(c) for c in cols]
    if fill:                                                                    # the device fills the multiplicity columns
        for g_ in args:
            if g_[0] != "perm":
                cols[g_[3]] = [0] * len(cols[0])
    with Dev(eng) as dev:
        return eng.dev_air_prove(xn.mirror(air, args), dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, lb, t, grind_bits=bits, check=check,
                                 fill_multiplicities=fill, **kw)


def other_lists(args):
    """-> {name: a list the proof was NOT made for}: one flag removed, one flag moved to another member, and the list of the
    copy-column formulation (column 9 where next(c1) stood -- in that formulation c9 would hold the rotated copy)"""
    swap = lambda a, g_: args[:a] + [g_] + args[a + 1:]
    return {"one flag removed": swap(1, ("lookup", [1], args[1][2], 2)),
            "one flag moved to another member": swap(2, ("lookup", [("next", 3)], [("per", 0)], 4)),
            "the copy-column list": swap(1, ("lookup", [9], args[1][2], 2))}


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_row_leaf_proof_bytes_equal_the_restatement_and_the_verifiers_agree(engines, oracle, p, g):
    eng, log_n, lb, t, bits = engines[p], 5, 3, 4, 8
    air, cols, args = scene(log_n, p, 8, shared=False)
    A = len(args)
    air2, args2 = xn.restate(air, args, cols, p)
    d, E = eng.air_plan(xn.mirror(air, args), W, log_n, lb)
    assert (d, E) == (xg.plan(air2, args2, lb)[0], xg.plan(air2, args2, lb)[2])
    res = gpu_prove(eng, air, args, cols, log_n, lb, t, bits, fill=True, **ROWS)
    want = xg.prove(oracle, air2, args2, cols, p, g, log_n, lb, t, TAU, g, E, bits)   # commits the W real columns alone
    assert want["closes"] == res["closes"] == [True] * A
    assert res["column_roots"].tobytes() == want["roots"] and res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    ok, why = eng.air_verify(xn.mirror(air, args), res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **ROWS)
    assert ok, why
    assert xg.verify(oracle, air2, args2, want["roots"], want["proof"], p, g, log_n, lb, t, TAU, g, E, bits) == (True, "")
    roots = want["roots"]
    for name, args_v in other_lists(args).items():
        air_v, args_v2 = xn.restate(air, args_v, cols, p)
        ok_r, cls = xg.verify(oracle, air_v, args_v2, roots, res["proof"], p, g, log_n, lb, t, TAU, g, E, bits)
        assert not ok_r and cls == "composition", (name, cls)
        ok, why = eng.air_verify(xn.mirror(air, args_v), res["proof"], [roots[:32], roots[32:]], W, log_n, lb, t, grind_bits=bits, **ROWS)
        assert not ok and agc.reason_class(why) == "composition", (name, why)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_deep_proof_bytes_equal_the_restatement_and_the_verifiers_agree(engines, oracle, p, g):
    eng, log_n, lb, t = engines[p], 5, 2, 4
    air, cols, args = scene(log_n, p, 8, shared=False)
    A = len(args)
    air2, args2 = xn.restate(air, args, cols, p)
    res = gpu_prove(eng, air, args, cols, log_n, lb, t, fill=True, **DEEP)
    want = da.prove(oracle, air2, args2, cols, p, g, log_n, lb, t, TAU, g)
    assert [bytes(r) for r in res["column_roots"]] == want["roots"]
    assert [c for el in res["ood"] for c in el] == want["ood"]
    assert res["closes"] == want["closes"] == [True] * A and res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    ok, why = eng.air_verify(xn.mirror(air, args), res["proof"], res["column_roots"], W, log_n, lb, t, **DEEP)
    assert ok, why
    assert da.verify(oracle, air2, args2, res["proof"], want["roots"], p, g, W, log_n, lb, t, TAU, g) == (True, "")
    for name, args_v in other_lists(args).items():
        air_v, args_v2 = xn.restate(air, args_v, cols, p)
        ok_r, cls = da.verify(oracle, air_v, args_v2, res["proof"], want["roots"], p, g, W, log_n, lb, t, TAU, g)
        assert not ok_r and cls == "consistency", (name, cls)
        ok, why = eng.air_verify(xn.mirror(air, args_v), res["proof"], res["column_roots"], W, log_n, lb, t, **DEEP)
        assert not ok and da.keyword("consistency") in why, (name, why)


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_coset_leaf_deep_proof_verifies_and_its_record_is_the_restatement_at_z(engines, oracle, p, g):
    eng, log_n, lb, t = engines[p], 6, 2, 4
    air, cols, args = scene(log_n, p, 8, shared=False)
    air2, args2 = xn.restate(air, args, cols, p)
    res = gpu_prove(eng, air, args, cols, log_n, lb, t, **COSETS)
    ok, why = eng.air_verify(xn.mirror(air, args), res["proof"], res["column_roots"], W, log_n, lb, t, **COSETS)
    assert ok, why
    want = d4.prove_args(oracle, air2, args2, cols, p, g, log_n, lb, t, TAU, g)   # z from the transcript; u, v, a, b, s from the polynomials
    assert [bytes(r) for r in res["column_roots"]] == want["roots"]
    assert [c for el in res["ood"] for c in el] == want["ood"]
    assert res["proof"] == want["proof"]
    for name, args_v in other_lists(args).items():
        ok, why = eng.air_verify(xn.mirror(air, args_v), res["proof"], res["column_roots"], W, log_n, lb, t, **COSETS)
        assert not ok and da.keyword("consistency") in why, (name, why)
        air_v, args_v2 = xn.restate(air, args_v, cols, p)
        assert not d4.verify(oracle, air_v, args_v2, res["proof"], want["roots"], p, g, W, log_n, lb, t, TAU, g)[0], name


# ---------------------------------------------------------------------------------------------- the DFA of the README
def dfa_run(n, p, wrong=None):
    """a 3-state, 2-symbol automaton run for n rows as ONE lookup: (state[r], input[r], state[r + 1]) is a row of the public
    transition table, on every row but the last.  -> (air, cols): c0 state, c1 input, c2 multiplicities (left zero)"""
    from stark_rs_amd.mirror import Air
    delta = {(s, i): (2 * s + i + 1) % 3 for s in range(3) for i in range(2)}
    keys = sorted(delta) + [(0, 0), (0, 0)]                                     # eight table rows: a power of two
    S, I, Nx = [k[0] for k in keys], [k[1] for k in keys], [delta[k] for k in keys]
    rng = np.random.default_rng(n)
    inp = [int(v) for v in rng.integers(0, 2, n)]
    state = [1]
    for r in range(n - 1):
        state.append(delta[(state[r], inp[r])])
    if wrong is not None:
        state[wrong + 1] = (state[wrong + 1] + 1) % 3
    dfa = Air(3)
    ts, ti, tn = dfa.periodic(S), dfa.periodic(I), dfa.periodic(Nx)
    live = dfa.periodic([1] * (n - 1) + [0])
    dfa.add_lookup([0, 1, ("next", 0)], [("per", ts), ("per", ti), ("per", tn)], 2, sel=("per", live))
    return dfa, [state, inp, [0] * n]


@pytest.mark.parametrize("kw", [ROWS, DEEP], ids=["rows", "deep"])
def test_a_dfa_run_is_one_lookup(engines, kw):
    import stark_rs_amd as s
    p, g = xc.PRIMES[0]
    eng, log_n, lb, t = engines[p], 5, 3, 4
    n = 1 << log_n
    dfa, cols = dfa_run(n, p)
    with Dev(eng) as dev:
        res = eng.dev_air_prove(dfa, dev.upload(np.array(cols, dtype=np.uint64)), 3, log_n, lb, t, grind_bits=0, fill_multiplicities=True, **kw)
    assert res["closes"] == [True]
    ok, why = eng.air_verify(dfa, res["proof"], res["column_roots"], 3, log_n, lb, t, **kw)
    assert ok, why
    wrong = 11
    bad_dfa, bad = dfa_run(n, p, wrong=wrong)
    with pytest.raises(s.StarkMiError) as ei:                                  # the helper names the row whose successor is wrong
        with Dev(eng) as dev:
            eng.dev_air_prove(bad_dfa, dev.upload(np.array(bad, dtype=np.uint64)), 3, log_n, lb, t, grind_bits=0, fill_multiplicities=True, **kw)
    assert ei.value.status == -56 and f"the tuple of selected row {wrong} is in no selected table row" in str(ei.value)
    bad[2] = gpu_mult(eng, dfa, cols, None, 0)                                  # the honest run's multiplicities, forced
    with Dev(eng) as dev:
        forced = eng.dev_air_prove(bad_dfa, dev.upload(np.array(bad, dtype=np.uint64)), 3, log_n, lb, t, grind_bits=0, check=False, **kw)
    assert forced["closes"] == [False]
    ok, why = eng.air_verify(bad_dfa, forced["proof"], forced["column_roots"], 3, log_n, lb, t, **kw)
    assert not ok and why

