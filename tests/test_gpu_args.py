"""GPU: the argument list (include/stark_mi.h, "Argument list") -- smi_dev_args_columns, smi_dev_air_compose_args,
smi_dev_air_prove_args / smi_air_verify_args -- against the restatement over the CPU oracle's primitives
(tests/args_compose.py), the CPU emulator of the kernels, and, with one argument, the existing permutation and lookup
provers.  Every comparison is exact.  `pytest -m gpu`."""
import os

import numpy as np
import pytest

import air_compose as ac
import args_compose as agc
import ext_compose as xc
import lookup_compose as lc
import perm_compose as pm
import pow_compose as pc
from test_args_emu import LISTS, LOG_NS, SPECS, case, emu, emu_columns, pooled, rejection_list, restated_column  # noqa: F401  (emu is a fixture)
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_ext import _dev_cols
from test_lookup_emu import chall

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
LB, TAU = 3, 1
KW = dict(row_leaves=True, ext=True)


def args_air(n_cols, args):
    from stark_rs_amd.mirror import Air
    return agc.mirror_air(Air(n_cols), args)


def gpu_columns(eng, cols, args, ch, c_stride=None, lead=0):
    """-> (c (4 A, n) uint64, closes); lead: words in front of c, so that its base is not 16-byte aligned.  The words in front
    of c, between its columns and behind the last stay untouched."""
    cols = np.asarray(cols, dtype=np.uint64)
    W, n = cols.shape
    A = len(args)
    c_stride = n if c_stride is None else c_stride
    with Dev(eng) as dev:
        d_trace = dev.upload(cols)
        ct, d_c = _dev_cols(np.full((4 * A, n), 0x7ffffffe, dtype=np.uint32), c_stride, lead)
        closes = eng.dev_args_columns(args_air(W, args), d_trace, W, n.bit_length() - 1, ch, d_c, c_stride)
        eng.sync()
        whole = ct.cpu().numpy().view(np.uint32)
    assert np.all(whole[:lead] == 0x7fffffff)
    host = whole[lead:]
    for e in range(4 * A):
        assert np.all(host[e * c_stride + n:(e + 1) * c_stride] == 0x7fffffff)
    return np.stack([host[e * c_stride:e * c_stride + n] for e in range(4 * A)]).astype(np.uint64), closes


# ---------------------------------------------------------------------------------------------- the columns
@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("log_n", LOG_NS)
def test_dev_columns_equal_the_restatement_and_the_emulator(engines, emu, log_n, name):
    """the shapes of tests/test_args_emu.py against the GPU; the restatement is the emulator's own yardstick there, and here
    too up to 2^11 rows and for one list at 2^13"""
    p, g = xc.PRIMES[log_n % 2]
    n = 1 << log_n
    cols, eight = pooled(log_n, p)
    args = [eight[i] for i in LISTS[name]]
    ch = chall(log_n)
    c, closes = gpu_columns(engines[p], cols, args, ch)
    assert closes == [True] * len(args)
    st, ce, _closes, _key = emu_columns(emu, cols, args, ch, p, g)
    assert st == 0 and np.array_equal(c, ce)
    if log_n <= 11 or name == "LPL":
        assert np.array_equal(c, agc.columns(cols, args, ch, p, g, column_of=restated_column)[0])
    # the 4-byte path: a stride that is no multiple of 4, then a base that is one word off 16 bytes
    c4, closes = gpu_columns(engines[p], cols, args, ch, c_stride=n + 1)
    assert np.array_equal(c4, c) and all(closes)
    c4, closes = gpu_columns(engines[p], cols, args, ch, c_stride=n + 4, lead=1)
    assert np.array_equal(c4, c) and all(closes)


def test_dev_columns_large_by_the_recurrences(engines):
    """2^19 rows is the smallest trace whose workgroup aggregates (512) take both scan workgroups of [perm, lookup] round their
    loop twice: each column satisfies its section's recurrence and closes; with one cell changed only that argument's bit
    drops and the recurrences still hold"""
    log_n = 19
    p, g = xc.PRIMES[log_n % 2]
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    src = rng.integers(0, p, n, dtype=np.uint64)
    tab = rng.permutation(n).astype(np.uint64)
    pick = rng.integers(0, n, n)
    cols = np.stack([src, src[rng.permutation(n)], tab[pick], tab, np.bincount(pick, minlength=n).astype(np.uint64)])
    args = [("perm", [0], [1]), ("lookup", [2], [3], 4)]
    ch = chall(log_n)
    c, closes = gpu_columns(engines[p], cols, args, ch)
    assert closes == [True, True]
    assert agc.recurrences_hold(c, cols, args, ch, p, g) == [(True, True), (True, True)]
    for a, col in ((0, 1), (1, 4)):
        bad = cols.copy()
        bad[col][n - 7] = (bad[col][n - 7] + np.uint64(1)) % np.uint64(p)
        c, closes = gpu_columns(engines[p], bad, args, ch)
        assert closes == [a != 0, a != 1]
        assert agc.recurrences_hold(c, bad, args, ch, p, g) == [(True, a != 0), (True, a != 1)]


def test_dev_columns_of_eight_arguments_large_by_the_recurrences(engines):
    """the list of eight (widths 1, 2 and 8, grid.y = 8) at 2^19 rows: eight scan workgroups, each twice round its loop"""
    log_n = 19
    p, g = xc.PRIMES[log_n % 2]
    n = 1 << log_n
    rng = np.random.default_rng(log_n + 1)
    src = rng.integers(0, p, (8, n), dtype=np.uint64)
    tab = rng.integers(0, p, (8, n), dtype=np.uint64)
    tab[0] = rng.permutation(n).astype(np.uint64)                        # distinct tuples at every width: a plain count
    pick = rng.integers(0, n, n)
    M = np.bincount(pick, minlength=n).astype(np.uint64)
    cols, args = [src, tab[:, pick], tab], []
    for kind, m in agc.EIGHT:                                            # agc.pool's layout, in numpy
        W = sum(len(c) for c in cols)
        if kind == "perm":
            cols.append(src[:m, rng.permutation(n)])
            args.append(("perm", list(range(m)), list(range(W, W + m))))
        else:
            cols.append(M[None, :])
            args.append(("lookup", list(range(8, 8 + m)), list(range(16, 16 + m)), W))
    cols = np.concatenate(cols)
    assert len(cols) <= 64
    ch = chall(log_n)
    c, closes = gpu_columns(engines[p], cols, args, ch)
    assert closes == [True] * 8
    assert agc.recurrences_hold(c, cols, args, ch, p, g) == [(True, True)] * 8


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_zero_denominators_name_the_smallest_key_and_the_next_call_succeeds(engines, p, g):
    """a zero denominator in argument 0 and in argument 2 at once, the lower row in either"""
    import stark_rs_amd as s
    log_n = 11
    n = 1 << log_n
    cols, eight = pooled(log_n, p)
    args = [eight[0], eight[3], eight[6]]                                # perm m = 1, lookup m = 1, perm m = 1
    r0, r2 = eight[0][2], eight[6][2]
    seen = set()
    for row in (0, 5, n - 1):
        ch = pm.gamma_for_zero(cols, r2, chall(4), row, p, g)
        key = agc.columns(cols, args, ch, p, g)[2]
        value = cols[r2[0]][row]
        assert key == min(16 * cols[r0[0]].index(value) + 1, 16 * cols[r2[0]].index(value) + 4 + 1)
        with pytest.raises(s.StarkMiError) as ei:
            gpu_columns(engines[p], cols, args, ch)
        assert ei.value.status == -1 and "no inverse" in str(ei.value)
        assert f"argument {(key & 15) >> 1}: f_R is zero in row {key >> 4}:" in str(ei.value)
        seen.add((key & 15) >> 1)
        c, closes = gpu_columns(engines[p], cols, args, chall(4))        # the context stays usable
        assert all(closes) and np.array_equal(c, agc.columns(cols, args, chall(4), p, g, column_of=restated_column)[0])
    assert seen == {0, 2}                                                # either argument was the one named
    look = [eight[3]]                                                    # f_L and f_T of one row: side 0 is named
    both = [list(c) for c in cols]
    both[look[0][1][0]][2] = both[look[0][2][0]][2]
    ch = pm.gamma_for_zero(both, look[0][2], chall(4), 2, p, g)
    key = agc.columns(both, look, ch, p, g)[2]
    with pytest.raises(s.StarkMiError) as ei:
        gpu_columns(engines[p], both, look, ch)
    assert key % 16 == 0 and f"argument 0: f_L is zero in row {key >> 4}:" in str(ei.value)


def test_argument_checks(engines):
    import stark_rs_amd as s
    from stark_rs_amd.mirror import Air
    p, _g = xc.PRIMES[0]
    eng = engines[p]
    with Dev(eng) as dev:
        d = dev.alloc(4 * 5 * 16 * 8)
        for args, log_n, text in (([("perm", [0], [1]), ("perm", [0], [5])], 2, "argument 1: perm: right_col must be < n_cols"),
                                  ([("lookup", [0], [1], 1)], 2, "argument 0: lookup: mult_col must be none of the tuple columns"),
                                  ([("perm", [0], [1])], 0, "log_n must be in 1 .. 27")):
            with pytest.raises(s.StarkMiError) as ei:
                eng.dev_args_columns(args_air(5, args), d, 5, log_n, chall(1), d)
            assert ei.value.status == -50 and text in str(ei.value)
        with pytest.raises(s.StarkMiError, match="c_stride < n"):
            eng.dev_args_columns(args_air(5, [("perm", [0], [1])]), d, 5, 2, chall(1), d, c_stride=3)
        with pytest.raises(ValueError, match="no argument list"):
            eng.dev_args_columns(Air(3), d, 3, 4, chall(1), d)
        with pytest.raises(s.StarkMiError) as ei:                        # log_blowup = 2 with a lookup: E < 4
            eng.dev_air_prove(args_air(5, [("perm", [0], [1]), ("lookup", [2], [3], 4)]), d, 5, 4, 2, 2, check=False, **KW)
        assert ei.value.status == -10


# ---------------------------------------------------------------------------------------------- the composition
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name,log_n", [("PL", 3), ("LPL", 4), ("EIGHT", 5), ("P", 6), ("L", 7)])
def test_dev_air_compose_args_equals_the_restatement(engines, oracle, p, g, name, log_n):
    eng, h = engines[p], g
    n, N = 1 << log_n, 1 << (log_n + LB)
    air, cols, args = case(n, p, SPECS[name])
    W, K, A = len(cols), len(air.constraints), len(args)
    ch = chall(21)
    c, closes, zero = agc.columns(cols, args, ch, p, g)
    assert zero is None and all(closes)
    lde = np.array(ac.lde(oracle, cols, p, g, log_n, LB, TAU, h), dtype=np.uint64)
    cl = np.array(ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, LB, TAU, h), dtype=np.uint64)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 2 * A), dtype=np.uint64)]
    want = pm.main_codeword(oracle, air, cols, wch[:4 * (W + K)], p, g, log_n, LB, TAU, h)
    want = (want + agc.aux_terms(oracle, lde, cl, args, ch, wch[4 * (W + K):], p, g, log_n, LB, TAU, h)) % np.uint64(p)
    # aligned (16-byte accesses); every stride odd; bases off 16 bytes
    for stride, c_stride, out_stride, lead in ((N, N, N, 0), (N + 1, N + 3, N + 5, 0), (N + 4, N + 4, N + 4, 1)):
        with Dev(eng) as dev:
            lt, d_lde = _dev_cols(lde.astype(np.uint32), stride, lead)
            zt, d_cl = _dev_cols(cl.astype(np.uint32), c_stride, lead)
            ot, d_out = _dev_cols(np.zeros((4, N), dtype=np.uint32), out_stride, lead)
            d_w = dev.upload_u64(wch)
            eng.dev_air_compose_args(air, d_lde, d_cl, W, log_n, LB, ch, d_w, d_out, stride=stride, c_stride=c_stride, out_stride=out_stride,
                                     lde_offset=h)
            eng.sync()
            host = ot.cpu().numpy().view(np.uint32)[lead:]
        got = np.stack([host[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)
        assert np.array_equal(got, want), (stride, lead)
        for e in range(4):
            assert np.all(host[e * out_stride + N:(e + 1) * out_stride] == 0x7fffffff)


def test_compose_args_on_every_trip_of_the_grid_equals_the_restatement_at_sampled_points(engines):
    """air_xargs_compose_kernel, which a plain list runs, on four trips of its grid (tests/test_gpu_perm.py, looping_check) with
    the list [lookup 1, perm 2, lookup 2], against agc.aux_terms_at"""
    from test_gpu_perm import looping_check
    p, g = xc.PRIMES[1]
    eng = engines[p]
    args = [("lookup", [4], [5], 6), ("perm", [0, 1], [2, 3]), ("lookup", [0, 1], [2, 3], 7)]
    assert [(a[0], len(a[1])) for a in args] == SPECS["LPL"]
    looping_check(eng, p, 8, 4 * len(args), 22, lambda air: agc.mirror_air(air, args),
                  lambda air, d_lde, d_c, W, log_n, ch, d_w, d_out: eng.dev_air_compose_args(air, d_lde, d_c, W, log_n, LB, ch, d_w, d_out),
                  lambda idx, lde_at, c_at, c_next, ch, w, wN, log_n: agc.aux_terms_at(idx, lde_at, c_at, c_next, args, ch, w, p, g, wN, log_n, TAU, g))


# ---------------------------------------------------------------------------------------------- whole proofs
def gpu_prove(eng, air, cols, log_n, t, bits, **kw):
    with Dev(eng) as dev:
        return eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, LB, t, grind_bits=bits, **KW, **kw)


@pytest.mark.parametrize("kind", ["perm", "lookup"])
def test_one_argument_gives_the_bytes_of_the_existing_prover(engines, kind):
    """A = 1: proof bytes and both roots equal those of smi_dev_air_prove_perm / smi_dev_air_prove_lookup, and each verifier
    accepts the other's proof"""
    log_n, t, bits = 8, 4, 8
    p, g = xc.PRIMES[kind == "lookup"]
    eng, n = engines[p], 1 << log_n
    if kind == "perm":
        old, cols = pm.with_permutation(*ac.make("fib", n, p), 2, p)
        arg = ("perm",) + tuple(old.perm)
    else:
        old, cols = lc.with_range_lookup(*ac.make("fib", n, p), p)
        arg = ("lookup",) + tuple(old.lookup_arg)
    W = len(cols)
    new, _ = ac.make("fib", n, p)
    new.n_cols = W
    agc.mirror_air(new, [arg])
    assert eng.air_plan(old, W, log_n, LB) == eng.air_plan(new, W, log_n, LB)
    a, b = gpu_prove(eng, old, cols, log_n, t, bits), gpu_prove(eng, new, cols, log_n, t, bits, timed=True)
    assert a["closes"] is True and b["closes"] == [True]
    assert a["proof"] == b["proof"] and a["column_roots"].tobytes() == b["column_roots"].tobytes() and a["top_indices"] == b["top_indices"]
    assert list(b["stage_ms"]) == ["lde", "commit", "args", "compose", "fri", "open"]
    for air_v, res in ((old, b), (new, a)):
        ok, why = eng.air_verify(air_v, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
        assert ok, why


@pytest.mark.parametrize("bits", [0, 8])
@pytest.mark.parametrize("name", ["PL", "LPL"])
def test_prove_args_bytes_equal_the_restatement_and_verify_agrees(engines, oracle, name, bits):
    log_n, t = 4, 4
    p, g = xc.PRIMES[bits % 3 % 2]
    eng, n, N = engines[p], 1 << log_n, 1 << (log_n + LB)
    air, cols, args = case(n, p, SPECS[name])
    W, A = len(cols), len(args)
    d, E = eng.air_plan(air, W, log_n, LB)
    assert (d, E) == (agc.plan(air, args, LB)[0], agc.plan(air, args, LB)[2])
    res = gpu_prove(eng, air, cols, log_n, t, bits)
    want = agc.prove(oracle, air, args, cols, p, g, log_n, LB, t, TAU, g, E, bits)
    assert want["closes"] == res["closes"] == [True] * A
    assert res["column_roots"].tobytes() == want["roots"]
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    R = eng.fri_num_rounds(eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t))
    assert len(res["proof"]) == agc.proof_len(N, E, t, R, W, A)          # the formula in the header
    at = pc.nonce_offset(N, R)
    assert int.from_bytes(res["proof"][at + 9:at + 17], "little") == want["nonce"]
    blank = [list(c) for c in cols]                                      # the helper once per lookup argument: the same bytes
    for arg in args:
        if not agc.is_perm(arg):
            blank[arg[3]] = [0] * n
    filled = gpu_prove(eng, air, blank, log_n, t, bits, fill_multiplicities=True)
    assert filled["proof"] == res["proof"] and filled["column_roots"].tobytes() == want["roots"]
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert ok, why


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_verify_args_rejections_agree_with_the_restatement(engines, oracle, p, g):
    import stark_rs_amd as s
    from stark_rs_amd.mirror import Air
    eng, log_n, t, bits = engines[p], 4, 4, 8
    air, cols, args = case(1 << log_n, p, SPECS["LPL"])
    W = len(cols)
    _d, E = eng.air_plan(air, W, log_n, LB)
    res = gpu_prove(eng, air, cols, log_n, t, bits)
    proof, roots = res["proof"], res["column_roots"].tobytes()

    def under(args_v):
        a = Air(W)
        a._symbolic, a.boundaries = air._symbolic, air.boundaries
        return agc.mirror_air(a, args_v)

    sentences = set()
    for name, args_v, bad_proof, bad_roots, want_class in rejection_list(oracle, air, cols, args, p, g, log_n, LB, t, bits, proof, roots):
        ok_r, cls = agc.verify(oracle, air, args_v, bad_roots, bad_proof, p, g, log_n, LB, t, TAU, g, E, bits)   # the restated verdict first
        assert not ok_r and cls == want_class, (name, cls)
        ok, why = eng.air_verify(under(args_v), bad_proof, [bad_roots[:32], bad_roots[32:]], W, log_n, LB, t, grind_bits=bits, **KW)
        assert not ok and why, name
        assert agc.reason_class(why) == cls, (name, why, cls)
        sentences.add(why)
    core = open(os.path.join(os.path.dirname(s.__file__), "csrc", "args_core.h")).read()
    for sentence in (line.split('"')[1] for line in core.splitlines() if '"argument openings: ' in line):
        assert sentence in sentences, sentence                           # every "argument openings:" sentence is reached
    # a trace where only argument 1 fails to close: proved with the mask 0b101, and rejected
    bad = agc.spoil(cols, args[1], p)
    with pytest.raises(s.StarkMiError, match=r"the arguments \[1\] do not close"):
        gpu_prove(eng, air, bad, log_n, t, bits)
    res = gpu_prove(eng, air, bad, log_n, t, bits, check=False)
    want = agc.prove(oracle, air, args, bad, p, g, log_n, LB, t, TAU, g, E, bits, honest=False)
    assert res["closes"] == want["closes"] == [True, False, True]
    assert res["proof"] == want["proof"] and res["column_roots"].tobytes() == want["roots"]
    ok_r, cls = agc.verify(oracle, air, args, want["roots"], want["proof"], p, g, log_n, LB, t, TAU, g, E, bits)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert not ok_r and not ok and agc.reason_class(why) == cls, (why, cls)
