"""CPU: the argument list's kernels' own lane code (csrc/args_core.h over perm_core.h and lookup_core.h), run by the emulator
library for every lane, workgroup and argument with the kernels' lane batching and block split, against the Python
restatement (tests/args_compose.py).  Every comparison is exact.

The library's prover and verifier need a GPU context; what runs here of a whole proof is the restated prover with the
emulator's columns and composition held against what it commits to, and the restated verifier over the rejection list.
tests/test_gpu_args.py holds the library's bytes and verdicts against the same."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import args_compose as agc
import ext_compose as xc
import perm_compose as pm
from test_lookup_emu import chall, degree_below

U64_MAX = (1 << 64) - 1
NO_INVERSE = -1
LOG_NS = [1, 2, 3, 10, 11, 13]   # 1, 2: below one lane's four rows; 10: exactly one workgroup; 11: two; 13: eight
# lists as indices into agc.EIGHT: [perm], [lookup], [perm, lookup], [lookup, perm, lookup], all eight (m in 1, 2, 8)
LISTS = {"P": [2], "L": [5], "PL": [0, 1], "LPL": [1, 2, 3], "EIGHT": list(range(8))}


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp = C.c_void_p
    L.emu_args_columns.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.AirArgs), vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64,
                                   C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.emu_air_compose_args.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.POINTER(_lib.AirArgs), vp, C.c_uint64,
                                       vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_int, C.c_uint32]
    return L


def make_args(args):
    """-> a _lib.AirArgs of the restatement's argument tuples"""
    from stark_rs_amd.mirror import Air
    return agc.mirror_air(Air(64), args).flatten(xc.PRIMES[0][0]).args


def emu_columns(emu, cols, args, ch, p, g, c_stride=None):
    """-> (status, c (4 A, n) uint64, closes as a list of bools, key)"""
    cols = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    W, n = cols.shape
    A = len(args)
    c_stride = n if c_stride is None else c_stride
    c = np.full(4 * A * c_stride, 0xdeadbeef, dtype=np.uint32)
    cha = np.array(ch, dtype=np.uint64)
    mask, key = C.c_uint32(0), C.c_uint64(0)
    st = emu.emu_args_columns(p, g, C.byref(make_args(args)), cols.ctypes.data, W, n.bit_length() - 1, cha.ctypes.data, c.ctypes.data, c_stride,
                              C.byref(mask), C.byref(key))
    for e in range(4 * A):   # nothing written between the columns
        assert np.all(c[e * c_stride + n:(e + 1) * c_stride] == 0xdeadbeef)
    out = np.stack([c[e * c_stride:e * c_stride + n] for e in range(4 * A)]).astype(np.uint64)
    return st, out, [bool(mask.value >> a & 1) for a in range(A)], key.value


_restated = {}


def restated_column(cols, arg, ch, p, g):
    """agc.column, computed once per (trace, argument, challenges): the lists share their arguments"""
    key = (id(cols), arg[0], tuple(arg[1]), tuple(arg[2]), arg[3] if len(arg) > 3 else None, tuple(ch), p)
    if key not in _restated:
        _restated[key] = (cols, agc.column(cols, arg, ch, p, g))   # cols is kept so that its id stays its own
    return _restated[key][1]


_pools = {}


def pooled(log_n, p):
    if (log_n, p) not in _pools:
        _pools[(log_n, p)] = agc.pool(1 << log_n, p, seed=log_n)
    return _pools[(log_n, p)]


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("log_n", LOG_NS)
def test_emu_columns_equal_the_restatement(emu, p, g, log_n, name):
    cols, eight = pooled(log_n, p)
    args = [eight[i] for i in LISTS[name]]
    ch = chall(log_n)
    want, closes, zero = agc.columns(cols, args, ch, p, g, column_of=restated_column)
    assert zero is None and all(closes)
    n = 1 << log_n
    st, c, got_closes, _ = emu_columns(emu, cols, args, ch, p, g, c_stride=n + (log_n % 3))
    assert st == 0
    assert np.array_equal(c, want)
    assert got_closes == [True] * len(args)
    if log_n == 3:
        assert agc.recurrences_hold(c, cols, args, ch, p, g) == [(True, True)] * len(args)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("log_n", [3, 11])
def test_one_spoilt_argument_drops_its_own_bit_alone(emu, p, g, log_n, name):
    cols, eight = pooled(log_n, p)
    args = [eight[i] for i in LISTS[name]]
    ch = chall(7)
    for a in range(len(args)):
        bad = agc.spoil(cols, args[a], p)
        st, c, closes, _ = emu_columns(emu, bad, args, ch, p, g)
        assert st == 0 and closes == [i != a for i in range(len(args))], a
        if log_n == 3:
            assert np.array_equal(c, agc.columns(bad, args, ch, p, g)[0])


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_n", [3, 11])
def test_the_smallest_zero_denominator_key_is_named(emu, p, g, log_n):
    """a zero denominator in argument 0 and in argument 2 at once, the lower row in either: the key is 16 row + 2 a + side"""
    n = 1 << log_n
    cols, eight = pooled(log_n, p)
    args = [eight[0], eight[3], eight[6]]                                # perm m = 1, lookup m = 1, perm m = 1
    r0, r2 = eight[0][2], eight[6][2]                                    # the two permutations' own right columns
    for row in (0, 5 % n, n - 1):
        ch = pm.gamma_for_zero(cols, r2, chall(4), row, p, g)            # f_R of argument 2 is zero in `row` ...
        value = cols[r2[0]][row]                                         # ... and f_R of argument 0 where it holds that value
        want = min(16 * cols[r0[0]].index(value) + 1, 16 * cols[r2[0]].index(value) + 4 + 1)
        assert agc.columns(cols, args, ch, p, g) == (None, None, want)
        st, _c, _closes, key = emu_columns(emu, cols, args, ch, p, g)
        assert st == NO_INVERSE and key == want
    # side 0 before side 1 in one row and argument: a lookup whose f_L and f_T vanish together
    look = [eight[3]]
    both = [list(c) for c in cols]
    both[look[0][1][0]][2 % n] = both[look[0][2][0]][2 % n]              # the looked-up value of row 2 is the table value of row 2
    ch = pm.gamma_for_zero(both, look[0][2], chall(4), 2 % n, p, g)
    st, _c, _closes, key = emu_columns(emu, both, look, ch, p, g)
    assert st == NO_INVERSE and key == agc.columns(both, look, ch, p, g)[2] and key % 16 == 0
    st, c, _closes, _ = emu_columns(emu, cols, args, chall(4), p, g)     # the next call succeeds
    assert st == 0 and np.array_equal(c, agc.columns(cols, args, chall(4), p, g, column_of=restated_column)[0])


# ---------------------------------------------------------------------------------------------- the composition
def case(n, p, spec, name="fib", seed=9):
    """-> (air with the argument list, cols, args): the main AIR `name` beside a pool over columns of its own"""
    air, cols = ac.make(name, n, p)
    W = len(cols)
    more, args = agc.pool(n, p, seed, spec, first=W)
    air.n_cols = W + len(more)
    return agc.mirror_air(air, args), [list(c) for c in cols] + more, args


def emu_compose(emu, air, cols_lde, cl, ch, wch, p, g, log_n, lb, tau, h, stride=None, c_stride=None, out_stride=None, force_direct=0, grid=0):
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    W, CW = len(cols_lde), len(cl)
    stride, c_stride, out_stride = (N if v is None else v for v in (stride, c_stride, out_stride))
    a = air.flatten(p)
    cfg = _lib.StarkCfg(log_n, lb, W, 1, tau, h, 0, 1)
    lde = np.zeros(W * stride, dtype=np.uint32)
    for c in range(W):
        lde[c * stride:c * stride + N] = cols_lde[c]
    cb = np.zeros(CW * c_stride, dtype=np.uint32)
    for e in range(CW):
        cb[e * c_stride:e * c_stride + N] = cl[e]
    out = np.full(4 * out_stride, 0xdeadbeef, dtype=np.uint32)
    cha, wa = np.array(ch, dtype=np.uint64), np.array(wch, dtype=np.uint64)
    st = emu.emu_air_compose_args(p, g, C.byref(cfg), C.byref(a), C.byref(a.args), lde.ctypes.data, stride, cb.ctypes.data, c_stride, cha.ctypes.data,
                                  wa.ctypes.data, out.ctypes.data, out_stride, force_direct, grid)
    assert st == 0
    for e in range(4):
        assert np.all(out[e * out_stride + N:(e + 1) * out_stride] == 0xdeadbeef)
    return np.stack([out[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)


SPECS = {"P": [("perm", 2)], "L": [("lookup", 2)], "PL": [("perm", 1), ("lookup", 2)], "LPL": [("lookup", 1), ("perm", 2), ("lookup", 2)], "EIGHT": agc.EIGHT}


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("log_n", [2, 5])
def test_emu_air_compose_args_equals_the_restatement_and_the_degree_tells_one_spoilt_argument(oracle, emu, p, g, log_n, name):
    """the honest composition stays within its degree bound; with exactly one argument of the list spoilt, at each position in
    turn, it exceeds it"""
    lb, tau, h = 3, 1, g
    n, N = 1 << log_n, 1 << (log_n + lb)
    air, cols, args = case(n, p, SPECS[name])
    W, K, A = len(cols), len(air.constraints), len(args)
    _d, D, _E = agc.plan(air, args, lb)
    ch = chall(11)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 2 * A), dtype=np.uint64)]
    for spoilt in [None] + list(range(A)):
        tr = cols if spoilt is None else agc.spoil(cols, args[spoilt], p)
        c, closes, zero = agc.columns(tr, args, ch, p, g)
        assert zero is None and closes == [a != spoilt for a in range(A)]
        lde = ac.lde(oracle, tr, p, g, log_n, lb, tau, h)
        cl = ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)
        want = pm.main_codeword(oracle, air, tr, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
        want = (want + agc.aux_terms(oracle, lde, np.asarray(cl, dtype=np.uint64), args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h)) % np.uint64(p)
        got = emu_compose(emu, air, lde, cl, ch, wch, p, g, log_n, lb, tau, h)
        assert np.array_equal(got, want), (name, spoilt)
        assert degree_below(oracle, got, D * n, p, g, log_n + lb, h) == (spoilt is None), (name, spoilt)
        if spoilt is None:   # the shapes of the 4-byte path and a grid that makes every lane loop
            assert np.array_equal(emu_compose(emu, air, lde, cl, ch, wch, p, g, log_n, lb, tau, h, stride=N + 1, c_stride=N + 3, out_stride=N + 5), want)
            assert np.array_equal(emu_compose(emu, air, lde, cl, ch, wch, p, g, log_n, lb, tau, h, force_direct=1, grid=1), want)


# ---------------------------------------------------------------------------------------------- whole proofs, restated
@pytest.mark.parametrize("bits", [0, 8])
@pytest.mark.parametrize("name", ["PL", "LPL"])
def test_restated_proofs_commit_to_the_emulators_columns_and_codeword(oracle, emu, name, bits):
    log_n, lb = 4, 3
    p, g = xc.PRIMES[bits % 3 % 2]
    n, N, t, tau, h = 1 << log_n, 1 << (log_n + lb), 4, 1, g
    air, cols, args = case(n, p, SPECS[name])
    W, A = len(cols), len(args)
    _d, _D, E = agc.plan(air, args, lb)
    want = agc.prove(oracle, air, args, cols, p, g, log_n, lb, t, tau, h, E, bits)
    assert all(want["closes"])
    st, c, closes, _ = emu_columns(emu, cols, args, want["ch"], p, g)
    assert st == 0 and all(closes) and np.array_equal(c, want["c"])
    lde = ac.lde(oracle, cols, p, g, log_n, lb, tau, h)
    cl = ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)
    assert np.array_equal(emu_compose(emu, air, lde, cl, want["ch"], want["wch"], p, g, log_n, lb, tau, h), want["cw"])
    _, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
    R = oracle.fri_num_rounds(oracle.fri_cfg(wN, h, N, E, t, p))
    assert len(want["proof"]) == agc.proof_len(N, E, t, R, W, A)         # the formula in the header
    assert agc.verify(oracle, air, args, want["roots"], want["proof"], p, g, log_n, lb, t, tau, h, E, bits) == (True, "")


def offsets(W, A, log_N, t, plen):
    """byte offsets inside a proof: (section 1, its paths, section 2, its paths)"""
    s1 = plen - agc.opening_len(W, A, log_N, t)
    p1 = s1 + 4 * t * (9 + 8 * W)
    s2 = p1 + 4 * t * (9 + 32 * log_N)
    p2 = s2 + 4 * t * (9 + 32 * A)
    return s1, p1, s2, p2


def rejection_list(oracle, air, cols, args, p, g, log_n, lb, t, bits, proof, roots):
    """-> [(name, arguments to verify under, proof, roots, class)]: every entry must be rejected.  args has three arguments."""
    log_N, tau, h = log_n + lb, 1, g
    W, A = len(cols), len(args)
    _d, _D, E = agc.plan(air, args, lb)
    s1, p1, s2, p2 = offsets(W, A, log_N, t, len(proof))
    rec1, rec2, prec = 9 + 8 * W, 9 + 32 * A, 9 + 32 * log_N
    out = []
    flips = [("row tag 1", s1 + 2 * rec1, "record"), ("a trace value", s1 + 3 * rec1 + 9 + 8 * (W - 1), "path"),
             ("path tag 1", p1 + prec, "record"), ("path digest 1", p1 + 5 * prec + 9 + 40, "path"),
             ("row tag 2", s2 + rec2, "record"), ("path tag 2", p2 + 3 * prec, "record"), ("path digest 2", p2 + 7 * prec + 9 + 3, "path")]
    flips += [(f"a coordinate of column {a}", s2 + 6 * rec2 + 9 + 8 * (4 * a + a % 4), "path") for a in range(A)]
    for name, at, cls in flips:
        bad = bytearray(proof)
        bad[at] ^= 1
        out.append((name, args, bytes(bad), roots, cls))
    tam = agc.prove(oracle, air, args, cols, p, g, log_n, lb, t, tau, h, E, bits, c_plus_p=4 * A - 2)
    out.append(("non-canonical coordinate", args, tam["proof"], tam["roots"], "canonical"))
    out.append(("section 2 cut short", args, proof[:-1], roots, "length"))
    out.append(("section 2 missing", args, proof[:s2], roots, "length"))
    out.append(("section 1 cut short", args, proof[:p1 - 1], roots, "length"))
    out.append(("cut inside FRI", args, proof[:s1 // 2], roots, "fri"))
    out.append(("swapped roots", args, proof, roots[32:] + roots[:32], "fri"))
    out.append(("the list in another order", [args[2], args[1], args[0]], proof, roots, "composition"))
    swapped = list(args)
    swapped[1] = (args[1][0], args[1][2], args[1][1]) + tuple(args[1][3:])
    out.append(("one argument's columns swapped", swapped, proof, roots, "composition"))
    out.append(("A - 1 arguments", args[:-1], proof, roots, "fri"))      # fewer weights: another transcript, another seed
    return out


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_restated_verifier_rejects_the_list(oracle, p, g):
    log_n, lb, t, bits, tau, h = 4, 3, 4, 8, 1, g
    air, cols, args = case(1 << log_n, p, SPECS["LPL"])
    _d, _D, E = agc.plan(air, args, lb)
    res = agc.prove(oracle, air, args, cols, p, g, log_n, lb, t, tau, h, E, bits)
    assert agc.verify(oracle, air, args, res["roots"], res["proof"], p, g, log_n, lb, t, tau, h, E, bits) == (True, "")
    for name, args_v, bad_proof, bad_roots, cls in rejection_list(oracle, air, cols, args, p, g, log_n, lb, t, bits, res["proof"], res["roots"]):
        assert agc.verify(oracle, air, args_v, bad_roots, bad_proof, p, g, log_n, lb, t, tau, h, E, bits) == (False, cls), name
    # a trace where only argument 1 fails to close is proved and rejected
    bad = agc.spoil(cols, args[1], p)
    res = agc.prove(oracle, air, args, bad, p, g, log_n, lb, t, tau, h, E, bits, honest=False)
    assert res["closes"] == [True, False, True]
    assert not agc.verify(oracle, air, args, res["roots"], res["proof"], p, g, log_n, lb, t, tau, h, E, bits)[0]
