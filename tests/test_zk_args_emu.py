"""CPU: zero-knowledge DEEP proofs with an argument list (include/stark_mi.h) -- the lane bodies of csrc/zkargs_core.h run by the
emulator library (csrc/emu_zkargs.cpp) against the Python restatement (tests/zk_args_compose.py): the tail step of the auxiliary
columns at aligned and misaligned bases, the three auxiliary quotients, the multiplicity helper with a row bound, the derived
AIR with both exemption columns, the plan with its refusals, the left side of the verifier's consistency check, and the
restated prover against the restated verifier with every rejection the GPU test repeats on the library.  Every comparison
is exact.

smi_air_verify_deep_zk_xargs takes a context, which takes a GPU: the library's verifier runs in tests/test_gpu_zk_args.py alone.
Here the rejections go through the restated verifier (za.verify), and the one step of the verifier that is new arithmetic --
the left side of the consistency check over the derived AIR -- is the library's own code (zkargs_core.h zkx_ood_lhs through
emu_zkx_ood_lhs), compared with the restatement's on every restated proof."""
import ctypes as C
import functools

import numpy as np
import pytest

import air_compose as ac
import deep_compose as dc
import ext_compose as xc
import perm_compose as pm
import xargs_compose as xa
import zk_args_compose as za
import zk_compose as zk
from test_lookup_emu import chall, degree_below
from test_xargs_emu import flat

P_REF, G_REF = xc.PRIMES[0]
SEED = bytes(range(32))
U64_MAX = (1 << 64) - 1
LOOKUP_MISSING = -56
LISTS = {"vm": za.vm, "selectors": za.selectors}


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.emu_zk_args_tail.argtypes = [vp, u64, u32, u32, u32, vp, C.c_int, vp, C.POINTER(u32)]
    L.emu_air_compose_zk_xargs.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), vp, u64, vp, u64, vp, vp, vp,
                                           u64, C.c_int, u32]
    L.emu_zkx_derived_air.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), vp, vp, vp, vp, vp, vp, vp, vp]
    L.emu_xargs_multiplicities_rows.argtypes = [u64, u64, C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), u32, vp, u32, u32, u64, vp, C.c_int, C.POINTER(u64)]
    L.emu_xargs_multiplicities.argtypes = [u64, u64, C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), u32, vp, u32, u32, vp, C.c_int, C.POINTER(u64)]
    L.emu_xargs_columns.argtypes = [u64, u64, C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), vp, u32, u32, vp, vp, u64, C.POINTER(u32), C.POINTER(u64)]
    L.emu_zkx_ood_lhs.argtypes =[u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), vp, vp, vp, vp, vp]
    return L


def w_of(o, log_n, p, g):
    return o.ff_prim_nth_root_g(1 << log_n, p, g)


# ---------------------------------------------------------------------------------------------- the tail step
def emu_tail(emu, c, log_n, kt, A, rnd, lead, pad, aligned):
    """c: (4 A, n) -> (columns after the step, closing values, misplaced 16-byte stores); the buffer starts `lead` words into an
    aligned allocation and the columns are n + pad apart"""
    n = 1 << log_n
    cs = n + pad
    buf = np.full(4 * A * cs + lead + 8, 0xdeadbeef, dtype=np.uint32)
    for col in range(4 * A):
        buf[lead + col * cs:lead + col * cs + n] = c[col]
    r = np.ascontiguousarray(np.array(rnd, dtype=np.uint32))
    closing, bad = np.zeros(4 * A, dtype=np.uint64), C.c_uint32(7)
    assert emu.emu_zk_args_tail(buf.ctypes.data + 4 * lead, cs, log_n, kt, A, r.ctypes.data, int(aligned), closing.ctypes.data, C.byref(bad)) == 0
    assert np.all(buf[:lead] == 0xdeadbeef) and np.all(buf[lead + 4 * A * cs:] == 0xdeadbeef)
    for col in range(4 * A):                                  # nothing written between the columns
        assert np.all(buf[lead + col * cs + n:lead + (col + 1) * cs] == 0xdeadbeef)
    out = np.stack([buf[lead + col * cs:lead + col * cs + n] for col in range(4 * A)]).astype(np.uint64)
    return out, [int(v) for v in closing], bad.value


@pytest.mark.parametrize("log_n,t,A", [(6, 1, 1), (7, 2, 3), (8, 5, 8), (11, 32, 3)])
@pytest.mark.parametrize("pad", [0, 1, 2, 4])
def test_the_tail_step_overwrites_exactly_the_tail(emu, log_n, t, A, pad):
    """rows <= n_a stay, rows n_a + 1 .. n - 1 take the column's k_t - 1 words, the closing values are row n_a; n_a + 1 is odd in
    every shape, and with a stride that is no multiple of 4 the columns' tails start at every residue mod 4"""
    n, kt = 1 << log_n, za.k_t(t)
    na = n - kt
    assert (na + 1) % 2 == 1 and na % 8 == 0
    rng = np.random.default_rng(log_n + pad)
    c = rng.integers(0, P_REF, (4 * A, n), dtype=np.uint64)
    rnd = rng.integers(0, P_REF, 4 * A * (kt - 1), dtype=np.uint64)
    want = c.copy()
    for col in range(4 * A):
        want[col, na + 1:] = rnd[col * (kt - 1):(col + 1) * (kt - 1)]
    for lead, aligned in ((0, True), (0, False), (1, False), (3, False)):
        got, closing, bad = emu_tail(emu, c, log_n, kt, A, rnd, lead, pad, aligned)
        assert np.array_equal(got, want), (lead, aligned)
        assert closing == [int(v) for v in c[:, na]] and bad == 0


def test_the_tail_step_equals_the_restated_columns(oracle, emu):
    """the emulator's tail over the library's column build = the restatement's columns, closing values and verdicts"""
    from test_xargs_emu import emu_columns
    p, g, log_n, t = P_REF, G_REF, 7, 1
    n, kt = 1 << log_n, za.k_t(t)
    air, cols, args = za.selectors(log_n, t, p)
    trace = za.randomised(cols, zk.rng(oracle, SEED, zk.STREAM_ROWS, len(cols) * kt, p), t)
    ch = chall(5)
    tail = zk.rng(oracle, SEED, za.STREAM_TAIL, 4 * len(args) * (kt - 1), p)
    want, closes, closing, zero = za.columns(xa.widen(trace, air, p), args, ch, p, g, len(cols), t, tail)
    assert zero is None and closes == [True] * 3
    st, c, _wrap, _key = emu_columns(emu, air, trace, args, ch, p, g)
    assert st == 0
    got, got_closing, bad = emu_tail(emu, c, log_n, kt, len(args), tail, 0, 0, True)
    assert np.array_equal(got, want) and got_closing == [v for el in closing for v in el] and bad == 0
    broken = [list(col) for col in cols]                      # a lookup miss on an active row: the closing value is not init
    broken[0][cols[3].index(1)] = p - 1
    trace = za.randomised(broken, zk.rng(oracle, SEED, zk.STREAM_ROWS, len(cols) * kt, p), t)
    _c, closes, _closing, zero = za.columns(xa.widen(trace, air, p), args, ch, p, g, len(cols), t, tail)
    assert zero is None and closes == [False, True, True]


# ---------------------------------------------------------------------------------------------- the multiplicities
def emu_mult_rows(emu, air, cols, args, a, p, g, rows, order=0):
    cols = np.ascontiguousarray(np.array(cols, dtype=np.uint32))
    n_cols, n = cols.shape
    f = flat(air, args, p)
    M = np.full(n + 2, 0xdeadbeef, dtype=np.uint32)
    missing = C.c_uint64(0)
    log_n = n.bit_length() - 1
    if rows is None:
        st = emu.emu_xargs_multiplicities(p, g, C.byref(f), C.byref(f.xargs), a, cols.ctypes.data, n_cols, log_n, M[1:].ctypes.data, order, C.byref(missing))
    else:
        st = emu.emu_xargs_multiplicities_rows(p, g, C.byref(f), C.byref(f.xargs), a, cols.ctypes.data, n_cols, log_n, rows, M[1:].ctypes.data, order,
                                               C.byref(missing))
    assert M[0] == M[-1] == 0xdeadbeef
    return st, [int(v) for v in M[1:-1]], missing.value


@pytest.mark.parametrize("name", sorted(LISTS))
def test_the_row_bound_of_the_multiplicity_helper(emu, name):
    p, g, log_n, t = P_REF, G_REF, 7, 1
    n, na = 1 << log_n, (1 << log_n) - za.k_t(t)
    air, cols, args = LISTS[name](log_n, t, p)
    for a, arg in enumerate(args):
        if arg[0] != "lookup":
            assert emu_mult_rows(emu, air, cols, args, a, p, g, na)[0] == -50
            continue
        for order in (0, 1):
            assert emu_mult_rows(emu, air, cols, args, a, p, g, n, order) == emu_mult_rows(emu, air, cols, args, a, p, g, None, order)
            st, M, _ = emu_mult_rows(emu, air, cols, args, a, p, g, na, order)
            assert st == 0 and M == cols[arg[3]] and not any(M[na:])
    if name == "vm":
        missed = [list(c) for c in cols]                                         # a tail lookup row that would miss over all n rows
        missed[4][na + 1] = 4 * n + 9
        st, _M, missing = emu_mult_rows(emu, air, missed, args, 1, p, g, None)
        assert st == LOOKUP_MISSING and missing == na + 1
        st, M, _ = emu_mult_rows(emu, air, missed, args, 1, p, g, na)
        assert st == 0 and M == cols[6]
        moved = [list(c) for c in cols]                                          # a value that only a TAIL table row holds
        moved[5][na + 2] = moved[4][3] = 4 * n + 5
        st, _M, missing = emu_mult_rows(emu, air, moved, args, 1, p, g, na)
        assert st == LOOKUP_MISSING and missing == 3
    assert emu_mult_rows(emu, air, cols, args, 0 if name == "selectors" else 1, p, g, n + 1)[0] == -50
    assert emu_mult_rows(emu, air, cols, args, 0 if name == "selectors" else 1, p, g, 0)[0] == -50


# ---------------------------------------------------------------------------------------------- the derived AIR and the plan
def emu_derived(emu, air, W, log_n, t, p, g, tau=1, lb=2):
    from stark_rs_amd import _lib
    a = air.flatten(p)
    cfg = _lib.StarkCfg(log_n, lb, W, 1, tau, g, t, 1)
    head = np.zeros(6, dtype=np.uint64)
    none = None
    assert emu.emu_zkx_derived_air(p, g, C.byref(cfg), C.byref(a), head.ctypes.data, none, none, none, none, none, none, none) == 0
    K, nt, nf, nb, Q, npv = [int(v) for v in head]
    arrs = [np.zeros(K + 1, dtype=np.uint32), np.zeros(nt, dtype=np.uint64), np.zeros(nt + 1, dtype=np.uint32), np.zeros(nf, dtype=np.uint32),
            np.zeros(nf, dtype=np.uint32), np.zeros(Q, dtype=np.uint32), np.zeros(npv, dtype=np.uint64)]
    assert emu.emu_zkx_derived_air(p, g, C.byref(cfg), C.byref(a), head.ctypes.data, *[x.ctypes.data for x in arrs]) == 0
    return (K, nt, nf, nb, Q), [[int(v) for v in x] for x in arrs]


def constrained(log_n, t, p):
    """an AIR with constraints that read a periodic column at this row and the next, and a trace: a' = a + k (k of period 4),
    b' = b a k'"""
    from stark_rs_amd.mirror import Air
    n = 1 << log_n
    air = Air(2)
    k = air.periodic([3, 1, 4, 1])
    air.transition({("next", 0): 1, ("cur", 0): -1, ("per", k): -1})
    air.transition({("next", 1): 1, (("cur", 1), ("cur", 0), ("per_next", k)): -1})
    a, b = [2], [5]
    for r in range(n - 1):
        a.append((a[-1] + [3, 1, 4, 1][r % 4]) % p)
        b.append(b[-1] * a[-2] % p * [3, 1, 4, 1][(r + 1) % 4] % p)
    air.boundary(0, 0, 2).boundary(1, 0, 5)
    return air, [a, b]


@pytest.mark.parametrize("log_n,t", [(6, 1), (7, 2), (8, 3)])
def test_the_library_derives_the_restated_air_with_both_exemption_columns(oracle, emu, log_n, t):
    p, g, n = P_REF, G_REF, 1 << log_n
    na = n - za.k_t(t)
    air, _cols = constrained(log_n, t, p)
    for tau in (1, 5):
        w = w_of(oracle, log_n, p, g)
        want = za.derived_air(air, log_n, t, p, tau, w).flatten(p)
        head, arrs = emu_derived(emu, air, 2, log_n, t, p, g, tau)
        assert head == (want.n_constraints, want.n_terms, want.n_factors, want.n_boundary, want.n_periodic)
        assert arrs == [[int(v) for v in k] for k in (want._keep[0], want._keep[1], want._keep[2], want._keep[3], want._keep[4], want._keep[8], want._keep[9])]
        E, EA = arrs[6][-2 * n:-n], arrs[6][-n:]
        assert (E, EA) == za.exemption_columns(n, t, p, tau, w)
        assert [r for r in range(n) if E[r] == 0] == list(range(na - 1, n - 1)) and [r for r in range(n) if EA[r] == 0] == list(range(na, n))
        assert 2 * 2 + 3 + 0 in arrs[3] and 2 * 2 + 2 not in arrs[3]          # k at the next row: variable 2 W + (Q + 2) + 0; E_A (2 W + Q + 1) is read by none


def test_mirror_derives_the_list_form(oracle):
    p, g, log_n, t = P_REF, G_REF, 6, 1
    air, _cols = constrained(log_n, t, p)
    air.add_permutation([0], [1])
    w = w_of(oracle, log_n, p, g)
    got, want = air.zk_derived(p, log_n, t, 5, w, with_args=True), za.derived_air(air, log_n, t, p, 5, w)
    assert got.periodics == want.periodics and got._symbolic == want._symbolic and got.args == [] and len(air.args) == 1


def lib_plan(air, args, W, log_n, lb, t, p=P_REF, g=G_REF, layout=False):
    import stark_rs_amd as s
    from stark_rs_amd import _lib
    cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, g, t, 1)
    f = flat(air, args, p)
    return (s.engine.air_deep_zk_args_layout if layout else s.engine.air_plan_deep_zk_args)(p, f, f.xargs, cfg)


@pytest.mark.parametrize("name,log_n,lb,t,numbers", [("vm", 6, 2, 1, (4, 5, 24, 5)), ("vm", 7, 3, 2, (4, 5, 32, 9)), ("selectors", 7, 2, 1, (4, 5, 24, 5)),
                                                     ("vm", 11, 3, 32, (4, 5, 272, 129))])
def test_plan_and_layout_numbers(name, log_n, lb, t, numbers):
    """the numbers are written out: a lookup's degree 4 gives D = 4 (= B at log_blowup 2) and D' = 5"""
    air, cols, args = LISTS[name](log_n, t, P_REF)
    assert lib_plan(air, args, 9, log_n, lb, t) == za.plan(air, args, log_n, t) == numbers
    assert lib_plan(air, args, 9, log_n, lb, t, layout=True) == za.layout(9, 3, numbers[1], log_n, lb, t)
    only_perm = [args[0]] if name == "vm" else [("perm", [4], [5])]
    assert lib_plan(air, only_perm, 9, log_n, lb, t)[:2] == za.plan(air, only_perm, log_n, t)[:2] == (3, 3 if log_n < 11 else 3)


def test_plan_refusals():
    from stark_rs_amd import StarkMiError
    from stark_rs_amd.mirror import Air
    p = P_REF

    def refused(air, args, W, log_n, lb, t, words):
        with pytest.raises(StarkMiError) as e:
            lib_plan(air, args, W, log_n, lb, t)
        assert e.value.status == -50 and words in str(e.value), str(e.value)
    perm = [("perm", [0], [1])]
    refused(Air(2), perm, 2, 5, 2, 1, "zk deep argument: k_t = 8 t + 16 = 24 >= n / 2")
    assert lib_plan(Air(2), perm, 2, 6, 2, 1) == (3, 3, 24, 5)
    full = Air(2)
    for _ in range(15):
        full.periodic([1, 2])
    refused(full, perm, 2, 6, 2, 1, "zk deep argument: Q + 2 = 17 > SMI_AIR_MAX_PERIODIC (16)")
    full.periodics.pop()
    assert lib_plan(full, perm, 2, 6, 2, 1) == (3, 3, 24, 5)
    late = Air(2)
    late.boundary(1, 40, 3)
    refused(late, perm, 2, 6, 2, 1, "zk deep argument: boundary point 0 lies on row 40 >= n - k_t = 40, a randomiser row")
    late.boundaries[-1] = (1, 39, 3)
    assert lib_plan(late, perm, 2, 6, 2, 1) == (3, 3, 24, 5)
    deep = Air(2)
    deep.transition({("next", 0): 1, ("cur", 0, 9): -1})          # degree 10 with the factor: D = 16, D' = 17
    refused(deep, perm, 2, 8, 4, 1, "zk deep argument: 4 D' + 5 = 73 > 64")
    refused(Air(3), [("lookup", [0], [1], 2)], 3, 6, 1, 1, "zk deep argument: D > 2^log_blowup")      # a lookup needs D = 4 > B = 2
    refused(Air(2), [("perm", [0], [("per", 0)])], 2, 6, 2, 1, "xargs: argument 0")                    # the list is checked against the caller's Q


def test_the_entry_points_are_declared_everywhere():
    import os
    import re
    import stark_rs_amd
    from stark_rs_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stark_mi.h")).read()
    rust = open(os.path.join(root, "bindings", "stark_mi.rs")).read()
    assert "Zero-knowledge DEEP proofs with an argument list" in header and "Left out: argument lists" not in header
    stark_rs_amd.build()
    names = ["smi_air_plan_deep_zk_xargs", "smi_air_deep_zk_xargs_layout", "smi_dev_zk_args_tail", "smi_dev_air_compose_zk_xargs",
             "smi_dev_xargs_multiplicities_rows", "smi_dev_air_prove_deep_zk_xargs", "smi_air_verify_deep_zk_xargs"]
    for name in names:
        assert re.search(r"\bint %s\(" % name, header), name
        assert "pub fn %s(" % name in rust, name
        assert getattr(_lib.lib(), name).argtypes is not None, name
    assert set(names) <= set(stark_rs_amd.declared_symbols())


# ---------------------------------------------------------------------------------------------- the auxiliary quotients
def emu_compose(emu, air, args, cols_lde, cl, ch, wch, p, g, log_n, lb, t, tau, h, stride=None, c_stride=None, out_stride=None, force_direct=0, grid=0):
    from stark_rs_amd import _lib
    N = 1 << (log_n + lb)
    n_cols, CW = len(cols_lde), len(cl)
    stride, c_stride, out_stride = (N if v is None else v for v in (stride, c_stride, out_stride))
    f = flat(air, args, p)
    cfg = _lib.StarkCfg(log_n, lb, n_cols, 1, tau, h, t, 1)
    lde = np.zeros(n_cols * stride, dtype=np.uint32)
    for c in range(n_cols):
        lde[c * stride:c * stride + N] = cols_lde[c]
    cb = np.zeros(CW * c_stride, dtype=np.uint32)
    for e in range(CW):
        cb[e * c_stride:e * c_stride + N] = cl[e]
    out = np.full(4 * out_stride, 0xdeadbeef, dtype=np.uint32)
    cha, wa = np.array(ch, dtype=np.uint64), np.array(wch, dtype=np.uint64)
    st = emu.emu_air_compose_zk_xargs(p, g, C.byref(cfg), C.byref(f), C.byref(f.xargs), lde.ctypes.data, stride, cb.ctypes.data, c_stride, cha.ctypes.data,
                                      wa.ctypes.data, out.ctypes.data, out_stride, force_direct, grid)
    assert st == 0
    for e in range(4):
        assert np.all(out[e * out_stride + N:(e + 1) * out_stride] == 0xdeadbeef)
    return np.stack([out[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name,log_n,lb,t", [("vm", 6, 2, 1), ("selectors", 7, 2, 1), ("vm", 7, 3, 2)])
def test_emu_air_compose_zk_xargs_equals_the_restatement(oracle, emu, p, g, name, log_n, lb, t):
    """the composition of the derived AIR plus the 3 A quotients: equal to the restatement's and of degree < D n on a statement;
    without E_A, or with a column that does not close, it exceeds the bound (where the bound is below N)"""
    tau, h = 1, g
    n, N, kt = 1 << log_n, 1 << (log_n + lb), za.k_t(t)
    air, cols, args = LISTS[name](log_n, t, p)
    W, K, A = len(cols), len(air.constraints), len(args)
    D = za.segments_unmasked(air, args)
    w = w_of(oracle, log_n, p, g)
    dair = za.derived_air(air, log_n, t, p, tau, w)
    trace = za.randomised(cols, zk.rng(oracle, SEED, zk.STREAM_ROWS, W * kt, p), t)
    wide = xa.widen(trace, dair, p)
    ch = chall(11)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 3 * A), dtype=np.uint64)]
    c, closes, _closing, zero = za.columns(wide, args, ch, p, g, W, t, zk.rng(oracle, SEED, za.STREAM_TAIL, 4 * A * (kt - 1), p))
    assert zero is None and all(closes)
    lde_wide = np.asarray(ac.lde(oracle, wide, p, g, log_n, lb, tau, h), dtype=np.uint64)
    cl = ac.lde(oracle, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)
    main = dc.composition(oracle, dair, trace, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
    aux = lambda **kw: za.aux_terms(oracle, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W, t, len(wide) - 1, **kw)
    want = (main + aux()) % np.uint64(p)
    got = emu_compose(emu, air, args, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, t, tau, h)
    assert np.array_equal(got, want)
    tight = D * n < N                                                    # at D = B every codeword has degree < D n: the bound says nothing
    assert degree_below(oracle, got, D * n, p, g, log_n + lb, h)
    assert not tight or not degree_below(oracle, (main + aux(no_ea=True)) % np.uint64(p), D * n, p, g, log_n + lb, h)
    assert np.array_equal(emu_compose(emu, air, args, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, t, tau, h, stride=N + 1, c_stride=N + 3, out_stride=N + 5), want)
    assert np.array_equal(emu_compose(emu, air, args, lde_wide[:W], cl, ch, wch, p, g, log_n, lb, t, tau, h, force_direct=1, grid=1), want)
    bad = c.copy()                                                       # a column that does not close: cq_a is no polynomial
    bad[0, n - kt] = (bad[0, n - kt] + np.uint64(1)) % np.uint64(p)
    cl_bad = ac.lde(oracle, [[int(v) for v in bad[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)
    assert not tight or not degree_below(oracle, emu_compose(emu, air, args, lde_wide[:W], cl_bad, ch, wch, p, g, log_n, lb, t, tau, h), D * n, p, g,
                                         log_n + lb, h)


# ---------------------------------------------------------------------------------------------- the proof, restated
@functools.lru_cache(maxsize=None)
def restated(oracle, name, log_n, lb, t, p, g, seed=SEED, **kw):
    air, cols, args = LISTS[name](log_n, t, p)
    return air, cols, args, za.prove(oracle, air, args, cols, seed, p, g, log_n, lb, t, 1, g, **kw)


def emu_lhs(emu, air, args, W, log_n, lb, t, ch, weights, z, ood, p, g):
    from stark_rs_amd import _lib
    f = flat(air, args, p)
    cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, g, t, 1)
    arr = [np.array([int(v) for v in x], dtype=np.uint64) for x in (ch, weights, z, ood)]
    out = np.zeros(4, dtype=np.uint64)
    assert emu.emu_zkx_ood_lhs(p, g, C.byref(cfg), C.byref(f), C.byref(f.xargs), *[a.ctypes.data for a in arr], out.ctypes.data) == 0
    return [int(v) for v in out]


@pytest.mark.parametrize("name,log_n,lb,t", [("vm", 6, 2, 1), ("selectors", 7, 2, 1)])
def test_the_restated_prover_and_verifier_agree_and_reject(oracle, emu, name, log_n, lb, t):
    p, g = P_REF, G_REF
    air, cols, args, res = restated(oracle, name, log_n, lb, t, p, g)
    W, A, K, Dp = len(cols), len(args), len(air.constraints), res["Dp"]
    proof, roots = res["proof"], res["roots"]
    assert res["closes"] == [True] * A and Dp == za.plan(air, args, log_n, t)[1]
    assert (lib_plan(air, args, W, log_n, lb, t, layout=True)[1], za.layout(W, A, Dp, log_n, lb, t)[1]) == (len(proof), len(proof))
    said = lambda pr, rt=roots: za.verify(oracle, air, args, pr, rt, p, g, W, log_n, lb, t, 1, g)
    assert said(proof) == (True, "")
    off = za.offsets(W, A, Dp, log_n, lb, t)
    assert off["end"] == len(proof)
    # the library's left side of the consistency check, over the library's derived AIR, is the restatement's
    tr, ch = pm.challenges(oracle, roots[0])
    tr, weights = pm.weights(oracle, tr, roots[1], W + K + 3 * A)
    z = [c % p for c in dc.draw(oracle, bytearray(tr) + roots[2], 8 + 4 * (W + K + 3 * A), 4)]
    dair = za.derived_air(air, log_n, t, p, 1, w_of(oracle, log_n, p, g))
    assert emu_lhs(emu, air, args, W, log_n, lb, t, ch, weights, z, res["ood"], p, g) == \
        [int(v) for v in za.ood_lhs(oracle, dair, args, W, ch, weights, z, res["ood"], p, g, log_n, 1, t)]
    for what, at, why in (("a salt byte of tree 2", off["rec 1"] + 9 + 8 * 4 * 4 * A, za.WORDS["auth"]), ("an auxiliary value", off["rec 1"] + 9, za.WORDS["auth"]),
                          ("a_0", off["a0"], za.FRONT["consistency"]), ("b_0", off["b0"] + 8, za.FRONT["consistency"]),
                          ("b_last", off["b0"] + 32 * (A - 1), za.FRONT["consistency"]), ("s_0", off["s0"], za.FRONT["consistency"]),
                          ("a salt byte of tree 1", off["rec 0"] + 9 + 8 * 4 * W, za.WORDS["auth"]),
                          ("a value of R", off["rec 2"] + 9 + 8 * 4 * 4 * Dp, za.WORDS["auth"]), ("the record's count", 1, za.FRONT["record"])):
        m = bytearray(proof)
        m[at] ^= 1
        assert said(bytes(m)) == (False, why), what
    for kw in (dict(omit_cq=True), dict(no_ea=True)):                    # the dishonest provers
        bad = restated(oracle, name, log_n, lb, t, p, g, **kw)[3]
        assert said(bad["proof"], bad["roots"]) == (False, za.FRONT["consistency"]), kw
    other = restated(oracle, name, log_n, lb, t, p, g, seed=bytes(32))[3]
    assert len(other["proof"]) == len(proof) and all(other["roots"][k] != roots[k] for k in range(3)) and said(other["proof"], other["roots"]) == (True, "")


def test_a_lookup_miss_inside_and_outside_the_statement(oracle):
    """a self-check of the restatement (no library code runs): tests/test_gpu_zk_args.py repeats both cases on the library and
    needs the restated prover and verifier to agree on them first"""
    p, g, log_n, lb, t = P_REF, G_REF, 6, 2, 1
    air, cols, args = za.vm(log_n, t, p)
    na = (1 << log_n) - za.k_t(t)
    inside = [list(c) for c in cols]
    inside[4][na - 1] = p - 1                                            # the last active row looks up a value that is in no table row
    res = za.prove(oracle, air, args, inside, SEED, p, g, log_n, lb, t, 1, g)
    assert res["closes"] == [True, False, True]
    assert za.verify(oracle, air, args, res["proof"], res["roots"], p, g, 9, log_n, lb, t, 1, g) == (False, za.FRONT["consistency"])
    outside = [list(c) for c in cols]
    outside[4][na] = p - 2                                               # row n_a: overwritten, outside the statement
    same = za.prove(oracle, air, args, outside, SEED, p, g, log_n, lb, t, 1, g)
    assert same["proof"] == restated(oracle, "vm", log_n, lb, t, p, g)[3]["proof"] and same["closes"] == [True] * 3
