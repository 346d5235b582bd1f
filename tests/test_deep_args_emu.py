"""CPU: out-of-domain sampling with an argument list (include/stark_mi.h, "Out-of-domain sampling with an argument list") --
the lane body of deep_compose_args_kernel (csrc/deep_core.h) run by the emulator library with the kernel's block split, the
table builder, the extended consistency check and Q at a point from three rows, against the Python restatement
(tests/deep_args_compose.py).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import air_compose as ac
import deep_args_compose as da
import deep_compose as dc
import ext_compose as xc
import xargs_compose as xa
from test_deep_emu import emu_compose
from test_gpu_boundary_primes import GEN, THREE, U64, u64_set

SHAPES = [(1, 1, 1), (3, 2, 2), (9, 8, 4), (64, 8, 16)]
ADICITY = {998244353: 23, 469762049: 26, 1073692673: 14, 536813569: 13, 536903681: 15}


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd
    from stark_rs_amd import _lib
    stark_rs_amd.build()
    L = C.CDLL(_lib.EMU_PATH)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.emu_deep_compose.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), u32, vp, u64, vp, u64, vp, vp, vp, vp, u64, u32]
    L.emu_deep_compose_args.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), u32, u32, vp, u64, vp, u64, vp, u64, vp, vp, vp, vp, u64, u32]
    L.emu_deep_compose_args_table.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), u32, u32, vp, vp, vp, vp, u64]
    L.emu_deep_args_q_at.argtypes = [u64, u64, u32, u32, u32, u64, u64, vp, vp, vp, vp, vp, vp, vp]
    L.emu_deep_xargs_ood_sides.argtypes = [u64, u64, C.POINTER(_lib.StarkCfg), C.POINTER(_lib.Air), C.POINTER(_lib.AirXArgs), vp, vp, vp, vp, vp, vp]
    return L


def _u64(v):
    return np.array([int(x) for x in v], dtype=np.uint64)


def emu_compose_args(emu, lde, cl, seg, log_n, lb, z, ood, ch, p, g, h, grid=0, odd=False):
    """odd: strides N + 1, N + 3, N + 5, N + 7 from bases one word into their buffers -- the 4-byte path of the kernel"""
    from stark_rs_amd import _lib
    arrs = [np.asarray(a, dtype=np.uint32) for a in (lde, cl, seg)]
    N = arrs[0].shape[1]
    strides = [N + 1, N + 3, N + 5, N + 7] if odd else [N] * 4
    lead = 1 if odd else 0

    def spread(a, stride):
        host = np.full(lead + a.shape[0] * stride, 0x7fffffff, dtype=np.uint32)
        for c in range(a.shape[0]):
            host[lead + c * stride:lead + c * stride + N] = a[c]
        return host
    hosts = [spread(a, s) for a, s in zip(arrs, strides)]
    out = np.full(lead + 4 * strides[3], 0xdeadbeef, dtype=np.uint32)
    cfg = _lib.StarkCfg(log_n, lb, arrs[0].shape[0], 1, 1, h, 0, 1)
    za, oa, ca = _u64(z), _u64(ood), _u64(ch)
    st = emu.emu_deep_compose_args(p, g, C.byref(cfg), arrs[1].shape[0] // 4, arrs[2].shape[0] // 4, hosts[0].ctypes.data + 4 * lead, strides[0],
                                   hosts[1].ctypes.data + 4 * lead, strides[1], hosts[2].ctypes.data + 4 * lead, strides[2], za.ctypes.data,
                                   oa.ctypes.data, ca.ctypes.data, out.ctypes.data + 4 * lead, strides[3], grid)
    assert st == 0, st
    assert np.all(out[:lead] == 0xdeadbeef)
    for e in range(4):
        assert np.all(out[lead + e * strides[3] + N:lead + (e + 1) * strides[3]] == 0xdeadbeef)
    return np.stack([out[lead + e * strides[3]:lead + e * strides[3] + N] for e in range(4)]).astype(np.uint64)


def check_lane_body(emu, oracle, p, g, log_N, shapes, challenge_sets=("random",), grids=(0,)):
    N = 1 << log_N
    for k, (W, A, D) in enumerate(shapes):
        lb = 2 if log_N < 5 else 2 + k % 3
        log_n = log_N - lb
        w, _wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
        x = dc.points(oracle, p, g, log_n, lb, g)
        for cs in challenge_sets:
            kind = "random" if cs == "random" else "extreme"
            u = {"u64": u64_set(p), "max": [U64], "pm1": [p - 1]}.get(cs)
            lde, cl, seg, z, ood, ch = da.compose_inputs(p, W, A, D, N, kind, seed=k + log_N, u=u)
            want = da.q_codeword(lde, cl, seg, x, z, ood, ch, w, p, g)
            for grid in grids:
                for odd in (False, True):
                    got = emu_compose_args(emu, lde, cl, seg, log_n, lb, z, ood, ch, p, g, g, grid=grid, odd=odd)
                    assert np.array_equal(got, want), (log_N, W, A, D, cs, grid, odd)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("log_N", [3, 4, 10, 11, 13])
def test_the_lane_body_equals_the_restatement(emu, oracle, p, g, log_N):
    """random and all-(p - 1) cells, both access layouts; at 2^13 also a grid of one workgroup, so that every lane loops"""
    check_lane_body(emu, oracle, p, g, log_N, SHAPES, ("random", "u64"), grids=(0, 1) if log_N == 13 else (0,))


@pytest.mark.parametrize("p", THREE)
@pytest.mark.parametrize("log_N", [4, 11])
def test_the_lane_body_at_boundary_moduli(emu, oracle, p, log_N):
    check_lane_body(emu, oracle, p, GEN[p], log_N, SHAPES, ("random", "u64", "max", "pm1"), grids=(0, 1))


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_with_every_delta_zero_the_kernel_is_deep_compose(emu, oracle, p, g):
    for log_N, (W, A, D) in ((4, (1, 1, 1)), (10, (3, 2, 2)), (11, (9, 8, 4))):
        lb, N = 2, 1 << log_N
        lde, cl, seg, z, ood, ch = da.compose_inputs(p, W, A, D, N, "random", seed=log_N)
        for i in range(4 * 2 * W, 4 * (2 * W + 2 * A)):
            ch[i] = 0 if i % 2 else p                                       # zero mod p, both ways
        plain = lambda v: v[:8 * W] + v[4 * (2 * W + 2 * A):]
        got = emu_compose_args(emu, lde, cl, seg, log_N - lb, lb, z, ood, ch, p, g, g)
        assert np.array_equal(got, emu_compose(emu, lde, seg, log_N - lb, lb, z, plain(ood), plain(ch), p, g, g)), (W, A, D)


@pytest.mark.parametrize("p,g", list(xc.PRIMES) + [(q, GEN[q]) for q in THREE])
def test_the_table_and_the_point_function(emu, oracle, p, g):
    from stark_rs_amd import _lib
    R = (1 << 32) % p
    for k, (W, A, D) in enumerate(SHAPES):
        log_n, lb = 4, 2
        N = 1 << (log_n + lb)
        w, _wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
        x = dc.points(oracle, p, g, log_n, lb, g)
        for kind in ("random", "extreme"):
            lde, cl, seg, z, ood, ch = da.compose_inputs(p, W, A, D, N, kind, seed=k, u=u64_set(p))
            words = 8 * W + 16 * A + 8 * D + 16
            tab = np.zeros(words, dtype=np.uint32)
            cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, g, 0, 1)
            za, oa, ca = _u64(z), _u64(ood), _u64(ch)
            assert emu.emu_deep_compose_args_table(p, g, C.byref(cfg), A, D, za.ctypes.data, oa.ctypes.data, ca.ctypes.data, tab.ctypes.data, words) == 0
            assert emu.emu_deep_compose_args_table(p, g, C.byref(cfg), A, D, za.ctypes.data, oa.ctypes.data, ca.ctypes.data, tab.ctypes.data, words - 1) == -50
            el = lambda v, i: [int(c) % p for c in v[4 * i:4 * i + 4]]
            mont = lambda v: [c * R % p for c in v]
            prep = lambda v: mont(v) + mont([c * g % p for c in v])
            want, c1, c2 = [], [0] * 4, [0] * 4
            for c in range(2 * W):
                want += mont(el(ch, c))
            for a in range(A):
                want += prep(el(ch, 2 * W + a)) + prep(el(ch, 2 * W + A + a))
            for j in range(D):
                want += prep(el(ch, 2 * W + 2 * A + j))
            for i in list(range(W)) + list(range(2 * W, 2 * W + A)) + list(range(2 * W + 2 * A, 2 * W + 2 * A + D)):
                c1 = xc.add(c1, xc.mul(el(ch, i), el(ood, i), p, g), p)
            for i in list(range(W, 2 * W)) + list(range(2 * W + A, 2 * W + 2 * A)):
                c2 = xc.add(c2, xc.mul(el(ch, i), el(ood, i), p, g), p)
            want += [(p - c) % p for c in c1] + [(p - c) % p for c in c2] + mont(z) + mont(dc.scale_q(z, w, p))
            assert [int(v) for v in tab] == want, (W, A, D, kind)
            Q = da.q_codeword(lde, cl, seg, x, z, ood, ch, w, p, g)
            for i in (0, 5, N - 1):
                got = np.zeros(4, dtype=np.uint64)
                tr, cr, sr = _u64(lde[:, i]), _u64(cl[:, i]), _u64(seg[:, i])
                assert emu.emu_deep_args_q_at(p, g, W, A, D, w, int(x[i]), za.ctypes.data, oa.ctypes.data, ca.ctypes.data, tr.ctypes.data, cr.ctypes.data,
                                              sr.ctypes.data, got.ctypes.data) == 0
                assert [int(v) for v in got] == [int(v) for v in Q[:, i]] == da.q_at(lde[:, i], cl[:, i], seg[:, i], int(x[i]), z, ood, ch, w, p, g)


def lib_sides(emu, air, args, W, log_n, lb, ch, wch, z, ood, p, g):
    from stark_rs_amd import _lib
    flat = xa.mirror_air(air, args).flatten(p)
    assert flat.xargs is not None
    cfg = _lib.StarkCfg(log_n, lb, W, 1, 1, g, 0, 1)
    lhs, rhs = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    ca, wa, za, oa = _u64(ch), _u64(wch), _u64(z), _u64(ood)
    st = emu.emu_deep_xargs_ood_sides(p, g, C.byref(cfg), C.byref(flat), C.byref(flat.xargs), ca.ctypes.data, wa.ctypes.data, za.ctypes.data, oa.ctypes.data,
                                      lhs.ctypes.data, rhs.ctypes.data)
    assert st == 0, st
    return [int(v) for v in lhs], [int(v) for v in rhs]


def fresh(air):
    """a copy of a mirror.Air without its argument list, flattened to smi_air_xargs whatever the list holds"""
    import copy
    out = copy.deepcopy(air)
    out.args = []
    out.xargs_always = True
    return out


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_the_consistency_check_is_the_restatement_s_and_holds_for_an_honest_record(emu, oracle, p, g):
    """each argument kind with and without selectors, a periodic table member, K = 0; and a transition that reads a periodic
    column (the scene of tests/xargs_compose.py has three periodic columns and eight arguments)"""
    log_n, lb, t = 4, 2, 2
    cases = dict(da.small_lists(1 << log_n, p))
    air, cols, args = xa.scene(1 << log_n, p, (4, 8, 2), A=8)
    cases["scene"] = (air, cols, args)
    for name, (air, cols, args) in cases.items():
        W, K, A = len(cols), len(air.constraints), len(args)
        _d, D = da.plan(air, args)
        res = da.prove(oracle, air, args, cols, p, g, log_n, lb, t, 1, g)
        assert all(res["closes"]), name
        bad = list(res["ood"])
        bad[4 * (2 * W) + 1] = (bad[4 * (2 * W) + 1] + 1) % p               # a_0
        for ood, same in ((res["ood"], True), (bad, False)):
            want = da.ood_sides(oracle, air, args, W, D, res["ch"], res["wch"], res["z"], ood, p, g, log_n, 1)
            assert lib_sides(emu, fresh(air), args, W, log_n, lb, res["ch"], res["wch"], res["z"], ood, p, g) == want, name
            assert (want[0] == want[1]) == same, name


def with_transition(n, p):
    """x' = x + k with k periodic, next to a lookup of x's low cells: a periodic column inside a transition constraint"""
    from stark_rs_amd.mirror import Air
    ks = [3, 5, 7, 11]
    x = [1]
    for r in range(n - 1):
        x.append((x[-1] + ks[r % 4]) % p)
    air = Air(3)
    k = air.periodic(ks)
    air.transition({("next", 0): 1, ("cur", 0): -1, (("per", k),): -1})
    air.boundary(0, 0, 1)
    cols = [x, list(x), [1] * n]                                              # every x looked up in a copy of the column, once each
    return air, cols, [("lookup", [0], [1], 2)]


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_the_restated_prover_and_verifier_agree_and_every_defect_has_its_reason(emu, oracle, p, g):
    t = 4
    # n = 2^3 at B = 4 and t = 4 has no FRI fold (one round): there is no layer-0 triple, and the verifier says so, as
    # smi_air_verify_deep does at such a shape
    air, cols, args = da.small_lists(8, p)["lookup"]
    res = da.prove(oracle, air, args, cols, p, g, 3, 2, t, 1, g)
    assert da.verify(oracle, air, args, res["proof"], res["roots"], p, g, 3, 3, 2, t, 1, g) == (False, "no layer")
    for log_n, lb, name in ((3, 3, "lookup"), (6, 2, "lookup_per"), (6, 3, "perm_sel"), (6, 2, "transition")):
        air, cols, args = with_transition(1 << log_n, p) if name == "transition" else da.small_lists(1 << log_n, p)[name]
        W, A, K, n, N = len(cols), len(args), len(air.constraints), 1 << log_n, 1 << (log_n + lb)
        _d, D = da.plan(air, args)
        res = da.prove(oracle, air, args, cols, p, g, log_n, lb, t, 1, g)
        proof, roots = res["proof"], res["roots"]
        assert len(proof) == da.proof_len(oracle, W, A, D, log_n, lb, t, p, g, g), name
        V = lambda pr, rt=roots, ar_=args: da.verify(oracle, air, ar_, pr, rt, p, g, W, log_n, lb, t, 1, g)
        assert V(proof) == (True, ""), name
        # the emulated kernel on the restatement's columns, and deg Q < n
        assert np.array_equal(emu_compose_args(emu, np.array(res["lde"]), np.array(res["cl"]), res["seg"], log_n, lb, res["z"], res["ood"], res["gammas"],
                                               p, g, g), res["Q"]), name
        _w, wN = ac.roots_of_unity(oracle, p, g, log_n, lb)
        assert not any(np.asarray(oracle.fast_intt(res["Q"][e], wN, g, p))[n:].any() for e in range(4)), name
        lhs, rhs = lib_sides(emu, fresh(air), args, W, log_n, lb, res["ch"], res["wch"], res["z"], res["ood"], p, g)
        assert lhs == rhs, name
        flip = lambda at: bytes(proof[:at]) + bytes([proof[at] ^ 1]) + bytes(proof[at + 1:])
        assert V(flip(1)) == (False, "record"), name
        assert V(proof[:9] + xc._u64(int.from_bytes(proof[9:17], "little") + p) + proof[17:]) == (False, "record canonical"), name
        for i in (2 * W, 2 * W + A, 2 * W + 2 * A):                           # a_0, b_0, s_0
            assert V(flip(9 + 32 * i + 8)) == (False, "consistency"), (name, i)
        m, path = 2 * t, 9 + 32 * (log_n + lb)
        lens = [m * (9 + 8 * wd) + m * path for wd in (W, 4 * A, 4 * D)]
        start = len(proof) - sum(lens)
        for v, wd in enumerate((W, 4 * A, 4 * D)):
            assert V(flip(start + 9)) == (False, "auth"), (name, v)          # a value
            assert V(flip(start + 1)) == (False, "row"), (name, v)           # a width
            assert V(flip(start + m * (9 + 8 * wd) + 9)) == (False, "auth"), (name, v)   # a path's digest
            assert V(flip(start + m * (9 + 8 * wd) + 1)) == (False, "path"), (name, v)
            start += lens[v]
        assert V(proof[:-1]) == (False, "length"), name
        assert V(proof, [roots[0], roots[2], roots[1]])[0] is False, name
    # the list in another order, a selector removed
    air, cols, args = xa.scene(16, p, (4, 8, 2), A=3)
    res = da.prove(oracle, air, args, cols, p, g, 4, 2, t, 1, g)
    V = lambda ar_: da.verify(oracle, air, ar_, res["proof"], res["roots"], p, g, len(cols), 4, 2, t, 1, g)
    assert V(args) == (True, "")
    assert V([args[2], args[1], args[0]]) == (False, "consistency")
    assert V([args[0][:4], args[1], args[2]]) == (False, "consistency")
    # a trace whose lookup does not close still yields a proof, which is rejected
    air, cols, args = da.small_lists(64, p)["lookup"]
    cols = [list(c) for c in cols]
    cols[2][cols[2].index(max(cols[2]))] -= 1
    res = da.prove(oracle, air, args, cols, p, g, 6, 2, t, 1, g, honest=False)
    assert res["closes"] == [False]
    assert da.verify(oracle, air, args, res["proof"], res["roots"], p, g, 3, 6, 2, t, 1, g) == (False, "consistency")
    # proofs of the neighbouring variants under this verifier
    other = dc.prove(oracle, air, cols, p, g, 6, 2, t, 1, g)
    assert da.verify(oracle, air, args, other["proof"], other["roots"] + [other["roots"][0]], p, g, 3, 6, 2, t, 1, g) == (False, "record")
    air, cols, args = da.small_lists(64, p)["lookup"]
    other = xa.prove(oracle, air, args, cols, p, g, 6, 3, t, 1, g, 4, 0)
    assert da.verify(oracle, air, args, other["proof"], [other["roots"][:32], other["roots"][32:], other["roots"][:32]], p, g, 3, 6, 3, t, 1, g) == (False, "record")
