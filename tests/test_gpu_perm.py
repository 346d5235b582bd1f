"""GPU: the permutation argument (include/stark_mi.h, "Permutation argument") -- smi_dev_perm_column,
smi_dev_air_compose_perm, smi_dev_air_prove_perm / smi_air_verify_perm -- against the restatement over the CPU oracle's
primitives (tests/perm_compose.py) and the CPU emulator of the kernels.  Every comparison is exact.  `pytest -m gpu`."""
import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import air_rows as ar
import ext_compose as xc
import perm_compose as pm
import pow_compose as pc
from test_gpu_air import Dev, engines  # noqa: F401  (engines is a fixture)
from test_gpu_ext import _dev_cols
from test_perm_emu import chall, emu, emu_column, shaped  # noqa: F401  (emu is a fixture)

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
LB, TAU = 3, 1


def perm_air(n_cols, left, right):
    from stark_rs_amd.mirror import Air
    return Air(n_cols).permutation(left, right)


def gpu_column(eng, cols, left, right, ch, z_stride=None, lead=0):
    """-> (z (4, n) uint64, closes); lead: words in front of z, so that its base is not 16-byte aligned"""
    cols = np.asarray(cols, dtype=np.uint64)
    W, n = cols.shape
    z_stride = n if z_stride is None else z_stride
    with Dev(eng) as dev:
        d_trace = dev.upload(cols)
        zt, d_z = _dev_cols(np.full((4, n), 0x7ffffffe, dtype=np.uint32), z_stride, lead)
        closes = eng.dev_perm_column(perm_air(W, left, right), d_trace, W, n.bit_length() - 1, ch, d_z, z_stride)
        eng.sync()
        host = zt.cpu().numpy().view(np.uint32)[lead:]
    for e in range(4):   # nothing written between the columns
        assert np.all(host[e * z_stride + n:(e + 1) * z_stride] == 0x7fffffff)
    return np.stack([host[e * z_stride:e * z_stride + n] for e in range(4)]).astype(np.uint64), closes


# ---------------------------------------------------------------------------------------------- the column
@pytest.mark.parametrize("log_n", range(1, 14))
def test_dev_perm_column_equals_the_restatement_and_the_emulator(engines, emu, log_n):
    p, g = xc.PRIMES[log_n % 2]
    n = 1 << log_n
    for kind in ("m2", ["m1", "m8", "overlap"][log_n % 3]):
        cols, left, right = shaped(kind, n, p, log_n)
        ch = chall(log_n)
        want, closes, zero = pm.column(cols, left, right, ch, p, g)
        assert zero is None
        z, got = gpu_column(engines[p], cols, left, right, ch)
        assert np.array_equal(z, want), kind
        assert got == closes, kind
        st, ze, _c, _z = emu_column(emu, cols, left, right, ch, p, g)
        assert st == 0 and np.array_equal(z, ze), kind
    # the 4-byte path: a stride that is no multiple of 4, then a base that is not 16-byte aligned
    z, got = gpu_column(engines[p], cols, left, right, ch, z_stride=n + 1)
    assert np.array_equal(z, want) and got == closes
    z, got = gpu_column(engines[p], cols, left, right, ch, z_stride=n + 4, lead=1)
    assert np.array_equal(z, want) and got == closes


@pytest.mark.parametrize("log_n", [19, 20])
def test_dev_perm_column_large_by_the_recurrence(engines, log_n):
    """2^19 rows is the smallest trace whose workgroup products (512) take perm_scan_kernel round its loop twice; z[0] = 1
    and z[r+1] f_R[r] = z[r] f_L[r] determine z, and a shuffled copy closes"""
    p, g = xc.PRIMES[log_n % 2]
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    src = rng.integers(0, p, (2, n), dtype=np.uint64)
    order = rng.permutation(n)
    cols = np.stack([src[0], src[1], src[0][order], src[1][order]])
    ch = chall(log_n)
    z, closes = gpu_column(engines[p], cols, [0, 1], [2, 3], ch)
    assert closes
    assert pm.recurrence_holds(z, cols, [0, 1], [2, 3], ch, p, g)
    cols[3][n - 7] = (cols[3][n - 7] + np.uint64(1)) % np.uint64(p)
    z, closes = gpu_column(engines[p], cols, [0, 1], [2, 3], ch)
    assert not closes
    assert pm.recurrence_holds(z, cols, [0, 1], [2, 3], ch, p, g)


@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("where", ["first", "last", "inside", "two"])
def test_a_zero_denominator_is_no_inverse_and_the_next_call_succeeds(engines, p, g, where):
    import stark_rs_amd as s
    log_n = 11
    n = 1 << log_n
    cols, left, right = pm.shuffled_copy(n, 2, p, 8)
    rows = {"first": [0], "last": [n - 1], "inside": [6], "two": [n // 2 + 1, 5]}[where]
    for r in rows[1:]:
        for c in right:
            cols[c][r] = cols[c][rows[0]]
    ch = pm.gamma_for_zero(cols, right, chall(4), rows[0], p, g)
    assert pm.column(cols, left, right, ch, p, g) == (None, None, min(rows))
    with pytest.raises(s.StarkMiError) as ei:
        gpu_column(engines[p], cols, left, right, ch)
    assert ei.value.status == -1 and "no inverse" in str(ei.value) and f"row {min(rows)}:" in str(ei.value)
    z, _closes = gpu_column(engines[p], cols, left, right, chall(4))
    assert np.array_equal(z, pm.column(cols, left, right, chall(4), p, g)[0])


def test_column_argument_checks(engines):
    import stark_rs_amd as s
    p, _g = xc.PRIMES[0]
    eng = engines[p]
    with Dev(eng) as dev:
        d = dev.alloc(4 * 4 * 16)
        for left, right, log_n, text in (([], [], 2, "width must be in 1 .. SMI_PERM_MAX_WIDTH (8)"), (list(range(9)), list(range(9)), 2, "width must be in"),
                                         ([0], [4], 2, "right_col must be < n_cols"), ([4], [0], 2, "left_col must be < n_cols"),
                                         ([0], [1], 0, "log_n must be in 1 .. 27")):
            with pytest.raises(s.StarkMiError) as ei:
                eng.dev_perm_column(perm_air(4, left, right), d, 4, log_n, chall(1), d)
            assert ei.value.status == -50 and text in str(ei.value)
        with pytest.raises(s.StarkMiError, match="z_stride < n"):
            eng.dev_perm_column(perm_air(4, [0], [1]), d, 4, 2, chall(1), d, z_stride=3)


# ---------------------------------------------------------------------------------------------- the composition
@pytest.mark.parametrize("p,g", xc.PRIMES)
@pytest.mark.parametrize("name,m", [("empty", 2), ("mixer", 1), ("mimc", 1)])
def test_dev_air_compose_perm_is_compose_ext_plus_the_restated_auxiliary_terms(engines, oracle, p, g, name, m):
    eng, log_n, h = engines[p], 10, g
    n, N = 1 << log_n, 1 << (log_n + LB)
    air, cols = (ap if name == "mimc" else ac).make(name, n, p)
    air, cols = pm.with_permutation(air, cols, m, p)
    W, K = len(cols), len(air.constraints)
    left, right = air.perm
    ch = chall(21)
    z, closes, zero = pm.column(cols, left, right, ch, p, g)
    assert zero is None and closes
    lde = np.array(ac.lde(oracle, cols, p, g, log_n, LB, TAU, h), dtype=np.uint64)
    zl = np.array(ac.lde(oracle, [[int(v) for v in z[e]] for e in range(4)], p, g, log_n, LB, TAU, h), dtype=np.uint64)
    wch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, U64_MAX, 4 * (W + K + 2), dtype=np.uint64)]
    aux = pm.aux_terms(oracle, lde, zl, left, right, ch, wch[4 * (W + K):4 * (W + K) + 4], wch[4 * (W + K) + 4:], p, g, log_n, LB, TAU, h)
    want = None
    # aligned; every stride odd; bases off 16 bytes
    for stride, z_stride, out_stride, lead in ((N, N, N, 0), (N + 1, N + 3, N + 5, 0), (N + 4, N + 4, N + 4, 1)):
        with Dev(eng) as dev:
            lt, d_lde = _dev_cols(lde.astype(np.uint32), stride, lead)
            zt, d_zl = _dev_cols(zl.astype(np.uint32), z_stride, lead)
            ot, d_out = _dev_cols(np.zeros((4, N), dtype=np.uint32), out_stride, lead)
            d_w = dev.upload_u64(wch)
            if want is None:
                eng.dev_air_compose_ext(air, d_lde, W, log_n, LB, d_w, d_out, lde_offset=h)
                eng.sync()
                main = np.stack([ot.cpu().numpy().view(np.uint32)[e * N:(e + 1) * N] for e in range(4)]).astype(np.uint64)
                want = (main + aux) % np.uint64(p)
            eng.dev_air_compose_perm(air, d_lde, d_zl, W, log_n, LB, ch, d_w, d_out, stride=stride, z_stride=z_stride, out_stride=out_stride,
                                     lde_offset=h)
            eng.sync()
            host = ot.cpu().numpy().view(np.uint32)[lead:]
        got = np.stack([host[e * out_stride:e * out_stride + N] for e in range(4)]).astype(np.uint64)
        assert np.array_equal(got, want), (stride, lead)
        for e in range(4):
            assert np.all(host[e * out_stride + N:(e + 1) * out_stride] == 0x7fffffff)


def looping_shape(p):
    """-> (log_n, trip): the smallest trace at blowup 2^LB whose N / 1024 workgroups' worth of points are at least four trips of
    a grid of 8 workgroups per CU -- the cap of the three streaming compose launches -- and the points of one trip"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    log_n = 1
    while (1 << (log_n + LB)) // 1024 < 4 * 8 * cus:
        log_n += 1
    N = 1 << (log_n + LB)
    assert N // 1024 >= 4 * 8 * cus                                      # a one-trip launch is not what the callers test
    assert (p - 1) % N == 0 and log_n <= 27
    return log_n, 8 * cus * 1024


def looping_sample(rng, N, B, trip):
    """-> at least 4096 distinct points of 0 .. N - 1, among them the first and the last point of every trip and the points
    round the row step B and the wrap"""
    edges = [i for k in range(-(-N // trip)) for i in (k * trip, min((k + 1) * trip, N) - 1)]
    assert len(edges) >= 8 and all(k * trip in edges and k * trip - 1 in edges for k in range(1, 4))
    must = edges + [0, B - 1, B, N - B - 1, N - B, N - 1]
    idx = np.unique(np.concatenate([rng.integers(0, N, 4200), np.array(must)]))
    assert len(idx) >= 4096 and set(must) <= set(int(i) for i in idx)
    return idx


def looping_inputs(p, n_cols, n_aux, log_n, seed):
    """-> (air, lde, aux, main, full, wch of 4 (W + K) + 8 n_aux / 4 challenges): the mixer AIR with its last-row boundaries moved
    to row n - 1, over seeded random residues generated on the device.  The compose kernels work point by point: their
    inputs need not be extensions of anything"""
    import torch
    n, N = 1 << log_n, 1 << (log_n + LB)
    air, _ = ac.make("mixer", 64, p)
    air.boundaries = [(c, (n - 1 if r == 63 else r), v) for (c, r, v) in air.boundaries]
    air.n_cols = n_cols
    gen = torch.Generator(device="cuda").manual_seed(seed)
    lde = torch.randint(0, p, (n_cols, N), generator=gen, device="cuda", dtype=torch.int32)
    aux = torch.randint(0, p, (n_aux, N), generator=gen, device="cuda", dtype=torch.int32)
    main, full = torch.empty((4, N), dtype=torch.int32, device="cuda"), torch.empty((4, N), dtype=torch.int32, device="cuda")
    count = 4 * (n_cols + len(air.constraints)) + 2 * n_aux
    wch = [int(x) for x in np.random.default_rng(seed).integers(1 << 62, U64_MAX, count, dtype=np.uint64)]
    torch.cuda.synchronize()
    return air, lde, aux, main, full, wch


def gathered(t, at):
    """the columns `at` (a device index tensor) of a device int32 matrix, as uint64 on the host"""
    return t[:, at].cpu().numpy().view(np.uint32).astype(np.uint64)


def looping_check(eng, p, n_cols, n_aux, seed, state, compose, restated):
    """One streaming compose launch on at least four trips of its grid (looping_shape), over looping_inputs:
    state(air) adds the argument(s) to the AIR; compose(air, d_lde, d_aux, W, log_n, ch, d_w, d_out) is the launch under test;
    restated(idx, lde_at, aux_at, aux_next, ch, wch_aux, wN, log_n) its auxiliary part at the points idx.
    (compose - compose_ext) mod p equals it in all four coordinates at >= 4096 sampled points, the edges of every trip
    among them (looping_sample); a failure names the coordinate, the first wrong point and its trip"""
    import torch
    from test_gpu_ext import _dev_u64
    g = dict(xc.PRIMES)[p]
    B = 1 << LB
    log_n, trip = looping_shape(p)
    N = 1 << (log_n + LB)
    air, lde, aux, main, full, wch = looping_inputs(p, n_cols, n_aux, log_n, seed)
    state(air)
    K, ch = len(air.constraints), chall(seed)
    t_w, d_w = _dev_u64(wch)
    torch.cuda.synchronize()
    eng.dev_air_compose_ext(air, lde.data_ptr(), n_cols, log_n, LB, d_w, main.data_ptr())
    compose(air, lde.data_ptr(), aux.data_ptr(), n_cols, log_n, ch, d_w, full.data_ptr())
    eng.sync()
    idx = looping_sample(np.random.default_rng(seed), N, B, trip)
    ti = torch.from_numpy(idx).cuda()
    got = (gathered(full, ti) + np.uint64(p) - gathered(main, ti)) % np.uint64(p)
    want = restated(idx, gathered(lde, ti), gathered(aux, ti), gathered(aux, (ti + B) % N), ch, wch[4 * (n_cols + K):], pow(g, (p - 1) // N, p), log_n)
    for e in range(4):
        bad = np.flatnonzero(got[e] != want[e])
        assert not len(bad), (e, int(idx[bad[0]]), int(idx[bad[0]]) // trip)


def test_compose_perm_on_every_trip_of_the_grid_equals_the_restatement_at_sampled_points(engines):
    """air_perm_compose_kernel launches at most 8 workgroups per CU and strides over the rest: from 2^23 points on (256 CUs)
    every lane makes four trips, advancing x by omega^(4 x 256 x gridDim.x) per trip.  Width 2, against pm.aux_terms_at"""
    p, g = xc.PRIMES[1]
    eng = engines[p]
    looping_check(eng, p, 4, 4, 20, lambda air: air.permutation([0, 1], [2, 3]),
                  lambda air, d_lde, d_z, W, log_n, ch, d_w, d_out: eng.dev_air_compose_perm(air, d_lde, d_z, W, log_n, LB, ch, d_w, d_out),
                  lambda idx, lde_at, z_at, z_next, ch, w, wN, log_n: pm.aux_terms_at(idx, lde_at, z_at, z_next, [0, 1], [2, 3], ch, w[:4], w[4:8], p, g, wN,
                                                                                      log_n, TAU, g))


# ---------------------------------------------------------------------------------------------- whole proofs
def case(name, n, p, spoil=False):
    """-> (air with its permutation, cols)"""
    if name == "cubic":
        air, cols = pm.cubic(n, p)
    elif name == "mimc":
        air, cols = ap.make("mimc", n, p)
    else:
        air, cols = ac.make(name, n, p)
    return pm.with_permutation(air, cols, 2 if name == "empty" else 1, p, spoil=spoil)


def plan_E(air):
    d, D = max(air.degree, 2), 1
    while D < d - 1:
        D *= 2
    return (1 << LB) // D


def gpu_prove(eng, air, cols, log_n, t, bits, **kw):
    with Dev(eng) as dev:
        return eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n, LB, t, row_leaves=True, ext=True, grind_bits=bits, **kw)


KW = dict(row_leaves=True, ext=True)
SHAPES = [(8, 8, 0), (8, 32, 8), (10, 8, 8), (10, 32, 0)]


@pytest.mark.parametrize("name", ["empty", "cubic", "mimc"])
@pytest.mark.parametrize("shape", range(4))
def test_prove_perm_bytes_equal_the_restatement_and_verify_agrees(engines, oracle, name, shape):
    log_n, t, bits = SHAPES[shape]
    p, g = xc.PRIMES[(shape + len(name)) % 2]
    eng, n, N = engines[p], 1 << log_n, 1 << (log_n + LB)
    air, cols = case(name, n, p)
    W, K = len(cols), len(air.constraints)
    left, right = air.perm
    d, E = eng.air_plan(air, W, log_n, LB)
    assert (d, E) == (max(air.degree, 2), plan_E(air))
    res = gpu_prove(eng, air, cols, log_n, t, bits, timed=True)
    want = pm.prove(oracle, air, left, right, cols, p, g, log_n, LB, t, TAU, g, E, bits)
    assert want["closes"] and res["closes"]
    assert res["column_roots"].tobytes() == want["roots"]
    assert res["top_indices"] == want["top"]
    assert res["proof"] == want["proof"]
    R = eng.fri_num_rounds(eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t))
    assert len(res["proof"]) == pm.proof_len(N, E, t, R, W)          # the formula in the header
    at = pc.nonce_offset(N, R)
    assert int.from_bytes(res["proof"][at + 9:at + 17], "little") == want["nonce"]
    assert list(res["stage_ms"]) == ["lde", "commit", "perm", "compose", "fri", "open"]
    assert pm.verify(oracle, air, left, right, want["roots"], want["proof"], p, g, log_n, LB, t, TAU, g, E, bits) == (True, "")
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert ok, why


def _offsets(W, log_N, t, plen):
    """byte offsets inside a proof: (section 1, its paths, section 2, its paths)"""
    s1 = plen - pm.opening_len(W, log_N, t)
    p1 = s1 + 4 * t * (9 + 8 * W)
    s2 = p1 + 4 * t * (9 + 32 * log_N)
    p2 = s2 + 4 * t * (9 + 32)
    return s1, p1, s2, p2


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_verify_perm_rejections_agree_with_the_restatement(engines, oracle, p, g):
    eng, log_n, t, bits = engines[p], 8, 8, 8
    n, N, log_N = 1 << log_n, 1 << (log_n + LB), log_n + LB
    air, cols = case("cubic", n, p)
    W, K = len(cols), len(air.constraints)
    left, right = air.perm
    _d, E = eng.air_plan(air, W, log_n, LB)
    res = gpu_prove(eng, air, cols, log_n, t, bits)
    proof, roots = res["proof"], res["column_roots"].tobytes()
    assert proof == pm.prove(oracle, air, left, right, cols, p, g, log_n, LB, t, TAU, g, E, bits)["proof"]

    def both(name, air_v, bad_proof, bad_roots, want_class=None):
        """the restated verdict first, then the library's: the same verdict and the same class of reason"""
        lv, rv = air_v.perm
        ok_r, cls = pm.verify(oracle, air_v, lv, rv, bad_roots, bad_proof, p, g, log_n, LB, t, TAU, g, E, bits)
        assert not ok_r, name                                            # a case the restatement accepts would be replaced
        if want_class:
            assert cls == want_class, (name, cls)
        ok, why = eng.air_verify(air_v, bad_proof, [bad_roots[:32], bad_roots[32:]], W, log_n, LB, t, grind_bits=bits, **KW)
        assert not ok and why, name
        assert pm.reason_class(why) == cls, (name, why, cls)

    s1, p1, s2, p2 = _offsets(W, log_N, t, len(proof))
    rec1, prec = 9 + 8 * W, 9 + 32 * log_N
    flips = [("row tag 1", s1 + 2 * rec1, "record"), ("row width 1", s1 + rec1 + 1, "record"), ("row value 1", s1 + 3 * rec1 + 9 + 8, "path"),
             ("path tag 1", p1 + prec, "record"), ("path depth 1", p1 + 2 * prec + 1, "record"), ("path digest 1", p1 + 5 * prec + 9 + 40, "path"),
             ("row tag 2", s2 + 41, "record"), ("row width 2", s2 + 2 * 41 + 1, "record"), ("z value", s2 + 6 * 41 + 9 + 16, "path"),
             ("path tag 2", p2 + 3 * prec, "record"), ("path depth 2", p2 + 1, "record"), ("path digest 2", p2 + 7 * prec + 9 + 3, "path")]
    for name, at, cls in flips:
        bad = bytearray(proof)
        bad[at] ^= 1
        both(name, air, bytes(bad), roots, cls)
    # a z coordinate plus p in the bytes: the leaf no longer hashes to the committed one
    bad = bytearray(proof)
    v = int.from_bytes(bad[s2 + 9 + 24:s2 + 9 + 32], "little")
    bad[s2 + 9 + 24:s2 + 9 + 32] = xc._u64(v + p)
    both("z + p in the bytes", air, bytes(bad), roots, "path")
    # ... and committed that way: every path verifies and the canonical check is what rejects
    tam = pm.prove(oracle, air, left, right, cols, p, g, log_n, LB, t, TAU, g, E, bits, z_plus_p=3)
    both("non-canonical z coordinate", air, tam["proof"], tam["roots"], "canonical")
    tam = pm.prove(oracle, air, left, right, cols, p, g, log_n, LB, t, TAU, g, E, bits, trace_plus_p=1)
    both("non-canonical trace value", air, tam["proof"], tam["roots"], "canonical")
    both("one byte short", air, proof[:-1], roots, "length")
    both("section 2 missing", air, proof[:s2], roots, "length")
    both("one byte more", air, proof + b"\x00", roots, "length")
    both("cut inside FRI", air, proof[:s1 // 2], roots, "fri")
    wrong = bytearray(roots)
    wrong[40] ^= 1
    both("wrong root_2", air, proof, bytes(wrong), "fri")
    wrong = bytearray(roots)
    wrong[3] ^= 1
    both("wrong root_1", air, proof, bytes(wrong), "fri")
    other, _ = case("cubic", n, p)
    other.perm = ([1], [W - 1])
    both("a swapped column", other, proof, roots, "composition")
    other, _ = case("cubic", n, p)
    other.perm = ([0, 1], [W - 1, 1])
    both("a different width", other, proof, roots, "composition")
    # the proof of smi_dev_air_prove_ext_pow offered here, and this proof offered to smi_air_verify_ext_pow
    plain, _ = case("cubic", n, p)
    plain.perm = None
    root, xproof, _top, _nonce = pc.air_proof(oracle, plain, cols, p, g, log_n, LB, t, TAU, g, E, bits)
    both("the ext-pow proof", air, xproof, root + root, "fri")
    prior, _ch = xc.air_transcript(oracle, W, K, roots[:32])
    _, wN = ac.roots_of_unity(oracle, p, g, log_n, LB)
    assert not pc.verify(oracle, oracle.fri_cfg(wN, g, N, E, t, p), proof, g, prior, bits)[0]
    ok, why = eng.air_verify(plain, proof, [roots[:32]], W, log_n, LB, t, grind_bits=bits, **KW)
    assert not ok and why


@pytest.mark.parametrize("kind", ["cell", "multiplicity", "columnwise"])
def test_a_trace_that_does_not_close_is_proved_and_rejected(engines, oracle, kind):
    import stark_rs_amd as s
    p, g = xc.PRIMES[len(kind) % 2]
    eng, log_n, t, bits = engines[p], 8, 8, 0
    cols, left, right = pm.non_closing(kind, 1 << log_n, p)
    W = len(cols)
    air = perm_air(W, left, right)
    _d, E = eng.air_plan(air, W, log_n, LB)
    with pytest.raises(s.StarkMiError, match="does not close"):
        gpu_prove(eng, air, cols, log_n, t, bits)
    res = gpu_prove(eng, air, cols, log_n, t, bits, check=False)
    want = pm.prove(oracle, air, left, right, cols, p, g, log_n, LB, t, TAU, g, E, bits, honest=False)
    assert not want["closes"] and not res["closes"]
    assert res["proof"] == want["proof"] and res["column_roots"].tobytes() == want["roots"]
    ok_r, cls = pm.verify(oracle, air, left, right, want["roots"], want["proof"], p, g, log_n, LB, t, TAU, g, E, bits)
    assert not ok_r
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert not ok and pm.reason_class(why) == cls, (why, cls)


def test_mode_checks(engines):
    p, _g = xc.PRIMES[0]
    eng = engines[p]
    cols, left, right = pm.shuffled_copy(16, 1, p)
    air = perm_air(len(cols), left, right)
    with Dev(eng) as dev:
        d = dev.upload(np.array(cols, dtype=np.uint64))
        for kw in (dict(), dict(row_leaves=True), dict(ext=True)):
            with pytest.raises(ValueError, match="row_leaves=True, ext=True"):
                eng.dev_air_prove(air, d, len(cols), 4, LB, 2, **kw)
            with pytest.raises(ValueError, match="row_leaves=True, ext=True"):
                eng.air_verify(air, b"", [bytes(32), bytes(32)], len(cols), 4, LB, 2, **kw)
        from stark_rs_amd.mirror import Air
        with pytest.raises(ValueError, match="no permutation"):
            eng.dev_perm_column(Air(3), d, 3, 4, chall(1), d)


def test_prove_perm_headline_shape_is_accepted(engines):
    """2^22 x 4, B = 8, t = 32, m = 2 on the second prime at 16 bits: accepted, and the proof has the predicted length"""
    import torch
    p, g = xc.PRIMES[1]
    eng, log_n, t, W, bits = engines[p], 22, 32, 4, 16
    n, N = 1 << log_n, 1 << (log_n + LB)
    rng = np.random.default_rng(1)
    src = rng.integers(0, p, (2, n), dtype=np.int64)
    order = rng.permutation(n)
    cols = np.stack([src[0], src[1], src[0][order], src[1][order]])
    air = perm_air(W, [0, 1], [2, 3])
    air.boundary(0, 0, int(cols[0][0])).boundary(3, n - 1, int(cols[3][n - 1]))
    _d, E = eng.air_plan(air, W, log_n, LB)
    trace = torch.from_numpy(cols.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    res = eng.dev_air_prove(air, trace.data_ptr(), W, log_n, LB, t, timed=True, grind_bits=bits, **KW)
    assert res["closes"]
    R = eng.fri_num_rounds(eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t))
    assert len(res["proof"]) == pm.proof_len(N, E, t, R, W)
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)
    assert ok, why
    bad = bytearray(res["proof"])
    bad[-5] ^= 1
    assert not eng.air_verify(air, bytes(bad), res["column_roots"], W, log_n, LB, t, grind_bits=bits, **KW)[0]
    print("stage_ms", res["stage_ms"])
