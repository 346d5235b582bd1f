"""Extension FRI at folding factor 4 at the moduli of tests/test_gpu_boundary_primes.py, where the range bound of its one-
reduction product is tight: fold4_element_ext (csrc/fri_core.h) chains three fold_pair_ext, each an ext_mul_prepared whose
mont_reduce64 takes a sum of four products next to 4 (p - 1)^2 against p 2^32, and fold4_ext_alpha forms alpha^2 by the same
product.  The second fold's inputs are outputs of the first: canonical only if every fp_add before them was.  Operands on the
bounds: every coordinate p - 1, the edge values, the unreduced u64 alphas a transcript can hand over, and two back-solved
inputs (at_the_bound4) that put each of the three products of a lane exactly on 4 (p - 1)^2.
References: tests/fold4_compose.py, which takes (p, g) -- the Lagrange fold, and two folds by 2 of tests/ext_compose.py where
the length is past the Lagrange loop; never the device's factor-2 kernel.  Every comparison is exact.  Without a GPU the lane
body runs in the CPU emulator; `pytest -m gpu` for the kernel, the provers and the verifiers.
No GPU case is left out for a prime's two-adicity: the longest fold is 2^12 points and the proofs are at most 2^11 points,
within the two-adicity of every prime they run at (12289: 12; the three range-bound primes: 13 and more) -- 0 cases."""
import numpy as np
import pytest

import ext_compose as xc
import fold4_compose as f4
from test_fold4_emu import batchings, emu, emu_fold4  # noqa: F401  (emu is a fixture)
from test_gpu_boundary_primes import ADICITY, ALL, GEN, KINDS, LARGE, THREE, U64, _alpha_vectors, _fold_ints, at_the_bound, engines, operands, u64_set  # noqa: F401  (engines is a fixture)
from test_gpu_boundary_primes_args import challenge_sets  # noqa: F401

R = 1 << 32                                     # the Montgomery radix of the kernels
ONE = [1, 0, 0, 0]
SMALLEST = 12289
FAMILIES = ["alpha", "alpha2"]
# the offsets (j0, j1, j2, j3) of the first T = (p - 1 - j0, ..) with a square root of T 2^-32 in F_q; re-derived below
T_OFFSETS = {p: (0, 0, 0, 0) for p in LARGE}
T_OFFSETS[536903681] = (0, 0, 1, 0)


def same(got, want):
    """the comparison of every GPU test of this module: shape and every word"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.array_equal(got, want))


# ---------------------------------------------------------------------------------------------- the bound inputs
def fq_is_square(a, p, g):
    """Euler's criterion in F_q^*, of order p^4 - 1"""
    return xc.power(a, (p ** 4 - 1) // 2, p, g) == ONE


def fq_sqrt(a, p, g):
    """Tonelli-Shanks over xc.mul / xc.power -> a root of the square a"""
    order = p ** 4 - 1
    s = (order & -order).bit_length() - 1
    m = order >> s
    z = next(c for c in ([k, 1, 0, 0] for k in range(p)) if not fq_is_square(c, p, g))
    c, x, t, M = xc.power(z, m, p, g), xc.power(a, (m + 1) // 2, p, g), xc.power(a, m, p, g), s
    while t != ONE:
        i, t2 = 0, t
        while t2 != ONE:
            t2, i = xc.mul(t2, t2, p, g), i + 1
        b = xc.power(c, 1 << (M - i - 1), p, g)
        x, c = xc.mul(x, b, p, g), xc.mul(b, b, p, g)
        t, M = xc.mul(t, c, p, g), i
    return x


def offsets_in_order():
    """(j0, j1, j2, j3) by j0 + j1 + j2 + j3, then lexicographically"""
    s = 0
    while True:
        for j0 in range(s + 1):
            for j1 in range(s - j0 + 1):
                for j2 in range(s - j0 - j1 + 1):
                    yield (j0, j1, j2, s - j0 - j1 - j2)
        s += 1


_alpha2 = {}


def alpha2_root(p, g):
    """-> (offsets j, T, alpha): T = (p - 1 - j0, ..) the first vector for which T 2^-32 is a square of F_q, alpha a root of
    it, so that the Montgomery form of alpha^2 is T"""
    if p not in _alpha2:
        rinv = pow(R, -1, p)
        for j in offsets_in_order():
            T = [p - 1 - v for v in j]
            a = xc.scale(T, rinv, p)
            if fq_is_square(a, p, g):
                _alpha2[p] = (j, T, fq_sqrt(a, p, g))
                break
    return _alpha2[p]


def unreduced(a, p):
    """four residues handed over as a transcript may: as it is, + p, the largest k p + a below 2^64, + p 2^31"""
    return [a[0], a[1] + p, a[2] + (U64 - a[2]) // p * p, a[3] + (p << 31)]


def at_the_bound4(o, L, p, omega, offset, family):
    """-> (codeword (4, L), alpha) that put the three products of fold4_element_ext on and just under the largest sum
    ext_mul_prepared can hand its one reduction.  Back-solved per output element i < q = L / 4, with t0 = 1 / (2 x_i),
    t1 = t0 / iota, t2 = 1 / (2 x_i^2): the fold factors d0, d1 (which fold_pair_ext multiplies by alpha) and d2 (by alpha^2)
    are chosen, every coordinate within 2^12 of p - 1 and exactly p - 1 at element 0; c0 is random, c2 = c0 - d0 / t0,
    y0 = (c0 + c2) / 2 + alpha d0, y1 = y0 - d2 / t2, (c1 + c3) / 2 = y1 - alpha d1, (c1 - c3) / 2 = d1 / (2 t1).
    family "alpha":  at_the_bound's alpha, Montgomery coordinates p - 1 - j: the first two products are next to 4 (p - 1)^2
                     at element 0, and fold4_ext_alpha's own product alpha_m * alpha_m has every factor within 3 of p - 1;
    family "alpha2": alpha a root of T 2^-32 (alpha2_root), so that alpha^2 has the Montgomery form T and the THIRD
                     product sits on the bound."""
    g, q, P = GEN[p], L // 4, np.uint64(p)
    if family == "alpha":
        a = [(p - 1 - j) * pow(R, -1, p) % p for j in range(4)]
    else:
        a = alpha2_root(p, g)[2]
    x = xc._powers(omega, q, p) * np.uint64(offset % p) % P
    iota = pow(omega, q, p)
    d0, d1, d2 = (np.stack([P - np.uint64(1) - o.splitmix64(80 + 4 * k + e, q) % np.uint64(4096) for e in range(4)]) for k in range(3))
    for d in (d0, d1, d2):
        d[:, 0] = p - 1
    inv2 = np.uint64(pow(2, -1, p))
    c0 = np.stack([o.splitmix64(70 + e, q) % P for e in range(4)])
    c2 = (c0 + P - x * np.uint64(2) % P * d0 % P) % P
    y0 = ((c0 + c2) % P * inv2 % P + xc.mul_arr(d0, a, p, g)) % P
    y1 = (y0 + P - x * x % P * np.uint64(2) % P * d2 % P) % P
    s1 = (y1 + P - xc.mul_arr(d1, a, p, g)) % P
    h1 = x * np.uint64(iota) % P * d1 % P
    c1, c3 = (s1 + h1) % P, (s1 + P - h1) % P
    return np.concatenate([c0, c1, c2, c3], axis=1), unreduced(a, p)


def fold4_ints(cw, alpha, offset, omega, p, g):
    """the fold by 4 on Python ints: _fold_ints under alpha, then under alpha^2 on the squared domain"""
    mid = _fold_ints(cw, alpha, offset, omega, p, g)
    return _fold_ints(mid, f4.alpha_squared(alpha, p, g), offset * offset % p, omega * omega % p, p, g)


def fold_factors(cw, alpha, offset, omega, p, g):
    """-> [(d0, d1, d2) of output element i] on Python ints: what the three fold_pair_ext calls multiply by alpha, alpha, alpha^2"""
    L = cw.shape[1]
    q = L // 4
    iota, inv2, al = pow(omega, q, p), pow(2, -1, p), [v % p for v in alpha]
    out = []
    for i in range(q):
        x = offset * pow(omega, i, p) % p
        c = [[int(v) for v in cw[:, i + j * q]] for j in range(4)]
        t0 = inv2 * pow(x, -1, p) % p
        t1, t2 = t0 * pow(iota, -1, p) % p, inv2 * pow(x * x, -1, p) % p
        d0, d1 = xc.scale(xc.sub(c[0], c[2], p), t0, p), xc.scale(xc.sub(c[1], c[3], p), t1, p)
        y0 = xc.add(xc.scale(xc.add(c[0], c[2], p), inv2, p), xc.mul(d0, al, p, g), p)
        y1 = xc.add(xc.scale(xc.add(c[1], c[3], p), inv2, p), xc.mul(d1, al, p, g), p)
        out.append((d0, d1, xc.scale(xc.sub(y0, y1, p), t2, p)))
    return out


def operand_sets(o, L, p):
    """the three KINDS, coordinate e rolled by e as in the factor-2 test"""
    return [(kind, np.stack([np.roll(operands(o, kind, L, p, 3 + e), e) for e in range(4)])) for kind in KINDS]


# ---------------------------------------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("p", LARGE)
def test_the_first_root_of_the_alpha2_family_is_the_pinned_one(p):
    g = GEN[p]
    j, T, alpha = alpha2_root(p, g)
    assert j == T_OFFSETS[p] and T == [p - 1 - v for v in j]
    for k in offsets_in_order():                                            # no earlier vector has a root
        if k == j:
            break
        assert (sum(k), k) < (sum(j), j) and not fq_is_square(xc.scale([p - 1 - v for v in k], pow(R, -1, p), p), p, g), k
    assert [c * R % p for c in xc.mul(alpha, alpha, p, g)] == T


@pytest.mark.parametrize("p", LARGE)
def test_the_bound_inputs_are_what_they_say_and_the_restatements_agree_on_them(oracle, p):
    """on Python ints: the alpha forms, the ranges of d0, d1, d2 and the exact element 0, the sums the reductions meet; then
    f4.fold4 (Lagrange), f4.two_folds (numpy) and the Python-int fold agree on both families and on the extreme and edge
    operand sets -- ext_compose.mul_arr reduces every product before adding it, which is held here where every factor is p - 1"""
    g = GEN[p]
    assert (p - 1) ** 2 < 1 << 60 and 4 * (p - 1) ** 2 < p << 32
    for L in (4, 16, 64):
        omega = oracle.ff_prim_nth_root_g(L, p, g)
        for family in FAMILIES:
            cw, al = at_the_bound4(oracle, L, p, omega, g, family)
            assert all(a < 1 << 64 for a in al) and int(cw.max()) < p
            a = [v % p for v in al]
            a2 = xc.mul(a, a, p, g)
            if family == "alpha":
                assert al == at_the_bound(oracle, 2, p, p - 1, g)[1] and [v * R % p for v in a] == [p - 1 - j for j in range(4)]
                assert sum((p - 1) * (v * R % p) for v in a) == (p - 1) * (4 * (p - 1) - 6)  # d * alpha at element 0, coordinate 3
            else:
                assert [v * R % p for v in a2] == alpha2_root(p, g)[1]                       # d2 * alpha^2 at element 0: on the bound
                assert sum((p - 1) * (v * R % p) for v in a2) == (p - 1) * (4 * (p - 1) - sum(T_OFFSETS[p]))
            for i, ds in enumerate(fold_factors(cw, al, g, omega, p, g)):
                assert all(p - 4096 <= v < p for d in ds for v in d), (family, L, i)
                assert i or ds == ([p - 1] * 4,) * 3, (family, L)
            want = fold4_ints(cw, al, g, omega, p, g)
            assert np.array_equal(f4.fold4(cw, al, g, omega, p, g), want), (family, L)
            assert np.array_equal(f4.two_folds(cw, al, g, omega, p, g), want), (family, L)
        for kind, cw in operand_sets(oracle, L, p):
            if kind == "random":
                continue
            for al in ([p - 1] * 4, [u64_set(p)[-1]] * 4, u64_set(p)[3:7]):
                want = fold4_ints(cw, al, g, omega, p, g)
                assert np.array_equal(f4.fold4(cw, al, g, omega, p, g), want), (kind, L, al)
                assert np.array_equal(f4.two_folds(cw, al, g, omega, p, g), want), (kind, L, al)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("p", LARGE)
def test_emu_fold4_on_the_bound_inputs(oracle, emu, p, family):
    """fold4_element_ext as the CPU emulator compiles it, with both of the kernel's batchings"""
    g = GEN[p]
    for L in (4, 16, 1 << 8):
        omega = oracle.ff_prim_nth_root_g(L, p, g)
        cw, al = at_the_bound4(oracle, L, p, omega, g, family)
        want = f4.fold4(cw, al, g, omega, p, g)
        for vec in batchings(L):
            assert np.array_equal(emu_fold4(emu, cw, al, g, omega, p, g, vec), want), (L, vec)
        assert np.array_equal(emu_fold4(emu, cw, al, g, omega, p, g, 0, stride=L + 1, out_stride=L // 4 + 2 - L // 4 % 2), want), L


def test_emu_fold4_at_the_smallest_field(oracle, emu):
    """12289, which the emulator test of the boundary moduli leaves out"""
    p, g = SMALLEST, GEN[SMALLEST]
    for L in (4, 16, 1 << 8):
        omega = oracle.ff_prim_nth_root_g(L, p, g)
        for kind, cw in operand_sets(oracle, L, p):
            for al in ([p - 1] * 4, u64_set(p)[5:9], [U64] * 4):
                want = f4.fold4(cw, al, g, omega, p, g)
                for vec in batchings(L):
                    assert np.array_equal(emu_fold4(emu, cw, al, g, omega, p, g, vec), want), (L, kind, al, vec)


def test_the_comparison_of_the_gpu_tests_fails_on_one_flipped_word():
    """host arrays only: one word of the expected array flipped, one bit, at either end and in the middle"""
    want = np.arange(4 * 64, dtype=np.uint64).reshape(4, 64)
    assert same(want.copy(), want) and same(want.astype(np.uint32), want)
    for at in ((0, 0), (2, 31), (3, 63)):
        bad = want.copy()
        bad[at] ^= np.uint64(1)
        assert not same(want, bad), at
    assert not same(want[:, :63], want) and not same(want.reshape(-1), want)
    a, b = b"\x02" + bytes(40), bytearray(b"\x02" + bytes(40))
    b[17] ^= 1
    assert proof_equal((a, [3, 5], 7), (a, [3, 5], 7))
    assert not proof_equal((a, [3, 5], 7), (bytes(b), [3, 5], 7)) and not proof_equal((a, [3, 5], 7), (a, [3, 4], 7)) and not proof_equal((a, [3, 5], 7), (a, [3, 5], 6))


def proof_equal(got, want):
    """(proof bytes, top indices, nonce) of a prover against the restatement's"""
    return bytes(got[0]) == bytes(want[0]) and list(got[1]) == list(want[1]) and int(got[2]) == int(want[2])


# ---------------------------------------------------------------------------------------------- on the GPU: the fold
gpu = pytest.mark.gpu


def _odd_out_stride(q):
    return q + 2 - q % 2


@gpu
@pytest.mark.parametrize("log_len", [2, 3, 4, 12])
@pytest.mark.parametrize("p", LARGE + [SMALLEST])
def test_dev_fold4_with_every_factor_at_its_bound(engines, oracle, p, log_len):
    """smi_dev_fri_fold4_ext at q = 1, q = 2 (no 16-byte variant), the first 16-byte launch, and 2^12 (one workgroup in the
    16-byte variant, four in the 4-byte one): the three operand sets under the alphas of the u64 set -- contiguous, with an
    odd stride and with an odd out_stride -- and, at the six large primes, both bound families aligned and odd-strided.
    Against the Lagrange restatement up to 2^4; at 2^12 against two folds by 2 of the numpy restatement, tied to Lagrange
    and to Python ints on the same families without a GPU"""
    from test_gpu_fold4 import gpu_fold4
    o, eng, g = oracle, engines[p], GEN[p]
    L = 1 << log_len
    q = L // 4
    omega = o.ff_prim_nth_root_g(L, p, g)
    ref = f4.fold4 if log_len <= 4 else f4.two_folds
    for kind, cw in operand_sets(o, L, p):
        for al in _alpha_vectors(p):
            want = ref(cw, al, g, omega, p, g)
            assert same(gpu_fold4(eng, cw, al, g, omega), want), (kind, al)
            assert same(gpu_fold4(eng, cw, al, g, omega, stride=L + 1), want), (kind, al)
            assert same(gpu_fold4(eng, cw, al, g, omega, out_stride=_odd_out_stride(q)), want), (kind, al)
    if p == SMALLEST:
        return
    for family in FAMILIES:
        cw, al = at_the_bound4(o, L, p, omega, g, family)
        want = ref(cw, al, g, omega, p, g)
        assert same(gpu_fold4(eng, cw, al, g, omega), want), family
        assert same(gpu_fold4(eng, cw, al, g, omega, stride=L + 1, out_stride=_odd_out_stride(q)), want), family


# ---------------------------------------------------------------------------------------------- on the GPU: proofs
PROOFS = [(5, 4, 1, 0), (8, 8, 5, 8), (9, 4, 5, 0)]     # (log N, E, t, bits)
LAST_DEGREE = "last codeword does not correspond to polynomial of low enough degree"


def _accepted_by_both(eng, oracle, cfg, cfg_o, g, proof, bits):
    ok_o, pv_o, used_o, _top, why_o = f4.verify(oracle, cfg_o, proof, g, b"", bits)
    ok, pv, used, why = eng.fri_verify_ext(cfg, proof, b"", grind_bits=bits, folding=4)
    assert ok_o and ok, (why_o, why)
    assert pv == pv_o and used == used_o == len(proof)


def _rejected_by_both(eng, oracle, cfg, cfg_o, g, proof, bits=0):
    ok_o, _pv, _used, _top, why_o = f4.verify(oracle, cfg_o, proof, g, b"", bits)
    ok, _pv, _used, why = eng.fri_verify_ext(cfg, proof, b"", grind_bits=bits, folding=4)
    assert not ok_o and not ok and why == why_o
    return why


@gpu
@pytest.mark.parametrize("log_N,E,t,bits", PROOFS)
@pytest.mark.parametrize("p", THREE)
def test_prove_fold4_bytes_equal_the_restatement_and_both_verifiers_accept(engines, oracle, p, log_N, E, t, bits):
    """a random codeword of low degree, and the constant codeword with every coordinate p - 1 (degree 0: an honest proof)"""
    from test_gpu_fold4 import gpu_prove4
    eng, g, N = engines[p], GEN[p], 1 << log_N
    cfg_o, cw, want, want_top, want_nonce = f4.shared_proof(oracle, p, g, log_N, E, t, bits)
    cfg = eng.fri_cfg(int(cfg_o.omega), g, N, E, t)
    got = gpu_prove4(eng, cfg, cw, b"", bits)
    assert proof_equal(got, (want, want_top, want_nonce))
    assert len(got[0]) == f4.layout(N, E, t)[3]
    _accepted_by_both(eng, oracle, cfg, cfg_o, g, got[0], bits)
    top = np.full((4, N), p - 1, dtype=np.uint64)
    want = f4.prove(oracle, cfg_o, top, g, b"", bits)
    got = gpu_prove4(eng, cfg, top, b"", bits)
    assert proof_equal(got, want)
    _accepted_by_both(eng, oracle, cfg, cfg_o, g, got[0], bits)


@gpu
@pytest.mark.parametrize("p", THREE)
def test_a_crooked_layer_and_a_coordinate_of_too_high_degree_are_rejected(engines, oracle, p):
    """tests/test_gpu_fold4.py's crooked prover (a fold that is off by one in coordinate 2 of every later layer: honest trees,
    paths that verify, cosets that do not fold to the next layer) gets FOLD4_MISMATCH from both verifiers; the device's proof
    of a codeword with one random coordinate gets the last-codeword sentence"""
    from test_gpu_fold4 import gpu_prove4
    eng, g = engines[p], GEN[p]
    log_N, E, t = 8, 4, 3
    N = 1 << log_N
    cw, omega = f4.low_degree_codeword(oracle, p, g, N, E, g, 5)
    cfg_o, cfg = oracle.fri_cfg(omega, g, N, E, t, p), eng.fri_cfg(omega, g, N, E, t)
    real = f4.fold4
    try:
        def crooked(c, alpha, offset, om, pp, gg):
            out = real(c, alpha, offset, om, pp, gg)
            out[2] = (out[2] + np.uint64(1)) % np.uint64(pp)
            return out
        f4.fold4 = crooked
        proof, _top, _nonce = f4.prove(oracle, cfg_o, cw, g)
    finally:
        f4.fold4 = real
    assert _rejected_by_both(eng, oracle, cfg, cfg_o, g, proof) == f4.FOLD4_MISMATCH
    N, t = 1 << 9, 5
    for spoil in (p % 4, 3 - p % 4):
        cw, omega = f4.low_degree_codeword(oracle, p, g, N, E, g, 11, spoil=spoil)
        cfg_o, cfg = oracle.fri_cfg(omega, g, N, E, t, p), eng.fri_cfg(omega, g, N, E, t)
        proof, _top, _nonce = gpu_prove4(eng, cfg, cw)
        assert _rejected_by_both(eng, oracle, cfg, cfg_o, g, proof) == LAST_DEGREE, spoil


# ---------------------------------------------------------------------------------------------- on the GPU: the AIR proof over it
def _air(name, p, n):
    import air_compose as ac
    import air_periodic as ap
    return (ap.make if name == "mimc" else ac.make)(name, n, p)


@gpu
@pytest.mark.parametrize("bits", [0, 8])
@pytest.mark.parametrize("name", ["mixer", "mimc"])
@pytest.mark.parametrize("p", THREE)
def test_air_prove_fold4_bytes_equal_the_restatement_and_verify_accepts(engines, oracle, p, name, bits):
    """n = 2^8, blowup 8, t = 4: smi_dev_air_prove_ext_fold4 against fold4_compose.air_proof, both verifiers accept"""
    from test_gpu_air import Dev
    from test_gpu_fold4 import KW4
    eng, g, log_n, lb, t = engines[p], GEN[p], 8, 3, 4
    air, cols = _air(name, p, 1 << log_n)
    W = len(cols)
    _d, E = eng.air_plan(air, W, log_n, lb)
    with Dev(eng) as dev:
        res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, grind_bits=bits, **KW4)
    root, want, top, _nonce = f4.air_proof(oracle, air, cols, p, g, log_n, lb, t, 1, g, E, bits)
    assert bytes(res["column_roots"][0]) == root
    assert proof_equal((res["proof"], res["top_indices"], 0), (want, top, 0))
    assert eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **KW4) == (True, "")
    assert f4.air_verify(oracle, air, root, want, p, g, log_n, lb, t, 1, g, E, bits) == (True, "")


@gpu
@pytest.mark.parametrize("p", THREE)
def test_air_verify_fold4_recomputes_the_composition_and_checks_canonical_values(engines, oracle, p):
    """an honest proof under a statement with one boundary value changed gets the composition sentence, and a column opened
    as value + p under an honest tree the canonical sentence -- from the GPU verifier and from the restated one"""
    import air_compose as ac
    from test_gpu_air import Dev
    from test_gpu_air_rows import _mixer_like
    from test_gpu_fold4 import KW4
    eng, g, log_n, lb, t, bits = engines[p], GEN[p], 8, 3, 4, 0
    n = 1 << log_n
    mixer, cols = ac.make("mixer", n, p)
    W = len(cols)
    E = eng.air_plan(mixer, W, log_n, lb)[1]
    with Dev(eng) as dev:
        res = eng.dev_air_prove(mixer, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, grind_bits=bits, **KW4)
    a_last = cols[0][-1]
    for statement, want in ((mixer, (True, "")), (_mixer_like(n, p, a_last=a_last), (True, "")),
                            (_mixer_like(n, p, a0=6, a_last=a_last), (False, f4.AIR_WORDS["composition"]))):
        assert eng.air_verify(statement, res["proof"], res["column_roots"], W, log_n, lb, t, grind_bits=bits, **KW4) == want
        assert f4.air_verify(oracle, statement, bytes(res["column_roots"][0]), res["proof"], p, g, log_n, lb, t, 1, g, E, bits) == want
    for col in (0, W - 1):
        root, proof, _top, _nonce = f4.air_proof(oracle, mixer, cols, p, g, log_n, lb, t, 1, g, E, bits, plus_p_col=col)
        want = (False, f4.AIR_WORDS["canonical"])
        assert f4.air_verify(oracle, mixer, root, proof, p, g, log_n, lb, t, 1, g, E, bits) == want
        assert eng.air_verify(mixer, proof, [root], W, log_n, lb, t, grind_bits=bits, **KW4) == want
