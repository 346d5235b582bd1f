"""GPU: zerofier, evaluation and interpolation on arbitrary points (smi_poly_zerofier / smi_poly_eval_points /
smi_poly_interpolate_points, subproduct trees on the device) through the C ABI: the reference's KATs on their own
domains, the oracle on both primes, exact agreement with the NTT path on randomly permuted cosets, large random
domains, and the number of launches.  `pytest -m gpu`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, G = 998244353, 3
P2, G2 = 469762049, 3
B = 256   # SMI_POLY_BLOCK
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 31, 33, B - 1, B, B + 1, 2 * B - 1, 2 * B + 1, 1000]


@pytest.fixture(scope="module")
def engines():
    import stark_rs_amd as s
    out = {P: s.Engine(P, G, 0), P2: s.Engine(P2, G2, 0)}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def eng(engines):
    return engines[P]


def distinct_points(rng, p, n, special=True):
    pts = set([0, 1, p - 1][:n] if special else [])
    while len(pts) < n:
        pts.update(int(v) for v in rng.integers(0, p, n - len(pts), dtype=np.uint64))
    out = np.array(sorted(pts), dtype=np.uint64)
    rng.shuffle(out)
    return out


def host_prod(x, dom, p):
    """prod (x - d) mod p on the host"""
    a = (np.uint64(x) + np.uint64(p) - dom) % np.uint64(p)
    while len(a) > 1:
        if len(a) % 2:
            a = np.append(a, np.uint64(1))
        a = (a[0::2] * a[1::2]) % np.uint64(p)
    return int(a[0])


# ---- the reference's KATs on their original domains
def test_interpolation_kats(eng):
    """src/univariate/interpolate.rs:61-163"""
    assert list(eng.poly_interpolate_points([1, 2, 3], [1, 4, 9])) == [0, 0, 1]            # test_x2
    assert list(eng.poly_interpolate_points([1, 3], [5, 9])) == [3, 2]                     # test_linear_polynomial
    assert list(eng.poly_interpolate_points([1, 2, 3], [2, 5, 10])) == [1, 0, 1]           # test_quadratic_polynomial
    dom, vals = [0, 1, 2, 4], [3, 7, 13, 35]                                               # test_interpolation_matches_values
    c = eng.poly_interpolate_points(dom, vals)
    assert list(eng.poly_eval_points(c, dom)) == vals
    dom, vals = [0, 1, P - 5], [P - 2, 6, 48]                                              # test_lagrange_three_points
    c = eng.poly_interpolate_points(dom, vals)
    assert list(c) == [P - 2, 5, 3] and list(eng.poly_eval_points(c, dom)) == vals


def test_zerofier_kats(eng, oracle):
    """src/univariate/mod.rs:320-413"""
    assert list(eng.poly_zerofier([5])) == [P - 5, 1]                                      # test_zerofier_single_point
    assert list(eng.poly_zerofier([2, 3])) == [6, P - 5, 1]                                # test_zerofier_two_points
    assert list(eng.poly_zerofier([1, 2, 3])) == [P - 6, 11, P - 6, 1]                     # test_zerofier_three_points
    assert list(eng.poly_zerofier([0])) == [0, 1]                                          # test_zerofier_zero_point
    assert list(eng.poly_eval_points(eng.poly_zerofier([1, 2]), [5])) == [12]              # test_zerofier_nonzero_evaluation
    for n in (1, 2, 5, 10, 33):                                                            # test_zerofier_degree
        dom = list(range(1, n + 1))
        assert [int(v) for v in eng.poly_zerofier(dom)] == oracle.poly_zerofier(dom)


def test_statuses(engines):
    from stark_rs_amd import StarkMiError
    for p, e in engines.items():
        with pytest.raises(StarkMiError, match="no inverse") as ex:
            e.poly_interpolate_points([1, 2, 3, 2], [5, 6, 7, 8])
        assert ex.value.status == -1
        with pytest.raises(StarkMiError) as ex:
            e.poly_interpolate_points([], [])
        assert ex.value.status == -15
        with pytest.raises(StarkMiError) as ex:
            e.poly_zerofier([])
        assert ex.value.status == -15
        for call in (lambda: e.poly_zerofier([1, p]), lambda: e.poly_interpolate_points([1, 2], [1, p]),
                     lambda: e.poly_eval_points([1, p], [1, 2]), lambda: e.poly_eval_points([1, 2], [p + 1])):
            with pytest.raises(StarkMiError) as ex:
                call()
            assert ex.value.status == -51
        big = 1 << (e.two_adicity + 1)
        with pytest.raises(StarkMiError) as ex:
            e.poly_eval_points([1], np.zeros(big // 2 + 1, dtype=np.uint64))
        assert ex.value.status == -4
        assert not e.poly_eval_points([], [4, 5]).any() and len(e.poly_eval_points([1, 2], [])) == 0
        # still usable after every refusal
        assert list(e.poly_interpolate_points([1, 3], [5, 9])) == [3, 2]


# ---- the oracle, both primes
@pytest.mark.parametrize("p", [P, P2])
def test_against_oracle(engines, oracle, p):
    e = engines[p]
    rng = np.random.default_rng(p % 1000)
    for n in SIZES:
        dom = distinct_points(rng, p, n)
        assert [int(v) for v in e.poly_zerofier(dom)] == oracle.poly_zerofier(dom, p), n
        dup = rng.integers(0, 5, n, dtype=np.uint64)
        assert [int(v) for v in e.poly_zerofier(dup)] == oracle.poly_zerofier(dup, p), n
        pts = dom.copy()
        pts[n // 2] = pts[0]
        f = rng.integers(0, p, 3 * n, dtype=np.uint64)
        for nc in sorted({0, 1, n - 1, n, n + 1, 3 * n}):
            assert np.array_equal(e.poly_eval_points(f[:nc], pts), oracle.poly_eval_domain(f[:nc], pts, p)), (n, nc)
        vals = rng.integers(0, p, n, dtype=np.uint64)
        c = e.poly_interpolate_points(dom, vals)
        if n <= 300:
            assert oracle.poly_eq(c, oracle.poly_interpolate_domain(dom, vals, p), p), n
        else:
            idx = rng.choice(n, 64, replace=False)
            assert [oracle.poly_eval(c, int(dom[i]), p) for i in idx] == [int(vals[i]) for i in idx], n


# ---- exact agreement with the independently tested NTT path on permuted cosets (not geometric in order)
@pytest.mark.parametrize("log_n", [16, 20])
def test_permuted_coset_matches_ntt(eng, log_n):
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    omega, offset = eng.prim_nth_root(n), 7
    coset = np.empty(n, dtype=np.uint64)
    coset[0] = offset
    step = np.array([pow(omega, k, P) for k in range(1 << 10)], dtype=np.uint64)
    big = pow(omega, 1 << 10, P)
    hi = 1
    for b in range(n >> 10):      # offset * omega^(1024 b + k)
        coset[b << 10:(b + 1) << 10] = step * np.uint64(offset * hi % P) % np.uint64(P)
        hi = hi * big % P
    perm = rng.permutation(n)
    f = rng.integers(0, P, n, dtype=np.uint64)
    evals = eng.coset_ntt(f, log_n, offset)
    assert np.array_equal(eng.poly_eval_points(f, coset[perm]), evals[perm])
    assert np.array_equal(eng.poly_interpolate_points(coset[perm], evals[perm]), f)
    vals = rng.integers(0, P, n, dtype=np.uint64)
    assert np.array_equal(eng.poly_interpolate_points(coset[perm], vals[perm]), eng.intt(vals, offset))


# ---- large random domains
@pytest.mark.parametrize("p,n", [(P, 1 << 18), (P2, 1 << 18), (P2, (1 << 20) + 1)])
def test_random_domains(engines, oracle, p, n):
    e = engines[p]
    rng = np.random.default_rng(n + p % 97)
    dom = rng.integers(0, p, n, dtype=np.uint64)
    z = e.poly_zerofier(dom)
    assert len(z) == n + 1 and z[n] == 1
    for i in rng.choice(n, 8, replace=False):
        assert oracle.poly_eval(z, int(dom[i]), p) == 0
    for x in rng.integers(0, p, 4, dtype=np.uint64):
        assert oracle.poly_eval(z, int(x), p) == host_prod(int(x), dom, p)
    dom = np.unique(dom)
    rng.shuffle(dom)
    n = len(dom)
    f = rng.integers(0, p, n, dtype=np.uint64)
    vals = e.poly_eval_points(f, dom)
    idx = rng.choice(n, 16, replace=False)
    assert [int(vals[i]) for i in idx] == [oracle.poly_eval(f, int(dom[i]), p) for i in idx]
    c = e.poly_interpolate_points(dom, vals)
    assert np.array_equal(c, f)
    vals = rng.integers(0, p, n, dtype=np.uint64)
    c = e.poly_interpolate_points(dom, vals)
    assert [oracle.poly_eval(c, int(dom[i]), p) for i in idx] == [int(vals[i]) for i in idx]


def test_launch_count_grows_with_log_n(eng):
    """no host loop per node: a 2^16-point interpolation records at most 64 log2 n launches"""
    n = 1 << 16
    rng = np.random.default_rng(5)
    dom = distinct_points(rng, P, n)
    vals = rng.integers(0, P, n, dtype=np.uint64)
    eng.poly_interpolate_points(dom, vals)   # warm-up: buffers and tables
    eng.profile_read()
    eng.profile(True)
    try:
        c = eng.poly_interpolate_points(dom, vals)
        rec = eng.profile_read()
    finally:
        eng.profile(False)
    launches = sum(r["launches"] for r in rec.values())
    assert any(k.startswith("poly_block_kernel") for k in rec) and "poly_horner_kernel" in rec
    assert 0 < launches <= 64 * 16, launches
    assert np.array_equal(eng.poly_eval_points(c, dom[:512]), vals[:512])
