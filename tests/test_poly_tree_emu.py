"""CPU: the subproduct-tree entry points (zerofier, evaluation and interpolation on arbitrary points) through the
emulator library -- the driver of csrc/poly_tree.h over emu_ntt and the kernels' per-thread bodies of csrc/poly_core.h,
the same sequence smi_poly_zerofier / smi_poly_eval_points / smi_poly_interpolate_points run on the device -- checked
against the oracle on both primes."""
import ctypes as C

import numpy as np
import pytest

P, G = 998244353, 3
P2, G2 = 469762049, 3
B = 256   # SMI_POLY_BLOCK: points per LDS block
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 31, 33, B - 1, B, B + 1, 2 * B - 1, 2 * B + 1, 1000]
PRIMES = [(P, G), (P2, G2)]
vp = C.c_void_p

OK, NO_INVERSE, EMPTY_DOMAIN, NON_CANONICAL = 0, -1, -15, -51


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd as s
    s.build()
    from stark_rs_amd._lib import EMU_PATH as path
    L = C.CDLL(path)
    L.emu_poly_zerofier.argtypes = [C.c_uint64, C.c_uint64, vp, C.c_size_t, vp]
    L.emu_poly_eval_points.argtypes = [C.c_uint64, C.c_uint64, vp, C.c_size_t, vp, C.c_size_t, vp]
    L.emu_poly_interpolate_points.argtypes = [C.c_uint64, C.c_uint64, vp, vp, C.c_size_t, vp]
    return L


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def zerofier(emu, p, g, dom):
    d = _u64(dom)
    out = np.zeros(len(d) + 1, dtype=np.uint64)
    return emu.emu_poly_zerofier(p, g, d.ctypes.data, len(d), out.ctypes.data), out


def eval_points(emu, p, g, coeffs, pts):
    c, x = _u64(coeffs), _u64(pts)
    out = np.zeros(max(len(x), 1), dtype=np.uint64)
    return emu.emu_poly_eval_points(p, g, c.ctypes.data, len(c), x.ctypes.data, len(x), out.ctypes.data), out[:len(x)]


def interpolate(emu, p, g, dom, vals):
    d, v = _u64(dom), _u64(vals)
    out = np.zeros(max(len(d), 1), dtype=np.uint64)
    return emu.emu_poly_interpolate_points(p, g, d.ctypes.data, v.ctypes.data, len(d), out.ctypes.data), out[:len(d)]


def distinct_points(rng, p, n, special=True):
    """n distinct points, with 0, 1 and p - 1 among them when special"""
    pts = set([0, 1, p - 1][:n] if special else [])
    while len(pts) < n:
        pts.update(int(v) for v in rng.integers(0, p, n - len(pts), dtype=np.uint64))
    out = np.array(sorted(pts), dtype=np.uint64)
    rng.shuffle(out)
    return out


@pytest.mark.parametrize("p,g", PRIMES)
@pytest.mark.parametrize("n", SIZES)
def test_emulated_zerofier_matches_oracle(emu, oracle, p, g, n):
    rng = np.random.default_rng(1000 + n)
    for dom in (distinct_points(rng, p, n), rng.integers(0, 4, n, dtype=np.uint64)):   # the second has duplicates (and 0)
        rc, z = zerofier(emu, p, g, dom)
        assert rc == OK
        assert [int(v) for v in z] == oracle.poly_zerofier(dom, p)
        assert z[n] == 1


@pytest.mark.parametrize("p,g", PRIMES)
@pytest.mark.parametrize("n", SIZES)
def test_emulated_eval_points_matches_oracle(emu, oracle, p, g, n):
    rng = np.random.default_rng(2000 + n)
    pts = distinct_points(rng, p, n)
    pts[n // 2] = pts[0]                                      # a duplicate point
    f = rng.integers(0, p, 3 * n, dtype=np.uint64)
    f[0] = p - 1
    for nc in sorted({0, 1, n - 1, n, n + 1, 3 * n}):
        rc, vals = eval_points(emu, p, g, f[:nc], pts)
        assert rc == OK
        assert np.array_equal(vals, oracle.poly_eval_domain(f[:nc], pts, p)), nc


@pytest.mark.parametrize("p,g", PRIMES)
@pytest.mark.parametrize("n", SIZES)
def test_emulated_interpolate_points_matches_oracle(emu, oracle, p, g, n):
    rng = np.random.default_rng(3000 + n)
    dom = distinct_points(rng, p, n)
    vals = rng.integers(0, p, n, dtype=np.uint64)
    rc, coeffs = interpolate(emu, p, g, dom, vals)
    assert rc == OK
    if n <= 300:   # the reference's O(n^3) Lagrange body
        assert oracle.poly_eq(coeffs, oracle.poly_interpolate_domain(dom, vals, p), p)
    else:
        idx = rng.choice(n, 64, replace=False)
        assert [oracle.poly_eval(coeffs, int(dom[i]), p) for i in idx] == [int(vals[i]) for i in idx]


def test_emulated_eval_points_of_interpolant_round_trips(emu):
    rng = np.random.default_rng(7)
    for p, g in PRIMES:
        dom = distinct_points(rng, p, 700)
        vals = rng.integers(0, p, 700, dtype=np.uint64)
        rc, coeffs = interpolate(emu, p, g, dom, vals)
        assert rc == OK
        rc, back = eval_points(emu, p, g, coeffs, dom)
        assert rc == OK and np.array_equal(back, vals)


@pytest.mark.parametrize("p,g", PRIMES)
def test_emulated_poly_tree_statuses(emu, p, g):
    rc, _ = interpolate(emu, p, g, [1, 2, 3, 2], [5, 6, 7, 8])
    assert rc == NO_INVERSE                                   # a repeated point: field.inv(0), interpolate.rs:34
    rng = np.random.default_rng(11)
    dom = distinct_points(rng, p, 600)
    dom[599] = dom[3]
    assert interpolate(emu, p, g, dom, np.ones(600, dtype=np.uint64))[0] == NO_INVERSE
    assert interpolate(emu, p, g, [], [])[0] == EMPTY_DOMAIN
    assert zerofier(emu, p, g, [])[0] == EMPTY_DOMAIN
    assert zerofier(emu, p, g, [1, p])[0] == NON_CANONICAL
    assert interpolate(emu, p, g, [1, p + 3], [1, 2])[0] == NON_CANONICAL
    assert interpolate(emu, p, g, [1, 2], [1, p])[0] == NON_CANONICAL
    assert eval_points(emu, p, g, [1, p], [1, 2])[0] == NON_CANONICAL
    assert eval_points(emu, p, g, [1, 2], [p])[0] == NON_CANONICAL
    assert eval_points(emu, p, g, [], [p])[0] == NON_CANONICAL
    rc, vals = eval_points(emu, p, g, [], [4, 5])
    assert rc == OK and not vals.any()
    assert eval_points(emu, p, g, [1, 2], [])[0] == OK
