"""Every modulus-generic kernel at the moduli where its range bounds are tight: the largest primes below 2^30 (4 p < 2^32 by
0.02 %, the sum of four products in ext_mul_prepared against p 2^32), the largest below 2^29 (the NTT's 8 p lazy range,
8 p = 0.9999 2^32), the first at or above 2^29 (the first on the 4 p range) and the smallest field the context accepts --
with operands that sit on the bounds: every element p - 1, the edge values, and the unreduced u64 challenges a transcript
can hand over.  References: the p-generic oracle (fast_intt, fast_coset_ntt, fri_fold_codeword, poly_*, fri_prove) and the
Python restatements tests/ext_compose.py, tests/air_compose.py, tests/air_periodic.py.  Every comparison is exact.
The table of primes is re-derived without a GPU; `pytest -m gpu` for the rest."""
import numpy as np
import pytest

import air_compose as ac
import air_periodic as ap
import ext_compose as xc

# (role, p, two-adicity, a primitive root)
TABLE = [
    ("largest usable prime below 2^30", 1073692673, 14, 3),
    ("largest below 2^30 with two-adicity >= 20", 1053818881, 20, 7),
    ("largest below 2^29", 536813569, 13, 7),
    ("largest below 2^29 with two-adicity >= 20", 531628033, 20, 5),
    ("smallest at or above 2^29", 536903681, 15, 7),
    ("smallest at or above 2^29 with two-adicity >= 20", 576716801, 21, 6),
    ("smallest field the context accepts", 12289, 12, 11),
]
GEN = {p: g for _r, p, _k, g in TABLE}
ADICITY = {p: k for _r, p, k, _g in TABLE}
ALL = [p for _r, p, _k, _g in TABLE]
LARGE = ALL[:6]
THREE = [1073692673, 536813569, 536903681]        # one per range bound: 4 p, 8 p, and the first prime past the switch
TWO = [1073692673, 536813569]
FIRST_ABOVE_2_30 = 1073741827
U64 = (1 << 64) - 1
UNSUPPORTED_PRIME = -52


def u64_set(p):
    """the unreduced challenges, weights and alphas: around 0, p, 2^32 and 2^64, and the largest k p + (p - 1) below 2^64"""
    return [0, p - 1, p, p + 1, (1 << 32) - 1, 1 << 32, U64, (1 << 64) - p, ((1 << 64) - p) // p * p + p - 1]


def operands(o, kind, n, p, seed=1):
    if kind == "random":
        return o.splitmix64(seed, n) % np.uint64(p)
    if kind == "extreme":
        return np.full(n, p - 1, dtype=np.uint64)
    edge = [0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    return np.resize(np.array(edge, dtype=np.uint64), n)


KINDS = ["random", "extreme", "edge"]


# ---------------------------------------------------------------------------------------------- without a GPU
def _is_prime(n):
    """Miller-Rabin on the first twelve primes as bases: deterministic below 3.3 10^24"""
    if n < 2:
        return False
    small = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37]
    for q in small:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _factors(n):
    out, q = set(), 2
    while q * q <= n:
        while n % q == 0:
            out.add(q)
            n //= q
        q += 1
    return out | ({n} if n > 1 else set())


def _adicity(p):
    return ((p - 1) & -(p - 1)).bit_length() - 1


def _usable(n, least=12):
    return _is_prime(n) and _adicity(n) >= least


def _search(start, step, stop, least):
    """the first n = 1 mod 2^least from start in direction step that is a usable prime"""
    n = start - (start - 1) % (1 << least) if step < 0 else start + (-(start - 1)) % (1 << least)
    while n != stop and not _usable(n, least):
        n += step * (1 << least)
    return n


def _composite_below_2_30():
    n = (1 << 30) - (1 << 12) + 1
    while _is_prime(n):
        n -= 1 << 12
    return n


def test_the_table_of_primes_is_what_it_says():
    for role, p, k, g in TABLE:
        assert _is_prime(p) and _adicity(p) == k >= 12 and p % 4 == 1, role
        assert all(pow(g, (p - 1) // q, p) != 1 for q in _factors(p - 1)), role       # g generates F_p^*
        assert xc.field_ok(p, g), role                                                # ... so X^4 - g is irreducible
    assert _search((1 << 30) - 1, -1, 0, 12) == TABLE[0][1] and _search((1 << 30) - 1, -1, 0, 20) == TABLE[1][1]
    assert _search((1 << 29) - 1, -1, 0, 12) == TABLE[2][1] and _search((1 << 29) - 1, -1, 0, 20) == TABLE[3][1]
    assert _search(1 << 29, 1, 0, 12) == TABLE[4][1] and _search(1 << 29, 1, 0, 20) == TABLE[5][1]
    assert _search(3, 1, 0, 12) == TABLE[6][1]
    assert 8 * TABLE[2][1] < 1 << 32 <= 8 * TABLE[4][1] and 4 * TABLE[0][1] < 1 << 32
    assert _is_prime(FIRST_ABOVE_2_30) and not any(_is_prime(n) for n in range((1 << 30) + 1, FIRST_ABOVE_2_30))
    n = _composite_below_2_30()
    assert not _is_prime(n) and n < 1 << 30 and _adicity(n) >= 12


def at_the_bound(o, L, p, omega, offset):
    """-> (codeword, alpha) that put ext_mul_prepared's sum on and just under its largest value: hi = lo - 2 x d makes the
    fold's factor (lo - hi) 2^-1 x^-1 the chosen d, every coordinate within 2^12 of p - 1 and exactly p - 1 at element 0;
    alpha_j = (p - 1 - j) 2^-32 (mod p, handed over unreduced) has the Montgomery form p - 1 - j.  Coordinate 3 of d * alpha,
    the one without a factor g, is then the one reduction of a sum next to 4 (p - 1)^2 -- exactly that for j = 0 alone --
    and with half a codeword of distinct sums every low word the reduction can meet there is met"""
    half, P = L // 2, np.uint64(p)
    x = xc._powers(omega, half, p) * np.uint64(offset) % P
    lo = np.stack([o.splitmix64(70 + e, half) % P for e in range(4)])
    d = np.stack([P - np.uint64(1) - o.splitmix64(80 + e, half) % np.uint64(4096) for e in range(4)])
    d[:, 0] = p - 1
    hi = (lo + P - x * np.uint64(2) % P * d % P) % P
    a = [(p - 1 - j) * pow(1 << 32, -1, p) % p for j in range(4)]
    return np.concatenate([lo, hi], axis=1), [a[0], a[1] + p, a[2] + ((1 << 64) - 1 - a[2]) // p * p, a[3] + (p << 31)]


def _fold_ints(cw, alpha, offset, omega, p, g):
    """tests/ext_compose.py's fold on Python ints"""
    half = len(cw[0]) // 2
    inv2, out = pow(2, -1, p), [[0] * half for _ in range(4)]
    for i in range(half):
        lo, hi = [int(c[i]) for c in cw], [int(c[half + i]) for c in cw]
        xinv = pow(offset * pow(omega, i, p) % p, -1, p)
        s = xc.scale(xc.add(lo, hi, p), inv2, p)
        d = xc.scale(xc.sub(lo, hi, p), inv2 * xinv % p, p)
        v = xc.add(s, xc.mul(d, [a % p for a in alpha], p, g), p)
        for e in range(4):
            out[e][i] = v[e]
    return np.array(out, dtype=np.uint64)


@pytest.mark.parametrize("p", LARGE)
def test_the_numpy_restatement_is_exact_at_the_extreme_operands(oracle, p):
    """ext_compose.mul_arr / fold reduce every product (< 2^60) before adding it: no partial sum passes 4 p < 2^32, far
    from 2^64.  Held against Python-int arithmetic where every factor is p - 1 and at the edge values"""
    g = GEN[p]
    assert (p - 1) ** 2 < 1 << 60 and 4 * (p - 1) + p < 1 << 64
    for L in (2, 8):
        omega = oracle.ff_prim_nth_root_g(L, p, g)
        for kind in ("extreme", "edge"):
            cw = np.stack([np.roll(operands(oracle, kind, L, p), e) for e in range(4)])
            for alpha in ([p - 1] * 4, [u64_set(p)[-1]] * 4, u64_set(p)[3:7]):
                assert np.array_equal(xc.fold(cw, alpha, g, omega, p, g), _fold_ints(cw, alpha, g, omega, p, g))
        cw, alpha = at_the_bound(oracle, L, p, omega, g)
        assert all(a < 1 << 64 and a * (1 << 32) % p == p - 1 - j for j, a in enumerate(alpha))
        assert np.array_equal(xc.fold(cw, alpha, g, omega, p, g), _fold_ints(cw, alpha, g, omega, p, g))
        half, inv2 = L // 2, pow(2, -1, p)
        for i in range(half):       # the fold's d: p - 1 in every coordinate of element 0, within 2^12 of it elsewhere
            d = [(int(cw[e, i]) - int(cw[e, half + i])) * inv2 * pow(g * pow(omega, i, p), -1, p) % p for e in range(4)]
            assert all(p - 4096 <= v < p for v in d) and (i or d == [p - 1] * 4)


@pytest.mark.parametrize("p", LARGE)
def test_the_emulated_fold_ext_at_the_bound(oracle, p):
    """fold_element_ext (csrc/fri_core.h) as the CPU emulator compiles it, on the input of at_the_bound and the operand sets"""
    import ctypes as C
    import stark_rs_amd
    from stark_rs_amd import _lib
    from test_ext_emu import emu_fold
    stark_rs_amd.build()
    emu = C.CDLL(_lib.EMU_PATH)
    emu.emu_fold_ext.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    g = GEN[p]
    for L in (2, 8, 1 << 12):
        omega = oracle.ff_prim_nth_root_g(L, p, g)
        cw, al = at_the_bound(oracle, L, p, omega, g)
        assert np.array_equal(emu_fold(emu, cw, al, g, omega, p, g), xc.fold(cw, al, g, omega, p, g)), L
        for kind in KINDS:
            cw = np.stack([np.roll(operands(oracle, kind, L, p, 3 + e), e) for e in range(4)])
            for al in ([p - 1] * 4, u64_set(p)[5:9], [U64] * 4):
                assert np.array_equal(emu_fold(emu, cw, al, g, omega, p, g), xc.fold(cw, al, g, omega, p, g)), (L, kind, al)


@pytest.mark.parametrize("p", LARGE)
def test_host_ext_mul_and_inv_at_the_extreme_element(p):
    """smi_ext_mul / smi_ext_inv (host code): 4 (p - 1)^2 is the largest sum ext_mul_prepared hands to its one reduction"""
    from stark_rs_amd.engine import ext_inv, ext_mul
    g = GEN[p]
    top = [p - 1] * 4
    elems = [top, [0, p - 1, 0, p - 1], [p - 1, 0, 0, 0], [1, p - 1, (p - 1) // 2, (p + 1) // 2], [p - 2, p - 1, p - 1, p - 2]]
    for a in elems:
        for b in elems:
            assert ext_mul(p, g, a, b) == xc.mul(a, b, p, g), (a, b)
        inv = ext_inv(p, g, a)
        assert inv == xc.inv(a, p, g), a
        assert ext_mul(p, g, a, inv) == [1, 0, 0, 0], a


# ---------------------------------------------------------------------------------------------- on the GPU
from test_gpu_air import Dev  # noqa: E402

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """one context per prime of the table, made on first use, closed at the end of the module"""
    import stark_rs_amd as s

    class Lazy(dict):
        def __missing__(self, p):
            self[p] = s.Engine(p, GEN[p], 0)
            return self[p]
    es = Lazy()
    yield es
    for e in es.values():
        e.close()


def _logs(p):
    return sorted({l for l in (12, 13, 14, 16, 20, ADICITY[p]) if l <= min(ADICITY[p], 20)})


@gpu
@pytest.mark.parametrize("p,logn", [(p, l) for p in ALL for l in _logs(p)])
def test_transforms_at_every_plan_a_small_size_takes(engines, oracle, p, logn):
    """12 and the prime's two-adicity, and of 13, 14, 16, 20 what the prime admits.  Constant and alternating p - 1 push every
    sum of the lazy butterflies to the bound the kernels track (tests/test_gpu_parity.py, test_ntt_extreme_values_lazy_ranges)"""
    o, eng, g = oracle, engines[p], GEN[p]
    n = 1 << logn
    w = o.ff_prim_nth_root_g(n, p, g)
    inputs = [operands(o, k, n, p, logn) for k in KINDS]
    if logn < 20:
        inputs += [np.where(np.arange(n) % 2 == 0, p - 1, 0).astype(np.uint64), np.where((np.arange(n) >> 4) % 2 == 0, p - 1, 1).astype(np.uint64)]
    for k, vals in enumerate(inputs):
        for offset in (1, g):
            assert np.array_equal(eng.intt(vals, offset), o.fast_intt(vals, w, offset, p)), (k, offset)
            assert np.array_equal(eng.coset_ntt(vals, logn, offset), o.fast_coset_ntt(vals, n, w, offset, p)), (k, offset)
        assert np.array_equal(eng.coset_ntt(vals[:n // 8], logn, g), o.fast_coset_ntt(vals[:n // 8], n, w, g, p)), k


# 12289 has two-adicity 12: no blowup of 2^12 rows fits -- the one prime of seven this item leaves out
@gpu
@pytest.mark.parametrize("p,lb", [(p, lb) for p in ALL for lb in range(1, min(4, ADICITY[p] - 12) + 1)])
def test_lde_of_2_12_rows(engines, oracle, p, lb):
    o, eng, g, log_n = oracle, engines[p], GEN[p], 12
    n, N = 1 << log_n, 1 << (log_n + lb)
    w, wN = o.ff_prim_nth_root_g(n, p, g), o.ff_prim_nth_root_g(N, p, g)
    cols = np.stack([operands(o, k, n, p, 40 + lb) for k in KINDS])
    out = eng.lde(cols, lb, 1, g)
    for c in range(3):
        assert np.array_equal(out[c], o.fast_coset_ntt(o.fast_intt(cols[c], w, 1, p), N, wN, g, p)), KINDS[c]


# 2^14 points on 12289 (two-adicity 12) is the one case of 21 that cannot run
@gpu
@pytest.mark.parametrize("p,log_len", [(p, l) for p in ALL for l in (1, 10, 14) if l <= ADICITY[p]])
def test_fold_host_device_and_shards(engines, oracle, p, log_len):
    """smi_fri_fold, smi_dev_fri_fold and smi_dev_fri_fold_shard (two uneven shards) against Fri::fold_codeword"""
    o, eng, g = oracle, engines[p], GEN[p]
    n, half = 1 << log_len, 1 << (log_len - 1)
    omega, offset = o.ff_prim_nth_root_g(n, p, g), g
    cfg = o.fri_cfg(omega, offset, max(n, 4), 4, 1, p)
    alphas = u64_set(p)
    cut = half // 3
    with Dev(eng) as dev:
        d_al = dev.upload_u64(alphas)
        d_out = dev.alloc(4 * half)
        for kind in KINDS:
            cw = operands(o, kind, n, p, 7 + log_len)
            d_in, d_hi = dev.upload(cw), dev.upload(cw[half:])
            for k, alpha in enumerate(alphas):
                want = o.fri_fold_codeword(cfg, cw, alpha, offset, omega)
                assert np.array_equal(eng.fri_fold(cw, alpha, offset, omega), want), (kind, k)
                eng.dev_fri_fold(d_in, n, d_al + 8 * k, offset, omega, d_out)
                assert np.array_equal(eng.dev_download(d_out, half), want), (kind, k)
                eng.dev_upload(np.zeros(half, dtype=np.uint64), d_out)
                for i0, i1 in ((0, cut), (cut, half)):
                    if i1 > i0:
                        eng.dev_fri_fold_shard(d_in + 4 * i0, d_hi + 4 * i0, i1 - i0, i0, n, d_al + 8 * k, offset, omega, d_out + 4 * i0)
                assert np.array_equal(eng.dev_download(d_out, half), want), (kind, k)


def _alpha_vectors(p):
    u = u64_set(p)
    return [[u[(k + e) % len(u)] for e in range(4)] for k in range(len(u))] + [[p - 1] * 4, [u[-1]] * 4, [U64] * 4]


@gpu
@pytest.mark.parametrize("p", LARGE)
@pytest.mark.parametrize("log_len", [1, 3, 12])
def test_fold_ext_with_every_factor_at_its_bound(engines, oracle, p, log_len):
    """the three operand sets under alphas of the u64 set, and the input that hands mont_reduce64 exactly 4 (p - 1)^2 against
    its bound p 2^32 (at_the_bound: with every codeword coordinate p - 1 the difference lo - hi, the factor of alpha, is 0).
    Contiguous columns (16-byte accesses from length 8 on) and an odd stride (scalar accesses)"""
    from test_gpu_ext import gpu_fold
    o, eng, g = oracle, engines[p], GEN[p]
    L = 1 << log_len
    omega = o.ff_prim_nth_root_g(L, p, g)
    for kind in KINDS:
        cw = np.stack([np.roll(operands(o, kind, L, p, 3 + e), e) for e in range(4)])
        for al in _alpha_vectors(p):
            want = xc.fold(cw, al, g, omega, p, g)
            assert np.array_equal(gpu_fold(eng, cw, al, g, omega), want), (kind, al)
            if kind == "extreme" or al[0] == p - 1:
                assert np.array_equal(gpu_fold(eng, cw, al, g, omega, stride=L + 1), want), (kind, al)
    cw, al = at_the_bound(o, L, p, omega, g)
    want = xc.fold(cw, al, g, omega, p, g)
    assert np.array_equal(gpu_fold(eng, cw, al, g, omega), want)
    assert np.array_equal(gpu_fold(eng, cw, al, g, omega, stride=L + 1), want)


def _weights(p, count, shift=0):
    u = u64_set(p)
    return [u[(shift + 2 * j) % len(u)] for j in range(count)]


def _airs(p, n):
    yield "fib", ac.make("fib", n, p)
    yield "mixer", ac.make("mixer", n, p)
    yield "mimc", ap.make("mimc", n, p)


def _strided(lde, stride):
    import torch
    W, N = lde.shape
    host = np.zeros(W * stride, dtype=np.uint32)
    for c in range(W):
        host[c * stride:c * stride + N] = lde[c]
    t = torch.from_numpy(host.view(np.int32)).cuda()
    torch.cuda.synchronize()
    return t


@gpu
@pytest.mark.parametrize("p", THREE)
def test_compose_and_compose_ext_under_unreduced_weights(engines, oracle, p):
    """2^8 rows, blowup 8: smi_dev_air_compose against the polynomial route, smi_dev_air_compose_ext coordinate by coordinate
    against the route under weights e, tiled and (from columns an odd stride apart) without tiles"""
    import torch
    o, eng, g, log_n, lb = oracle, engines[p], GEN[p], 8, 3
    N = 1 << (log_n + lb)
    for name, (air, cols) in _airs(p, 1 << log_n):
        W, K = len(cols), len(air.constraints)
        wts, ch = _weights(p, W + K), _weights(p, 4 * (W + K), 1)
        want = np.asarray(ap.route(o, air, cols, wts, p, g, log_n, lb, 1, g)[0], dtype=np.uint64)
        want4 = [np.asarray(ap.route(o, air, cols, xc.weight_vector(ch, e), p, g, log_n, lb, 1, g)[0], dtype=np.uint64) for e in range(4)]
        with Dev(eng) as dev:
            d_lde, d_out, d_out4 = dev.alloc(4 * W * N), dev.alloc(4 * N), dev.alloc(16 * N)
            eng.dev_lde(dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, d_lde)
            d_w, d_ch = dev.upload_u64(wts), dev.upload_u64(ch)
            eng.dev_air_compose(air, d_lde, W, log_n, lb, d_w, d_out)
            assert np.array_equal(eng.dev_download(d_out, N), want), name
            eng.dev_air_compose_ext(air, d_lde, W, log_n, lb, d_ch, d_out4)
            got4 = eng.dev_download(d_out4, 4 * N).reshape(4, N)
            for e in range(4):
                assert np.array_equal(got4[e], want4[e]), (name, e)
            lde = eng.dev_download(d_lde, W * N).astype(np.uint32).reshape(W, N)
            t_lde = _strided(lde, N + 1)
            t_out = torch.zeros(4 * (N + 3), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            eng.dev_air_compose(air, t_lde.data_ptr(), W, log_n, lb, d_w, t_out.data_ptr(), stride=N + 1)
            eng.sync()
            assert np.array_equal(t_out.cpu().numpy().view(np.uint32)[:N], want.astype(np.uint32)), name
            eng.dev_air_compose_ext(air, t_lde.data_ptr(), W, log_n, lb, d_ch, t_out.data_ptr(), stride=N + 1, out_stride=N + 3)
            eng.sync()
            got = t_out.cpu().numpy().view(np.uint32)
            for e in range(4):
                assert np.array_equal(got[e * (N + 3):e * (N + 3) + N], want4[e].astype(np.uint32)), (name, e)


@gpu
@pytest.mark.parametrize("p", THREE)
def test_air_check_names_the_first_violated_row(engines, p):
    eng, log_n = engines[p], 8
    n = 1 << log_n
    for name, (air, cols) in _airs(p, n):
        bad = [list(c) for c in cols]
        col, row = (0, n // 2) if bad[0][n // 2] != p - 1 else (0, n // 2 + 1)
        bad[col][row] = p - 1
        want = air.first_violation(p, bad)
        assert want is not None and air.first_violation(p, cols) is None, name
        with Dev(eng) as dev:
            assert eng.dev_air_check(air, dev.upload(np.array(cols, dtype=np.uint64)), len(cols), log_n) == (True, None, None, ""), name
            okc, con, at, _sentence = eng.dev_air_check(air, dev.upload(np.array(bad, dtype=np.uint64)), len(cols), log_n)
        assert (okc, con, at) == (False,) + tuple(want), name


def _trim(c):
    c = [int(v) for v in c]
    while c and c[-1] == 0:
        c.pop()
    return c


@gpu
@pytest.mark.parametrize("p", TWO)
@pytest.mark.parametrize("n", [257, 4096])
def test_poly_tree_on_random_distinct_points(engines, oracle, p, n):
    """the interpolant at 4096 points is past the oracle's O(n^3) Lagrange: it is the one polynomial of degree < n that takes
    the values, and the oracle's Polynomial::eval_domain checks that it does"""
    o, eng = oracle, engines[p]
    raw = [p - 1, 0, 1] + [int(x) for x in o.splitmix64(n, 2 * n) % np.uint64(p)]
    pts = np.array(list(dict.fromkeys(raw))[:n], dtype=np.uint64)   # distinct, in no order
    assert len(pts) == n
    vals = operands(o, "random", n, p, 99)
    vals[:6] = operands(o, "edge", 6, p)
    assert [int(v) for v in eng.poly_zerofier(pts)] == o.poly_zerofier(pts, p)
    coeffs = operands(o, "random", n, p, 17)
    coeffs[-1] = p - 1
    assert np.array_equal(eng.poly_eval_points(coeffs, pts), o.poly_eval_domain(coeffs, pts, p))
    got = eng.poly_interpolate_points(pts, vals)
    assert len(got) == n and np.array_equal(o.poly_eval_domain(got, pts, p), vals)
    if n == 257:
        assert _trim(got) == _trim(o.poly_interpolate_domain(pts, vals, p))


@gpu
@pytest.mark.parametrize("p", TWO)
def test_poly_mul_div_scale_across_the_transform_path(engines, oracle, p):
    o, eng = oracle, engines[p]
    for na, nb in ((5, 9), (100, 157), (700, 325), (1024, 1024)):
        for kind in ("random", "extreme"):
            a, b = operands(o, kind, na, p, na), operands(o, kind, nb, p, nb)
            assert [int(v) for v in eng.poly_mul(a, b)] == o.poly_mul(a, b, p), (na, nb, kind)
    for na, nb in ((9, 5), (157, 100), (700, 325), (1024, 1), (1500, 2)):
        for kind in ("random", "extreme"):
            a, b = operands(o, kind, na, p, 3 * na), operands(o, kind, nb, p, 5 * nb)
            q, r = eng.poly_div(a, b)
            wq, wr = o.poly_div(a, b, p)
            assert [int(v) for v in q] == [int(v) for v in wq] and _trim(r) == _trim(wr), (na, nb, kind)
    for kind in KINDS:
        c = operands(o, kind, 1000, p, 3)
        for factor in (0, 1, p - 1, p - 2):
            assert [int(v) for v in eng.poly_scale(c, factor)] == o.poly_scale(c, factor, p), (kind, factor)


@gpu
@pytest.mark.parametrize("p", TWO)
def test_combine_columns_of_p_minus_one_under_unreduced_weights(engines, oracle, p):
    o, eng, W, N = oracle, engines[p], 4, 1 << 12
    u = u64_set(p)
    for kind in ("extreme", "edge", "random"):
        cols = np.stack([np.roll(operands(o, kind, N, p, 60 + c), c) for c in range(W)])
        with Dev(eng) as dev:
            d_cols, d_out = dev.upload(cols), dev.alloc(4 * N)
            for k in range(len(u)):
                wts = [u[(k + 3 * c) % len(u)] for c in range(W)]
                eng.dev_combine_columns(d_cols, W, N, N, dev.upload_u64(wts), d_out)
                want = sum(cols[c] * np.uint64(wts[c] % p) % np.uint64(p) for c in range(W)) % np.uint64(p)
                assert np.array_equal(eng.dev_download(d_out, N), want), (kind, k)


# ---------------------------------------------------------------------------------------------- end to end, once per boundary
@gpu
@pytest.mark.parametrize("p", THREE)
def test_fri_prove_bytes_equal_the_oracle(engines, oracle, p):
    o, eng, g = oracle, engines[p], GEN[p]
    N, expansion, t = 1 << 12, 4, 8
    omega = o.ff_prim_nth_root_g(N, p, g)
    cw = o.fast_coset_ntt(operands(o, "random", N // expansion, p, 12), N, omega, g, p)
    cfg_o, cfg = o.fri_cfg(omega, g, N, expansion, t, p), eng.fri_cfg(omega, g, N, expansion, t)
    want, want_top = o.fri_prove(cfg_o, cw)
    got, top = eng.fri_prove(cfg, cw)
    assert top == want_top
    assert got == want
    assert o.fri_verify(cfg_o, got), o.fri_last_reject()
    ok, _pv, why = eng.fri_verify(cfg, got)
    assert ok, why


@gpu
@pytest.mark.parametrize("p", THREE)
def test_fri_prove_ext_bytes_equal_the_restatement(engines, oracle, p):
    from test_gpu_ext import gpu_prove, low_degree_codeword
    o, eng, g = oracle, engines[p], GEN[p]
    N, expansion, t = 1 << 10, 4, 6
    cw, omega = low_degree_codeword(o, p, g, N, expansion, g, 10)
    cfg_o, cfg = o.fri_cfg(omega, g, N, expansion, t, p), eng.fri_cfg(omega, g, N, expansion, t)
    want, want_top = xc.prove(o, cfg_o, cw, g, b"prior")
    got, top = gpu_prove(eng, cfg, cw, b"prior")
    assert top == want_top
    assert got == want
    ok, _pv, used, why = eng.fri_verify_ext(cfg, got, b"prior")
    assert ok and used == len(got), why
    assert xc.verify(o, cfg_o, got, g, b"prior")[0]


@gpu
@pytest.mark.parametrize("p", THREE)
def test_air_prove_ext_bytes_equal_the_restatement(engines, oracle, p):
    from test_gpu_ext import restated_air_proof
    o, eng, g, log_n, lb, t = oracle, engines[p], GEN[p], 8, 3, 4
    air, cols = ac.make("mixer", 1 << log_n, p)
    W = len(cols)
    _d, expansion = eng.air_plan(air, W, log_n, lb)
    with Dev(eng) as dev:
        res = eng.dev_air_prove(air, dev.upload(np.array(cols, dtype=np.uint64)), W, log_n, lb, t, row_leaves=True, ext=True)
    root, want, top = restated_air_proof(o, air, cols, p, g, log_n, lb, t, 1, g, expansion)
    assert bytes(res["column_roots"][0]) == root
    assert res["top_indices"] == top
    assert res["proof"] == want
    ok, why = eng.air_verify(air, res["proof"], res["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True)
    assert ok, why


@gpu
def test_a_modulus_outside_the_bound_is_refused(engines):
    """before anything is launched: field_setup refuses a prime above 2^30 and a composite below it"""
    import stark_rs_amd as s
    for n, g in ((FIRST_ABOVE_2_30, 2), (_composite_below_2_30(), 3)):
        with pytest.raises(s.StarkMiError) as ei:
            s.Engine(n, g, 0)
        assert ei.value.status == UNSUPPORTED_PRIME, n
    p = TABLE[0][1]
    assert engines[p].mul(p - 1, p - 1) == 1                     # a context next to the refusals goes on working
