"""The AIR feature's checker, from the CPU oracle's primitives only: the four test AIRs with their traces, the
composition codeword by the polynomial route (interpolate the columns, compose each constraint with poly_mul /
poly_add, divide by the zerofiers with a zero remainder, weight, evaluate on the coset), the Fiat-Shamir transcript
of smi_dev_air_prove and the oracle-side restatement of its openings.
Not a test module: imported by tests/test_air_emu.py and tests/test_gpu_air.py."""
import numpy as np

from stark_rs_amd.mirror import Air

PRIMES = [(998244353, 3), (469762049, 3)]


def make(name, n, p, seed=7):
    """-> (Air, columns as lists of ints) for fib | mixer | wide4 | empty"""
    rng = np.random.default_rng(seed)
    if name == "empty":
        W = 4
        return Air(W), [[int(x) for x in rng.integers(0, p, n)] for _ in range(W)]
    if name == "fib":
        a, b = [1], [1]
        for _ in range(n - 1):
            a.append(b[-1])
            b.append((a[-2] + b[-1]) % p)
        air = Air(2)
        air.transition({("next", 0): 1, ("cur", 1): -1})
        air.transition({("next", 1): 1, ("cur", 0): -1, ("cur", 1): -1})
        air.boundary(0, 0, 1).boundary(1, 0, 1).boundary(0, n - 1, a[-1])
        return air, [a, b]
    a, b, c, d = [5], [11], [0], [7]
    for _ in range(n - 1):
        a.append((a[-1] * b[-1] + c[-1]) % p)
        b.append((a[-2] * a[-2] % p * c[-1] + 3 * b[-1]) % p)
        d.append((d[-1] + a[-2] * c[-1]) % p)
        c.append((c[-1] + 1) % p)
    air = Air(4)
    air.transition({("next", 0): 1, (("cur", 0), ("cur", 1)): -1, ("cur", 2): -1})            # a' = a b + c
    air.transition({("next", 1): 1, (("cur", 0, 2), ("cur", 2)): -1, ("cur", 1): -3})        # b' = a^2 c + 3 b
    air.transition({("next", 2): 1, ("cur", 2): -1, (): -1})                                  # c' = c + 1
    air.boundary(0, 0, 5).boundary(1, 0, 11).boundary(2, 0, 0).boundary(2, n - 1, (n - 1) % p).boundary(0, n - 1, a[-1])
    if name == "wide4":
        air.transition({("next", 3): 1, ("cur", 3): -1, (("cur", 0), ("cur", 2)): -1})        # d' = d + a c
        air.boundary(3, 0, 7)
    else:
        assert name == "mixer"
        d = [int(x) for x in rng.integers(0, p, n)]
    return air, [a, b, c, d]


def synthetic(W, K, p, n, seed=11):
    """K degree-2 constraints over W random columns (not satisfied by them: the codeword is still defined point by
    point), two boundary points on every fourth column -- the widest shapes the kernel's tiles and caps meet"""
    rng = np.random.default_rng(seed)
    air = Air(W)
    for k in range(K):
        air.transition({("next", k % W): 1, (("cur", (k + 1) % W), ("cur", (3 * k + 2) % W)): -(k + 1), ("cur", (5 * k) % W, 2): 7, (): k})
    cols = [[int(x) for x in rng.integers(0, p, n)] for _ in range(W)]
    for c in range(0, W, 4):
        air.boundary(c, 0, cols[c][0]).boundary(c, n - 1 - c, cols[c][n - 1 - c])
    return air, cols


def weights_for(air, seed=3):
    """unreduced u64 weights, the top bit set now and then"""
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(1 << 62, (1 << 64) - 1, air.n_cols + len(air.constraints), dtype=np.uint64)]


def roots_of_unity(o, p, g, log_n, log_blowup):
    n, N = 1 << log_n, 1 << (log_n + log_blowup)
    return o.ff_prim_nth_root_g(n, p, g), o.ff_prim_nth_root_g(N, p, g)


def lde(o, cols, p, g, log_n, log_blowup, tau, h):
    w, wN = roots_of_unity(o, p, g, log_n, log_blowup)
    N = 1 << (log_n + log_blowup)
    return [o.fast_coset_ntt(o.fast_intt(np.array(col, dtype=np.uint64), w, tau, p), N, wN, h, p) for col in cols]


def _ints(a):
    return [int(v) for v in a]


def codeword_poly_route(o, air, cols, weights, p, g, log_n, log_blowup, tau, h, want_zero_remainder=True):
    """-> (codeword over the coset, every division's remainder was zero)"""
    n, N = 1 << log_n, 1 << (log_n + log_blowup)
    w, wN = roots_of_unity(o, p, g, log_n, log_blowup)
    polys = [_ints(o.fast_intt(np.array(col, dtype=np.uint64), w, tau, p)) for col in cols]

    def next_row(poly):            # f(w x): coefficient j times w^j
        out, k = [], 1
        for cf in poly:
            out.append(cf * k % p)
            k = k * w % p
        return out
    var = polys + [next_row(q) for q in polys]
    dom = [tau * pow(w, i, p) % p for i in range(n)]
    clean = True
    xn = [0] * (n + 1)
    xn[0], xn[n] = (p - pow(tau, n, p)) % p, 1
    ZT, rem = o.poly_div(xn, [(p - dom[n - 1]) % p, 1], p)
    assert not any(_ints(rem))
    quotients = []
    for c in range(air.n_cols):
        pts = [(r, v) for (cc, r, v) in air.boundaries if cc == c]
        if not pts:
            quotients.append(polys[c])
            continue
        bd = [dom[r] for r, _ in pts]
        interp = _ints(o.poly_interpolate_domain(bd, [v % p for _, v in pts], p))
        q, rem = o.poly_div(_ints(o.poly_sub(polys[c], interp, p)), _ints(o.poly_zerofier(bd, p)), p)
        clean &= not any(_ints(rem))
        quotients.append(_ints(q))
    for con in air.constraints:
        acc = []
        for cf, factors in con:
            m = [cf % p]
            for v, e in factors:
                for _ in range(e):
                    m = _ints(o.poly_mul(m, var[v], p))
            acc = _ints(o.poly_add(acc, m, p))
        q, rem = o.poly_div(acc, _ints(ZT), p)
        clean &= not any(_ints(rem))
        quotients.append(_ints(q))
    comb = []
    for wt, q in zip(weights, quotients):
        comb = _ints(o.poly_add(comb, o.poly_mul(q, [wt % p], p), p))
    if want_zero_remainder:
        assert clean, "a division left a remainder: the trace does not satisfy the AIR"
    return o.fast_coset_ntt(np.array(comb, dtype=np.uint64), N, wN, h, p), clean


def transcript(o, air, column_roots):
    """-> (the 32 W + 8 K transcript bytes FRI continues, the W + K weights)"""
    fs, tr, wts = o.FiatShamir(), bytearray(), []
    for r in column_roots:
        fs.absorb(bytes(r))
        tr += bytes(r)
        wts.append(fs.challenge())
    for k in range(len(air.constraints)):
        b = int(k).to_bytes(8, "little")
        fs.absorb(b)
        tr += b
        wts.append(fs.challenge())
    return bytes(tr), wts


def openings_bytes(o, lde_cols, top, N, B, with_next):
    """smi_dev_air_prove's opening section restated with the oracle: per test the rows at a, b (and a+B, b+B when there
    are transition constraints), then per (test, column) the MerklePaths in the same position order"""
    u64 = lambda v: int(v).to_bytes(8, "little")
    W, half = len(lde_cols), N // 2
    trees = [o.merkle_new(o.leaf_hashes(col)) for col in lde_cols]

    def positions(s):
        a = s % half
        return [a, a + half] + ([(a + B) % N, (a + half + B) % N] if with_next else [])
    out = bytearray()
    for s in top:
        for i in positions(s):
            out += b"\x02" + u64(W) + b"".join(u64(col[i]) for col in lde_cols)
    for s in top:
        for c in range(W):
            for i in positions(s):
                path = o.merkle_open(trees[c], N, i)
                out += b"\x03" + u64(len(path)) + b"".join(bytes(d) for d in path)
    return bytes(out)
