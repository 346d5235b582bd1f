"""The checker of the AIR's periodic columns, from the CPU oracle's primitives only.  A periodic column is, as a
polynomial, the interpolant of its values tiled to the trace length, so the expected codeword of an AIR with W trace and
Q periodic columns is tests/air_compose.codeword_poly_route on the augmented AIR: W + Q trace columns, the Q extra ones
holding v_j[r mod P_j] under weight 0 and without a boundary point.  Here: the example AIRs with their traces and that
augmentation.  Not a test module: imported by tests/test_air_periodic_emu.py and tests/test_gpu_air_periodic.py."""
import numpy as np

import air_compose as ac
from stark_rs_amd.mirror import Air

CASES = [(3, 1, None), (4, 5, 7)]   # (log_blowup, trace_offset, lde_offset or the generator)
NAMES = ["mimc", "switch", "public"]
W_OF = {"mimc": 1, "switch": 2, "public": 4}


def round_constants(period, p, seed=64):
    return [int(x) for x in np.random.default_rng(seed).integers(1, p, period)]


def make(name, n, p, seed=7):
    """-> (Air with periodic columns, trace columns as lists of ints) for mimc | switch | public"""
    rng = np.random.default_rng(seed)
    if name == "mimc":          # x' = (x + k)^3, k of period 64
        ks = round_constants(64, p)
        assert n >= 64
        x = [3]
        for r in range(n - 1):
            x.append(pow(x[-1] + ks[r % 64], 3, p))
        air = Air(1)
        k = air.periodic(ks)
        air.transition({("next", 0): 1, ("cur", 0, 3): -1, (("cur", 0, 2), ("per", k)): -3, (("cur", 0), ("per", k, 2)): -3, ("per", k, 3): -1})
        air.boundary(0, 0, x[0]).boundary(0, n - 1, x[-1])
        return air, [x]
    if name == "switch":        # s = 1: a' = a b; s = 0: a' = a + b.  b' = s a + s' b + 3
        sel = [1, 0]
        a, b = [2], [9]
        for r in range(n - 1):
            s, s1 = sel[r % 2], sel[(r + 1) % 2]
            a.append((a[-1] * b[-1] if s else a[-1] + b[-1]) % p)
            b.append((s * a[-2] + s1 * b[-1] + 3) % p)
        air = Air(2)
        s = air.periodic(sel)
        # a' - s (a b) - (1 - s) (a + b)
        air.transition({("next", 0): 1, (("per", s), ("cur", 0), ("cur", 1)): -1, ("cur", 0): -1, ("cur", 1): -1,
                        (("per", s), ("cur", 0)): 1, (("per", s), ("cur", 1)): 1})
        air.transition({("next", 1): 1, (("per", s), ("cur", 0)): -1, (("per_next", s), ("cur", 1)): -1, (): -3})
        air.boundary(0, 0, 2).boundary(1, 0, 9).boundary(0, n - 1, a[-1])
        return air, [a, b]
    assert name == "public"     # the mixer with a public column u (period n) and a constant step kc (period 1)
    u, kc = [int(v) for v in rng.integers(0, p, n)], 12345
    a, b, c = [5], [11], [0]
    for r in range(n - 1):
        a.append((a[-1] * b[-1] + c[-1] + u[r]) % p)
        b.append((a[-2] * a[-2] % p * c[-1] + 3 * b[-1]) % p)
        c.append((c[-1] + kc) % p)
    d = [int(v) for v in rng.integers(0, p, n)]
    air = Air(4)
    ju, jk = air.periodic(u), air.periodic([kc])
    air.transition({("next", 0): 1, (("cur", 0), ("cur", 1)): -1, ("cur", 2): -1, ("per", ju): -1})   # a' = a b + c + u
    air.transition({("next", 1): 1, (("cur", 0, 2), ("cur", 2)): -1, ("cur", 1): -3})                 # b' = a^2 c + 3 b
    air.transition({("next", 2): 1, ("cur", 2): -1, ("per", jk): -1})                                 # c' = c + kc
    air.boundary(0, 0, 5).boundary(1, 0, 11).boundary(2, 0, 0).boundary(2, n - 1, c[-1]).boundary(0, n - 1, a[-1])
    return air, [a, b, c, d]


def degree4():
    """k^2 x^2: one more than the examples; for smi_air_plan only"""
    air = Air(1)
    k = air.periodic([1, 2])
    return air.transition({("next", 0): 1, (("per", k, 2), ("cur", 0, 2)): -1})


def tiled(values, n, p):
    return [int(values[r % len(values)]) % p for r in range(n)]


def augment(air, cols, weights, p):
    """-> (augmented Air, its W + Q columns, its weights): the periodic columns as trace columns under weight 0"""
    n, W = len(cols[0]), air.n_cols
    aug = air.with_periodic_as_trace()
    return aug, [list(c) for c in cols] + [tiled(v, n, p) for v in air.periodics], list(weights[:W]) + [0] * len(air.periodics) + list(weights[W:])


def route(o, air, cols, weights, p, g, log_n, lb, tau, h, want_zero_remainder=True):
    """the expected codeword of an AIR with periodic columns: the polynomial route on the augmented AIR"""
    aug, acols, awts = augment(air, cols, weights, p)
    return ac.codeword_poly_route(o, aug, acols, awts, p, g, log_n, lb, tau, h, want_zero_remainder)


def _pow_arr(a, e, p):
    """a^e mod p for a uint64 array (p < 2^30: every product fits 64 bits)"""
    out, a = np.ones_like(a), a.copy()
    while e:
        if e & 1:
            out = out * a % np.uint64(p)
        a = a * a % np.uint64(p)
        e >>= 1
    return out


def fast_route(o, air, cols, weights, p, g, log_n, lb, tau, h):
    """ac.codeword_poly_route for trace lengths its schoolbook products cannot reach, from the oracle's fast
    transforms: the same polynomials -- interpolate the columns, compose the constraints, divide by the zerofiers,
    weight -- with every product and exact division done pointwise on the coset h <omega_M>, M = 4 n >= the degree of
    any numerator (d <= 3), which does not meet the trace domain.  The combination is brought back to coefficients,
    where the quotients' degree bound (< 2 n) is checked -- a division that left a remainder breaks it -- and then
    evaluated on the evaluation coset.  tests/test_air_periodic_emu.py pins it to codeword_poly_route where both run."""
    P = np.uint64(p)
    aug, acols, awts = augment(air, cols, weights, p)
    assert aug.degree <= 3
    n, N, M = 1 << log_n, 1 << (log_n + lb), 4 << log_n
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    wM = o.ff_prim_nth_root_g(M, p, g)
    inv = lambda v: pow(int(v) % p, p - 2, p)
    x = np.ones(M, dtype=np.uint64)
    x[0] = h
    for i in range(1, M):                       # h * wM^i
        x[i] = int(x[i - 1]) * wM % p
    polys = [o.fast_intt(np.array(c, dtype=np.uint64), w, tau, p) for c in acols]
    cur = [o.fast_coset_ntt(q, M, wM, h, p) for q in polys]
    var = cur + [np.roll(c, -(M // n)) for c in cur]          # f(w x): w = wM^(M / n)
    dom = lambda r: tau * pow(w, r, p) % p
    comb = np.zeros(M, dtype=np.uint64)
    for c in range(aug.n_cols):
        pts = [(r, v) for (cc, r, v) in aug.boundaries if cc == c]
        term = cur[c]
        if pts:
            interp = o.poly_interpolate_domain([dom(r) for r, _ in pts], [v % p for _, v in pts], p)
            ix, z = np.zeros(M, dtype=np.uint64), np.ones(M, dtype=np.uint64)
            for cf in reversed([int(v) for v in interp]):
                ix = (ix * x + np.uint64(cf)) % P
            for r, _ in pts:
                z = z * ((x + np.uint64(p - dom(r))) % P) % P
            term = (term + P - ix) % P * _pow_arr(z, p - 2, p) % P
        comb = (comb + np.uint64(awts[c] % p) * term) % P
    xn = _pow_arr(x, n, p)                                     # M / n distinct values
    zt_inv = {int(v): inv(int(v) - pow(tau, n, p)) for v in set(int(v) for v in xn[:M // n])}
    zt = (x + np.uint64(p - dom(n - 1))) % P * np.array([zt_inv[int(v)] for v in xn], dtype=np.uint64) % P
    for k, con in enumerate(aug.constraints):
        acc = np.zeros(M, dtype=np.uint64)
        for cf, factors in con:
            m = np.full(M, cf % p, dtype=np.uint64)
            for v, e in factors:
                for _ in range(e):
                    m = m * var[v] % P
            acc = (acc + m) % P
        comb = (comb + np.uint64(awts[aug.n_cols + k] % p) * (acc * zt % P)) % P
    coeffs = o.fast_intt(comb, wM, h, p)
    assert not coeffs[2 * n:].any(), "a division left a remainder: the trace does not satisfy the AIR"
    return o.fast_coset_ntt(coeffs[:2 * n], N, wN, h, p)


def synthetic(W, Q, K, p, n, seed=11):
    """ac.synthetic (K degree-2 constraints over W random columns, not satisfied by them) with Q periodic columns of
    mixed periods and Q more constraints of degree 3 that use them at this row and the next"""
    air, cols = ac.synthetic(W, K, p, n, seed)
    rng = np.random.default_rng(seed + 1)
    periods = [64, n, 2, 1, 8, n // 2, 4, 64, 16, n, 32, 2, 128, 1, 256, 4][:Q]
    for P in periods:
        air.periodic([int(v) for v in rng.integers(0, p, P)])
    for j in range(Q):
        air.transition({("next", j % W): 1, (("per", j), ("cur", (j + 1) % W), ("per_next", (j + 1) % Q)): -(j + 2), ("per", j, 2): 5,
                        (("per_next", j), ("next", (2 * j + 1) % W)): 3})
    return air, cols


def lanes(periods, p, seed=5):
    """len(periods) lanes x' = (x + k)^3, lane c with its own constants k_c of period periods[c]; lane 0 also reads the
    next row of lane 1's constants"""
    rng = np.random.default_rng(seed)
    air = Air(len(periods))
    for c, P in enumerate(periods):
        k = air.periodic([int(v) for v in rng.integers(0, p, P)])
        assert k == c
    for c in range(len(periods)):
        poly = {("next", c): 1, ("cur", c, 3): -1, (("cur", c, 2), ("per", c)): -3, (("cur", c), ("per", c, 2)): -3, ("per", c, 3): -1}
        if c == 0 and len(periods) > 1:
            poly[(("per_next", 1), ("cur", 0))] = 7
        air.transition(poly)
    return air
