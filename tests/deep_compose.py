"""The checker of out-of-domain sampling (include/stark_mi.h, "Out-of-domain sampling"), restated in Python ints and numpy
over the CPU oracle's primitives and the existing routes: the composition per coordinate by ap.route / ap.fast_route, the
segments by o.fast_intt / o.fast_coset_ntt, the out-of-domain values by Horner over F_q, the DEEP codeword from its formula,
extension FRI with grinding at E = B (pc.prove / pc.verify), the row openings of tests/air_rows.py, and the verifier with the
constraints evaluated over F_q operands.
Not a test module: imported by tests/test_deep_host.py, tests/test_deep_emu.py, tests/test_gpu_deep.py and
tests/test_gpu_boundary_primes_deep.py."""
import numpy as np

import air_compose as ac
import air_periodic as ap
import air_rows as ar
import ext_compose as xc
import perm_compose as pm
import pow_compose as pc

# reason class of the restated verifier -> a keyword of the library's sentence for it
KEYWORD = {"record": "out-of-domain record", "record canonical": "out-of-domain coordinate is not canonical", "base field": "base field",
           "consistency": "consistency check fails", "no layer": "no fold", "length": "deep openings: wrong length",
           "row": "deep openings: malformed row", "path": "deep openings: malformed path", "auth": "authentication path does not verify",
           "canonical": "deep openings: an opened value is not canonical", "quotient": "DEEP quotient"}


# reason of the restated FRI verifier (pc.verify, reported here as "fri: <reason>") -> a keyword of the library's sentence
FRI_KEYWORD = {"root": "Merkle root", "last codeword": "last codeword", "canonical": "not canonical", "last root": "not well formed",
               "degree": "low enough degree", "nonce record": "nonce", "proof of work": "proof of work", "triple": "triple",
               "colinearity": "colinearity", "path": "path"}


def keyword(reason):
    """the keyword the library's sentence must hold for a reason class of verify()"""
    return FRI_KEYWORD[reason[5:]] if reason.startswith("fri: ") else KEYWORD[reason]


def compose_combos(log_N):
    """(log_blowup, W, D) for the point-function tests at N = 2^log_N: four combinations that rotate with the size, and one
    more; over log_N = 10 .. 16 they take every B in {4, 8, 16}, W in {1, 4, 12, 64} and D in {1, 2, 4, 16}"""
    r = log_N % 4
    Ws, Ds = [1, 4, 12, 64], [1, 2, 4, 16]
    return [(2 + (i + r) % 3, Ws[i], Ds[(i + r) % 4]) for i in range(4)] + [(2 + r % 3, Ws[(r + 1) % 4], Ds[r])]


def plan(air):
    """-> (d, D): the degree and the number of segments, D the smallest power of two >= max(1, d - 1)"""
    d, D = air.degree, 1
    while D < d - 1:
        D <<= 1
    return d, D


# ---------------------------------------------------------------------------------------------- F_q helpers
def scale_q(a, k, p):
    return [x * k % p for x in a]


def horner(coeffs, z, p, g):
    """sum_i coeffs[i] z^i; a coefficient is an int (base field) or four ints"""
    acc = [0, 0, 0, 0]
    for a in reversed(coeffs):
        acc = xc.mul(acc, z, p, g)
        acc = xc.add(acc, a, p) if isinstance(a, (list, tuple)) else [(acc[0] + int(a)) % p] + acc[1:]
    return acc


def _mul_const(a, b, p, g):
    """a: (4, ...) uint64 residues times the four ints b; every partial sum stays below 2^64 for p < 2^30"""
    P = np.uint64(p)
    bb = [np.uint64(v % p) for v in b]
    gb = [np.uint64(g * int(v) % p) for v in bb]
    out = np.zeros_like(a)
    for k in range(4):
        acc = np.zeros(a.shape[1:], dtype=np.uint64)
        for i in range(4):
            acc += a[i] * (bb[k - i] if i <= k else gb[k + 4 - i]) % P
        out[k] = acc % P
    return out


def eval_cols(cols, z, p, g):
    """every row of cols (m, n) as a polynomial at z, by halving: f(z) = f_even(z^2) + z f_odd(z^2) on arrays
    -> [[c0..c3] per column].  tests/test_deep_host.py pins it to horner."""
    cols = np.asarray(cols, dtype=np.uint64)
    m, n = cols.shape
    L = 1
    while L < n:
        L <<= 1
    a = np.zeros((4, m, L), dtype=np.uint64)
    a[0, :, :n] = cols % np.uint64(p)
    zp = [int(v) % p for v in z]
    while L > 1:
        a = (a[:, :, 0::2] + _mul_const(np.ascontiguousarray(a[:, :, 1::2]), zp, p, g)) % np.uint64(p)
        zp = xc.mul(zp, zp, p, g)
        L >>= 1
    return [[int(a[e, c, 0]) for e in range(4)] for c in range(m)]


def inv_vec(a, p, g):
    """elementwise inverse of a (4, n) array of non-zero elements through the tower F_p < F_p[Y]/(Y^2 - g) < F_q, Y = X^2;
    tests/test_deep_host.py pins it to xc.inv (a^(q - 2))"""
    P, G = np.uint64(p), np.uint64(g)
    mul = lambda x, y: x * y % P

    def qmul(x, y):     # (u + v Y)(u' + v' Y)
        return (mul(x[0], y[0]) + mul(G, mul(x[1], y[1]))) % P, (mul(x[0], y[1]) + mul(x[1], y[0])) % P
    A, B = (a[0], a[2]), (a[1], a[3])
    A2, B2 = qmul(A, A), qmul(B, B)
    Du, Dv = (A2[0] + P - mul(G, B2[1])) % P, (A2[1] + P - B2[0]) % P
    norm = (mul(Du, Du) + P - mul(G, mul(Dv, Dv))) % P
    ni = ap._pow_arr(norm, p - 2, p)
    Di = (mul(Du, ni), mul((P - Dv) % P, ni))
    rA, rB = qmul(A, Di), qmul(B, Di)
    return np.stack([rA[0], (P - rB[0]) % P, rA[1], (P - rB[1]) % P])


def points(o, p, g, log_n, lb, h):
    """x_i = h omega_N^i as uint64"""
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    N = 1 << (log_n + lb)
    return xc._powers(wN, N, p) * np.uint64(h) % np.uint64(p)


# ---------------------------------------------------------------------------------------------- the DEEP codeword
def q_codeword(lde, seg, x, z, ood, ch, w_n, p, g):
    """lde: (W, N), seg: (4 D, N), x: the N points, z: four canonical ints, ood: 4 (2 W + D) canonical values, ch: as many
    unreduced challenges -> Q as a (4, N) array, term by term from the formula"""
    lde, seg = np.asarray(lde, dtype=np.uint64), np.asarray(seg, dtype=np.uint64)
    W, D, N, P = lde.shape[0], seg.shape[0] // 4, lde.shape[1], np.uint64(p)
    el = lambda v, i: [int(c) % p for c in v[4 * i:4 * i + 4]]
    n1, n2 = np.zeros((4, N), dtype=np.uint64), np.zeros((4, N), dtype=np.uint64)

    def minus(vals, e4):    # the (4, N) element array vals - e4
        return np.stack([(vals[e] + P - np.uint64(e4[e])) % P for e in range(4)])
    zero = np.zeros(N, dtype=np.uint64)
    for c in range(W):
        f = [lde[c], zero, zero, zero]
        n1 = (n1 + _mul_const(minus(f, el(ood, c)), el(ch, c), p, g)) % P
        n2 = (n2 + _mul_const(minus(f, el(ood, W + c)), el(ch, W + c), p, g)) % P
    for j in range(D):
        n1 = (n1 + _mul_const(minus(seg[4 * j:4 * j + 4], el(ood, 2 * W + j)), el(ch, 2 * W + j), p, g)) % P
    zw = scale_q(z, w_n, p)
    xs = [np.asarray(x, dtype=np.uint64), zero, zero, zero]
    return (pm.mul_vec(n1, inv_vec(minus(xs, z), p, g), p, g) + pm.mul_vec(n2, inv_vec(minus(xs, zw), p, g), p, g)) % P


def q_at(trow, srow, x, z, ood, ch, w_n, p, g):
    """Q(x) from one trace row and one segment row, Python ints"""
    W, D = len(trow), len(srow) // 4
    el = lambda v, i: [int(c) % p for c in v[4 * i:4 * i + 4]]
    n1, n2 = [0] * 4, [0] * 4
    for c in range(W):
        f = xc.embed(int(trow[c]), p)
        n1 = xc.add(n1, xc.mul(el(ch, c), xc.sub(f, el(ood, c), p), p, g), p)
        n2 = xc.add(n2, xc.mul(el(ch, W + c), xc.sub(f, el(ood, W + c), p), p, g), p)
    for j in range(D):
        n1 = xc.add(n1, xc.mul(el(ch, 2 * W + j), xc.sub(el(srow, j), el(ood, 2 * W + j), p), p, g), p)
    d1, d2 = xc.sub(xc.embed(x, p), z, p), xc.sub(xc.embed(x, p), scale_q(z, w_n, p), p)
    return xc.add(xc.mul(n1, xc.inv(d1, p, g), p, g), xc.mul(n2, xc.inv(d2, p, g), p, g), p)


# ---------------------------------------------------------------------------------------------- the transcript
def draw(o, tr, first, count):
    """absorbs first .. first + count - 1 as 8 little-endian bytes with a challenge after each"""
    out = []
    for m in range(first, first + count):
        tr += xc._u64(m)
        out.append(xc.challenge(o, tr))
    return out


def composition(o, air, cols, ch, p, g, log_n, lb, tau, h):
    """H as four coordinate codewords under the 4 (W + K) challenges"""
    if log_n <= 8 or air.degree > 3:
        cw = [ap.route(o, air, cols, xc.weight_vector(ch, e), p, g, log_n, lb, tau, h)[0] for e in range(4)]
    else:
        cw = [ap.fast_route(o, air, cols, xc.weight_vector(ch, e), p, g, log_n, lb, tau, h) for e in range(4)]
    return np.stack([np.asarray(c, dtype=np.uint64) for c in cw])


def segments(o, H, D, p, g, log_n, lb, h):
    """-> (the coefficients of H's coordinates (4, N), the 4 D segment columns (4 D, N))"""
    n, N = 1 << log_n, 1 << (log_n + lb)
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    hc = np.stack([np.asarray(o.fast_intt(H[e], wN, h, p), dtype=np.uint64) for e in range(4)])
    seg = [o.fast_coset_ntt(np.ascontiguousarray(hc[e, j * n:(j + 1) * n]), N, wN, h, p) for j in range(D) for e in range(4)]
    return hc, np.stack([np.asarray(s, dtype=np.uint64) for s in seg])


def ood_values(o, cols, hc, D, z, p, g, log_n, tau):
    """u, v, s as a flat list of 4 (2 W + D) canonical values: Horner over F_q"""
    n = 1 << log_n
    w = o.ff_prim_nth_root_g(n, p, g)
    polys = [[int(v) for v in o.fast_intt(np.array(c, dtype=np.uint64), w, tau, p)] for c in cols]
    zw = scale_q(z, w, p)
    u, v = [horner(q, z, p, g) for q in polys], [horner(q, zw, p, g) for q in polys]
    s = [horner([[int(hc[e, j * n + i]) for e in range(4)] for i in range(n)], z, p, g) for j in range(D)]
    return [c for el in u + v + s for c in el]


def prove(o, air, cols, p, g, log_n, lb, t, tau, h, bits=0):
    """-> dict(roots, proof, top, ood, z, gammas, H, seg, Q) of smi_dev_air_prove_deep"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K = len(cols), len(air.constraints)
    _d, D = plan(air)
    assert D <= B and B >= 4 and 4 * D <= 64
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    lde = ac.lde(o, cols, p, g, log_n, lb, tau, h)
    nodes1 = o.merkle_new(ar.row_leaves(o, lde))
    root1 = bytes(nodes1[-1])
    tr, ch = xc.air_transcript(o, W, K, root1)
    tr = bytearray(tr)
    H = composition(o, air, cols, ch, p, g, log_n, lb, tau, h)
    hc, seg = segments(o, H, D, p, g, log_n, lb, h)
    assert not hc[:, D << log_n:].any(), "the composition has coefficients at or above D n"
    nodes2 = o.merkle_new(ar.row_leaves(o, list(seg)))
    root2 = bytes(nodes2[-1])
    tr += root2
    z = [c % p for c in draw(o, tr, 4 * (W + K), 4)]
    assert any(z[1:]), "z lies in the base field"
    ood = ood_values(o, cols, hc, D, z, p, g, log_n, tau)
    record = xc._elems(ood)
    tr += record[9:]
    gammas = draw(o, tr, 4 * (W + K) + 4, 4 * (2 * W + D))
    assert len(tr) == 32 * (3 + W + K + 2 * (2 * W + D))
    Q = q_codeword(lde, seg, points(o, p, g, log_n, lb, h), z, ood, gammas, w, p, g)
    cfg_o = o.fri_cfg(wN, h, N, B, t, p)
    fri, top, _nonce = pc.prove(o, cfg_o, Q, g, bytes(tr), bits)
    proof = record + fri + ar.openings_bytes(o, lde, top, N, B, False, nodes1) + ar.openings_bytes(o, list(seg), top, N, B, False, nodes2)
    return {"roots": [root1, root2], "proof": proof, "top": top, "ood": ood, "z": z, "gammas": gammas, "H": H, "seg": seg, "Q": Q, "lde": lde}


def proof_len(o, W, D, log_n, lb, t, p, g, h):
    N, B, log_N = 1 << (log_n + lb), 1 << lb, log_n + lb
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    R = o.fri_num_rounds(o.fri_cfg(wN, h, N, B, t, p))
    return (9 + 32 * (2 * W + D) + pc.proof_len(N, B, t, R) + 2 * t * (9 + 8 * W) + 2 * t * (9 + 32 * log_N) + 2 * t * (9 + 32 * D)
            + 2 * t * (9 + 32 * log_N))


# ---------------------------------------------------------------------------------------------- the verifier
def constraint_q(air, k, X, p, g):
    """C_k over F_q operands X[v] (smi_air's numbering)"""
    acc = [0] * 4
    for cf, factors in air.constraints[k]:
        m = xc.embed(cf % p, p)
        for v, e in factors:
            m = xc.mul(m, xc.power(X[v], e, p, g), p, g)
        acc = xc.add(acc, m, p)
    return acc


def periodic_q(o, air, x, p, g, log_n, tau, w):
    """pi_j(x) = q_j((x / tau)^(n / P_j)) with q_j interpolated on the P_j-th roots of unity, Horner over F_q"""
    n, out = 1 << log_n, []
    for vals in air.periodics:
        P = len(vals)
        wP = pow(w, n // P, p)
        q = o.poly_interpolate_domain([pow(wP, r, p) for r in range(P)], [v % p for v in vals], p) if P > 1 else [vals[0] % p]
        y = xc.power(scale_q(x, pow(tau, p - 2, p), p), n // P, p, g)
        out.append(horner([int(c) for c in q], y, p, g))
    return out


def ood_sides(o, air, W, D, weights, z, ood, p, g, log_n, tau):
    """-> (sum_c w_c term_c(z) + sum_k w_{W+k} tq_k(z), sum_j z^(j n) s_j)"""
    n, K = 1 << log_n, len(air.constraints)
    w = o.ff_prim_nth_root_g(n, p, g)
    el = lambda v, i: [int(c) % p for c in v[4 * i:4 * i + 4]]
    u, v, s = [el(ood, c) for c in range(W)], [el(ood, W + c) for c in range(W)], [el(ood, 2 * W + j) for j in range(D)]
    acc = [0] * 4
    for c in range(W):
        pts = [(tau * pow(w, r, p) % p, val % p) for (cc, r, val) in air.boundaries if cc == c]
        term = u[c]
        if pts:
            interp = [int(x) for x in o.poly_interpolate_domain([r for r, _ in pts], [val for _, val in pts], p)]
            zc = xc.embed(1, p)
            for r, _ in pts:
                zc = xc.mul(zc, xc.sub(z, xc.embed(r, p), p), p, g)
            term = xc.mul(xc.sub(u[c], horner(interp, z, p, g), p), xc.inv(zc, p, g), p, g)
        acc = xc.add(acc, xc.mul(el(weights, c), term, p, g), p)
    if K:
        zw = scale_q(z, w, p)
        X = u + v + periodic_q(o, air, z, p, g, log_n, tau, w) + periodic_q(o, air, zw, p, g, log_n, tau, w)
        zt = xc.mul(xc.sub(z, xc.embed(tau * pow(w, n - 1, p) % p, p), p),
                    xc.inv(xc.sub(xc.power(z, n, p, g), xc.embed(pow(tau, n, p), p), p), p, g), p, g)
        for k in range(K):
            acc = xc.add(acc, xc.mul(el(weights, W + k), xc.mul(constraint_q(air, k, X, p, g), zt, p, g), p, g), p)
    rhs, zn, pw = [0] * 4, xc.power(z, n, p, g), xc.embed(1, p)
    for j in range(D):
        rhs = xc.add(rhs, xc.mul(pw, s[j], p, g), p)
        pw = xc.mul(pw, zn, p, g)
    return acc, rhs


def _section(o, sec, width, log_N, positions, root):
    """one opening section -> (rows, None) or (None, reason class): every row's tag and width, every path's, then the paths"""
    rec, prec, m = 9 + 8 * width, 9 + 32 * log_N, len(positions)
    rows = []
    for q in range(m):
        r = sec[q * rec:(q + 1) * rec]
        if r[0] != 2 or int.from_bytes(r[1:9], "little") != width:
            return None, "row"
        rows.append([int.from_bytes(r[9 + 8 * c:17 + 8 * c], "little") for c in range(width)])
    for q in range(m):
        pr = sec[m * rec + q * prec:m * rec + (q + 1) * prec]
        if pr[0] != 3 or int.from_bytes(pr[1:9], "little") != log_N:
            return None, "path"
    return rows, None


def _auth(o, sec, width, log_N, positions, root):
    rec, prec, m = 9 + 8 * width, 9 + 32 * log_N, len(positions)
    for q in range(m):
        pr = sec[m * rec + q * prec:m * rec + (q + 1) * prec]
        path = [bytes(pr[9 + 32 * i:41 + 32 * i]) for i in range(log_N)]
        if not o.merkle_verify(o.hash_from_bytes(bytes(sec[q * rec + 9:(q + 1) * rec])), positions[q], path, root):
            return False
    return True


def verify(o, air, proof, roots, p, g, W, log_n, lb, t, tau, h, bits=0):
    """-> (accept, reason class) of smi_air_verify_deep, in its order"""
    N, B, log_N, K = 1 << (log_n + lb), 1 << lb, log_n + lb, len(air.constraints)
    _d, D = plan(air)
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cnt = 4 * (2 * W + D)
    obj = xc._pop(proof, 0)
    if obj is None or obj[0] != 2 or len(obj[1]) != cnt:
        return False, "record"
    ood, at = obj[1], obj[2]
    if any(v >= p for v in ood):
        return False, "record canonical"
    tr, weights = xc.air_transcript(o, W, K, bytes(roots[0]))
    tr = bytearray(tr) + bytes(roots[1])
    z = [c % p for c in draw(o, tr, 4 * (W + K), 4)]
    if not any(z[1:]):
        return False, "base field"
    tr += proof[9:at]
    gammas = draw(o, tr, 4 * (W + K) + 4, cnt)
    lhs, rhs = ood_sides(o, air, W, D, weights, z, ood, p, g, log_n, tau)
    if lhs != rhs:
        return False, "consistency"
    cfg_o = o.fri_cfg(wN, h, N, B, t, p)
    ok, pv, used, top, why = pc.verify(o, cfg_o, proof[at:], g, bytes(tr), bits)
    if not ok:
        return False, "fri: " + why
    if len(pv) != 2 * t:
        return False, "no layer"
    rest = proof[at + used:]
    m = 2 * t
    lens = [m * (9 + 8 * W) + m * (9 + 32 * log_N), m * (9 + 32 * D) + m * (9 + 32 * log_N)]
    if len(rest) != sum(lens):
        return False, "length"
    secs, widths = [rest[:lens[0]], rest[lens[0]:]], [W, 4 * D]
    pos = [i for s in top for i in ar.positions(s, N, B, False)]
    rows = []
    for v in range(2):
        r, why = _section(o, secs[v], widths[v], log_N, pos, roots[v])
        if r is None:
            return False, why
        rows.append(r)
    for v in range(2):
        if not _auth(o, secs[v], widths[v], log_N, pos, bytes(roots[v])):
            return False, "auth"
    if any(x >= p for r in rows for row in r for x in row):
        return False, "canonical"
    for q, i in enumerate(pos):
        x = h * pow(wN, i, p) % p
        if q_at(rows[0][q], rows[1][q], x, z, ood, gammas, w, p, g) != [int(c) for c in pv[q][1]] or pv[q][0] != i:
            return False, "quotient"
    return True, ""
