"""The checker of the permutation argument (include/stark_mi.h, "Permutation argument"), restated in Python from the CPU
oracle's primitives: the column z from its definition, the two auxiliary quotients point by point, the transcript of the two
roots, the prover and the verifier.  Built on tests/ext_compose.py (mul, inv, mul_arr, the FRI stream helpers),
tests/pow_compose.py (extension FRI with a nonce record) and tests/air_rows.py (row leaves, the opening section).
Not a test module: imported by tests/test_perm_host.py, tests/test_perm_emu.py and tests/test_gpu_perm.py."""
import numpy as np

import air_compose as ac
import air_periodic as ap
import air_rows as ar
import ext_compose as xc
import pow_compose as pw

ONE = [1, 0, 0, 0]


def alpha_gamma(ch, p):
    """the 8 unreduced challenges -> (alpha, gamma), four canonical coordinates each"""
    return [int(c) % p for c in ch[:4]], [int(c) % p for c in ch[4:8]]


def alpha_powers(alpha, m, p, g):
    out, pw_ = [], list(ONE)
    for _ in range(m):
        out.append(pw_)
        pw_ = xc.mul(pw_, alpha, p, g)
    return out


def tuple_value(row, cols_idx, apow, gamma, p):
    """gamma + sum_j alpha^j * row[cols_idx[j]]: an F_q element times a base-field cell is a scaling"""
    f = list(gamma)
    for j, c in enumerate(cols_idx):
        f = xc.add(f, xc.scale(apow[j], int(row[c]) % p, p), p)
    return f


# ---------------------------------------------------------------------------------------------- the column
def column(cols, left, right, ch, p, g):
    """-> (z as a (4, n) uint64 array, closes, None) or (None, None, the smallest row with f_R = 0).
    z[r] = prod_{i<r} f_L(i) / prod_{i<r} f_R(i), straight from the definition; the n denominators' inverses come from ONE
    inversion of their product walked back down (q^-1 of a prefix = q^-1 of the next prefix times the factor between them)."""
    n = len(cols[0])
    alpha, gamma = alpha_gamma(ch, p)
    apow = alpha_powers(alpha, len(left), p, g)
    fl = [tuple_value([c[r] for c in cols], left, apow, gamma, p) for r in range(n)]
    fr = [tuple_value([c[r] for c in cols], right, apow, gamma, p) for r in range(n)]
    zeros = [r for r in range(n) if not any(fr[r])]
    if zeros:
        return None, None, zeros[0]
    num, den = [list(ONE)], [list(ONE)]                         # prefix products, num[r] = prod_{i<r}
    for r in range(n):
        num.append(xc.mul(num[-1], fl[r], p, g))
        den.append(xc.mul(den[-1], fr[r], p, g))
    inv = xc.inv(den[n], p, g)
    closes = xc.mul(num[n], inv, p, g) == ONE
    z = np.zeros((4, n), dtype=np.uint64)
    for r in range(n, 0, -1):                                   # inv = 1 / den[r]
        inv = xc.mul(inv, fr[r - 1], p, g)                      # 1 / den[r - 1]
        z[:, r - 1] = xc.mul(num[r - 1], inv, p, g)
    return z, closes, None


def mul_vec(a, b, p, g):
    """elementwise product of two (4, n) uint64 arrays of residues; four products below 2^60 each sum below 2^64"""
    P, G = np.uint64(p), np.uint64(g)
    out = np.zeros_like(a)
    for k in range(4):
        lo = np.zeros(a.shape[1], dtype=np.uint64)
        hi = np.zeros(a.shape[1], dtype=np.uint64)
        for i in range(4):
            if i <= k:
                lo += a[i] * b[k - i] % P
            else:
                hi += a[i] * b[k + 4 - i] % P
        out[k] = (lo + hi % P * G) % P
    return out


def tuples_vec(cols, cols_idx, ch, p, g):
    """f(r) for every row as a (4, n) array; cols: (W, n) uint64"""
    alpha, gamma = alpha_gamma(ch, p)
    apow = alpha_powers(alpha, len(cols_idx), p, g)
    cols = np.asarray(cols, dtype=np.uint64)
    f = np.zeros((4, cols.shape[1]), dtype=np.uint64)
    for e in range(4):
        acc = np.full(cols.shape[1], gamma[e], dtype=np.uint64)
        for j, c in enumerate(cols_idx):
            acc = (acc + cols[c] * np.uint64(apow[j][e]) % np.uint64(p)) % np.uint64(p)
        f[e] = acc
    return f


def recurrence_holds(z, cols, left, right, ch, p, g):
    """z[0] == 1 and z[r+1] f_R[r] == z[r] f_L[r] for r < n - 1: with every f_R != 0 this determines z"""
    z = np.asarray(z, dtype=np.uint64)
    fl, fr = tuples_vec(cols, left, ch, p, g), tuples_vec(cols, right, ch, p, g)
    if [int(v) for v in z[:, 0]] != ONE:
        return False
    return bool(np.array_equal(mul_vec(z[:, 1:], fr[:, :-1], p, g), mul_vec(z[:, :-1], fl[:, :-1], p, g)))


def gamma_for_zero(cols, right, ch, row, p, g):
    """the challenges with gamma replaced so that f_R(row) = 0: gamma = -sum_j alpha^j T[r_j][row]"""
    alpha, _ = alpha_gamma(ch, p)
    apow = alpha_powers(alpha, len(right), p, g)
    s = tuple_value([c[row] for c in cols], right, apow, [0, 0, 0, 0], p)
    return list(ch[:4]) + [(p - v) % p for v in s]


# ---------------------------------------------------------------------------------------------- the auxiliary quotients
def point_inverses(idx, p, wN, log_n, tau, h):
    """-> (1 / (x_i - tau), 1 / (x_i^n - tau^n)) for the points i of idx as uint64 arrays, x_i = h wN^i by one pow per point"""
    n, tn = 1 << log_n, pow(tau, 1 << log_n, p)
    x = [h * pow(wN, int(i), p) % p for i in idx]
    ixt = np.array([pow((xi - tau) % p, p - 2, p) for xi in x], dtype=np.uint64)
    izt = np.array([pow((pow(xi, n, p) - tn) % p, p - 2, p) for xi in x], dtype=np.uint64)
    return ixt, izt


def aux_terms_at(idx, lde_at, z_at, z_next, left, right, ch, wb, wt, p, g, wN, log_n, tau, h):
    """w_b (z(x_i) - 1) / (x_i - tau) + w_t (z(w x_i) f_R(x_i) - z(x_i) f_L(x_i)) / (x_i^n - tau^n) at the points i of idx
    alone, as (4, len(idx)).  lde_at: (W, len(idx)) the extended trace columns at idx; z_at, z_next: (4, len(idx)) the extended
    column z at idx and at (idx + B) mod N; wN: the N-th root of unity of the evaluation domain; wb, wt: four unreduced ints
    each.  Nothing here is as long as N: the cost is per sampled point"""
    P = np.uint64(p)
    lde_at, z_at, z_next = (np.asarray(a, dtype=np.uint64) for a in (lde_at, z_at, z_next))
    ixt, izt = point_inverses(idx, p, wN, log_n, tau, h)
    fl, fr = tuples_vec(lde_at, left, ch, p, g), tuples_vec(lde_at, right, ch, p, g)
    tq = (mul_vec(z_next, fr, p, g) + P - mul_vec(z_at, fl, p, g)) % P * izt % P
    zm = z_at.copy()
    zm[0] = (zm[0] + P - np.uint64(1)) % P
    bq = zm * ixt % P
    return (xc.mul_arr(bq, [int(v) % p for v in wb], p, g) + xc.mul_arr(tq, [int(v) % p for v in wt], p, g)) % P


def aux_terms(o, lde, zl, left, right, ch, wb, wt, p, g, log_n, lb, tau, h):
    """aux_terms_at for every i, as (4, N); lde: (W, N), zl: (4, N) extended columns"""
    B, N = 1 << lb, 1 << (log_n + lb)
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    zl = np.asarray(zl, dtype=np.uint64)
    return aux_terms_at(np.arange(N), lde, zl, np.roll(zl, -B, axis=1), left, right, ch, wb, wt, p, g, wN, log_n, tau, h)


def main_codeword(o, air, cols, ch_w, p, g, log_n, lb, tau, h, honest=True):
    """smi_dev_air_compose_ext's codeword under the 4 (W + K) challenges ch_w, coordinate by coordinate by the polynomial route"""
    if log_n <= 8:
        cw = [ap.route(o, air, cols, xc.weight_vector(ch_w, e), p, g, log_n, lb, tau, h, want_zero_remainder=honest)[0] for e in range(4)]
    else:
        cw = [ap.fast_route(o, air, cols, xc.weight_vector(ch_w, e), p, g, log_n, lb, tau, h) for e in range(4)]
    return np.stack([np.asarray(c, dtype=np.uint64) for c in cw])


# ---------------------------------------------------------------------------------------------- transcript, prover, verifier
def challenges(o, root1):
    """-> (transcript after the 8 challenges, the 8 unreduced challenges)"""
    tr, ch = bytearray(bytes(root1)), []
    for m in range(8):
        tr += xc._u64(m)
        ch.append(xc.challenge(o, tr))
    return tr, ch


def weights(o, tr, root2, n_weights):
    """absorbs root_2, then 8 + m for m < 4 n_weights with a challenge after each -> (transcript, challenges)"""
    tr = bytearray(tr) + bytes(root2)
    out = []
    for m in range(4 * n_weights):
        tr += xc._u64(8 + m)
        out.append(xc.challenge(o, tr))
    return tr, out


def transcript_len(W, K):
    return 32 + 64 + 32 + 32 * (W + K + 2)


def opening_len(W, log_N, t):
    return t * 4 * (9 + 8 * W) + t * 4 * (9 + 32 * log_N) + t * 4 * (9 + 32) + t * 4 * (9 + 32 * log_N)


def proof_len(N, E, t, R, W):
    return pw.proof_len(N, E, t, R) + opening_len(W, N.bit_length() - 1, t)


def prove(o, air, left, right, cols, p, g, log_n, lb, t, tau, h, E, bits, honest=True, z_plus_p=None, trace_plus_p=None):
    """-> dict(roots, proof, top, nonce, closes, ch, z) of smi_dev_air_prove_perm from the oracle's primitives.
    z_plus_p = e / trace_plus_p = c: a dishonest prover that COMMITS and opens coordinate e of the extended z / extended trace
    column c with p added to every value (the codeword is the honest one): every path verifies, no such value is canonical"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K = len(cols), len(air.constraints)
    lde = ac.lde(o, cols, p, g, log_n, lb, tau, h)
    shown = [np.asarray(c, dtype=np.uint64) + np.uint64(p if c_i == trace_plus_p else 0) for c_i, c in enumerate(lde)]
    nodes1 = o.merkle_new(ar.row_leaves(o, shown))
    root1 = bytes(nodes1[-1])
    tr, ch = challenges(o, root1)
    z, closes, zero = column(cols, left, right, ch, p, g)
    assert zero is None, zero
    zl = ac.lde(o, [[int(v) for v in z[e]] for e in range(4)], p, g, log_n, lb, tau, h)
    zshown = [np.asarray(c, dtype=np.uint64) + np.uint64(p if e == z_plus_p else 0) for e, c in enumerate(zl)]
    nodes2 = o.merkle_new(ar.row_leaves(o, zshown))
    root2 = bytes(nodes2[-1])
    tr, wch = weights(o, tr, root2, W + K + 2)
    assert len(tr) == transcript_len(W, K)
    cw = main_codeword(o, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h, honest)
    cw = (cw + aux_terms(o, lde, zl, left, right, ch, wch[4 * (W + K):4 * (W + K) + 4], wch[4 * (W + K) + 4:], p, g, log_n, lb, tau, h)) % np.uint64(p)
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    fri, top, nonce = pw.prove(o, cfg_o, cw, g, bytes(tr), bits)
    proof = fri + ar.openings_bytes(o, shown, top, N, B, True, nodes1) + ar.openings_bytes(o, zshown, top, N, B, True, nodes2)
    return dict(roots=root1 + root2, proof=proof, top=top, nonce=nonce, closes=closes, ch=ch, z=z, cw=cw)


def _section(o, sec, width, log_N, positions, root, p):
    """one opening section -> (rows, None) or (None, reason class)"""
    rec, prec, m = 9 + 8 * width, 9 + 32 * log_N, len(positions)
    rows = []
    for q in range(m):
        r = sec[q * rec:(q + 1) * rec]
        pr = sec[m * rec + q * prec:m * rec + (q + 1) * prec]
        if r[0] != 2 or int.from_bytes(r[1:9], "little") != width or pr[0] != 3 or int.from_bytes(pr[1:9], "little") != log_N:
            return None, "record"
        rows.append([int.from_bytes(r[9 + 8 * c:17 + 8 * c], "little") for c in range(width)])
    for q in range(m):
        pr = sec[m * rec + q * prec:m * rec + (q + 1) * prec]
        path = [bytes(pr[9 + 32 * i:41 + 32 * i]) for i in range(log_N)]
        if not o.merkle_verify(o.hash_from_bytes(bytes(sec[q * rec + 9:(q + 1) * rec])), positions[q], path, root):
            return None, "path"
    return rows, None


def verify(o, air, left, right, roots, proof, p, g, log_n, lb, t, tau, h, E, bits):
    """-> (accept, reason class): "fri" | "length" | "record" | "path" | "canonical" | "composition" | "" """
    n, B = 1 << log_n, 1 << lb
    N, log_N = n * B, log_n + lb
    W, K = air.n_cols, len(air.constraints)
    root1, root2 = bytes(roots[:32]), bytes(roots[32:64])
    tr, ch = challenges(o, root1)
    tr, wch = weights(o, tr, root2, W + K + 2)
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    ok, pv, used, top, _why = pw.verify(o, cfg_o, proof, g, bytes(tr), bits)
    if not ok:
        return False, "fri"
    rest = proof[used:]
    if len(rest) != opening_len(W, log_N, t):
        return False, "length"
    positions = [i for s in top for i in ar.positions(s, N, B, True)]
    len1 = t * 4 * (9 + 8 * W) + t * 4 * (9 + 32 * log_N)
    # tags and widths of both sections before any path
    for sec, width in ((rest[:len1], W), (rest[len1:], 4)):
        rec, prec, m = 9 + 8 * width, 9 + 32 * log_N, 4 * t
        for q in range(m):
            if sec[q * rec] != 2 or int.from_bytes(sec[q * rec + 1:q * rec + 9], "little") != width:
                return False, "record"
            at = m * rec + q * prec
            if sec[at] != 3 or int.from_bytes(sec[at + 1:at + 9], "little") != log_N:
                return False, "record"
    rows, why = _section(o, rest[:len1], W, log_N, positions, root1, p)
    if rows is None:
        return False, why
    zrows, why = _section(o, rest[len1:], 4, log_N, positions, root2, p)
    if zrows is None:
        return False, why
    if any(v >= p for r in rows + zrows for v in r):
        return False, "canonical"
    alpha, gamma = alpha_gamma(ch, p)
    apow = alpha_powers(alpha, len(left), p, g)
    wb = [c % p for c in wch[4 * (W + K):4 * (W + K) + 4]]
    wt = [c % p for c in wch[4 * (W + K) + 4:4 * (W + K) + 8]]
    tn = pow(tau, n, p)
    for s in range(t):
        for k in range(2):
            i = positions[4 * s + k]
            cur, nxt, zc, zn = rows[4 * s + k], rows[4 * s + k + 2], zrows[4 * s + k], zrows[4 * s + k + 2]
            x = h * pow(wN, i, p) % p
            got = [air.compose_at(p, log_n, lb, tau, h, wN, i, cur, nxt, xc.weight_vector(wch[:4 * (W + K)], e)) for e in range(4)]
            fl, fr = tuple_value(cur, left, apow, gamma, p), tuple_value(cur, right, apow, gamma, p)
            tq = xc.scale(xc.sub(xc.mul(zn, fr, p, g), xc.mul(zc, fl, p, g), p), pow((pow(x, n, p) - tn) % p, p - 2, p), p)
            bq = xc.scale(xc.sub(zc, ONE, p), pow((x - tau) % p, p - 2, p), p)
            got = xc.add(got, xc.add(xc.mul(bq, wb, p, g), xc.mul(tq, wt, p, g), p), p)
            if got != [v % p for v in pv[2 * s + k][1]]:
                return False, "composition"
    return True, ""


REASON_CLASS = [                         # the library's sentence (smi_last_error) -> the restatement's class
    ("perm openings: wrong length", "length"),
    ("perm openings: malformed", "record"),
    ("perm openings: authentication path", "path"),
    ("perm openings: an opened value is not canonical", "canonical"),
    ("perm openings: the composition", "composition"),
]


def reason_class(sentence):
    for head, cls in REASON_CLASS:
        if sentence.startswith(head):
            return cls
    return "fri" if sentence else ""


# ---------------------------------------------------------------------------------------------- traces
def shuffled_copy(n, m, p, seed=5, extra=1):
    """-> (cols, left, right): m random columns, m columns that hold the same tuples in another row order, `extra` random
    columns behind them"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, p, (m, n), dtype=np.int64)
    perm = rng.permutation(n)
    cols = [[int(v) for v in src[j]] for j in range(m)] + [[int(v) for v in src[j][perm]] for j in range(m)]
    cols += [[int(v) for v in rng.integers(0, p, n)] for _ in range(extra)]
    return cols, list(range(m)), list(range(m, 2 * m))


def non_closing(kind, n, p, seed=5):
    """-> (cols, left, right) whose multisets differ: "cell" one changed cell; "multiplicity" equal sets with different
    multiplicities; "columnwise" m = 2 with the two right columns shuffled independently (column-wise a permutation,
    tuple-wise not: the case that tests alpha)"""
    rng = np.random.default_rng(seed)
    if kind == "cell":
        cols, left, right = shuffled_copy(n, 1, p, seed)
        cols[1][n // 2] = (cols[1][n // 2] + 1) % p
        return cols, left, right
    if kind == "multiplicity":
        a = [int(v) for v in rng.integers(0, p, n // 2)]
        left_col = a + a                                        # every value twice
        right_col = a + [a[0]] * (n // 2)                       # the same set, other multiplicities (n >= 4)
        return [left_col, right_col], [0], [1]
    if kind == "columnwise":
        src = rng.integers(0, p, (2, n), dtype=np.int64)
        cols = [[int(v) for v in src[0]], [int(v) for v in src[1]], [int(v) for v in src[0][rng.permutation(n)]], [int(v) for v in src[1][rng.permutation(n)]]]
        return cols, [0, 1], [2, 3]
    raise ValueError(kind)


def with_permutation(air, cols, m, p, seed=9, spoil=False):
    """widens (air, cols) by m columns that hold the tuples of the first m columns in another row order and states that
    permutation; spoil: one cell of the copy is changed, so the product does not close (the AIR itself stays satisfied)"""
    W, n = len(cols), len(cols[0])
    order = np.random.default_rng(seed).permutation(n)
    new = [[cols[j][int(r)] for r in order] for j in range(m)]
    if spoil:
        new[0][n // 3] = (new[0][n // 3] + 1) % p
    air.n_cols = W + m
    air.permutation(list(range(m)), list(range(W, W + m)))
    return air, [list(c) for c in cols] + new


def cubic(n, p, seed=21):
    """x' = x^3 + 1 on one column next to a random one: a degree-3 AIR with K = 1, so D = 2 and FRI runs at B / 2"""
    from stark_rs_amd.mirror import Air
    rng = np.random.default_rng(seed)
    x = [int(rng.integers(0, p))]
    for _ in range(n - 1):
        x.append((pow(x[-1], 3, p) + 1) % p)
    air = Air(2)
    air.transition({("next", 0): 1, ("cur", 0, 3): -1, (): -1})
    air.boundary(0, 0, x[0])
    return air, [x, [int(v) for v in rng.integers(0, p, n)]]
