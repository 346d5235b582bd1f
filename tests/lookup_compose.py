"""The checker of the lookup argument (include/stark_mi.h, "Lookup argument"), restated in Python from the CPU oracle's
primitives: the multiplicities with a dict where the lowest row wins, the column s from its definition, the two auxiliary
quotients point by point, the transcript of the two roots, the prover and the verifier.  Built on tests/perm_compose.py (the
tuple values, the transcript and the section parser, which the two arguments share), tests/ext_compose.py, tests/pow_compose.py
and tests/air_rows.py.
Not a test module: imported by tests/test_lookup_host.py, tests/test_lookup_emu.py and tests/test_gpu_lookup.py."""
import numpy as np

import air_compose as ac
import air_rows as ar
import ext_compose as xc
import perm_compose as pm
import pow_compose as pw

ZERO = [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- the multiplicities
def multiplicities(cols, lookup, table):
    """-> (M as a list of n ints, the smallest row whose lookup tuple is in no table row or None).  A tuple that several
    table rows hold is credited to the lowest of them; a missing lookup is not counted."""
    n = len(cols[0])
    first = {}
    for t in range(n):
        first.setdefault(tuple(int(cols[c][t]) for c in table), t)
    M, missing = [0] * n, None
    for r in range(n):
        t = first.get(tuple(int(cols[c][r]) for c in lookup))
        if t is None:
            missing = r if missing is None else missing
        else:
            M[t] += 1
    return M, missing


# ---------------------------------------------------------------------------------------------- the column
def column(cols, lookup, table, mult_col, ch, p, g):
    """-> (s as a (4, n) uint64 array, closes, None) or (None, None, (the smallest row with a zero, "f_L" | "f_T")).
    s[r] = sum_{i<r} (1 / f_L(i) - M[i] / f_T(i)), straight from the definition; the 2 n inverses come from ONE inversion of
    the product of all denominators walked back down."""
    n = len(cols[0])
    alpha, gamma = pm.alpha_gamma(ch, p)
    apow = pm.alpha_powers(alpha, len(lookup), p, g)
    fl = [pm.tuple_value([c[r] for c in cols], lookup, apow, gamma, p) for r in range(n)]
    ft = [pm.tuple_value([c[r] for c in cols], table, apow, gamma, p) for r in range(n)]
    for r in range(n):
        if not any(fl[r]):
            return None, None, (r, "f_L")
        if not any(ft[r]):
            return None, None, (r, "f_T")
    den = [v for r in range(n) for v in (fl[r], ft[r])]
    pre = [list(pm.ONE)]
    for d in den:
        pre.append(xc.mul(pre[-1], d, p, g))
    inv = xc.inv(pre[-1], p, g)
    invs = [None] * (2 * n)
    for i in range(2 * n, 0, -1):                               # inv = 1 / pre[i]
        invs[i - 1] = xc.mul(inv, pre[i - 1], p, g)
        inv = xc.mul(inv, den[i - 1], p, g)
    s = np.zeros((4, n), dtype=np.uint64)
    cur = list(ZERO)
    for r in range(n):
        s[:, r] = cur
        cur = xc.sub(xc.add(cur, invs[2 * r], p), xc.scale(invs[2 * r + 1], int(cols[mult_col][r]) % p, p), p)
    return s, cur == ZERO, None


def recurrence_holds(s, cols, lookup, table, mult_col, ch, p, g):
    """s[0] == 0 and (s[r+1] - s[r]) f_L[r] f_T[r] == f_T[r] - M[r] f_L[r] for r < n - 1 -> (holds, closes): with every
    denominator non-zero this determines s; closes: the same relation from row n - 1 round to row 0"""
    P = np.uint64(p)
    s, cols = np.asarray(s, dtype=np.uint64), np.asarray(cols, dtype=np.uint64)
    fl, ft = pm.tuples_vec(cols, lookup, ch, p, g), pm.tuples_vec(cols, table, ch, p, g)
    if [int(v) for v in s[:, 0]] != ZERO:
        return False, False
    ds = (np.roll(s, -1, axis=1) + P - s) % P                   # the last column wraps to s[0] = 0
    lhs = pm.mul_vec(ds, pm.mul_vec(fl, ft, p, g), p, g)
    rhs = (ft + P - fl * (cols[mult_col] % P) % P) % P
    same = lhs == rhs
    return bool(np.all(same[:, :-1])), bool(np.all(same[:, -1]))


def gamma_for_zero(cols, idx, ch, row, p, g):
    """the challenges with gamma replaced so that the tuple over the columns idx is zero in `row`"""
    return pm.gamma_for_zero(cols, idx, ch, row, p, g)


# ---------------------------------------------------------------------------------------------- the auxiliary quotients
def aux_terms_at(idx, lde_at, s_at, s_next, lookup, table, mult_col, ch, wb, wt, p, g, wN, log_n, tau, h):
    """w_b s(x_i) / (x_i - tau) + w_t ((s(w x_i) - s(x_i)) f_L f_T - f_T + M f_L)(x_i) / (x_i^n - tau^n) at the points i of idx
    alone, as (4, len(idx)).  lde_at: (W, len(idx)) the extended trace columns at idx; s_at, s_next: (4, len(idx)) the extended
    column s at idx and at (idx + B) mod N; wN: the N-th root of unity of the evaluation domain; wb, wt: four unreduced ints
    each.  Nothing here is as long as N: the cost is per sampled point (pm.point_inverses)"""
    P = np.uint64(p)
    lde_at, s_at, s_next = (np.asarray(a, dtype=np.uint64) for a in (lde_at, s_at, s_next))
    ixt, izt = pm.point_inverses(idx, p, wN, log_n, tau, h)
    fl, ft = pm.tuples_vec(lde_at, lookup, ch, p, g), pm.tuples_vec(lde_at, table, ch, p, g)
    ds = (s_next + P - s_at) % P
    num = (pm.mul_vec(ds, pm.mul_vec(fl, ft, p, g), p, g) + P - ft + fl * (lde_at[mult_col] % P) % P) % P
    tq = num * izt % P
    bq = s_at * ixt % P
    return (xc.mul_arr(bq, [int(v) % p for v in wb], p, g) + xc.mul_arr(tq, [int(v) % p for v in wt], p, g)) % P


def aux_terms(o, lde, sl, lookup, table, mult_col, ch, wb, wt, p, g, log_n, lb, tau, h):
    """aux_terms_at for every i, as (4, N); lde: (W, N), sl: (4, N) extended columns"""
    B, N = 1 << lb, 1 << (log_n + lb)
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    sl = np.asarray(sl, dtype=np.uint64)
    return aux_terms_at(np.arange(N), lde, sl, np.roll(sl, -B, axis=1), lookup, table, mult_col, ch, wb, wt, p, g, wN, log_n, tau, h)


# ---------------------------------------------------------------------------------------------- prover, verifier
def prove(o, air, lookup, table, mult_col, cols, p, g, log_n, lb, t, tau, h, E, bits, honest=True, s_plus_p=None):
    """-> dict(roots, proof, top, nonce, closes, ch, s, cw) of smi_dev_air_prove_lookup from the oracle's primitives; the
    transcript is the permutation argument's (pm.challenges, pm.weights).  s_plus_p = e: a dishonest prover that COMMITS and
    opens coordinate e of the extended s with p added to every value: every path verifies, no such value is canonical"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K = len(cols), len(air.constraints)
    lde = ac.lde(o, cols, p, g, log_n, lb, tau, h)
    shown = [np.asarray(c, dtype=np.uint64) for c in lde]
    nodes1 = o.merkle_new(ar.row_leaves(o, shown))
    root1 = bytes(nodes1[-1])
    tr, ch = pm.challenges(o, root1)
    s, closes, zero = column(cols, lookup, table, mult_col, ch, p, g)
    assert zero is None, zero
    sl = ac.lde(o, [[int(v) for v in s[e]] for e in range(4)], p, g, log_n, lb, tau, h)
    sshown = [np.asarray(c, dtype=np.uint64) + np.uint64(p if e == s_plus_p else 0) for e, c in enumerate(sl)]
    nodes2 = o.merkle_new(ar.row_leaves(o, sshown))
    root2 = bytes(nodes2[-1])
    tr, wch = pm.weights(o, tr, root2, W + K + 2)
    assert len(tr) == pm.transcript_len(W, K)
    cw = pm.main_codeword(o, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h, honest)
    cw = (cw + aux_terms(o, lde, sl, lookup, table, mult_col, ch, wch[4 * (W + K):4 * (W + K) + 4], wch[4 * (W + K) + 4:], p, g, log_n, lb, tau,
                         h)) % np.uint64(p)
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    fri, top, nonce = pw.prove(o, cfg_o, cw, g, bytes(tr), bits)
    proof = fri + ar.openings_bytes(o, shown, top, N, B, True, nodes1) + ar.openings_bytes(o, sshown, top, N, B, True, nodes2)
    return dict(roots=root1 + root2, proof=proof, top=top, nonce=nonce, closes=closes, ch=ch, wch=wch, s=s, cw=cw)


def verify(o, air, lookup, table, mult_col, roots, proof, p, g, log_n, lb, t, tau, h, E, bits):
    """-> (accept, reason class): "fri" | "length" | "record" | "path" | "canonical" | "composition" | "" """
    n, B = 1 << log_n, 1 << lb
    N, log_N = n * B, log_n + lb
    W, K = air.n_cols, len(air.constraints)
    root1, root2 = bytes(roots[:32]), bytes(roots[32:64])
    tr, ch = pm.challenges(o, root1)
    tr, wch = pm.weights(o, tr, root2, W + K + 2)
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    ok, pv, used, top, _why = pw.verify(o, cfg_o, proof, g, bytes(tr), bits)
    if not ok:
        return False, "fri"
    rest = proof[used:]
    if len(rest) != pm.opening_len(W, log_N, t):
        return False, "length"
    positions = [i for s in top for i in ar.positions(s, N, B, True)]
    len1 = t * 4 * (9 + 8 * W) + t * 4 * (9 + 32 * log_N)
    for sec, width in ((rest[:len1], W), (rest[len1:], 4)):     # tags and widths of both sections before any path
        rec, prec, m = 9 + 8 * width, 9 + 32 * log_N, 4 * t
        for q in range(m):
            if sec[q * rec] != 2 or int.from_bytes(sec[q * rec + 1:q * rec + 9], "little") != width:
                return False, "record"
            at = m * rec + q * prec
            if sec[at] != 3 or int.from_bytes(sec[at + 1:at + 9], "little") != log_N:
                return False, "record"
    rows, why = pm._section(o, rest[:len1], W, log_N, positions, root1, p)
    if rows is None:
        return False, why
    srows, why = pm._section(o, rest[len1:], 4, log_N, positions, root2, p)
    if srows is None:
        return False, why
    if any(v >= p for r in rows + srows for v in r):
        return False, "canonical"
    alpha, gamma = pm.alpha_gamma(ch, p)
    apow = pm.alpha_powers(alpha, len(lookup), p, g)
    wb = [c % p for c in wch[4 * (W + K):4 * (W + K) + 4]]
    wt = [c % p for c in wch[4 * (W + K) + 4:4 * (W + K) + 8]]
    tn = pow(tau, n, p)
    for s in range(t):
        for k in range(2):
            i = positions[4 * s + k]
            cur, nxt, sc, sn = rows[4 * s + k], rows[4 * s + k + 2], srows[4 * s + k], srows[4 * s + k + 2]
            x = h * pow(wN, i, p) % p
            got = [air.compose_at(p, log_n, lb, tau, h, wN, i, cur, nxt, xc.weight_vector(wch[:4 * (W + K)], e)) for e in range(4)]
            fl, ft = pm.tuple_value(cur, lookup, apow, gamma, p), pm.tuple_value(cur, table, apow, gamma, p)
            num = xc.add(xc.sub(xc.mul(xc.sub(sn, sc, p), xc.mul(fl, ft, p, g), p, g), ft, p), xc.scale(fl, cur[mult_col] % p, p), p)
            tq = xc.scale(num, pow((pow(x, n, p) - tn) % p, p - 2, p), p)
            bq = xc.scale(sc, pow((x - tau) % p, p - 2, p), p)
            got = xc.add(got, xc.add(xc.mul(bq, wb, p, g), xc.mul(tq, wt, p, g), p), p)
            if got != [v % p for v in pv[2 * s + k][1]]:
                return False, "composition"
    return True, ""


REASON_CLASS = [                         # the library's sentence (smi_last_error) -> the restatement's class
    ("lookup openings: wrong length", "length"),
    ("lookup openings: malformed", "record"),
    ("lookup openings: authentication path", "path"),
    ("lookup openings: an opened value is not canonical", "canonical"),
    ("lookup openings: the composition", "composition"),
]


def reason_class(sentence):
    for head, cls in REASON_CLASS:
        if sentence.startswith(head):
            return cls
    return "fri" if sentence else ""


# ---------------------------------------------------------------------------------------------- traces
def shaped(kind, n, p, seed=5, m=2, extra=1):
    """-> (cols, lookup, table, mult_col) with the multiplicity column filled by `multiplicities`: m lookup columns, m table
    columns, the multiplicities, `extra` random columns.  kind:
      "range"   the table's first member is a shuffled 0 .. n-1 (distinct tuples), the lookups are random table rows;
      "dups"    the table holds max(1, n / 4) distinct tuples, each in several rows: the lowest row is credited;
      "one"     all n lookups hit the tuple of table row n / 3: M = n in one cell;
      "overlap" lookup columns [0, 1], table columns [1, 2]: (c0, c1)[r] = (c1, c2)[sigma(r)]."""
    rng = np.random.default_rng(seed)
    if kind == "overlap":
        sigma = rng.permutation(n)
        c1 = rng.permutation(n).astype(np.int64) * 3 % p
        c0 = c1[sigma]
        c2 = np.zeros(n, dtype=np.int64)
        c2[sigma] = c1
        cols = [[int(v) for v in c0], [int(v) for v in c1], [int(v) for v in c2], [0] * n]
        cols += [[int(v) for v in rng.integers(0, p, n)] for _ in range(extra)]
        lookup, table, mult_col = [0, 1], [1, 2], 3
    else:
        tab = rng.integers(0, p, (m, n), dtype=np.int64)
        tab[0] = rng.permutation(n)
        if kind == "dups":
            tab = tab[:, rng.integers(0, max(1, n // 4), n)]
        pick = np.full(n, n // 3) if kind == "one" else rng.integers(0, n, n)
        look = tab[:, pick]
        cols = [[int(v) for v in look[j]] for j in range(m)] + [[int(v) for v in tab[j]] for j in range(m)] + [[0] * n]
        cols += [[int(v) for v in rng.integers(0, p, n)] for _ in range(extra)]
        lookup, table, mult_col = list(range(m)), list(range(m, 2 * m)), 2 * m
    M, missing = multiplicities(cols, lookup, table)
    assert missing is None
    cols[mult_col] = M
    return cols, lookup, table, mult_col


def absent_value(cols, table):
    """a value that the first table column does not hold"""
    have = set(int(v) for v in cols[table[0]])
    return next(v for v in range(len(have) + 1) if v not in have)


def non_closing(kind, n, p, seed=5):
    """-> (cols, lookup, table, mult_col) whose sum does not close: "multiplicity" one M off by one; "absent" one lookup
    swapped for a value the table does not hold, M kept"""
    cols, lookup, table, mult_col = shaped("range", n, p, seed)
    if kind == "multiplicity":
        cols[mult_col][n // 2] = (cols[mult_col][n // 2] + 1) % p
    elif kind == "absent":
        cols[lookup[0]][n // 2] = absent_value(cols, table)
    else:
        raise ValueError(kind)
    return cols, lookup, table, mult_col


def with_range_lookup(air, cols, p, seed=9, spoil=None):
    """widens (air, cols) by three columns -- looked-up values, a table holding a shuffled 0 .. n-1, the multiplicities --
    and states that lookup: a range check beside the main AIR, which stays satisfied.  spoil: see non_closing"""
    W, n = len(cols), len(cols[0])
    rng = np.random.default_rng(seed)
    table = [int(v) for v in rng.permutation(n)]
    look = [int(v) for v in rng.integers(0, n, n)]
    new = [look, table, [0] * n]
    M, _ = multiplicities(new, [0], [1])
    new[2] = M
    if spoil == "multiplicity":
        new[2][n // 2] = (new[2][n // 2] + 1) % p
    elif spoil == "absent":
        new[0][n // 2] = n
    air.n_cols = W + 3
    air.lookup([W], [W + 1], W + 2)
    return air, [list(c) for c in cols] + new


def perm_twin(n, p, seed=4):
    """-> (air with a lookup, air with a permutation, cols): the cubic AIR (degree 3, so both arguments plan the same d, D and
    E) beside a column that is a shuffled copy of a table of distinct values, every multiplicity one.  Both statements hold
    over the same columns, transcript and proof layout are the same, and only the recomputed composition tells a proof of
    one from a proof of the other."""
    from stark_rs_amd.mirror import Air
    rng = np.random.default_rng(seed)
    air_l, cols = pm.cubic(n, p)
    air_p, _ = pm.cubic(n, p)
    W = len(cols)
    table = [int(v) for v in rng.permutation(n)]
    look = [table[int(r)] for r in rng.permutation(n)]
    cols = [list(c) for c in cols] + [look, table, [1] * n]
    for a in (air_l, air_p):
        a.n_cols = W + 3
    assert isinstance(air_l, Air)
    air_l.lookup([W], [W + 1], W + 2)
    air_p.permutation([W], [W + 1])
    return air_l, air_p, cols
