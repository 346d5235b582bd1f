"""The checker of the argument list (include/stark_mi.h, "Argument list"), restated in Python: the looping layer over
tests/perm_compose.py and tests/lookup_compose.py -- every argument's column and its two quotients are those modules', taken
once per argument at that argument's coordinates and weights -- with the transcript, the prover and the verifier of a proof
whose second tree has rows of 4 A values.  An argument is ("perm", left, right) or ("lookup", columns, table columns,
multiplicity column), as in mirror.Air.args.
Not a test module: imported by tests/test_args_host.py, tests/test_args_emu.py and tests/test_gpu_args.py."""
import numpy as np

import air_compose as ac
import air_rows as ar
import ext_compose as xc
import lookup_compose as lc
import perm_compose as pm
import pow_compose as pw


def is_perm(arg):
    return arg[0] == "perm"


# ---------------------------------------------------------------------------------------------- the columns
def column(cols, arg, ch, p, g):
    """one argument -> (column (4, n), closes, None) or (None, None, (row, side)); side 0: f_L, side 1: f_R or f_T"""
    if is_perm(arg):
        z, closes, zero = pm.column(cols, arg[1], arg[2], ch, p, g)
        return z, closes, (None if zero is None else (zero, 1))
    s, closes, zero = lc.column(cols, arg[1], arg[2], arg[3], ch, p, g)
    return s, closes, (None if zero is None else (zero[0], 0 if zero[1] == "f_L" else 1))


def columns(cols, args, ch, p, g, column_of=column):
    """-> (c as a (4 A, n) uint64 array, [closes of argument a], None) or (None, None, the smallest key 16 row + 2 a + side
    with a zero denominator)"""
    parts, closes, keys = [], [], []
    for a, arg in enumerate(args):
        c, cl, zero = column_of(cols, arg, ch, p, g)
        if zero is not None:
            keys.append(16 * zero[0] + 2 * a + zero[1])
            continue
        parts.append(c)
        closes.append(bool(cl))
    if keys:
        return None, None, min(keys)
    return np.concatenate(parts), closes, None


def recurrences_hold(c, cols, args, ch, p, g):
    """-> [(holds, closes) of argument a] from each section's recurrence over the coordinates 4 a .. 4 a + 3"""
    out = []
    for a, arg in enumerate(args):
        ca = c[4 * a:4 * a + 4]
        if is_perm(arg):
            holds = pm.recurrence_holds(ca, cols, arg[1], arg[2], ch, p, g)
            fl = pm.tuples_vec(np.asarray(cols, dtype=np.uint64)[:, -1:], arg[1], ch, p, g)
            fr = pm.tuples_vec(np.asarray(cols, dtype=np.uint64)[:, -1:], arg[2], ch, p, g)
            last = pm.mul_vec(np.asarray(ca, dtype=np.uint64)[:, -1:], fl, p, g)          # z[n-1] f_L[n-1] == 1 * f_R[n-1]
            out.append((holds, bool(np.array_equal(last, fr))))
        else:
            out.append(lc.recurrence_holds(ca, cols, arg[1], arg[2], arg[3], ch, p, g))
    return out


# ---------------------------------------------------------------------------------------------- the auxiliary quotients
def aux_terms_at(idx, lde_at, c_at, c_next, args, ch, wch_aux, p, g, wN, log_n, tau, h):
    """the 2 A auxiliary quotients at the points i of idx alone, as (4, len(idx)): pm.aux_terms_at / lc.aux_terms_at once per
    argument.  lde_at: (W, len(idx)) the extended trace columns at idx; c_at, c_next: (4 A, len(idx)) the extended columns at
    idx and at (idx + B) mod N; wch_aux: the 8 A unreduced challenges behind the main weights (argument a: boundary at 8 a,
    transition at 8 a + 4)"""
    total = np.zeros((4, len(idx)), dtype=np.uint64)
    for a, arg in enumerate(args):
        wb, wt = wch_aux[8 * a:8 * a + 4], wch_aux[8 * a + 4:8 * a + 8]
        ca, cn = c_at[4 * a:4 * a + 4], c_next[4 * a:4 * a + 4]
        if is_perm(arg):
            t = pm.aux_terms_at(idx, lde_at, ca, cn, arg[1], arg[2], ch, wb, wt, p, g, wN, log_n, tau, h)
        else:
            t = lc.aux_terms_at(idx, lde_at, ca, cn, arg[1], arg[2], arg[3], ch, wb, wt, p, g, wN, log_n, tau, h)
        total = (total + t) % np.uint64(p)
    return total


def aux_terms(o, lde, cl, args, ch, wch_aux, p, g, log_n, lb, tau, h):
    """aux_terms_at for every i, as (4, N); cl: (4 A, N) extended columns"""
    B, N = 1 << lb, 1 << (log_n + lb)
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cl = np.asarray(cl, dtype=np.uint64)
    return aux_terms_at(np.arange(N), lde, cl, np.roll(cl, -B, axis=1), args, ch, wch_aux, p, g, wN, log_n, tau, h)


# ---------------------------------------------------------------------------------------------- transcript, prover, verifier
def transcript_len(W, K, A):
    return 32 + 64 + 32 + 32 * (W + K + 2 * A)


def opening_len(W, A, log_N, t):
    return t * 4 * (9 + 8 * W) + t * 4 * (9 + 32 * log_N) + t * 4 * (9 + 32 * A) + t * 4 * (9 + 32 * log_N)


def proof_len(N, E, t, R, W, A):
    return pw.proof_len(N, E, t, R) + opening_len(W, A, N.bit_length() - 1, t)


def plan(air, args, lb):
    """-> (d, D, E) of smi_air_plan_args"""
    d = max([air.degree] + [2 if is_perm(arg) else 3 for arg in args])
    D = 1
    while D < d - 1:
        D *= 2
    return d, D, (1 << lb) // D


def prove(o, air, args, cols, p, g, log_n, lb, t, tau, h, E, bits, honest=True, c_plus_p=None):
    """-> dict(roots, proof, top, nonce, closes, ch, wch, c, cw) of smi_dev_air_prove_args from the oracle's primitives.
    c_plus_p = e: a dishonest prover that COMMITS and opens coordinate column e (< 4 A) of the extended columns with p added to
    every value: every path verifies, no such value is canonical"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K, A = len(cols), len(air.constraints), len(args)
    lde = ac.lde(o, cols, p, g, log_n, lb, tau, h)
    shown = [np.asarray(c, dtype=np.uint64) for c in lde]
    nodes1 = o.merkle_new(ar.row_leaves(o, shown))
    root1 = bytes(nodes1[-1])
    tr, ch = pm.challenges(o, root1)
    c, closes, zero = columns(cols, args, ch, p, g)
    assert zero is None, zero
    cl = ac.lde(o, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)
    cshown = [np.asarray(col, dtype=np.uint64) + np.uint64(p if e == c_plus_p else 0) for e, col in enumerate(cl)]
    nodes2 = o.merkle_new(ar.row_leaves(o, cshown))
    root2 = bytes(nodes2[-1])
    tr, wch = pm.weights(o, tr, root2, W + K + 2 * A)
    assert len(tr) == transcript_len(W, K, A)
    cw = pm.main_codeword(o, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h, honest)
    cw = (cw + aux_terms(o, lde, np.asarray(cl, dtype=np.uint64), args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h)) % np.uint64(p)
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    fri, top, nonce = pw.prove(o, cfg_o, cw, g, bytes(tr), bits)
    proof = fri + ar.openings_bytes(o, shown, top, N, B, True, nodes1) + ar.openings_bytes(o, cshown, top, N, B, True, nodes2)
    return dict(roots=root1 + root2, proof=proof, top=top, nonce=nonce, closes=closes, ch=ch, wch=wch, c=c, cw=cw)


def verify(o, air, args, roots, proof, p, g, log_n, lb, t, tau, h, E, bits):
    """-> (accept, reason class): "fri" | "length" | "record" | "path" | "canonical" | "composition" | "" -- the order of
    checks of pm.verify over a second section 4 A values wide"""
    n, B = 1 << log_n, 1 << lb
    N, log_N = n * B, log_n + lb
    W, K, A = air.n_cols, len(air.constraints), len(args)
    root1, root2 = bytes(roots[:32]), bytes(roots[32:64])
    tr, ch = pm.challenges(o, root1)
    tr, wch = pm.weights(o, tr, root2, W + K + 2 * A)
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    ok, pv, used, top, _why = pw.verify(o, cfg_o, proof, g, bytes(tr), bits)
    if not ok:
        return False, "fri"
    rest = proof[used:]
    if len(rest) != opening_len(W, A, log_N, t):
        return False, "length"
    positions = [i for s in top for i in ar.positions(s, N, B, True)]
    len1 = t * 4 * (9 + 8 * W) + t * 4 * (9 + 32 * log_N)
    for sec, width in ((rest[:len1], W), (rest[len1:], 4 * A)):   # tags and widths of both sections before any path
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
    crows, why = pm._section(o, rest[len1:], 4 * A, log_N, positions, root2, p)
    if crows is None:
        return False, why
    if any(v >= p for r in rows + crows for v in r):
        return False, "canonical"
    alpha, gamma = pm.alpha_gamma(ch, p)
    apow = pm.alpha_powers(alpha, 8, p, g)
    tn = pow(tau, n, p)
    for s in range(t):
        for k in range(2):
            i = positions[4 * s + k]
            cur, nxt = rows[4 * s + k], rows[4 * s + k + 2]
            x = h * pow(wN, i, p) % p
            izt, ixt = pow((pow(x, n, p) - tn) % p, p - 2, p), pow((x - tau) % p, p - 2, p)
            got = [air.compose_at(p, log_n, lb, tau, h, wN, i, cur, nxt, xc.weight_vector(wch[:4 * (W + K)], e)) for e in range(4)]
            for a, arg in enumerate(args):
                at = 4 * (W + K + 2 * a)
                wb, wt = [c % p for c in wch[at:at + 4]], [c % p for c in wch[at + 4:at + 8]]
                cc, cn = crows[4 * s + k][4 * a:4 * a + 4], crows[4 * s + k + 2][4 * a:4 * a + 4]
                fl, fr = pm.tuple_value(cur, arg[1], apow, gamma, p), pm.tuple_value(cur, arg[2], apow, gamma, p)
                if is_perm(arg):
                    tq = xc.scale(xc.sub(xc.mul(cn, fr, p, g), xc.mul(cc, fl, p, g), p), izt, p)
                    bq = xc.scale(xc.sub(cc, pm.ONE, p), ixt, p)
                else:
                    num = xc.add(xc.sub(xc.mul(xc.sub(cn, cc, p), xc.mul(fl, fr, p, g), p, g), fr, p), xc.scale(fl, cur[arg[3]] % p, p), p)
                    tq = xc.scale(num, izt, p)
                    bq = xc.scale(cc, ixt, p)
                got = xc.add(got, xc.add(xc.mul(bq, wb, p, g), xc.mul(tq, wt, p, g), p), p)
            if got != [v % p for v in pv[2 * s + k][1]]:
                return False, "composition"
    return True, ""


REASON_CLASS = [                         # the library's sentence (smi_last_error) -> the restatement's class
    ("argument openings: wrong length", "length"),
    ("argument openings: malformed", "record"),
    ("argument openings: authentication path", "path"),
    ("argument openings: an opened value is not canonical", "canonical"),
    ("argument openings: the composition", "composition"),
]


def reason_class(sentence):
    for head, cls in REASON_CLASS:
        if sentence.startswith(head):
            return cls
    return "fri" if sentence else ""


# ---------------------------------------------------------------------------------------------- traces
EIGHT = [("perm", 1), ("lookup", 2), ("perm", 8), ("lookup", 1), ("perm", 2), ("lookup", 8), ("perm", 1), ("lookup", 2)]


def pool(n, p, seed=5, spec=EIGHT, first=0):
    """-> (cols, arguments): ONE trace over which every argument of spec = [(kind, width), ...] holds.  With mm the largest
    width: columns 0 .. mm - 1 are random; the next mm are rows picked from the table in the mm after them, whose first
    column is a shuffled 0 .. n - 1, so that a lookup over any leading m of them holds with the same multiplicities.  Behind
    them every argument has columns of its own: a permutation of width m the leading m random columns in a row order of
    its own, a lookup its multiplicities.  The arguments overlap in the columns they read, and one cell of an argument's own
    columns breaks that argument alone (spoil).  first: the index of column 0 in the trace the columns will be part of."""
    rng = np.random.default_rng(seed)
    mm = max(m for _k, m in spec)
    src = rng.integers(0, p, (mm, n), dtype=np.int64)
    tab = rng.integers(0, p, (mm, n), dtype=np.int64)
    tab[0] = rng.permutation(n)
    look = tab[:, rng.integers(0, n, n)]
    cols = [[int(v) for v in r] for r in src] + [[int(v) for v in r] for r in look] + [[int(v) for v in r] for r in tab]
    M, missing = lc.multiplicities(cols, [mm], [2 * mm])
    assert missing is None
    args = []
    for kind, m in spec:
        W = first + len(cols)
        if kind == "perm":
            order = rng.permutation(n)
            cols += [[int(v) for v in src[j][order]] for j in range(m)]
            args.append(("perm", list(range(first, first + m)), list(range(W, W + m))))
        else:
            cols.append(list(M))
            args.append(("lookup", list(range(first + mm, first + mm + m)), list(range(first + 2 * mm, first + 2 * mm + m)), W))
    return cols, args


def spoil(cols, arg, p):
    """-> a copy of cols in which `arg` alone of the pool's arguments is broken: one multiplicity off by one, or one cell of a
    permutation's last right column"""
    out = [list(c) for c in cols]
    n = len(cols[0])
    c = arg[3] if not is_perm(arg) else arg[2][-1]
    out[c][n // 2] = (out[c][n // 2] + 1) % p
    return out


def mirror_air(air, args):
    """appends args to a mirror.Air's list"""
    for arg in args:
        if is_perm(arg):
            air.add_permutation(arg[1], arg[2])
        else:
            air.add_lookup(arg[1], arg[2], arg[3])
    return air
