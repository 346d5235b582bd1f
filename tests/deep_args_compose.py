"""The checker of out-of-domain sampling with an argument list (include/stark_mi.h, "Out-of-domain sampling with an argument
list"), restated in Python over the oracle's primitives and the two restatements it joins: tests/deep_compose.py (segments,
evaluation at points of F_q, extension FRI with grinding at E = B, the R = 2 row openings, the consistency check of a plain AIR)
and tests/xargs_compose.py (the widened trace, the A columns from their recurrences, the 2 A auxiliary quotients on the coset).
The auxiliary quotients AT z are written out here from the section's formulas over Python-int F_q arithmetic.
Not a test module: imported by tests/test_deep_args_host.py, tests/test_deep_args_emu.py, tests/test_gpu_deep_args.py and
tests/test_gpu_boundary_primes_deep_args.py."""
import numpy as np

import air_compose as ac
import air_rows as ar
import deep_compose as dc
import ext_compose as xc
import perm_compose as pm
import pow_compose as pc
import xargs_compose as xa

ONE, XGEN = [1, 0, 0, 0], [0, 1, 0, 0]

# reason class of the restated verifier -> a keyword of the library's sentence for it
KEYWORD = {"record": "out-of-domain record", "record canonical": "out-of-domain coordinate is not canonical", "base field": "base field",
           "consistency": "deep arguments: out-of-domain consistency check fails", "no layer": "no fold",
           "length": "deep argument openings: wrong length", "row": "deep argument openings: malformed row",
           "path": "deep argument openings: malformed path", "auth": "deep argument openings: authentication path does not verify",
           "canonical": "deep argument openings: an opened value is not canonical", "quotient": "deep argument openings: the DEEP quotient"}


def keyword(reason):
    return dc.FRI_KEYWORD[reason[5:]] if reason.startswith("fri: ") else KEYWORD[reason]


def plan(air, args):
    """-> (d, D) of smi_air_plan_deep_xargs: d by the list's rule, D the smallest power of two >= max(1, d - 1)"""
    d, D, _E = xa.plan(air, args, 0)
    return d, D


def record_len(W, A, D):
    return 4 * (2 * W + 2 * A + D)


def proof_len(o, W, A, D, log_n, lb, t, p, g, h):
    N, B, log_N = 1 << (log_n + lb), 1 << lb, log_n + lb
    _w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    R = o.fri_num_rounds(o.fri_cfg(wN, h, N, B, t, p))
    path = 2 * t * (9 + 32 * log_N)
    return 9 + 32 * (2 * W + 2 * A + D) + pc.proof_len(N, B, t, R) + 2 * t * (9 + 8 * W) + path + 2 * t * (9 + 32 * A) + path + 2 * t * (9 + 32 * D) + path


def transcript_len(W, K, A, D):
    return 32 * (6 + W + K + 2 * A + 2 * (2 * W + 2 * A + D))


# ---------------------------------------------------------------------------------------------- the DEEP codeword
def q_codeword(lde, cl, seg, x, z, ood, ch, w_n, p, g):
    """lde: (W, N), cl: (4 A, N), seg: (4 D, N), x: the N points, ood: the record's 4 (2 W + 2 A + D) canonical values in the
    order u, v, a, b, s, ch: as many unreduced challenges -> Q as a (4, N) array, term by term from the formula"""
    lde, cl, seg = (np.asarray(v, dtype=np.uint64) for v in (lde, cl, seg))
    W, A, D, N, P = lde.shape[0], cl.shape[0] // 4, seg.shape[0] // 4, lde.shape[1], np.uint64(p)
    el = lambda v, i: [int(c) % p for c in v[4 * i:4 * i + 4]]
    n1, n2 = np.zeros((4, N), dtype=np.uint64), np.zeros((4, N), dtype=np.uint64)

    def minus(vals, e4):
        return np.stack([(vals[e] + P - np.uint64(e4[e])) % P for e in range(4)])
    zero = np.zeros(N, dtype=np.uint64)
    for c in range(W):
        f = [lde[c], zero, zero, zero]
        n1 = (n1 + dc._mul_const(minus(f, el(ood, c)), el(ch, c), p, g)) % P
        n2 = (n2 + dc._mul_const(minus(f, el(ood, W + c)), el(ch, W + c), p, g)) % P
    for a in range(A):
        f = cl[4 * a:4 * a + 4]
        n1 = (n1 + dc._mul_const(minus(f, el(ood, 2 * W + a)), el(ch, 2 * W + a), p, g)) % P
        n2 = (n2 + dc._mul_const(minus(f, el(ood, 2 * W + A + a)), el(ch, 2 * W + A + a), p, g)) % P
    for j in range(D):
        i = 2 * W + 2 * A + j
        n1 = (n1 + dc._mul_const(minus(seg[4 * j:4 * j + 4], el(ood, i)), el(ch, i), p, g)) % P
    zw = dc.scale_q(z, w_n, p)
    xs = [np.asarray(x, dtype=np.uint64), zero, zero, zero]
    return (pm.mul_vec(n1, dc.inv_vec(minus(xs, z), p, g), p, g) + pm.mul_vec(n2, dc.inv_vec(minus(xs, zw), p, g), p, g)) % P


def q_at(trow, crow, srow, x, z, ood, ch, w_n, p, g):
    """Q(x) from one trace row, one row of the auxiliary columns' coordinates and one segment row, Python ints"""
    W, A, D = len(trow), len(crow) // 4, len(srow) // 4
    el = lambda v, i: [int(c) % p for c in v[4 * i:4 * i + 4]]
    n1, n2 = [0] * 4, [0] * 4
    term = lambda f, i: xc.mul(el(ch, i), xc.sub(f, el(ood, i), p), p, g)
    for c in range(W):
        f = xc.embed(int(trow[c]), p)
        n1, n2 = xc.add(n1, term(f, c), p), xc.add(n2, term(f, W + c), p)
    for a in range(A):
        f = el(crow, a)
        n1, n2 = xc.add(n1, term(f, 2 * W + a), p), xc.add(n2, term(f, 2 * W + A + a), p)
    for j in range(D):
        n1 = xc.add(n1, term(el(srow, j), 2 * W + 2 * A + j), p)
    d1, d2 = xc.sub(xc.embed(x, p), z, p), xc.sub(xc.embed(x, p), dc.scale_q(z, w_n, p), p)
    return xc.add(xc.mul(n1, xc.inv(d1, p, g), p, g), xc.mul(n2, xc.inv(d2, p, g), p, g), p)


# ---------------------------------------------------------------------------------------------- out-of-domain values
def _assemble(coords, p, g):
    """sum_e X^e coords[e] for four elements of F_q"""
    acc, xe = [0] * 4, list(ONE)
    for e in range(4):
        acc = xc.add(acc, xc.mul(xe, coords[e], p, g), p)
        xe = xc.mul(xe, XGEN, p, g)
    return acc


def ood_values(o, cols, c, hc, D, z, p, g, log_n, tau):
    """u, v, a, b, s as a flat list of 4 (2 W + 2 A + D) canonical values.  cols: the trace, c: the (4 A, n) unextended
    coordinate columns, hc: the coefficients of H's coordinates"""
    n, A = 1 << log_n, len(c) // 4
    w = o.ff_prim_nth_root_g(n, p, g)
    zw = dc.scale_q(z, w, p)
    polys = np.stack([np.asarray(o.fast_intt(np.array([int(v) % p for v in col], dtype=np.uint64), w, tau, p), dtype=np.uint64) for col in list(cols) + list(c)])
    at_z, at_zw = dc.eval_cols(polys, z, p, g), dc.eval_cols(polys, zw, p, g)
    W = len(cols)
    u, v = at_z[:W], at_zw[:W]
    a = [_assemble(at_z[W + 4 * i:W + 4 * i + 4], p, g) for i in range(A)]
    b = [_assemble(at_zw[W + 4 * i:W + 4 * i + 4], p, g) for i in range(A)]
    sj = [dc.eval_cols(np.stack([hc[e, j * n:(j + 1) * n] for e in range(4)]), z, p, g) for j in range(D)]
    s = [_assemble(co, p, g) for co in sj]
    return [x for el in u + v + a + b + s for x in el]


# ---------------------------------------------------------------------------------------------- the auxiliary quotients at z
def aux_at_z(o, air, args, ch, z, u, a_vals, b_vals, p, g, log_n, tau):
    """-> [(bq_a, wq_a)]: the two auxiliary quotients of every argument at z over F_q operands.  u: f_c(z) per trace column;
    a_vals, b_vals: c_a(z), c_a(z w)"""
    n, W = 1 << log_n, len(u)
    w = o.ff_prim_nth_root_g(n, p, g)
    per = dc.periodic_q(o, air, z, p, g, log_n, tau, w)
    wide = list(u) + list(per)
    alpha, gamma = pm.alpha_gamma(ch, p)
    ixt = xc.inv(xc.sub(z, xc.embed(tau % p, p), p), p, g)
    izt = xc.inv(xc.sub(xc.power(z, n, p, g), xc.embed(pow(tau, n, p), p), p), p, g)
    out = []
    for k, arg in enumerate(args):
        perm, ai, bi, mc, sa, sb = xa.norm(arg, W)
        apow = pm.alpha_powers(alpha, len(ai), p, g)

        def tup(idx):
            f = list(gamma)
            for j, c in enumerate(idx):
                f = xc.add(f, xc.mul(apow[j], wide[c], p, g), p)
            return f
        fl, fr = tup(ai), tup(bi)
        Sa, Sb = (ONE if sa is None else wide[sa]), (ONE if sb is None else wide[sb])
        ca, cb = a_vals[k], b_vals[k]
        if perm:
            gl = xc.add(ONE, xc.mul(Sa, xc.sub(fl, ONE, p), p, g), p)
            gr = xc.add(ONE, xc.mul(Sb, xc.sub(fr, ONE, p), p, g), p)
            bq = xc.mul(xc.sub(ca, ONE, p), ixt, p, g)
            wq = xc.mul(xc.sub(xc.mul(cb, gr, p, g), xc.mul(ca, gl, p, g), p), izt, p, g)
        else:
            num = xc.mul(xc.sub(cb, ca, p), xc.mul(fl, fr, p, g), p, g)
            num = xc.sub(num, xc.mul(Sa, fr, p, g), p)
            num = xc.add(num, xc.mul(xc.mul(wide[mc], Sb, p, g), fl, p, g), p)
            bq = xc.mul(ca, ixt, p, g)
            wq = xc.mul(num, izt, p, g)
        out.append((bq, wq))
    return out


def ood_sides(o, air, args, W, D, ch, weights, z, ood, p, g, log_n, tau):
    """-> both sides of the extended consistency check"""
    A, K = len(args), len(air.constraints)
    el = lambda v, i: [int(c) % p for c in v[4 * i:4 * i + 4]]
    plain = list(ood[:8 * W]) + list(ood[4 * (2 * W + 2 * A):])
    lhs, rhs = dc.ood_sides(o, air, W, D, weights[:4 * (W + K)], z, plain, p, g, log_n, tau)
    u = [el(ood, c) for c in range(W)]
    a_vals, b_vals = [el(ood, 2 * W + a) for a in range(A)], [el(ood, 2 * W + A + a) for a in range(A)]
    for a, (bq, wq) in enumerate(aux_at_z(o, air, args, ch, z, u, a_vals, b_vals, p, g, log_n, tau)):
        lhs = xc.add(lhs, xc.mul(el(weights, W + K + 2 * a), bq, p, g), p)
        lhs = xc.add(lhs, xc.mul(el(weights, W + K + 2 * a + 1), wq, p, g), p)
    return lhs, rhs


# ---------------------------------------------------------------------------------------------- prover and verifier
def prove(o, air, args, cols, p, g, log_n, lb, t, tau, h, bits=0, honest=True):
    """-> dict(roots, proof, top, ood, z, ch, wch, gammas, closes, c, lde, cl, seg, H, Q) of smi_dev_air_prove_deep_xargs.  honest=False:
    a trace whose list does not close; the composition's coefficients at and above D n are dropped, as the library drops them"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K, A = len(cols), len(air.constraints), len(args)
    _d, D = plan(air, args)
    assert D <= B and B >= 4 and 4 * D <= 64
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    wide = xa.widen(cols, air, p)
    lde_wide = ac.lde(o, wide, p, g, log_n, lb, tau, h)
    lde = [np.asarray(c, dtype=np.uint64) for c in lde_wide[:W]]
    nodes1 = o.merkle_new(ar.row_leaves(o, lde))
    root1 = bytes(nodes1[-1])
    tr, ch = pm.challenges(o, root1)
    c, closes, zero = xa.columns(wide, args, ch, p, g, W)
    assert zero is None, zero
    cl = [np.asarray(col, dtype=np.uint64) for col in ac.lde(o, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)]
    nodes2 = o.merkle_new(ar.row_leaves(o, cl))
    root2 = bytes(nodes2[-1])
    tr, wch = pm.weights(o, tr, root2, W + K + 2 * A)
    H = pm.main_codeword(o, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h, True)
    H = (H + xa.aux_terms(o, np.asarray(lde_wide, dtype=np.uint64), cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W)) % np.uint64(p)
    hc, seg = dc.segments(o, H, D, p, g, log_n, lb, h)
    assert not honest or not hc[:, D << log_n:].any(), "the composition has coefficients at or above D n"
    nodes3 = o.merkle_new(ar.row_leaves(o, list(seg)))
    root3 = bytes(nodes3[-1])
    tr = bytearray(tr) + root3
    first = 8 + 4 * (W + K + 2 * A)
    z = [v % p for v in dc.draw(o, tr, first, 4)]
    assert any(z[1:]), "z lies in the base field"
    ood = ood_values(o, cols, c, hc, D, z, p, g, log_n, tau)
    record = xc._elems(ood)
    tr += record[9:]
    gammas = dc.draw(o, tr, first + 4, record_len(W, A, D))
    assert len(tr) == transcript_len(W, K, A, D)
    Q = q_codeword(lde, cl, seg, dc.points(o, p, g, log_n, lb, h), z, ood, gammas, w, p, g)
    cfg_o = o.fri_cfg(wN, h, N, B, t, p)
    fri, top, _nonce = pc.prove(o, cfg_o, Q, g, bytes(tr), bits)
    proof = (record + fri + ar.openings_bytes(o, lde, top, N, B, False, nodes1) + ar.openings_bytes(o, cl, top, N, B, False, nodes2)
             + ar.openings_bytes(o, list(seg), top, N, B, False, nodes3))
    return {"roots": [root1, root2, root3], "proof": proof, "top": top, "ood": ood, "z": z, "ch": ch, "wch": wch, "gammas": gammas, "closes": closes,
            "c": c, "lde": lde, "cl": cl, "seg": seg, "H": H, "Q": Q}


def verify(o, air, args, proof, roots, p, g, W, log_n, lb, t, tau, h, bits=0):
    """-> (accept, reason class) of smi_air_verify_deep_xargs, in its order"""
    N, B, log_N, K, A = 1 << (log_n + lb), 1 << lb, log_n + lb, len(air.constraints), len(args)
    _d, D = plan(air, args)
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cnt = record_len(W, A, D)
    obj = xc._pop(proof, 0)
    if obj is None or obj[0] != 2 or len(obj[1]) != cnt:
        return False, "record"
    ood, at = obj[1], obj[2]
    if any(v >= p for v in ood):
        return False, "record canonical"
    tr, ch = pm.challenges(o, bytes(roots[0]))
    tr, wch = pm.weights(o, tr, bytes(roots[1]), W + K + 2 * A)
    tr = bytearray(tr) + bytes(roots[2])
    first = 8 + 4 * (W + K + 2 * A)
    z = [v % p for v in dc.draw(o, tr, first, 4)]
    if not any(z[1:]):
        return False, "base field"
    tr += proof[9:at]
    gammas = dc.draw(o, tr, first + 4, cnt)
    lhs, rhs = ood_sides(o, air, args, W, D, ch, wch, z, ood, p, g, log_n, tau)
    if lhs != rhs:
        return False, "consistency"
    cfg_o = o.fri_cfg(wN, h, N, B, t, p)
    ok, pv, used, top, why = pc.verify(o, cfg_o, proof[at:], g, bytes(tr), bits)
    if not ok:
        return False, "fri: " + why
    if len(pv) != 2 * t:
        return False, "no layer"
    rest = proof[at + used:]
    m, widths = 2 * t, [W, 4 * A, 4 * D]
    lens = [m * (9 + 8 * wd) + m * (9 + 32 * log_N) for wd in widths]
    if len(rest) != sum(lens):
        return False, "length"
    secs = [rest[:lens[0]], rest[lens[0]:lens[0] + lens[1]], rest[lens[0] + lens[1]:]]
    pos = [i for s in top for i in ar.positions(s, N, B, False)]
    rows = []
    for v in range(3):
        r, why = dc._section(o, secs[v], widths[v], log_N, pos, roots[v])
        if r is None:
            return False, why
        rows.append(r)
    for v in range(3):
        if not dc._auth(o, secs[v], widths[v], log_N, pos, bytes(roots[v])):
            return False, "auth"
    if any(x >= p for r in rows for row in r for x in row):
        return False, "canonical"
    for q, i in enumerate(pos):
        x = h * pow(wN, i, p) % p
        if q_at(rows[0][q], rows[1][q], rows[2][q], x, z, ood, gammas, w, p, g) != [int(c) for c in pv[q][1]] or pv[q][0] != i:
            return False, "quotient"
    return True, ""


# ---------------------------------------------------------------------------------------------- lists and traces
def compose_inputs(p, W, A, D, N, kind, seed=1, u=None):
    """-> (lde, cl, seg, z, ood, ch): random cells, or every operand p - 1 under challenges of the set u"""
    rng = np.random.default_rng(seed)
    cnt = record_len(W, A, D)
    if kind == "extreme":
        return (np.full((W, N), p - 1, dtype=np.uint64), np.full((4 * A, N), p - 1, dtype=np.uint64), np.full((4 * D, N), p - 1, dtype=np.uint64),
                [p - 1] * 4, [p - 1] * cnt, [u[(3 * i + seed) % len(u)] for i in range(cnt)])
    return (rng.integers(0, p, (W, N), dtype=np.uint64), rng.integers(0, p, (4 * A, N), dtype=np.uint64), rng.integers(0, p, (4 * D, N), dtype=np.uint64),
            [int(v) for v in rng.integers(1, p, 4)], [int(v) for v in rng.integers(0, p, cnt)],
            [int(v) for v in rng.integers(1 << 62, (1 << 64) - 1, cnt, dtype=np.uint64)])


def small_lists(n, p, seed=3):
    """-> {name: (air, cols, args)}: one permutation; one lookup; a permutation with selectors; a lookup into a periodic table
    with a periodic selector.  Traces of n rows over which every list closes."""
    from stark_rs_amd.mirror import Air
    rng = np.random.default_rng(seed)
    out = {}
    a = [int(v) for v in rng.integers(0, p, n)]
    order = [int(i) for i in rng.permutation(n)]
    out["perm"] = (Air(2), [a, [a[i] for i in order]], [("perm", [0], [1])])
    table = [int(v) for v in rng.permutation(4 * n)[:n]]
    looked = [table[int(i)] for i in rng.integers(0, n // 2, n)]
    air, cols, args = Air(3), [looked, table, [0] * n], [("lookup", [0], [1], 2)]
    cols[2] = xa.multiplicities(xa.widen(cols, air, p), args[0], 3)[0]
    out["lookup"] = (air, cols, args)
    sel = [int(v) for v in rng.integers(0, 2, n)]
    chosen = [a[r] for r in range(n) if sel[r]]
    chosen = [chosen[int(i)] for i in rng.permutation(len(chosen))]
    right, rsel = [int(v) for v in rng.integers(0, p, n)], [0] * n
    for v, r in zip(chosen, sorted(int(i) for i in rng.permutation(n)[:len(chosen)])):
        right[r], rsel[r] = v, 1
    out["perm_sel"] = (Air(4), [a, sel, right, rsel], [("perm", [0], [2], 1, 3)])
    P = min(n, 8)
    air = Air(2)
    vals = [int(v) for v in rng.permutation(4 * n)[:P]]
    s2 = [1] + [int(v) for v in rng.integers(0, 2, P - 1)]
    j0, j2 = air.periodic(vals), air.periodic(s2)
    good = [r for r in range(P) if s2[r]]
    cols = [[vals[good[int(i)]] for i in rng.integers(0, len(good), n)], [0] * n]
    args = [("lookup", [0], [("per", j0)], 1, None, ("per", j2))]
    cols[1] = xa.multiplicities(xa.widen(cols, air, p), args[0], 2)[0]
    out["lookup_per"] = (air, cols, args)
    return out


def readme_lists(n, p, seed=7):
    """-> {name: (air, cols, args)}: the two lists of README.md over traces of n rows that satisfy them -- "nine": a permutation
    of two columns and two lookups into one table column; "selectors": a selected lookup into a public (periodic) range table
    and a permutation between selected rows.  The multiplicity columns are filled."""
    from stark_rs_amd.mirror import Air
    rng = np.random.default_rng(seed)
    out = {}
    free = lambda: [int(v) for v in rng.integers(0, p, n)]
    order = [int(i) for i in rng.permutation(n)]
    c0, c1 = free(), free()
    table = [int(v) for v in rng.permutation(4 * n)[:n]]
    cols = [c0, c1, [c0[i] for i in order], [c1[i] for i in order], [table[int(i)] for i in rng.integers(0, n, n)], table, [0] * n,
            [table[int(i)] for i in rng.integers(0, max(1, n // 4), n)], [0] * n]
    air, args = Air(9), [("perm", [0, 1], [2, 3]), ("lookup", [4], [5], 6), ("lookup", [7], [5], 8)]
    for g in args[1:]:
        cols[g[3]] = xa.multiplicities(cols, g, 9)[0]
    out["nine"] = (air, cols, args)
    P = min(n, 256)
    air = Air(8)
    j = air.periodic(range(P))
    sel = [int(v) for v in rng.integers(0, 2, n)]
    looked = [int(rng.integers(0, P)) if sel[r] else p - 1 - r % 3 for r in range(n)]
    left, lsel = free(), [int(v) for v in rng.integers(0, 2, n)]
    chosen = [left[r] for r in range(n) if lsel[r]]
    chosen = [chosen[int(i)] for i in rng.permutation(len(chosen))]
    right, rsel = free(), [0] * n
    for v, r in zip(chosen, sorted(int(i) for i in rng.permutation(n)[:len(chosen)])):
        right[r], rsel[r] = v, 1
    cols = [looked, free(), [0] * n, sel, left, right, lsel, rsel]
    args = [("lookup", [0], [("per", j)], 2, 3, None), ("perm", [4], [5], 6, 7)]
    cols[2] = xa.multiplicities(xa.widen(cols, air, p), args[0], 8)[0]
    out["selectors"] = (air, cols, args)
    return out
