"""The checker of zero-knowledge DEEP proofs with an argument list (include/stark_mi.h, "Zero-knowledge DEEP proofs with an
argument list"), restated in Python ints over the CPU oracle's hash and the mirror's symbolic AIR, on top of the restatements
it joins: tests/zk_compose.py (the generator, k_s, the masked split, the mask), tests/deep_args_compose.py and
tests/xargs_compose.py (the widened trace, the columns from their recurrences, the record, the DEEP codeword with a list) and
tests/deep_fold4_compose.py (coset leaves, sections, fold-by-4 FRI).  New here: k_t = 8 t + 16, the derived AIR with both
exemption columns, the columns with their closing value and random tail, the three auxiliary quotients, prover and verifier.
The route is xargs_compose's: the two exemption columns are trace columns written out, extended like any column.
Not a test module: imported by tests/test_zk_args_emu.py and tests/test_gpu_zk_args.py."""
import copy

import numpy as np

import air_compose as ac
import deep_args_compose as da
import deep_compose as dc
import deep_fold4_compose as d4
import ext_compose as xc
import fold4_compose as f4
import perm_compose as pm
import xargs_compose as xa
import zk_compose as zk

STREAM_TAIL, STREAM_SALT_ARGS = 6, 7
ONE, ZERO = [1, 0, 0, 0], [0, 0, 0, 0]
_HEAD = "zk deep argument: "
FRONT = {"record": _HEAD + "the out-of-domain record is missing or has the wrong count",
         "record canonical": _HEAD + "an out-of-domain coordinate is not canonical",
         "base field": _HEAD + "the out-of-domain point z lies in the base field",
         "consistency": _HEAD + "out-of-domain consistency check fails: the derived AIR's constraints and the auxiliary quotients at z do not give the "
                                "masked segments' value",
         "no layer": _HEAD + "FRI has no fold at this shape (F = 0), so there is no layer-0 coset to compare the masked DEEP quotient with"}
WORDS = {k: "zk deep argument coset openings: " + v for k, v in
         {"length": "wrong length", "record": "malformed record", "path": "malformed path", "auth": "authentication path does not verify",
          "canonical": "an opened value is not canonical", "quotient": "the masked DEEP quotient of the opened cosets is not the codeword value"}.items()}
SENTENCES = set(FRONT.values()) | set(WORDS.values()) | f4.FRI_SENTENCES


# ---------------------------------------------------------------------------------------------- the plan
def k_t(t):
    return 8 * t + 16


k_s = zk.k_s


def contribution(arg):
    return 4 if arg[0] == "lookup" or len(arg) > 3 else 3


def plan(air, args, log_n, t):
    """-> (d, D', k_t, k_s) of smi_air_plan_deep_zk_xargs for a shape it accepts"""
    n = 1 << log_n
    d = max([air.degree + 1 if air.constraints else 1] + [contribution(g) for g in args])
    D = 1
    while D < d - 1:
        D <<= 1
    return d, -(-D * n // (n - k_s(t))), k_t(t), k_s(t)


def segments_unmasked(air, args):
    d = max([air.degree + 1 if air.constraints else 1] + [contribution(g) for g in args])
    D = 1
    while D < d - 1:
        D <<= 1
    return D


# ---------------------------------------------------------------------------------------------- the derived AIR
def exemption_columns(n, t, p, tau, w):
    """-> (E(tau w^r), E_A(tau w^r)) for r < n: the roots of E are the rows n_a - 1 .. n - 2, those of E_A the rows n_a .. n - 1"""
    na = n - k_t(t)
    pts = [tau * pow(w, r, p) % p for r in range(n)]

    def col(roots):
        out = []
        for r in range(n):
            v = 1
            for q in roots:
                v = v * (pts[r] - pts[q]) % p
            out.append(v)
        return out
    return col(range(na - 1, n - 1)), col(range(na, n))


def derived_air(air, log_n, t, p, tau, w):
    """the AIR the library composes: air with the two exemption columns as periodic columns Q and Q + 1, the first a factor of
    every transition term; without the list"""
    E, EA = exemption_columns(1 << log_n, t, p, tau, w)
    out = copy.deepcopy(air)
    out.args = []
    j = out.periodic(E)
    out._symbolic = [[(cf, list(factors) + [("per", j, 1)]) for cf, factors in con] for con in out._symbolic]
    out.periodic(EA)
    return out


def randomised(cols, seed_rows, t):
    """the trace with the last k_t rows of every column replaced: column c takes seed_rows[c k_t .. (c + 1) k_t)"""
    kt = k_t(t)
    return [list(c[:len(c) - kt]) + [int(v) for v in seed_rows[i * kt:(i + 1) * kt]] for i, c in enumerate(cols)]


# ---------------------------------------------------------------------------------------------- the columns
def columns(wide, args, ch, p, g, W, t, tail):
    """the A columns over the (randomised, widened) trace -> (c (4 A, n) with the random tail, [closes], closing values, None), or
    (None, None, None, key) when a denominator is zero in any of the n rows.  tail: 4 A (k_t - 1) values of stream 6."""
    n, kt = len(wide[0]), k_t(t)
    na = n - kt
    c, _wrap, zero = xa.columns(wide, args, ch, p, g, W)
    if zero is not None:
        return None, None, None, zero
    c = np.array(c, dtype=np.uint64)
    closing = [[int(v) for v in c[4 * a:4 * a + 4, na]] for a in range(len(args))]
    closes = [closing[a] == (ONE if arg[0] == "perm" else ZERO) for a, arg in enumerate(args)]
    for col in range(4 * len(args)):
        c[col, na + 1:] = [int(v) for v in tail[col * (kt - 1):(col + 1) * (kt - 1)]]
    return c, closes, closing, None


# ---------------------------------------------------------------------------------------------- the auxiliary quotients
def aux_terms(o, lde_wide, cl, args, ch, wch_aux, p, g, log_n, lb, tau, h, W, t, ea_index, omit_cq=False, no_ea=False):
    """the 3 A auxiliary quotients on the N points as (4, N): bq_a, wq_a = E_A T_a / (x^n - tau^n), cq_a under the weights
    12 a, 12 a + 4, 12 a + 8 of wch_aux.  lde_wide: the extension of the widened trace, whose row ea_index is E_A's.
    omit_cq / no_ea: the dishonest provers"""
    P = np.uint64(p)
    n, B, N = 1 << log_n, 1 << lb, 1 << (log_n + lb)
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    lde_wide, cl = np.asarray(lde_wide, dtype=np.uint64), np.asarray(cl, dtype=np.uint64)
    nxt = np.roll(cl, -B, axis=1)
    idx = np.arange(N)
    x = dc.points(o, p, g, log_n, lb, h)
    tna = tau * pow(w, n - k_t(t), p) % p
    ict = np.array([pow((int(xi) - tna) % p, p - 2, p) for xi in x], dtype=np.uint64)
    ea = np.ones(N, dtype=np.uint64) if no_ea else lde_wide[ea_index]
    total = np.zeros((4, N), dtype=np.uint64)
    zero4 = [0, 0, 0, 0]
    for a, arg in enumerate(args):
        wb, wt, wc = (list(wch_aux[12 * a + 4 * k:12 * a + 4 * k + 4]) for k in range(3))
        ca, cn = cl[4 * a:4 * a + 4], nxt[4 * a:4 * a + 4]
        bq = xa.aux_terms_at(idx, lde_wide, ca, cn, [arg], ch, wb + zero4, p, g, wN, log_n, tau, h, W)
        wq = xa.aux_terms_at(idx, lde_wide, ca, cn, [arg], ch, zero4 + wt, p, g, wN, log_n, tau, h, W) * ea % P
        total = (total + bq + wq) % P
        if not omit_cq:
            num = ca.copy()
            if arg[0] == "perm":
                num[0] = (num[0] + P - np.uint64(1)) % P
            total = (total + xc.mul_arr(num * ict % P, [int(v) % p for v in wc], p, g)) % P
    return total


def aux_at_z(o, dair, args, ch, z, u, a_vals, b_vals, p, g, log_n, tau, t):
    """-> [(bq_a, wq_a, cq_a)] at z: da.aux_at_z's two with E_A(z) on the second, and the closing quotient"""
    n = 1 << log_n
    w = o.ff_prim_nth_root_g(n, p, g)
    na = n - k_t(t)
    ea = list(ONE)
    for r in range(na, n):
        ea = xc.mul(ea, xc.sub(z, xc.embed(tau * pow(w, r, p) % p, p), p), p, g)
    ict = xc.inv(xc.sub(z, xc.embed(tau * pow(w, na, p) % p, p), p), p, g)
    out = []
    for k, (bq, wq) in enumerate(da.aux_at_z(o, dair, args, ch, z, u, a_vals, b_vals, p, g, log_n, tau)):
        init = ONE if args[k][0] == "perm" else ZERO
        out.append((bq, xc.mul(wq, ea, p, g), xc.mul(xc.sub(a_vals[k], init, p), ict, p, g)))
    return out


def ood_lhs(o, dair, args, W, ch, weights, z, ood, p, g, log_n, tau, t):
    """the left side of the consistency check over the derived AIR"""
    A, K = len(args), len(dair.constraints)
    el = lambda v, i: [int(c) % p for c in v[4 * i:4 * i + 4]]
    lhs, _ = dc.ood_sides(o, dair, W, 0, weights[:4 * (W + K)], z, list(ood[:8 * W]), p, g, log_n, tau)
    u = [el(ood, c) for c in range(W)]
    a_vals, b_vals = [el(ood, 2 * W + a) for a in range(A)], [el(ood, 2 * W + A + a) for a in range(A)]
    for a, qs in enumerate(aux_at_z(o, dair, args, ch, z, u, a_vals, b_vals, p, g, log_n, tau, t)):
        for k in range(3):
            lhs = xc.add(lhs, xc.mul(el(weights, W + K + 3 * a + k), qs[k], p, g), p)
    return lhs


# ---------------------------------------------------------------------------------------------- the proof
def layout(W, A, Dp, log_n, lb, t):
    """-> (folds, proof bytes) from the formula of the header section"""
    N, B, log_N = 1 << (log_n + lb), 1 << lb, log_n + lb
    _R2, F, _last, fri = f4.layout(N, B, t)
    return F, 9 + 32 * (2 * W + 2 * A + Dp) + fri + sum(d4.section_len(V, t, log_N) for V in (W + 1, 4 * A + 1, 4 * Dp + 5))


def offsets(W, A, Dp, log_n, lb, t):
    """-> {name: byte offset}: a_0 and b_0 in the record, s_0, the FRI part, and per group its first record and first path"""
    N, B, log_N = 1 << (log_n + lb), 1 << lb, log_n + lb
    out = {"a0": 9 + 32 * 2 * W, "b0": 9 + 32 * (2 * W + A), "s0": 9 + 32 * (2 * W + 2 * A), "fri": 9 + 32 * (2 * W + 2 * A + Dp)}
    at = out["fri"] + f4.layout(N, B, t)[3]
    for k, V in enumerate([W + 1, 4 * A + 1, 4 * Dp + 5]):
        out[f"rec {k}"], out[f"path {k}"] = at, at + t * (9 + 32 * V)
        at += d4.section_len(V, t, log_N)
    out["end"] = at
    return out


def prove(o, air, args, cols, seed, p, g, log_n, lb, t, tau, h, bits=0, omit_cq=False, no_ea=False, commit_as=None):
    """-> dict(roots, proof, top, ood, trace, closes, c, ...) of smi_dev_air_prove_deep_zk_xargs.  omit_cq: a dishonest prover
    that composes without the closing quotients (it relies on the wrap); no_ea: one that composes the wrapping transition
    quotient without E_A.  Both keep every other step."""
    n, N, B = 1 << log_n, 1 << (log_n + lb), 1 << lb
    W, K, A = len(cols), len(air.constraints), len(args)
    kt, ks = k_t(t), k_s(t)
    NW = W + K + 3 * A
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    dair = derived_air(air, log_n, t, p, tau, w)
    D = segments_unmasked(air, args)
    Dp = -(-D * n // (n - ks))
    assert D <= B and 4 * Dp + 5 <= 64 and d4.folds(log_n, lb, t) >= 1 and kt < n // 2
    trace = randomised(cols, zk.rng(o, seed, zk.STREAM_ROWS, W * kt, p), t)
    wide = xa.widen(trace, dair, p)
    lde_wide = np.asarray(ac.lde(o, wide, p, g, log_n, lb, tau, h), dtype=np.uint64)
    lde = [lde_wide[c] for c in range(W)]
    held1, nodes1 = d4._commit(o, 0, lde + [np.array(zk.rng(o, seed, zk.STREAM_SALT1, N, p), dtype=np.uint64)], N, commit_as)
    root1 = bytes(nodes1[-1])
    tr, ch = pm.challenges(o, root1)
    c, closes, closing, zero = columns(wide, args, ch, p, g, W, t, zk.rng(o, seed, STREAM_TAIL, 4 * A * (kt - 1), p))
    assert zero is None, zero
    cl = [np.asarray(col, dtype=np.uint64) for col in ac.lde(o, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)]
    held2, nodes2 = d4._commit(o, 1, cl + [np.array(zk.rng(o, seed, STREAM_SALT_ARGS, N, p), dtype=np.uint64)], N, commit_as)
    root2 = bytes(nodes2[-1])
    tr, wch = pm.weights(o, tr, root2, NW)
    H = dc.composition(o, dair, trace, wch[:4 * (W + K)], p, g, log_n, lb, tau, h)
    H = (H + aux_terms(o, lde_wide, cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W, t, len(wide) - 1, omit_cq, no_ea)) % np.uint64(p)
    hc = np.stack([np.asarray(o.fast_intt(H[e], wN, h, p), dtype=np.uint64) for e in range(4)])
    honest = all(closes) and not omit_cq and not no_ea
    assert not honest or not hc[:, D * n:].any(), "the composition has coefficients at or above D n"
    segc = zk.split(hc, D * n, log_n, ks, Dp, zk.rng(o, seed, zk.STREAM_RHO, 4 * (Dp - 1) * ks, p), p)
    mask = zk.rng(o, seed, zk.STREAM_MASK, 4 * n, p)
    coefs = segc + [mask[e * n:(e + 1) * n] for e in range(4)]
    seg = [np.asarray(o.fast_coset_ntt(np.array(col, dtype=np.uint64), N, wN, h, p), dtype=np.uint64) for col in coefs]
    held3, nodes3 = d4._commit(o, 2, seg + [np.array(zk.rng(o, seed, zk.STREAM_SALT2, N, p), dtype=np.uint64)], N, commit_as)
    root3 = bytes(nodes3[-1])
    tr = bytearray(tr) + root3
    first = 8 + 4 * NW
    z = [v % p for v in dc.draw(o, tr, first, 4)]
    assert any(z[1:]), "z lies in the base field"
    uvab = da.ood_values(o, trace, c, np.zeros((4, 0), dtype=np.uint64), 0, z, p, g, log_n, tau)
    s = [dc.horner([[segc[4 * j + e][i] for e in range(4)] for i in range(n)], z, p, g) for j in range(Dp)]
    ood = uvab + [x for el in s for x in el]
    record = xc._elems(ood)
    tr += record[9:]
    gammas = dc.draw(o, tr, first + 4, len(ood))
    Q = da.q_codeword(lde, cl, np.stack(seg[:4 * Dp]), dc.points(o, p, g, log_n, lb, h), z, ood, gammas, w, p, g)
    Q = (Q + np.stack(seg[4 * Dp:])) % np.uint64(p)
    fri, top, _nonce = f4.prove(o, o.fri_cfg(wN, h, N, B, t, p), Q, g, bytes(tr), bits)
    held, trees = [held1, held2, held3], [nodes1, nodes2, nodes3]
    secs = [d4.section(o, held[k], trees[k], top, N) for k in range(3)]
    return {"roots": [root1, root2, root3], "proof": record + fri + b"".join(secs), "top": top, "ood": ood, "trace": trace, "Dp": Dp, "closes": closes,
            "closing": closing, "c": c, "groups": held, "ch": ch}


def verify(o, air, args, proof, roots, p, g, W, log_n, lb, t, tau, h, bits=0):
    """-> (accept, sentence) of smi_air_verify_deep_zk_xargs, in its order"""
    n, N, B, log_N, K, A = 1 << log_n, 1 << (log_n + lb), 1 << lb, log_n + lb, len(air.constraints), len(args)
    ks = k_s(t)
    NW = W + K + 3 * A
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    dair = derived_air(air, log_n, t, p, tau, w)
    D = segments_unmasked(air, args)
    Dp = -(-D * n // (n - ks))
    cnt = 4 * (2 * W + 2 * A + Dp)
    obj = xc._pop(proof, 0)
    if obj is None or obj[0] != 2 or len(obj[1]) != cnt:
        return False, FRONT["record"]
    ood, at = obj[1], obj[2]
    if any(v >= p for v in ood):
        return False, FRONT["record canonical"]
    tr, ch = pm.challenges(o, bytes(roots[0]))
    tr, weights = pm.weights(o, tr, bytes(roots[1]), NW)
    tr = bytearray(tr) + bytes(roots[2])
    first = 8 + 4 * NW
    z = [c % p for c in dc.draw(o, tr, first, 4)]
    if not any(z[1:]):
        return False, FRONT["base field"]
    tr += proof[9:at]
    gammas = dc.draw(o, tr, first + 4, cnt)
    lhs = ood_lhs(o, dair, args, W, ch, weights, z, ood, p, g, log_n, tau, t)
    rhs, pw, zl = [0, 0, 0, 0], [1, 0, 0, 0], xc.power(z, n - ks, p, g)
    for j in range(Dp):
        rhs = xc.add(rhs, xc.mul(pw, [int(c) for c in ood[4 * (2 * W + 2 * A + j):4 * (2 * W + 2 * A + j) + 4]], p, g), p)
        pw = xc.mul(pw, zl, p, g)
    if [int(c) for c in lhs] != rhs:
        return False, FRONT["consistency"]
    if d4.folds(log_n, lb, t) == 0:
        return False, FRONT["no layer"]
    ok, pv, used, top, why = f4.verify(o, o.fri_cfg(wN, h, N, B, t, p), proof[at:], g, bytes(tr), bits)
    if not ok:
        return False, why
    widths = [W + 1, 4 * A + 1, 4 * Dp + 5]
    rest = proof[at + used:]
    if len(rest) != sum(d4.section_len(V, t, log_N) for V in widths):
        return False, WORDS["length"]
    q, depth = N // 4, log_N - 2
    recs, paths, off = [], [], 0
    for V in widths:
        rec, prec = 9 + 32 * V, 9 + 32 * depth
        rs, ps = [], []
        for s in range(t):
            r = rest[off + s * rec:off + (s + 1) * rec]
            if r[0] != 2 or int.from_bytes(r[1:9], "little") != 4 * V:
                return False, WORDS["record"]
            rs.append([int.from_bytes(r[9 + 8 * i:17 + 8 * i], "little") for i in range(4 * V)])
        for s in range(t):
            r = rest[off + t * rec + s * prec:off + t * rec + (s + 1) * prec]
            if r[0] != 3 or int.from_bytes(r[1:9], "little") != depth:
                return False, WORDS["path"]
            ps.append([bytes(r[9 + 32 * i:41 + 32 * i]) for i in range(depth)])
        recs.append(rs)
        paths.append(ps)
        off += t * (rec + prec)
    for k in range(3):                                       # the leaf is the record's u64s as they stand, salts included
        for s in range(t):
            if not o.merkle_verify(o.hash_from_field_elements(recs[k][s]), top[s] % q, paths[k][s], bytes(roots[k])):
                return False, WORDS["auth"]
    if any(v >= p for rs in recs for r in rs for v in r[:-4]):          # the salts are not looked at
        return False, WORDS["canonical"]
    iota = pow(wN, q, p)
    for s in range(t):
        a = top[s] % q
        for j in range(4):
            x = h * pow(wN, a, p) % p * pow(iota, j, p) % p
            trow = [recs[0][s][4 * c + j] for c in range(W)]
            crow = [recs[1][s][4 * c + j] for c in range(4 * A)]
            srow = [recs[2][s][4 * c + j] for c in range(4 * Dp)]
            got = da.q_at(trow, crow, srow, x, z, ood, gammas, w, p, g)
            got = [(got[e] + recs[2][s][4 * (4 * Dp + e) + j]) % p for e in range(4)]
            idx, want = pv[4 * s + j]
            assert idx == a + j * q
            if got != [int(c) for c in want]:
                return False, WORDS["quotient"]
    return True, ""


# ---------------------------------------------------------------------------------------------- statements
def statement(air, cols, args, log_n, t, p):
    """a list's trace made a statement of this variant: the multiplicity columns recounted over the active rows alone, so that
    every argument that closed over n rows for a reason that survives the cut closes over n_a rows.  A permutation closes over
    the active rows only when both sides hold the same multiset there; `vm` below builds such traces."""
    n = 1 << log_n
    na = n - k_t(t)
    cols = [list(c) for c in cols]
    head = [c[:na] for c in xa.widen(cols, air, p)]
    for g in args:
        if g[0] == "lookup":
            M, missing = xa.multiplicities(head, g, len(cols))
            assert missing is None, missing
            cols[g[3]] = M + [0] * (n - na)
    return cols


def vm(log_n, t, p, seed=7):
    """README's 9-column `vm` list (one permutation of two columns, two lookups into one table column) over a trace whose
    arguments close over the n_a active rows; the tail rows hold anything (here: values that are in no table)"""
    from stark_rs_amd.mirror import Air
    n = 1 << log_n
    na = n - k_t(t)
    rng = np.random.default_rng(seed)
    free = lambda: [int(v) for v in rng.integers(0, p, na)]
    order = [int(i) for i in rng.permutation(na)]
    c0, c1 = free(), free()
    table = [int(v) for v in rng.permutation(4 * n)[:na]]
    head = [c0, c1, [c0[i] for i in order], [c1[i] for i in order], [table[int(i)] for i in rng.integers(0, na, na)], table, [0] * na,
            [table[int(i)] for i in rng.integers(0, max(1, na // 4), na)], [0] * na]
    cols = [c + [p - 1 - (i + r) % 7 for r in range(n - na)] for i, c in enumerate(head)]
    air, args = Air(9), [("perm", [0, 1], [2, 3]), ("lookup", [4], [5], 6), ("lookup", [7], [5], 8)]
    return air, statement(air, cols, args, log_n, t, p), args


def selectors(log_n, t, p, seed=11):
    """a list with a trace selector, a periodic selector and a periodic table of period 16: a selected lookup into the public
    table, a lookup into it under a periodic selector, and a permutation between selected rows; closes over the active rows"""
    from stark_rs_amd.mirror import Air
    n = 1 << log_n
    na = n - k_t(t)
    rng = np.random.default_rng(seed)
    P = 16
    air = Air(9)
    vals = [int(v) for v in rng.permutation(4 * n)[:P]]
    s2 = [1, 0] * (P // 2)
    j0, j2 = air.periodic(vals), air.periodic(s2)
    free = lambda: [int(v) for v in rng.integers(0, p, n)]
    sel = [int(v) for v in rng.integers(0, 2, n)]
    looked = [vals[int(rng.integers(0, P))] if sel[r] else p - 1 - r % 3 for r in range(n)]
    looked2 = [vals[int(rng.integers(0, P))] if s2[r % P] else p - 2 - r % 5 for r in range(n)]
    left, lsel = free(), [int(v) for v in rng.integers(0, 2, na)] + [0] * (n - na)
    chosen = [left[r] for r in range(na) if lsel[r]]
    chosen = [chosen[int(i)] for i in rng.permutation(len(chosen))]
    right, rsel = free(), [0] * n
    for v, r in zip(chosen, sorted(int(i) for i in rng.permutation(na)[:len(chosen)])):
        right[r], rsel[r] = v, 1
    cols = [looked, looked2, [0] * n, sel, left, right, lsel, rsel, [0] * n]
    args = [("lookup", [0], [("per", j0)], 2, 3, None), ("perm", [4], [5], 6, 7), ("lookup", [1], [("per", j0)], 8, ("per", j2), None)]
    return air, statement(air, cols, args, log_n, t, p), args
