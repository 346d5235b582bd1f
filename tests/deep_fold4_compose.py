"""The checker of out-of-domain sampling over coset leaves (include/stark_mi.h, "Out-of-domain sampling over coset leaves"),
restated in Python from the three restatements it joins: tests/deep_compose.py and tests/deep_args_compose.py (transcripts,
composition, segments, values at z, the DEEP codeword, the consistency check, Q at one point) and tests/fold4_compose.py
(extension FRI at folding factor 4).  What is new here is small: a group of columns committed as a tree of coset leaves --
leaf i is the oracle's Hash::from_field_elements of the 4 V values, column c at i + j N / 4 being value 4 c + j --, the
opening sections of one record and one path per test and group, and the verifier's comparison of Q at the four points of a
coset, point by point through the existing q_at, with the layer-0 coset record of FRI.
Not a test module: imported by tests/test_deep_fold4_host.py, tests/test_deep_fold4_emu.py, tests/test_gpu_deep_fold4.py and
tests/test_gpu_boundary_primes_deep_fold4.py."""
import numpy as np

import air_compose as ac
import deep_args_compose as da
import deep_compose as dc
import ext_compose as xc
import fold4_compose as f4
import perm_compose as pm
import xargs_compose as xa

# every sentence the two verifiers can give that is not one of the FRI walk's (f4.FRI_SENTENCES)
FRONT = {"record": "deep: the out-of-domain record is missing or has the wrong count",
         "record canonical": "deep: an out-of-domain coordinate is not canonical",
         "base field": "deep: the out-of-domain point z lies in the base field",
         "consistency": "deep: out-of-domain consistency check fails: the constraints at z do not give the segments' value",
         "consistency args": "deep arguments: out-of-domain consistency check fails: the constraints and the auxiliary quotients at z do not give the "
                             "segments' value",
         "no layer": "deep fold4: FRI has no fold at this shape (F = 0), so there is no layer-0 coset to compare the DEEP quotient with"}
_TAILS = {"length": "wrong length", "record": "malformed record", "path": "malformed path", "auth": "authentication path does not verify",
          "canonical": "an opened value is not canonical", "quotient": "the DEEP quotient of the opened cosets is not the codeword value"}
WORDS = {k: "deep coset openings: " + v for k, v in _TAILS.items()}
ARGS_WORDS = {k: "deep argument coset openings: " + v for k, v in _TAILS.items()}
SENTENCES = set(FRONT.values()) | set(WORDS.values()) | set(ARGS_WORDS.values()) | f4.FRI_SENTENCES


# ---------------------------------------------------------------------------------------------- coset leaves
def coset_view(cols, N):
    """V columns of N values -> (4 V, N / 4): row 4 c + j is column c at the indices j q .. j q + q - 1, a leaf's value order"""
    a = np.stack([np.asarray(c, dtype=np.uint64)[:N] for c in cols])
    return np.ascontiguousarray(a.reshape(len(cols), 4, N // 4).reshape(4 * len(cols), N // 4))


def coset_leaves(o, cols, N):
    """(N / 4, 32) digests: leaf i = Hash::from_field_elements of the group's 4 V values at the coset of i"""
    return o.row_hashes(coset_view(cols, N))


def coset_tree(o, cols, N):
    return o.merkle_new(coset_leaves(o, cols, N))


def coset_record(cols, a, N):
    q = N // 4
    return [int(col[a + j * q]) for col in cols for j in range(4)]


def section(o, cols, nodes, top, N):
    """one group's opening section: t records of 4 V values, then t paths of log2 N - 2 digests, at a = top mod N / 4"""
    q = N // 4
    out = bytearray()
    for s in top:
        out += xc._elems(coset_record(cols, int(s) % q, N))
    for s in top:
        out += xc._path(o.merkle_open(nodes, q, int(s) % q))
    return bytes(out)


def section_len(V, t, log_N):
    return t * (9 + 32 * V) + t * (9 + 32 * (log_N - 2))


def layout(W, A, D, log_n, lb, t):
    """-> (folds, proof bytes) from the formula of the header section; A = 0: a plain AIR"""
    N, B, log_N = 1 << (log_n + lb), 1 << lb, log_n + lb
    _R2, F, _last, fri = f4.layout(N, B, t)
    groups = [W, 4 * D] if A == 0 else [W, 4 * A, 4 * D]
    return F, 9 + 32 * (2 * W + 2 * A + D) + fri + sum(section_len(V, t, log_N) for V in groups)


def folds(log_n, lb, t):
    return f4.layout(1 << (log_n + lb), 1 << lb, t)[1]


# tampering with what is committed (commit_as of prove / prove_args): the tree and the opened records hold the tampered
# columns, every other step the true ones
def plus_p(group, col, p):
    """column `col` of group `group` committed and opened as value + p: the same residues under a tree over the raw u64, so
    every path verifies and only the canonical check can refuse the proof"""
    def f(k, cols):
        return [np.asarray(c, dtype=np.uint64) + np.uint64(p if (k == group and j == col) else 0) for j, c in enumerate(cols)]
    return f


def swapped(group, col):
    """column `col` of group `group` committed with the coset points 0 and 1 of every leaf exchanged: every path verifies,
    every value is canonical, and only Q at those two points can refuse the proof"""
    def f(k, cols):
        out = [np.asarray(c, dtype=np.uint64).copy() for c in cols]
        if k == group:
            q = len(out[col]) // 4
            out[col][:q], out[col][q:2 * q] = out[col][q:2 * q].copy(), out[col][:q].copy()
        return out
    return f


def _commit(o, k, cols, N, commit_as):
    held = commit_as(k, cols) if commit_as else [np.asarray(c, dtype=np.uint64) for c in cols]
    return held, coset_tree(o, held, N)


# ---------------------------------------------------------------------------------------------- the two provers
def prove(o, air, cols, p, g, log_n, lb, t, tau, h, bits=0, commit_as=None):
    """-> dict(roots, proof, top, ood, ...) of smi_dev_air_prove_deep_fold4: dc.prove with coset trees, f4.prove and section()"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K = len(cols), len(air.constraints)
    _d, D = dc.plan(air)
    assert D <= B and B >= 4 and 4 * D <= 64 and folds(log_n, lb, t) >= 1
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    lde = ac.lde(o, cols, p, g, log_n, lb, tau, h)
    held1, nodes1 = _commit(o, 0, lde, N, commit_as)
    root1 = bytes(nodes1[-1])
    tr, ch = xc.air_transcript(o, W, K, root1)
    tr = bytearray(tr)
    H = dc.composition(o, air, cols, ch, p, g, log_n, lb, tau, h)
    hc, seg = dc.segments(o, H, D, p, g, log_n, lb, h)
    assert not hc[:, D << log_n:].any(), "the composition has coefficients at or above D n"
    held2, nodes2 = _commit(o, 1, list(seg), N, commit_as)
    root2 = bytes(nodes2[-1])
    tr += root2
    z = [c % p for c in dc.draw(o, tr, 4 * (W + K), 4)]
    assert any(z[1:]), "z lies in the base field"
    ood = dc.ood_values(o, cols, hc, D, z, p, g, log_n, tau)
    record = xc._elems(ood)
    tr += record[9:]
    gammas = dc.draw(o, tr, 4 * (W + K) + 4, 4 * (2 * W + D))
    Q = dc.q_codeword(lde, seg, dc.points(o, p, g, log_n, lb, h), z, ood, gammas, w, p, g)
    fri, top, _nonce = f4.prove(o, o.fri_cfg(wN, h, N, B, t, p), Q, g, bytes(tr), bits)
    secs = [section(o, held1, nodes1, top, N), section(o, held2, nodes2, top, N)]
    return {"roots": [root1, root2], "proof": record + fri + secs[0] + secs[1], "top": top, "ood": ood, "sections": secs, "fri_len": len(fri),
            "groups": [held1, held2], "trees": [nodes1, nodes2]}


def prove_args(o, air, args, cols, p, g, log_n, lb, t, tau, h, bits=0, honest=True, commit_as=None):
    """-> dict(roots, proof, top, ood, closes, ...) of smi_dev_air_prove_deep_xargs_fold4: da.prove in the same way"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K, A = len(cols), len(air.constraints), len(args)
    _d, D = da.plan(air, args)
    assert D <= B and B >= 4 and 4 * D <= 64 and folds(log_n, lb, t) >= 1
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    wide = xa.widen(cols, air, p)
    lde_wide = ac.lde(o, wide, p, g, log_n, lb, tau, h)
    lde = [np.asarray(c, dtype=np.uint64) for c in lde_wide[:W]]
    held1, nodes1 = _commit(o, 0, lde, N, commit_as)
    root1 = bytes(nodes1[-1])
    tr, ch = pm.challenges(o, root1)
    c, closes, zero = xa.columns(wide, args, ch, p, g, W)
    assert zero is None, zero
    cl = [np.asarray(col, dtype=np.uint64) for col in ac.lde(o, [[int(v) for v in c[e]] for e in range(4 * A)], p, g, log_n, lb, tau, h)]
    held2, nodes2 = _commit(o, 1, cl, N, commit_as)
    root2 = bytes(nodes2[-1])
    tr, wch = pm.weights(o, tr, root2, W + K + 2 * A)
    H = pm.main_codeword(o, air, cols, wch[:4 * (W + K)], p, g, log_n, lb, tau, h, True)
    H = (H + xa.aux_terms(o, np.asarray(lde_wide, dtype=np.uint64), cl, args, ch, wch[4 * (W + K):], p, g, log_n, lb, tau, h, W)) % np.uint64(p)
    hc, seg = dc.segments(o, H, D, p, g, log_n, lb, h)
    assert not honest or not hc[:, D << log_n:].any(), "the composition has coefficients at or above D n"
    held3, nodes3 = _commit(o, 2, list(seg), N, commit_as)
    root3 = bytes(nodes3[-1])
    tr = bytearray(tr) + root3
    first = 8 + 4 * (W + K + 2 * A)
    z = [v % p for v in dc.draw(o, tr, first, 4)]
    assert any(z[1:]), "z lies in the base field"
    ood = da.ood_values(o, cols, c, hc, D, z, p, g, log_n, tau)
    record = xc._elems(ood)
    tr += record[9:]
    gammas = dc.draw(o, tr, first + 4, da.record_len(W, A, D))
    assert len(tr) == da.transcript_len(W, K, A, D)
    Q = da.q_codeword(lde, cl, seg, dc.points(o, p, g, log_n, lb, h), z, ood, gammas, w, p, g)
    fri, top, _nonce = f4.prove(o, o.fri_cfg(wN, h, N, B, t, p), Q, g, bytes(tr), bits)
    held, trees = [held1, held2, held3], [nodes1, nodes2, nodes3]
    secs = [section(o, held[k], trees[k], top, N) for k in range(3)]
    return {"roots": [root1, root2, root3], "proof": record + fri + b"".join(secs), "top": top, "ood": ood, "closes": closes, "sections": secs,
            "fri_len": len(fri), "groups": held, "trees": trees}


# ---------------------------------------------------------------------------------------------- the verifier
def verify(o, air, args, proof, roots, p, g, W, log_n, lb, t, tau, h, bits=0):
    """-> (accept, sentence) of smi_air_verify_deep_fold4 (args None) or smi_air_verify_deep_xargs_fold4, in their order"""
    N, B, log_N, K = 1 << (log_n + lb), 1 << lb, log_n + lb, len(air.constraints)
    A = len(args) if args is not None else 0
    _d, D = da.plan(air, args) if A else dc.plan(air)
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cnt = 4 * (2 * W + 2 * A + D)
    obj = xc._pop(proof, 0)
    if obj is None or obj[0] != 2 or len(obj[1]) != cnt:
        return False, FRONT["record"]
    ood, at = obj[1], obj[2]
    if any(v >= p for v in ood):
        return False, FRONT["record canonical"]
    if A:
        tr, ch = pm.challenges(o, bytes(roots[0]))
        tr, weights = pm.weights(o, tr, bytes(roots[1]), W + K + 2 * A)
        tr = bytearray(tr) + bytes(roots[2])
        first = 8 + 4 * (W + K + 2 * A)
    else:
        tr, weights = xc.air_transcript(o, W, K, bytes(roots[0]))
        tr = bytearray(tr) + bytes(roots[1])
        first = 4 * (W + K)
    z = [c % p for c in dc.draw(o, tr, first, 4)]
    if not any(z[1:]):
        return False, FRONT["base field"]
    tr += proof[9:at]
    gammas = dc.draw(o, tr, first + 4, cnt)
    if A:
        lhs, rhs = da.ood_sides(o, air, args, W, D, ch, weights, z, ood, p, g, log_n, tau)
    else:
        lhs, rhs = dc.ood_sides(o, air, W, D, weights, z, ood, p, g, log_n, tau)
    if lhs != rhs:
        return False, FRONT["consistency args" if A else "consistency"]
    if folds(log_n, lb, t) == 0:
        return False, FRONT["no layer"]
    ok, pv, used, top, why = f4.verify(o, o.fri_cfg(wN, h, N, B, t, p), proof[at:], g, bytes(tr), bits)
    if not ok:
        return False, why
    say = ARGS_WORDS if A else WORDS
    widths = [W, 4 * A, 4 * D] if A else [W, 4 * D]
    rest = proof[at + used:]
    if len(rest) != sum(section_len(V, t, log_N) for V in widths):
        return False, say["length"]
    q, depth = N // 4, log_N - 2
    recs, paths, off = [], [], 0
    for V in widths:                                         # group by group: every record, then every path
        rec, prec = 9 + 32 * V, 9 + 32 * depth
        rs, ps = [], []
        for s in range(t):
            r = rest[off + s * rec:off + (s + 1) * rec]
            if r[0] != 2 or int.from_bytes(r[1:9], "little") != 4 * V:
                return False, say["record"]
            rs.append([int.from_bytes(r[9 + 8 * i:17 + 8 * i], "little") for i in range(4 * V)])
        for s in range(t):
            r = rest[off + t * rec + s * prec:off + t * rec + (s + 1) * prec]
            if r[0] != 3 or int.from_bytes(r[1:9], "little") != depth:
                return False, say["path"]
            ps.append([bytes(r[9 + 32 * i:41 + 32 * i]) for i in range(depth)])
        recs.append(rs)
        paths.append(ps)
        off += t * (rec + prec)
    for k in range(len(widths)):                             # the leaf is the record's u64s as they stand
        for s in range(t):
            if not o.merkle_verify(o.hash_from_field_elements(recs[k][s]), top[s] % q, paths[k][s], bytes(roots[k])):
                return False, say["auth"]
    if any(v >= p for rs in recs for r in rs for v in r):
        return False, say["canonical"]
    iota = pow(wN, q, p)
    for s in range(t):
        a = top[s] % q
        for j in range(4):
            x = h * pow(wN, a, p) % p * pow(iota, j, p) % p
            rows = [[recs[k][s][4 * c + j] for c in range(V)] for k, V in enumerate(widths)]
            got = da.q_at(rows[0], rows[1], rows[2], x, z, ood, gammas, w, p, g) if A else dc.q_at(rows[0], rows[1], x, z, ood, gammas, w, p, g)
            idx, want = pv[4 * s + j]
            assert idx == a + j * q
            if got != [int(c) for c in want]:
                return False, say["quotient"]
    return True, ""


# ---------------------------------------------------------------------------------------------- tampering
def object_offsets(W, A, D, log_n, lb, t):
    """-> {name: byte offset} of the places a tampering test touches: the out-of-domain record, the FRI part, and per group
    k the first record ("rec k") and the first path ("path k") of its section"""
    N, B, log_N = 1 << (log_n + lb), 1 << lb, log_n + lb
    out = {"ood": 0, "fri": 9 + 32 * (2 * W + 2 * A + D)}
    at = out["fri"] + f4.layout(N, B, t)[3]
    out["sections"] = at
    for k, V in enumerate([W, 4 * D] if A == 0 else [W, 4 * A, 4 * D]):
        out[f"rec {k}"] = at
        out[f"path {k}"] = at + t * (9 + 32 * V)
        at += section_len(V, t, log_N)
    out["end"] = at
    return out


def mutations(proof, W, A, D, log_n, lb, t, p):
    """-> [(name, mutated proof, sentence)]: the classes whose sentence does not depend on the data -- the record's count and a
    coordinate + p, a cut and an appended byte, and for every group a record's tag and count, a path's tag and count, a
    flipped value (the leaf no longer hashes to the tree), a flipped digest, a value swapped between two coset points of one
    column (likewise), and a value + p (likewise: the record is hashed as it stands, before the canonical check)"""
    off = object_offsets(W, A, D, log_n, lb, t)
    say = ARGS_WORDS if A else WORDS
    assert len(proof) == off["end"]
    out = []

    def put(name, at, new, why):
        m = bytearray(proof)
        m[at:at + len(new)] = new
        out.append((name, bytes(m), why))
    put("record count", 1, (int.from_bytes(proof[1:9], "little") - 1).to_bytes(8, "little"), FRONT["record"])
    put("record tag", 0, b"\x03", FRONT["record"])
    put("ood + p", 9, (int.from_bytes(proof[9:17], "little") + p).to_bytes(8, "little"), FRONT["record canonical"])
    out.append(("cut", proof[:-1], say["length"]))
    out.append(("appended", proof + b"\x00", say["length"]))
    for k in range(2 if A == 0 else 3):
        r, pa = off[f"rec {k}"], off[f"path {k}"]
        put(f"record tag {k}", r, b"\x03", say["record"])
        put(f"record count {k}", r + 1, (int.from_bytes(proof[r + 1:r + 9], "little") + 1).to_bytes(8, "little"), say["record"])
        put(f"path tag {k}", pa, b"\x02", say["path"])
        put(f"path count {k}", pa + 1, (int.from_bytes(proof[pa + 1:pa + 9], "little") - 1).to_bytes(8, "little"), say["path"])
        put(f"value {k}", r + 9, bytes([proof[r + 9] ^ 2]), say["auth"])
        put(f"digest {k}", pa + 9 + 5, bytes([proof[pa + 9 + 5] ^ 1]), say["auth"])
        put(f"value + p {k}", r + 9, (int.from_bytes(proof[r + 9:r + 17], "little") + p).to_bytes(8, "little"), say["auth"])
        v0, v1 = proof[r + 9:r + 17], proof[r + 17:r + 25]
        if v0 != v1:
            put(f"swap {k}", r + 9, v1 + v0, say["auth"])
    return out
