"""The checker of zero-knowledge DEEP proofs (include/stark_mi.h, "Zero-knowledge DEEP proofs"),
restated in Python ints over the CPU oracle's hash and the mirror's symbolic AIR: the random generator (the hash in counter
mode), k_t, k_s and D', the derived AIR with its exemption column, and the masked split of the composition's coefficients.
Not a test module: imported by tests/test_zk_emu.py and tests/test_gpu_zk.py."""
import copy

import deep_compose as dc
import ext_compose as xc


# ---------------------------------------------------------------------------------------------- random residues
def rng(o, seed, stream_id, count, p):
    """elements 0 .. count - 1 of stream stream_id: word i mod 4 of Hash::from_bytes(seed | stream_id | i // 4), little-endian
    u64s, mod p"""
    seed = bytes(seed)
    assert len(seed) == 32
    out = []
    for block in range((count + 3) // 4):
        d = bytes(o.hash_from_bytes(seed + xc._u64(stream_id) + xc._u64(block)))
        out += [int.from_bytes(d[8 * k:8 * k + 8], "little") % p for k in range(4)]
    return out[:count]


# ---------------------------------------------------------------------------------------------- the plan
def k_t(t):
    return 8 * t + 8


def k_s(t):
    return 4 * t + 1


def plan(air, log_n, t):
    """-> (d, D', k_t, k_s) of smi_air_plan_deep_zk for a shape it accepts: d and D by dc.plan with one more factor a term"""
    n = 1 << log_n
    d = air.degree + 1
    D = 1
    while D < d - 1:
        D <<= 1
    L = n - k_s(t)
    return d, -(-D * n // L), k_t(t), k_s(t)


# ---------------------------------------------------------------------------------------------- the derived AIR
def exempt_rows(n, t):
    return list(range(n - k_t(t) - 1, n - 1))


def exemption_column(n, t, p, tau, w):
    """E(tau w^r) for r < n, E(x) = prod over the exempt rows q of (x - tau w^q)"""
    pts = [tau * pow(w, r, p) % p for r in range(n)]
    out = []
    for r in range(n):
        v = 1
        for q in exempt_rows(n, t):
            v = v * (pts[r] - pts[q]) % p
        out.append(v)
    return out


def derived_air(air, log_n, t, p, tau, w):
    """the AIR the library proves: air with one more periodic column, the exemption column, as a factor of every term"""
    out = copy.deepcopy(air)
    j = out.periodic(exemption_column(1 << log_n, t, p, tau, w))
    out._symbolic = [[(cf, list(factors) + [("per", j, 1)]) for cf, factors in con] for con in out._symbolic]
    return out


def randomised(cols, seed_rows, t):
    """the trace with the last k_t rows of every column replaced: column c takes seed_rows[c k_t .. (c + 1) k_t)"""
    kt = k_t(t)
    return [list(c[:len(c) - kt]) + [int(v) for v in seed_rows[i * kt:(i + 1) * kt]] for i, c in enumerate(cols)]


# ---------------------------------------------------------------------------------------------- masked segments
def split(hc, h_len, log_n, ks, Dp, rho, p):
    """hc: four coefficient lists of H's coordinates; rho: 4 (D' - 1) k_s values, coordinate e of rho_j at (4 j + e) k_s
    -> 4 D' lists of n coefficients, list 4 j + e = coordinate e of H~_j"""
    n = 1 << log_n
    L = n - ks
    assert h_len <= Dp * L
    H = lambda e, i: int(hc[e][i]) if i < h_len else 0
    out = []
    for j in range(Dp):
        for e in range(4):
            col = [H(e, j * L + m) for m in range(L)] + [0] * ks
            if j >= 1:
                for m in range(ks):
                    col[m] = (col[m] - int(rho[(4 * (j - 1) + e) * ks + m])) % p
            if j < Dp - 1:
                for m in range(ks):
                    col[L + m] = int(rho[(4 * j + e) * ks + m])
            out.append(col)
    return out


def recombined_at(cols, log_n, ks, x, p, g):
    """sum_j x^(j L) H~_j(x) for x in F_q from the 4 D' lists of split()"""
    n = 1 << log_n
    L = n - ks
    acc, xl, pw = [0, 0, 0, 0], xc.power(x, L, p, g), [1, 0, 0, 0]
    for j in range(len(cols) // 4):
        s = dc.horner([[cols[4 * j + e][i] for e in range(4)] for i in range(n)], x, p, g)
        acc = xc.add(acc, xc.mul(pw, s, p, g), p)
        pw = xc.mul(pw, xl, p, g)
    return acc


# ---------------------------------------------------------------------------------------------- the proof
import numpy as np  # noqa: E402

import air_compose as ac  # noqa: E402
import deep_fold4_compose as d4  # noqa: E402
import fold4_compose as f4  # noqa: E402

STREAM_ROWS, STREAM_SALT1, STREAM_RHO, STREAM_MASK, STREAM_SALT2 = 1, 2, 3, 4, 5
FRONT = {"record": "zk deep: the out-of-domain record is missing or has the wrong count",
         "record canonical": "zk deep: an out-of-domain coordinate is not canonical",
         "base field": "zk deep: the out-of-domain point z lies in the base field",
         "consistency": "zk deep: out-of-domain consistency check fails: the derived AIR's constraints at z do not give the masked segments' value",
         "no layer": "zk deep: FRI has no fold at this shape (F = 0), so there is no layer-0 coset to compare the masked DEEP quotient with"}
WORDS = {"length": "zk deep coset openings: wrong length", "record": "zk deep coset openings: malformed record",
         "path": "zk deep coset openings: malformed path", "auth": "zk deep coset openings: authentication path does not verify",
         "canonical": "zk deep coset openings: an opened value is not canonical",
         "quotient": "zk deep coset openings: the masked DEEP quotient of the opened cosets is not the codeword value"}

SENTENCES = set(FRONT.values()) | set(WORDS.values()) | f4.FRI_SENTENCES          # every sentence verify() can give


def layout(W, Dp, log_n, lb, t):
    """-> (folds, proof bytes) from the formula of the header section"""
    N, B, log_N = 1 << (log_n + lb), 1 << lb, log_n + lb
    _R2, F, _last, fri = f4.layout(N, B, t)
    return F, 9 + 32 * (2 * W + Dp) + fri + d4.section_len(W + 1, t, log_N) + d4.section_len(4 * Dp + 5, t, log_N)


def offsets(W, Dp, log_n, lb, t):
    """-> {name: byte offset}: the record, s_0, the FRI part, and per group its first record and first path"""
    N, B, log_N = 1 << (log_n + lb), 1 << lb, log_n + lb
    out = {"s0": 9 + 32 * 2 * W, "fri": 9 + 32 * (2 * W + Dp)}
    at = out["fri"] + f4.layout(N, B, t)[3]
    for k, V in enumerate([W + 1, 4 * Dp + 5]):
        out[f"rec {k}"], out[f"path {k}"] = at, at + t * (9 + 32 * V)
        at += d4.section_len(V, t, log_N)
    out["end"] = at
    return out


plus_p, swapped = d4.plus_p, d4.swapped          # commit_as of prove: group 0 is the trace and its salt, group 1 the segments, R and its salt


def prove(o, air, cols, seed, p, g, log_n, lb, t, tau, h, bits=0, compose_with=None, commit_as=None):
    """-> dict(roots, proof, top, ood, trace, ...) of smi_dev_air_prove_deep_zk.  compose_with: a dishonest prover that skips the
    derivation -- it composes this AIR over the trace as it stands, without randomiser rows; the plan stays the derived AIR's.
    commit_as: a dishonest prover that commits and opens tampered columns (d4.plus_p, d4.swapped; the salt is the last column
    of its group) -- the trees and the opened records hold the tampered columns, every other step the true ones"""
    n, N, B = 1 << log_n, 1 << (log_n + lb), 1 << lb
    W, K = len(cols), len(air.constraints)
    kt, ks = k_t(t), k_s(t)
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    dair = derived_air(air, log_n, t, p, tau, w)
    _d, D = dc.plan(dair)
    Dp = -(-D * n // (n - ks))
    assert D <= B and 4 * Dp + 5 <= 64 and d4.folds(log_n, lb, t) >= 1
    trace = [list(c) for c in cols] if compose_with is not None else randomised(cols, rng(o, seed, STREAM_ROWS, W * kt, p), t)
    lde = [np.asarray(c, dtype=np.uint64) for c in ac.lde(o, trace, p, g, log_n, lb, tau, h)]
    held1, nodes1 = d4._commit(o, 0, lde + [np.array(rng(o, seed, STREAM_SALT1, N, p), dtype=np.uint64)], N, commit_as)
    root1 = bytes(nodes1[-1])
    tr, ch = xc.air_transcript(o, W, K, root1)
    tr = bytearray(tr)
    H = dc.composition(o, compose_with or dair, trace, ch, p, g, log_n, lb, tau, h)
    hc = np.stack([np.asarray(o.fast_intt(H[e], wN, h, p), dtype=np.uint64) for e in range(4)])
    assert compose_with is not None or not hc[:, D * n:].any(), "the composition has coefficients at or above D n"
    segc = split(hc, D * n, log_n, ks, Dp, rng(o, seed, STREAM_RHO, 4 * (Dp - 1) * ks, p), p)
    mask = rng(o, seed, STREAM_MASK, 4 * n, p)
    coefs = segc + [mask[e * n:(e + 1) * n] for e in range(4)]
    seg = [np.asarray(o.fast_coset_ntt(np.array(c, dtype=np.uint64), N, wN, h, p), dtype=np.uint64) for c in coefs]
    held2, nodes2 = d4._commit(o, 1, seg + [np.array(rng(o, seed, STREAM_SALT2, N, p), dtype=np.uint64)], N, commit_as)
    root2 = bytes(nodes2[-1])
    tr += root2
    z = [c % p for c in dc.draw(o, tr, 4 * (W + K), 4)]
    assert any(z[1:]), "z lies in the base field"
    polys = [[int(v) for v in o.fast_intt(np.array(c, dtype=np.uint64), w, tau, p)] for c in trace]
    zw = dc.scale_q(z, w, p)
    u, v = [dc.horner(q, z, p, g) for q in polys], [dc.horner(q, zw, p, g) for q in polys]
    s = [dc.horner([[segc[4 * j + e][i] for e in range(4)] for i in range(n)], z, p, g) for j in range(Dp)]
    ood = [c for el in u + v + s for c in el]
    record = xc._elems(ood)
    tr += record[9:]
    gammas = dc.draw(o, tr, 4 * (W + K) + 4, 4 * (2 * W + Dp))
    Q = dc.q_codeword(lde, np.stack(seg[:4 * Dp]), dc.points(o, p, g, log_n, lb, h), z, ood, gammas, w, p, g)
    Q = (Q + np.stack(seg[4 * Dp:])) % np.uint64(p)
    fri, top, _nonce = f4.prove(o, o.fri_cfg(wN, h, N, B, t, p), Q, g, bytes(tr), bits)
    secs = [d4.section(o, held1, nodes1, top, N), d4.section(o, held2, nodes2, top, N)]
    return {"roots": [root1, root2], "proof": record + fri + secs[0] + secs[1], "top": top, "ood": ood, "trace": trace, "Dp": Dp,
            "groups": [held1, held2], "polys": polys}


def verify(o, air, proof, roots, p, g, W, log_n, lb, t, tau, h, bits=0):
    """-> (accept, sentence) of smi_air_verify_deep_zk, in its order"""
    n, N, B, log_N, K = 1 << log_n, 1 << (log_n + lb), 1 << lb, log_n + lb, len(air.constraints)
    ks = k_s(t)
    w, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    dair = derived_air(air, log_n, t, p, tau, w)
    _d, D = dc.plan(dair)
    Dp = -(-D * n // (n - ks))
    cnt = 4 * (2 * W + Dp)
    obj = xc._pop(proof, 0)
    if obj is None or obj[0] != 2 or len(obj[1]) != cnt:
        return False, FRONT["record"]
    ood, at = obj[1], obj[2]
    if any(v >= p for v in ood):
        return False, FRONT["record canonical"]
    tr, weights = xc.air_transcript(o, W, K, bytes(roots[0]))
    tr = bytearray(tr) + bytes(roots[1])
    z = [c % p for c in dc.draw(o, tr, 4 * (W + K), 4)]
    if not any(z[1:]):
        return False, FRONT["base field"]
    tr += proof[9:at]
    gammas = dc.draw(o, tr, 4 * (W + K) + 4, cnt)
    lhs, _ = dc.ood_sides(o, dair, W, Dp, weights, z, ood, p, g, log_n, tau)
    rhs, pw, zl = [0, 0, 0, 0], [1, 0, 0, 0], xc.power(z, n - ks, p, g)
    for j in range(Dp):
        rhs = xc.add(rhs, xc.mul(pw, [int(c) for c in ood[4 * (2 * W + j):4 * (2 * W + j) + 4]], p, g), p)
        pw = xc.mul(pw, zl, p, g)
    if [int(c) for c in lhs] != rhs:
        return False, FRONT["consistency"]
    if d4.folds(log_n, lb, t) == 0:
        return False, FRONT["no layer"]
    ok, pv, used, top, why = f4.verify(o, o.fri_cfg(wN, h, N, B, t, p), proof[at:], g, bytes(tr), bits)
    if not ok:
        return False, why
    widths = [W + 1, 4 * Dp + 5]
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
    for k in range(2):                                       # the leaf is the record's u64s as they stand, salts included
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
            srow = [recs[1][s][4 * c + j] for c in range(4 * Dp)]
            got = dc.q_at(trow, srow, x, z, ood, gammas, w, p, g)
            got = [(got[e] + recs[1][s][4 * (4 * Dp + e) + j]) % p for e in range(4)]
            idx, want = pv[4 * s + j]
            assert idx == a + j * q
            if got != [int(c) for c in want]:
                return False, WORDS["quotient"]
    return True, ""
