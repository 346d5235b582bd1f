"""The checker of the quartic-extension entry points (include/stark_mi.h, "Quartic extension"), restated in Python from
the CPU oracle's primitives: F_q = F_p[X] / (X^4 - g) arithmetic, the fold of a four-column codeword, FRI commit / prove /
verify over F_q (row leaves, four counters per round), the AIR transcript with extension weights and the composition as
four calls of the base-field route.
Not a test module: imported by tests/test_ext_host.py, tests/test_ext_emu.py and tests/test_gpu_ext.py."""
import numpy as np

PRIMES = [(998244353, 3), (469762049, 3)]


def _u64(v):
    return int(v).to_bytes(8, "little")


# ---------------------------------------------------------------------------------------------- F_q on Python ints
def add(a, b, p):
    return [(x + y) % p for x, y in zip(a, b)]


def sub(a, b, p):
    return [(x - y) % p for x, y in zip(a, b)]


def scale(a, k, p):
    return [x * k % p for x in a]


def embed(v, p):
    return [v % p, 0, 0, 0]


def mul(a, b, p, g):
    """schoolbook product of two cubics, then X^(4+k) = g X^k"""
    prod = [0] * 7
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            prod[i + j] += x * y
    return [(prod[k] + g * (prod[k + 4] if k < 3 else 0)) % p for k in range(4)]


def power(a, e, p, g):
    r, b = embed(1, p), list(a)
    while e:
        if e & 1:
            r = mul(r, b, p, g)
        b = mul(b, b, p, g)
        e >>= 1
    return r


def inv(a, p, g):
    """a^(q - 2), q = p^4 (Lagrange in F_q^*: nothing of the tower the library inverts through); None for zero"""
    if not any(v % p for v in a):
        return None
    return power(a, p ** 4 - 2, p, g)


def field_ok(p, g):
    return p % 4 == 1 and pow(g, (p - 1) // 2, p) == p - 1


def colinear(xa, a, xb, b, xc, c, p, g):
    """(x_a, a), (x_b, b), (x_c, c) on one line over F_q: (b - a)(x_c - x_a) = (c - a)(x_b - x_a)"""
    return mul(sub(b, a, p), sub(xc, xa, p), p, g) == mul(sub(c, a, p), sub(xb, xa, p), p, g)


# ---------------------------------------------------------------------------------------------- the fold (numpy, p < 2^30)
def _powers(base, n, p):
    """base^i, i < n (n a power of two), as uint64"""
    out = np.ones(1, dtype=np.uint64)
    step = base % p
    while len(out) < n:
        out = np.concatenate([out, out * np.uint64(step) % np.uint64(p)])
        step = step * step % p
    return out[:n]


def mul_arr(a, b, p, g):
    """a: (4, n) uint64 residues, b: four ints -> (4, n); every partial sum stays below 2^64 for p < 2^30"""
    P = np.uint64(p)
    b = [np.uint64(v % p) for v in b]
    gb = [np.uint64(g * int(v) % p) for v in b]
    out = np.zeros_like(a)
    for k in range(4):
        acc = np.zeros(a.shape[1], dtype=np.uint64)
        for i in range(4):
            acc += a[i] * (b[k - i] if i <= k else gb[k + 4 - i]) % P
        out[k] = acc % P
    return out


def fold(cw, alpha, offset, omega, p, g):
    """element i of the next codeword = 2^-1 (lo + hi) + alpha * ((lo - hi) * 2^-1 * x_i^-1); cw: (4, L), alpha: four
    unreduced ints"""
    cw = np.asarray(cw, dtype=np.uint64)
    L, P = cw.shape[1], np.uint64(p)
    half = L // 2
    inv2 = pow(2, -1, p)
    xinv = _powers(pow(omega, -1, p), half, p) * np.uint64(pow(offset, -1, p) * inv2 % p) % P
    lo, hi = cw[:, :half], cw[:, half:]
    s = (lo + hi) % P * np.uint64(inv2) % P
    d = (lo + P - hi) % P * xinv % P
    return (s + mul_arr(d, [int(a) % p for a in alpha], p, g)) % P


# ---------------------------------------------------------------------------------------------- FRI over F_q
def challenge(o, tr):
    return int.from_bytes(o.hash_from_bytes(bytes(tr))[:8], "little")


def _elems(vals):
    return b"\x02" + _u64(len(vals)) + b"".join(_u64(v) for v in vals)


def _path(nodes):
    return b"\x03" + _u64(len(nodes)) + b"".join(bytes(n) for n in nodes)


def row_tree(o, cw):
    """the tree whose leaf i is Hash::from_field_elements([c0, c1, c2, c3]) of element i"""
    return o.merkle_new(o.row_hashes(np.ascontiguousarray(np.asarray(cw, dtype=np.uint64))))


def round_alpha(o, tr):
    """absorbs e = 0 .. 3 as 8 little-endian bytes with a challenge after each -> the four unreduced coordinates"""
    alpha = []
    for e in range(4):
        tr += _u64(e)
        alpha.append(challenge(o, tr))
    return alpha


def commit(o, cfg, cw, g, prior=b""):
    """-> (stream bytes, codewords, trees, roots, alphas, transcript as it stands after the last root)"""
    p, R = cfg.p, o.fri_num_rounds(cfg)
    cw = np.ascontiguousarray(np.asarray(cw, dtype=np.uint64))
    omega, offset = int(cfg.omega), int(cfg.offset)
    tr = bytearray(prior)
    out, cws, trees, roots, alphas = bytearray(), [], [], [], []
    for r in range(R):
        nodes = row_tree(o, cw)
        root = bytes(nodes[-1])
        out += b"\x00" + root
        tr += root
        cws.append(cw)
        trees.append(nodes)
        roots.append(root)
        if r == R - 1:
            break
        alphas.append(round_alpha(o, tr))
        cw = fold(cw, alphas[-1], offset, omega, p, g)
        omega, offset = omega * omega % p, offset * offset % p
    out += _elems([int(v) for v in cw.T.reshape(-1)])       # element i at 4 i .. 4 i + 3
    return bytes(out), cws, trees, roots, alphas, tr


def prove(o, cfg, cw, g, prior=b""):
    """-> (stream bytes, top-level indices)"""
    t = int(cfg.num_colinearity_tests)
    out, cws, trees, _roots, _alphas, tr = commit(o, cfg, cw, g, prior)
    out = bytearray(out)
    sample = cws[1].shape[1] if len(cws) > 1 else cws[0].shape[1]
    top = o.fri_sample_indices(o.hash_from_u64(challenge(o, tr)), sample, cws[-1].shape[1], t)
    idx = list(top)
    for i in range(len(cws) - 1):
        n, half = cws[i].shape[1], cws[i].shape[1] // 2
        idx = [x % half for x in idx]
        for c in idx:
            out += _elems([int(v) for v in cws[i][:, c]] + [int(v) for v in cws[i][:, c + half]] + [int(v) for v in cws[i + 1][:, c]])
        for c in idx:
            out += _path(o.merkle_open(trees[i], n, c))
            out += _path(o.merkle_open(trees[i], n, c + half))
            out += _path(o.merkle_open(trees[i + 1], half, c))
    return bytes(out), [int(v) for v in top]


def _pop(stream, at):
    """one object at byte `at` -> (tag, payload, next byte), or None when it is missing or cut short"""
    if at >= len(stream):
        return None
    tag = stream[at]
    if tag == 0:
        return (0, bytes(stream[at + 1:at + 33]), at + 33) if at + 33 <= len(stream) else None
    if tag not in (2, 3) or at + 9 > len(stream):
        return None
    n = int.from_bytes(stream[at + 1:at + 9], "little")
    w = 8 if tag == 2 else 32
    if at + 9 + w * n > len(stream):
        return None
    body = stream[at + 9:at + 9 + w * n]
    if tag == 2:
        return 2, [int.from_bytes(body[8 * i:8 * i + 8], "little") for i in range(n)], at + 9 + w * n
    return 3, [bytes(body[32 * i:32 * i + 32]) for i in range(n)], at + 9 + w * n


def verify(o, cfg, stream, g, prior=b""):
    """-> (accept, polynomial_values [(index, [c0..c3])] of layer 0, bytes consumed, top-level indices)"""
    p, t, N, R = cfg.p, int(cfg.num_colinearity_tests), int(cfg.domain_length), o.fri_num_rounds(cfg)
    E = int(cfg.expansion_factor)
    at, roots, alphas, pv = 0, [], [], []
    no = (False, pv, 0, [])
    if R == 0:
        return no
    tr = bytearray(prior)
    for r in range(R):
        obj = _pop(stream, at)
        if obj is None or obj[0] != 0:
            return no
        roots.append(obj[1])
        tr += obj[1]
        if r < R - 1:
            alphas.append(round_alpha(o, tr))
        at = obj[2]
    L = N >> (R - 1)
    obj = _pop(stream, at)
    if obj is None or obj[0] != 2 or len(obj[1]) != 4 * L:
        return no
    flat, at = obj[1], obj[2]
    if any(v >= p for v in flat):
        return no
    last = np.array(flat, dtype=np.uint64).reshape(L, 4).T
    if bytes(row_tree(o, last)[-1]) != roots[-1]:
        return no
    bound = L // E
    if bound == 0:
        return no
    omega, offset = int(cfg.omega), int(cfg.offset)
    lo, loff = omega, offset
    for _ in range(R - 1):
        lo, loff = lo * lo % p, loff * loff % p
    dom = [loff * pow(lo, i, p) % p for i in range(L)]
    for e in range(4):                                      # EVERY coordinate is of low degree
        poly = o.poly_interpolate_domain(dom, [int(v) for v in last[e]], p)
        if o.poly_deg(poly) > bound - 1:
            return no
    top = [int(v) for v in o.fri_sample_indices(o.hash_from_u64(challenge(o, tr)), N >> 1, L, t)]
    for r in range(R - 1):
        half = N >> (r + 1)
        c_idx = [i % half for i in top]
        trip = []
        for s in range(t):
            obj = _pop(stream, at)
            if obj is None or obj[0] != 2 or len(obj[1]) != 12 or any(v >= p for v in obj[1]):
                return no
            trip.append((obj[1][0:4], obj[1][4:8], obj[1][8:12]))
            at = obj[2]
        if r == 0:
            for s in range(t):
                pv += [(c_idx[s], trip[s][0]), (c_idx[s] + half, trip[s][1])]
        al = [a % p for a in alphas[r]]
        for s in range(t):
            xa = offset * pow(omega, c_idx[s], p) % p
            if not colinear(embed(xa, p), trip[s][0], embed(p - xa, p), trip[s][1], al, trip[s][2], p, g):
                return no
        for s in range(t):
            for leaf_v, idx, root in ((trip[s][0], c_idx[s], roots[r]), (trip[s][1], c_idx[s] + half, roots[r]),
                                      (trip[s][2], c_idx[s], roots[r + 1])):
                obj = _pop(stream, at)
                if obj is None or obj[0] != 3:
                    return no
                at = obj[2]
                if not o.merkle_verify(o.hash_from_field_elements(leaf_v), idx, obj[1], root):
                    return no
        omega, offset = omega * omega % p, offset * offset % p
    return True, pv, at, top


def proof_len(N, E, t, R):
    """bytes of an extension-FRI proof: R roots, the last codeword, per layer t triples of 12 and 3 t paths"""
    L = N >> (R - 1)
    n = 33 * R + 9 + 32 * L
    for r in range(R - 1):
        depth = (N >> r).bit_length() - 1
        n += t * (9 + 96) + t * (2 * (9 + 32 * depth) + 9 + 32 * (depth - 1))
    return n


# ---------------------------------------------------------------------------------------------- AIR with extension weights
def air_transcript(o, n_cols, n_constraints, root):
    """-> (the 32 + 32 (W + K) transcript bytes FRI continues, the 4 (W + K) unreduced challenges, weight j = [4 j .. 4 j + 3])"""
    tr, ch = bytearray(bytes(root)), []
    for m in range(4 * (n_cols + n_constraints)):
        tr += _u64(m)
        ch.append(challenge(o, tr))
    return bytes(tr), ch


def weight_vector(ch, e):
    """the base-field weight vector whose composition is coordinate e"""
    return [ch[4 * j + e] for j in range(len(ch) // 4)]


def ext_weights_for(air, seed=3):
    """4 (W + K) unreduced u64 challenges, the top bit set now and then"""
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(1 << 62, (1 << 64) - 1, 4 * (air.n_cols + len(air.constraints)), dtype=np.uint64)]
