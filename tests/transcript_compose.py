"""Fri::commit / Fri::prove / Fri::verify (reference src/fri.rs:105-156, 250-311, 313-504) composed op for op from the
CPU oracle's primitives, with a caller's FiatShamir that already holds `prior` (src/fiat_shamir.rs:15-25) -- the
checker for the *_fs entry points.  Serialization: src/stream.rs:35-64 (tags 0 root, 2 field elements, 3 path).
Not a test module: imported by tests/test_transcript_host.py and tests/test_gpu_transcript.py."""
import numpy as np


def _u64(v):
    return int(v).to_bytes(8, "little")


def _elems(vals):
    return b"\x02" + _u64(len(vals)) + b"".join(_u64(v) for v in vals)


def _path(nodes):
    return b"\x03" + _u64(len(nodes)) + b"".join(nodes)


def fiat_shamir(o, prior):
    fs = o.FiatShamir()
    if prior:
        fs.absorb(bytes(prior))
    return fs


def commit(o, cfg, codeword, prior=b"", fs=None):
    """Fri::commit -> (stream bytes it pushes, codewords, trees, roots, alphas).  fs (optional) is the caller's
    oracle.FiatShamir, left holding prior + roots; otherwise a fresh one seeded with prior."""
    fs = fiat_shamir(o, prior) if fs is None else fs
    p, R = cfg.p, o.fri_num_rounds(cfg)
    cw = np.ascontiguousarray(np.asarray(codeword, dtype=np.uint64))
    omega, offset = int(cfg.omega), int(cfg.offset)
    out, codewords, trees, roots, alphas = bytearray(), [], [], [], []
    for r in range(R):
        nodes = o.merkle_new(o.leaf_hashes(cw))              # fri.rs:118-127
        root = bytes(nodes[-1])
        out += b"\x00" + root                                   # :129
        fs.absorb(root)                                         # :131
        codewords.append(cw)
        trees.append(nodes)
        roots.append(root)
        if r == R - 1:
            break
        alpha = fs.challenge()                                  # :138
        alphas.append(alpha)
        cw = o.fri_fold_codeword(cfg, cw, alpha, offset, omega)  # :143
        omega, offset = omega * omega % p, offset * offset % p
    out += _elems(cw)                                           # :151
    return bytes(out), codewords, trees, roots, alphas


def prove(o, cfg, codeword, prior=b"", fs=None):
    """Fri::prove -> (stream bytes it pushes, top-level indices)"""
    fs = fiat_shamir(o, prior) if fs is None else fs
    t = int(cfg.num_colinearity_tests)
    out, cws, trees, _roots, _alphas = commit(o, cfg, codeword, fs=fs)
    out = bytearray(out)
    sample = len(cws[1]) if len(cws) > 1 else len(cws[0])      # fri.rs:266-270
    top = o.fri_sample_indices(o.hash_from_u64(fs.challenge()), sample, len(cws[-1]), t)
    idx = list(top)
    for i in range(len(cws) - 1):                               # :281-308, query :215-248
        n, half = len(cws[i]), len(cws[i]) // 2
        idx = [x % half for x in idx]
        for c in idx:
            out += _elems([cws[i][c], cws[i][c + half], cws[i + 1][c]])
        for c in idx:
            out += _path(o.merkle_open(trees[i], n, c))
            out += _path(o.merkle_open(trees[i], n, c + half))
            out += _path(o.merkle_open(trees[i + 1], half, c))
    return bytes(out), top


def _pop(stream, at):
    """one object of the serialized stream at byte `at` -> (tag, payload, next byte), or None"""
    if at >= len(stream):
        return None
    tag = stream[at]
    if tag == 0:
        return 0, bytes(stream[at + 1:at + 33]), at + 33
    n = int.from_bytes(stream[at + 1:at + 9], "little")
    w = 8 if tag == 2 else 32
    body = stream[at + 9:at + 9 + w * n]
    if tag == 2:
        return 2, [int.from_bytes(body[8 * i:8 * i + 8], "little") for i in range(n)], at + 9 + w * n
    return 3, [bytes(body[32 * i:32 * i + 32]) for i in range(n)], at + 9 + w * n


def verify(o, cfg, stream, prior=b"", fs=None):
    """Fri::verify -> (accept, polynomial_values [(index, value)], bytes of the objects popped)"""
    fs = fiat_shamir(o, prior) if fs is None else fs
    p, t, N, R = cfg.p, int(cfg.num_colinearity_tests), int(cfg.domain_length), o.fri_num_rounds(cfg)
    at, roots, alphas, pv = 0, [], [], []
    for _ in range(R):                                          # :325-334
        obj = _pop(stream, at)
        if obj is None or obj[0] != 0:
            return False, pv, 0
        roots.append(obj[1])
        fs.absorb(obj[1])
        alphas.append(fs.challenge())
        at = obj[2]
    obj = _pop(stream, at)                                      # :337-342
    if obj is None or obj[0] != 2:
        return False, pv, 0
    last, at = obj[1], obj[2]
    if o.merkle_commit(o.leaf_hashes(last)) != roots[-1]:       # :349-357
        return False, pv, 0
    degree_bound = len(last) // int(cfg.expansion_factor)      # :360-365
    if degree_bound == 0:
        return False, pv, 0
    omega, offset = int(cfg.omega), int(cfg.offset)
    lo, loff = omega, offset
    for _ in range(R - 1):
        lo, loff = lo * lo % p, loff * loff % p
    dom = [loff * pow(lo, i, p) % p for i in range(len(last))]
    poly = o.poly_interpolate_domain(dom, last, p)              # :368-381
    if [int(v) for v in o.poly_eval_domain(poly, dom, p)] != [int(v) for v in last]:
        return False, pv, 0
    if o.poly_deg(poly) > degree_bound - 1:                     # :392-397
        return False, pv, 0
    top = o.fri_sample_indices(o.hash_from_u64(fs.challenge()), N >> 1, N >> (R - 1), t)   # :400-405
    for r in range(R - 1):                                      # :408-502
        half = N >> (r + 1)
        c_idx = [i % half for i in top]
        b_idx = [i + half for i in c_idx]
        trip = []
        for s in range(t):
            obj = _pop(stream, at)
            if obj is None or obj[0] != 2 or len(obj[1]) != 3:
                return False, pv, 0
            trip.append(obj[1])
            at = obj[2]
        if r == 0:
            for s in range(t):
                pv += [(c_idx[s], trip[s][0]), (b_idx[s], trip[s][1])]
        ax = [offset * pow(omega, c, p) % p for c in c_idx]
        bx = [offset * pow(omega, b, p) % p for b in b_idx]
        for s in range(t):
            pts = [(ax[s], trip[s][0]), (bx[s], trip[s][1]), (alphas[r] % p, trip[s][2])]
            if not o.poly_test_colinearity(pts, p):
                return False, pv, 0
        for s in range(t):
            for leaf_v, idx, root in ((trip[s][0], c_idx[s], roots[r]), (trip[s][1], b_idx[s], roots[r]),
                                      (trip[s][2], c_idx[s], roots[r + 1])):
                obj = _pop(stream, at)
                if obj is None or obj[0] != 3:
                    return False, pv, 0
                at = obj[2]
                if not o.merkle_verify(o.hash_from_field_elements([leaf_v]), idx, obj[1], root):
                    return False, pv, 0
        omega, offset = omega * omega % p, offset * offset % p
    return True, pv, at
