"""The checker of the grinding entry points (include/stark_mi.h, "Grinding"), restated in Python over the CPU oracle's
hash: pow_ok and grind, extension FRI with the nonce absorbed before the index seed and its record behind the last
codeword (built from tests/ext_compose.py's commit, challenge, _elems, _path and _pop), and the AIR proof over it (the
transcript of ext_compose.air_transcript, the row openings of tests/air_rows.py).
Not a test module: imported by tests/test_pow_host.py, tests/test_pow_emu.py and tests/test_gpu_pow.py."""
import numpy as np

import air_compose as ac
import air_periodic as ap
import air_rows as ar
import ext_compose as xc

RECORD_BYTES = 17          # tag 2 | u64 1 | the nonce
MAX_BITS = 32

_found = {}                # (transcript, bits) -> grind: every test that needs a nonce shares the one search


def check_word(o, transcript, nonce):
    """the u64 read little-endian from bytes 24..31 of Hash::from_bytes(T || nonce as 8 little-endian bytes)"""
    return int.from_bytes(o.hash_from_bytes(bytes(transcript) + xc._u64(nonce))[24:32], "little")


def pow_ok(o, transcript, nonce, bits):
    return check_word(o, transcript, nonce) & ((1 << bits) - 1) == 0


def grind(o, transcript, bits):
    """the smallest valid nonce, by trying 0, 1, 2, ..."""
    key = (bytes(transcript), bits)
    if key not in _found:
        t, mask, nu = bytes(transcript), (1 << bits) - 1, 0
        while int.from_bytes(o.hash_from_bytes(t + xc._u64(nu))[24:32], "little") & mask:
            nu += 1
        _found[key] = nu
    return _found[key]


def valid_nonces(o, transcript, bits, below):
    """every valid nonce in [0, below), ascending"""
    return [nu for nu in range(below) if pow_ok(o, transcript, nu, bits)]


def record(nonce):
    return xc._elems([nonce])


# ---------------------------------------------------------------------------------------------- FRI over F_q with grinding
def prove(o, cfg, cw, g, prior=b"", bits=0):
    """-> (stream bytes, top-level indices, nonce)"""
    t = int(cfg.num_colinearity_tests)
    out, cws, trees, _roots, _alphas, tr = xc.commit(o, cfg, cw, g, prior)
    out = bytearray(out)
    nonce = grind(o, tr, bits)
    out += record(nonce)
    tr += xc._u64(nonce)
    sample = cws[1].shape[1] if len(cws) > 1 else cws[0].shape[1]
    top = o.fri_sample_indices(o.hash_from_u64(xc.challenge(o, tr)), sample, cws[-1].shape[1], t)
    idx = list(top)
    for i in range(len(cws) - 1):
        n, half = cws[i].shape[1], cws[i].shape[1] // 2
        idx = [x % half for x in idx]
        for c in idx:
            out += xc._elems([int(v) for v in cws[i][:, c]] + [int(v) for v in cws[i][:, c + half]] + [int(v) for v in cws[i + 1][:, c]])
        for c in idx:
            out += xc._path(o.merkle_open(trees[i], n, c))
            out += xc._path(o.merkle_open(trees[i], n, c + half))
            out += xc._path(o.merkle_open(trees[i + 1], half, c))
    return bytes(out), [int(v) for v in top], nonce


def verify(o, cfg, stream, g, prior=b"", bits=0):
    """-> (accept, polynomial_values [(index, [c0..c3])] of layer 0, bytes consumed, top-level indices, reason)"""
    p, t, N, R = cfg.p, int(cfg.num_colinearity_tests), int(cfg.domain_length), o.fri_num_rounds(cfg)
    E = int(cfg.expansion_factor)
    at, roots, alphas, pv = 0, [], [], []

    def no(why):
        return False, pv, 0, [], why
    if R == 0:
        return no("rounds")
    tr = bytearray(prior)
    for r in range(R):
        obj = xc._pop(stream, at)
        if obj is None or obj[0] != 0:
            return no("root")
        roots.append(obj[1])
        tr += obj[1]
        if r < R - 1:
            alphas.append(xc.round_alpha(o, tr))
        at = obj[2]
    L = N >> (R - 1)
    obj = xc._pop(stream, at)
    if obj is None or obj[0] != 2 or len(obj[1]) != 4 * L:
        return no("last codeword")
    flat, at = obj[1], obj[2]
    if any(v >= p for v in flat):
        return no("canonical")
    last = np.array(flat, dtype=np.uint64).reshape(L, 4).T
    if bytes(xc.row_tree(o, last)[-1]) != roots[-1]:
        return no("last root")
    bound = L // E
    if bound == 0:
        return no("bound")
    omega, offset = int(cfg.omega), int(cfg.offset)
    lo, loff = omega, offset
    for _ in range(R - 1):
        lo, loff = lo * lo % p, loff * loff % p
    dom = [loff * pow(lo, i, p) % p for i in range(L)]
    for e in range(4):
        poly = o.poly_interpolate_domain(dom, [int(v) for v in last[e]], p)
        if o.poly_deg(poly) > bound - 1:
            return no("degree")
    # the nonce record: exactly one value, a u64 (no canonical check); pow_ok on the transcript after the last root
    obj = xc._pop(stream, at)
    if obj is None or obj[0] != 2 or len(obj[1]) != 1:
        return no("nonce record")
    nonce, at = obj[1][0], obj[2]
    if not pow_ok(o, tr, nonce, bits):
        return no("proof of work")
    tr += xc._u64(nonce)
    top = [int(v) for v in o.fri_sample_indices(o.hash_from_u64(xc.challenge(o, tr)), N >> 1, L, t)]
    for r in range(R - 1):
        half = N >> (r + 1)
        c_idx = [i % half for i in top]
        trip = []
        for s in range(t):
            obj = xc._pop(stream, at)
            if obj is None or obj[0] != 2 or len(obj[1]) != 12 or any(v >= p for v in obj[1]):
                return no("triple")
            trip.append((obj[1][0:4], obj[1][4:8], obj[1][8:12]))
            at = obj[2]
        if r == 0:
            for s in range(t):
                pv += [(c_idx[s], trip[s][0]), (c_idx[s] + half, trip[s][1])]
        al = [a % p for a in alphas[r]]
        for s in range(t):
            xa = offset * pow(omega, c_idx[s], p) % p
            if not xc.colinear(xc.embed(xa, p), trip[s][0], xc.embed(p - xa, p), trip[s][1], al, trip[s][2], p, g):
                return no("colinearity")
        for s in range(t):
            for leaf_v, idx, root in ((trip[s][0], c_idx[s], roots[r]), (trip[s][1], c_idx[s] + half, roots[r]),
                                      (trip[s][2], c_idx[s], roots[r + 1])):
                obj = xc._pop(stream, at)
                if obj is None or obj[0] != 3:
                    return no("path")
                at = obj[2]
                if not o.merkle_verify(o.hash_from_field_elements(leaf_v), idx, obj[1], root):
                    return no("path")
        omega, offset = omega * omega % p, offset * offset % p
    return True, pv, at, top, ""


def proof_len(N, E, t, R):
    return xc.proof_len(N, E, t, R) + RECORD_BYTES


def nonce_offset(N, R):
    """where the nonce record starts: behind the R roots and the last-codeword record"""
    return 33 * R + 9 + 32 * (N >> (R - 1))


# ---------------------------------------------------------------------------------------------- the AIR proof
def air_proof(o, air, cols, p, g, log_n, lb, t, tau, h, E, bits):
    """-> (row root, proof bytes, top, nonce) of smi_dev_air_prove_ext_pow from the oracle's primitives"""
    N, B = 1 << (log_n + lb), 1 << lb
    W, K = len(cols), len(air.constraints)
    lde = ac.lde(o, cols, p, g, log_n, lb, tau, h)
    nodes = o.merkle_new(ar.row_leaves(o, lde))
    root = bytes(nodes[-1])
    tr, ch = xc.air_transcript(o, W, K, root)
    if log_n <= 8:
        cw = [ap.route(o, air, cols, xc.weight_vector(ch, e), p, g, log_n, lb, tau, h)[0] for e in range(4)]
    else:
        cw = [ap.fast_route(o, air, cols, xc.weight_vector(ch, e), p, g, log_n, lb, tau, h) for e in range(4)]
    cw = np.stack([np.asarray(c, dtype=np.uint64) for c in cw])
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    fri, top, nonce = prove(o, cfg_o, cw, g, tr, bits)
    return root, fri + ar.openings_bytes(o, lde, top, N, B, K > 0, nodes), top, nonce
