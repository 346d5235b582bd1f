"""The checker of extension FRI at folding factor 4 (include/stark_mi.h, "Extension FRI, folding factor 4"), restated in
Python over tests/ext_compose.py's field code: the fold by 4 as Lagrange interpolation through the four points of a coset,
evaluated at alpha -- an independent route, never two folds by 2 -- and the layout of the proof (folds, last length, bytes).
Not a test module: imported by tests/test_fold4_host.py, tests/test_fold4_emu.py and tests/test_gpu_fold4.py."""
import numpy as np

import ext_compose as xc


def fold4_element(c, x, iota, alpha, p, g):
    """P(alpha) for the cubic P over F_q with P(x iota^j) = c[j], j = 0 .. 3; c[j]: four ints, x and iota in F_p, alpha:
    four residues"""
    xs = [x * pow(iota, j, p) % p for j in range(4)]
    acc = [0, 0, 0, 0]
    for j in range(4):
        num, den = xc.embed(1, p), 1
        for k in range(4):
            if k != j:
                num = xc.mul(num, xc.sub(alpha, xc.embed(xs[k], p), p), p, g)
                den = den * (xs[j] - xs[k]) % p
        acc = xc.add(acc, xc.scale(xc.mul(num, c[j], p, g), pow(den, -1, p), p), p)
    return acc


def fold4(cw, alpha, offset, omega, p, g):
    """cw: (4, L) residues on offset * <omega>, omega of order L >= 4; alpha: four unreduced ints -> (4, L / 4): element i is
    the Lagrange interpolant through elements i, i + q, i + 2 q, i + 3 q (at x_i iota^j, iota = omega^q) evaluated at alpha"""
    cw = np.asarray(cw, dtype=np.uint64)
    L = cw.shape[1]
    q = L // 4
    iota = pow(omega, q, p)
    assert L >= 4 and pow(iota, 2, p) == p - 1, "omega must have order L"
    al = [int(a) % p for a in alpha]
    out = np.zeros((4, q), dtype=np.uint64)
    x = offset % p
    for i in range(q):
        c = [[int(v) for v in cw[:, i + j * q]] for j in range(4)]
        out[:, i] = fold4_element(c, x, iota, al, p, g)
        x = x * omega % p
    return out


def alpha_squared(alpha, p, g):
    """the second challenge of the two-fold identity: alpha * alpha in F_q, reduced"""
    a = [int(v) % p for v in alpha]
    return xc.mul(a, a, p, g)


def two_folds(cw, alpha, offset, omega, p, g):
    """the identity the header states: ext_compose.fold under alpha, then under alpha^2 on the squared domain (p < 2^30)"""
    mid = xc.fold(cw, alpha, offset, omega, p, g)
    return xc.fold(mid, alpha_squared(alpha, p, g), offset * offset % p, omega * omega % p, p, g)


# ---------------------------------------------------------------------------------------------- commit, prove, verify
import pow_compose as pc  # noqa: E402

FOLD4_MISMATCH = "folded coset does not match the next layer"


def coset_tree(o, cw):
    """the tree of q = L / 4 leaves whose leaf i is Hash::from_field_elements of the 16 values (coordinate outer, slot
    inner) of elements i, i + q, i + 2 q, i + 3 q"""
    cw = np.ascontiguousarray(np.asarray(cw, dtype=np.uint64))
    return o.merkle_new(o.row_hashes(np.ascontiguousarray(cw.reshape(16, cw.shape[1] // 4))))


def coset_values(cw, i):
    """the 16 values of leaf i, in leaf order"""
    q = cw.shape[1] // 4
    return [int(cw[e, i + j * q]) for e in range(4) for j in range(4)]


def commit(o, cfg, cw, g, prior=b""):
    """-> (stream bytes up to the last codeword, codewords, trees, roots, alphas, transcript after the last root)"""
    p = cfg.p
    N, E, t = int(cfg.domain_length), int(cfg.expansion_factor), int(cfg.num_colinearity_tests)
    _R2, F, _last, _n = layout(N, E, t)
    cw = np.ascontiguousarray(np.asarray(cw, dtype=np.uint64))
    omega, offset = int(cfg.omega), int(cfg.offset)
    tr = bytearray(prior)
    out, cws, trees, roots, alphas = bytearray(), [], [], [], []
    for r in range(F + 1):
        nodes = coset_tree(o, cw)
        root = bytes(nodes[-1])
        out += b"\x00" + root
        tr += root
        cws.append(cw)
        trees.append(nodes)
        roots.append(root)
        if r == F:
            break
        alphas.append(xc.round_alpha(o, tr))
        cw = fold4(cw, alphas[-1], offset, omega, p, g)
        omega, offset = pow(omega, 4, p), pow(offset, 4, p)
    out += xc._elems([int(v) for v in cw.T.reshape(-1)])
    return bytes(out), cws, trees, roots, alphas, tr


def prove(o, cfg, cw, g, prior=b"", bits=0):
    """-> (stream bytes, top-level indices, nonce)"""
    t = int(cfg.num_colinearity_tests)
    out, cws, trees, _roots, _alphas, tr = commit(o, cfg, cw, g, prior)
    out = bytearray(out)
    nonce = pc.grind(o, tr, bits)
    out += pc.record(nonce)
    tr += xc._u64(nonce)
    F, N = len(cws) - 1, cws[0].shape[1]
    top = [int(v) for v in o.fri_sample_indices(o.hash_from_u64(xc.challenge(o, tr)), N // 4 if F else N, cws[-1].shape[1], t)]
    for r in range(F):
        q = cws[r].shape[1] // 4
        for s in top:
            out += xc._elems(coset_values(cws[r], s % q))
        for s in top:
            out += xc._path(o.merkle_open(trees[r], q, s % q))
    return bytes(out), top, nonce


def verify(o, cfg, stream, g, prior=b"", bits=0):
    """-> (accept, layer-0 cosets [(index, [c0..c3])], bytes consumed, top-level indices, sentence)"""
    p, t, N, E = cfg.p, int(cfg.num_colinearity_tests), int(cfg.domain_length), int(cfg.expansion_factor)
    R2, F, L, _n = layout(N, E, t)
    at, roots, alphas, pv = 0, [], [], []

    def no(why):
        return False, pv, 0, [], why
    if R2 == 0:
        return no("No FRI roots extracted")
    tr = bytearray(prior)
    for r in range(F + 1):
        obj = xc._pop(stream, at)
        if obj is None or obj[0] != 0:
            return no("Failed to extract Merkle root")
        roots.append(obj[1])
        tr += obj[1]
        if r < F:
            alphas.append(xc.round_alpha(o, tr))
        at = obj[2]
    obj = xc._pop(stream, at)
    if obj is None or obj[0] != 2:
        return no("Failed to extract last codeword")
    if len(obj[1]) != 4 * L:
        return no("last codeword: expected four values per element of the last domain")
    flat, at = obj[1], obj[2]
    if any(v >= p for v in flat):
        return no("last codeword: a coordinate is not canonical")
    last = np.array(flat, dtype=np.uint64).reshape(L, 4).T
    if bytes(coset_tree(o, last)[-1]) != roots[-1]:
        return no("last codeword is not well formed")
    bound = L // E
    if bound == 0:
        return no("last codeword too small")
    omega, offset = int(cfg.omega), int(cfg.offset)
    lo, loff = pow(omega, 4 ** F, p), pow(offset, 4 ** F, p)
    dom = [loff * pow(lo, i, p) % p for i in range(L)]
    for e in range(4):
        poly = o.poly_interpolate_domain(dom, [int(v) for v in last[e]], p)
        if o.poly_deg(poly) > bound - 1:
            return no("last codeword does not correspond to polynomial of low enough degree")
    obj = xc._pop(stream, at)
    if obj is None or obj[0] != 2:
        return no("proof of work: failed to extract the nonce")
    if len(obj[1]) != 1:
        return no("proof of work: the nonce record must hold exactly one value")
    nonce, at = obj[1][0], obj[2]
    if not pc.pow_ok(o, tr, nonce, bits):
        return no("proof of work")
    tr += xc._u64(nonce)
    top = [int(v) for v in o.fri_sample_indices(o.hash_from_u64(xc.challenge(o, tr)), N // 4 if F else N, L, t)]
    folded = None
    for r in range(F):
        q = N >> (2 * r + 2)
        idx = [s % q for s in top]
        recs = []
        for s in range(t):
            obj = xc._pop(stream, at)
            if obj is None or obj[0] != 2:
                return no("Failed to extract triple values")
            if len(obj[1]) != 16:
                return no("Expected triple of values")
            if any(v >= p for v in obj[1]):
                return no("triple: a coordinate is not canonical")
            recs.append(obj[1])
            at = obj[2]
            if r == 0:
                pv += [(idx[s] + j * q, [obj[1][4 * e + j] for e in range(4)]) for j in range(4)]
        if r > 0:
            for s in range(t):
                j = (top[s] % (4 * q)) // q
                if [recs[s][4 * e + j] for e in range(4)] != folded[s]:
                    return no(FOLD4_MISMATCH)
        paths = []
        for s in range(t):                                   # every pop of the layer first, then the paths
            obj = xc._pop(stream, at)
            if obj is None or obj[0] != 3:
                return no("Failed to extract path for aa")
            at = obj[2]
            if len(obj[1]) != q.bit_length() - 1:
                return no("merkle authentication path verification fails for aa")
            paths.append(obj[1])
        for s in range(t):
            if not o.merkle_verify(o.hash_from_field_elements(recs[s]), idx[s], paths[s], roots[r]):
                return no("merkle authentication path verification fails for aa")
        om, off = pow(omega, 4 ** r, p), pow(offset, 4 ** r, p)
        iota, al = pow(om, q, p), [a % p for a in alphas[r]]
        folded = [fold4_element([[recs[s][4 * e + j] for e in range(4)] for j in range(4)], off * pow(om, idx[s], p) % p, iota, al, p, g)
                  for s in range(t)]
    if F:
        for s in range(t):
            if [int(v) for v in last[:, top[s] % L]] != folded[s]:
                return no(FOLD4_MISMATCH)
    return True, pv, at, top, ""


def low_degree_codeword(o, p, g, N, E, offset, seed, spoil=None):
    """four coordinates of degree < N / E on offset * <omega_N>; spoil: a coordinate that gets a random codeword instead
    -> (codeword (4, N), omega_N)"""
    rng = np.random.default_rng(seed)
    omega = o.ff_prim_nth_root_g(N, p, g)
    cw = np.stack([np.asarray(o.fast_coset_ntt(rng.integers(0, p, N // E, dtype=np.uint64), N, omega, offset, p), dtype=np.uint64) for _ in range(4)])
    if spoil is not None:
        cw[spoil] = rng.integers(0, p, N, dtype=np.uint64)
    return cw, omega


_proofs = {}


def shared_proof(o, p, g, log_n, E, t, bits, prior=b"", seed=1):
    """one restated proof per (p, log N, E, t, bits, prior), shared by every test that needs it and never changed
    -> (cfg, codeword, proof bytes, top, nonce)"""
    key = (p, log_n, E, t, bits, bytes(prior), seed)
    if key not in _proofs:
        N = 1 << log_n
        cw, omega = low_degree_codeword(o, p, g, N, E, g, seed)
        cfg = o.fri_cfg(omega, g, N, E, t, p)
        _proofs[key] = (cfg, cw) + prove(o, cfg, cw, g, prior, bits)
    return _proofs[key]


def objects(N, E, t):
    """-> [(kind, layer or None, byte offset)] of every object of a proof, in stream order, and the proof's length"""
    _R2, F, last, n = layout(N, E, t)
    out, at = [], 0
    for r in range(F + 1):
        out.append(("root", r, at))
        at += 33
    out.append(("last", None, at))
    at += 9 + 32 * last
    out.append(("nonce", None, at))
    at += 17
    for r in range(F):
        depth = (N >> (2 * r + 2)).bit_length() - 1
        for _ in range(t):
            out.append(("coset", r, at))
            at += 9 + 128
        for _ in range(t):
            out.append(("path", r, at))
            at += 9 + 32 * depth
    assert at == n
    return out, n


MISSING = {"root": "Failed to extract Merkle root", "last": "Failed to extract last codeword",
           "nonce": "proof of work: failed to extract the nonce", "coset": "Failed to extract triple values",
           "path": "Failed to extract path for aa"}
BAD_COUNT = {"last": "last codeword: expected four values per element of the last domain",
             "nonce": "proof of work: the nonce record must hold exactly one value", "coset": "Expected triple of values",
             "path": "merkle authentication path verification fails for aa"}


def mutations(proof, N, E, t, p):
    """-> [(name, mutated proof, the sentence every verifier must give or None where it depends on the data)]: truncation
    at every object boundary, a wrong tag and a wrong count per record kind, a flipped bit per kind, a coordinate + p"""
    objs, n = objects(N, E, t)
    assert len(proof) == n
    out = []

    def put(name, at, byte_fn, why):
        m = bytearray(proof)
        m[at] = byte_fn(m[at])
        out.append((name, bytes(m), why))
    for kind, r, at in objs:
        out.append((f"cut before {kind} {r} at {at}", proof[:at], MISSING[kind]))
    seen = set()
    for kind, r, at in objs:
        if kind in seen:
            continue
        seen.add(kind)
        put(f"tag of {kind}", at, lambda b: {0: 2, 2: 3, 3: 2}[b], MISSING[kind])
        if kind != "root":
            count = int.from_bytes(proof[at + 1:at + 9], "little")
            if count:
                m = bytearray(proof)
                m[at + 1:at + 9] = (0 if kind == "nonce" else count - 1).to_bytes(8, "little")
                out.append((f"count of {kind}", bytes(m), BAD_COUNT[kind]))
        body = at + (1 if kind == "root" else 9)
        if kind != "nonce":
            # bit 1 of a value's low byte (v +- 2 stays canonical unless v is p - 2 or p - 1, which the shared proofs do not hold
            # there): the last codeword no longer hashes to its root, a coset record no longer hashes to its leaf.  A flipped
            # root other than the last moves the transcript, and what then fails first depends on the data.
            why = {"path": BAD_COUNT["path"], "coset": BAD_COUNT["path"], "last": "last codeword is not well formed"}.get(kind)
            if kind == "root" and len([1 for k2, _r, _a in objs if k2 == "root"]) == 1:
                why = "last codeword is not well formed"
            put(f"bit in {kind}", body, lambda b: b ^ 0x02, why)
        if kind in ("last", "coset"):
            m = bytearray(proof)
            v = int.from_bytes(proof[body + 8:body + 16], "little") + p
            m[body + 8:body + 16] = v.to_bytes(8, "little")
            out.append((f"coordinate + p in {kind}", bytes(m),
                        "last codeword: a coordinate is not canonical" if kind == "last" else "triple: a coordinate is not canonical"))
    last_root = [at for kind, r, at in objs if kind == "root"][-1]
    put("bit in the last root", last_root + 9, lambda b: b ^ 1, "last codeword is not well formed")
    return out


# ---------------------------------------------------------------------------------------------- the AIR proof
def positions4(s, N, B, with_next):
    """the rows a test opens: the four points of its layer-0 coset, then (with transition constraints) the rows B further"""
    a = int(s) % (N // 4)
    here = [a + j * (N // 4) for j in range(4)]
    return here + ([(i + B) % N for i in here] if with_next else [])


def openings4_bytes(o, lde_cols, top, N, B, with_next, nodes):
    W = len(lde_cols)
    out = bytearray()
    for s in top:
        for i in positions4(s, N, B, with_next):
            out += b"\x02" + xc._u64(W) + b"".join(xc._u64(col[i]) for col in lde_cols)
    for s in top:
        for i in positions4(s, N, B, with_next):
            out += xc._path(o.merkle_open(nodes, N, i))
    return bytes(out)


def opening4_len(W, K, log_N, t):
    R = 8 if K else 4
    return t * R * (9 + 8 * W) + t * R * (9 + 32 * log_N)


def air_proof(o, air, cols, p, g, log_n, lb, t, tau, h, E, bits, plus_p_col=None):
    """-> (row root, proof bytes, top, nonce) of smi_dev_air_prove_ext_fold4: the commitment, transcript, weights and
    composition of the factor-2 restatement (pow_compose.air_proof), FRI at folding factor 4, the rows of positions4.
    plus_p_col: a column committed and opened as value + p in every row -- the same residues under a tree that holds the
    raw u64, so every path verifies and only the canonical check can refuse the proof"""
    import air_compose as ac
    import air_periodic as ap
    import air_rows as ar
    N, B = 1 << (log_n + lb), 1 << lb
    W, K = len(cols), len(air.constraints)
    lde = ac.lde(o, cols, p, g, log_n, lb, tau, h)
    if plus_p_col is not None:
        lde = [np.asarray(c, dtype=np.uint64) + np.uint64(p if j == plus_p_col else 0) for j, c in enumerate(lde)]
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
    return root, fri + openings4_bytes(o, lde, top, N, B, K > 0, nodes), top, nonce


AIR_WORDS = {"length": "air openings: wrong length", "row": "air openings: malformed row", "path": "air openings: malformed path",
             "auth": "air openings: authentication path does not verify", "canonical": "air openings: an opened value is not canonical",
             "composition": "air openings: the composition of the opened rows is not the codeword value"}
# every sentence the two factor-4 verifiers can give: the FRI walk's (verify above) and the opening section's
FRI_SENTENCES = {"No FRI roots extracted", "Failed to extract Merkle root", "Failed to extract last codeword",
                 "last codeword: expected four values per element of the last domain", "last codeword: a coordinate is not canonical",
                 "last codeword is not well formed", "last codeword too small",
                 "last codeword does not correspond to polynomial of low enough degree", "proof of work: failed to extract the nonce",
                 "proof of work: the nonce record must hold exactly one value", "proof of work", "Failed to extract triple values",
                 "Expected triple of values", "triple: a coordinate is not canonical", FOLD4_MISMATCH, "Failed to extract path for aa",
                 "merkle authentication path verification fails for aa"}


def air_verify(o, air, root, proof, p, g, log_n, lb, t, tau, h, E, bits, slots=(0, 1, 2, 3)):
    """The verifier of smi_air_verify_ext_fold4 from the oracle's primitives and mirror.Air.compose_at (the definition, term
    by term) -> (accept, sentence).  A shape without a fold raises ValueError (the library refuses it with a status).
    slots: the points of a coset whose composition is recomputed -- all four; a test passes fewer to show what only the
    others can detect."""
    import air_compose as ac
    N, B, logN = 1 << (log_n + lb), 1 << lb, log_n + lb
    W, K = air.n_cols, len(air.constraints)
    if layout(N, E, t)[1] == 0:
        raise ValueError("no fold at this shape")
    tr, ch = xc.air_transcript(o, W, K, root)
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    cfg_o = o.fri_cfg(wN, h, N, E, t, p)
    ok, pv, used, top, why = verify(o, cfg_o, proof, g, tr, bits)
    if not ok:
        return False, why
    R = 8 if K else 4
    m, rec, prec = R * t, 9 + 8 * W, 9 + 32 * logN
    sec = proof[used:]
    if len(sec) != m * rec + m * prec:
        return False, AIR_WORDS["length"]
    rows, paths = [], []
    for q in range(m):                                           # every row record, then every path record
        r = sec[q * rec:(q + 1) * rec]
        if r[0] != 2 or int.from_bytes(r[1:9], "little") != W:
            return False, AIR_WORDS["row"]
        rows.append([int.from_bytes(r[9 + 8 * c:17 + 8 * c], "little") for c in range(W)])
    for q in range(m):
        r = sec[m * rec + q * prec:m * rec + (q + 1) * prec]
        if r[0] != 3 or int.from_bytes(r[1:9], "little") != logN:
            return False, AIR_WORDS["path"]
        paths.append([bytes(r[9 + 32 * k:41 + 32 * k]) for k in range(logN)])
    pos = [i for s in top for i in positions4(s, N, B, K > 0)]
    for q in range(m):                                           # the leaf is the row's u64s as they stand
        if not o.merkle_verify(o.hash_from_field_elements(rows[q]), pos[q], paths[q], root):
            return False, AIR_WORDS["auth"]
    for s in range(t):
        for k in range(4):
            for r in range(k, R, 4):                             # this point's rows, in front of this point's composition
                if any(v >= p for v in rows[R * s + r]):
                    return False, AIR_WORDS["canonical"]
            if k not in slots:
                continue
            idx, want = pv[4 * s + k]
            assert idx == pos[R * s + k]
            cur, nxt = rows[R * s + k], rows[R * s + k + 4] if K else None
            got = [air.compose_at(p, log_n, lb, tau, h, wN, idx, cur, nxt, xc.weight_vector(ch, e)) for e in range(4)]
            if got != want:
                return False, AIR_WORDS["composition"]
    return True, ""


def num_rounds(N, E, t):
    """src/fri.rs:93-103"""
    R, n = 0, N
    while n > E and 4 * t < n:
        n //= 2
        R += 1
    return R


def layout(N, E, t):
    """-> (R2, folds F, last length, proof bytes): F + 1 roots, the last codeword (4 L_last values), the nonce record, per
    layer r < F t coset records of 16 values and t paths of log2(N / 4^(r+1)) digests"""
    R2 = num_rounds(N, E, t)
    F = (R2 - 1) // 2 if R2 else 0
    last = N >> (2 * F)
    n = 33 * (F + 1) + (9 + 32 * last) + 17
    for r in range(F):
        depth = (N >> (2 * r + 2)).bit_length() - 1
        n += t * (9 + 128) + t * (9 + 32 * depth)
    return R2, F, last, n
