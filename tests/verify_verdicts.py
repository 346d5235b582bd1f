"""The recorded verdicts of every verifier in csrc/verify.hip (tests/golden/verify_verdicts.json): the cases, the mutations
of a proof and the raw C-ABI calls, shared by the generator (tests/golden/make_verify_verdicts.py) and the replay
(tests/test_gpu_verify_verdicts.py).  A verdict is what a caller can observe: status, *accept, the smi_last_error sentence,
consumed, n_pv and a checksum of pv_indices / pv_values.  Proofs are made by the device provers when the cases are built:
proving is deterministic and the grinding nonce is the least one, so only the verdicts are stored.
Not a test module."""
import ctypes as C
import zlib

import numpy as np

import air_compose as ac
import air_periodic as ap
import air_rows as ar
import perm_compose as pm
import transcript_compose as tc

SENTINEL = 12345          # what *accept, *n_pv and *consumed hold before a call: a verdict shows whether they were written
U64 = lambda v: int(v).to_bytes(8, "little")

# every sentence csrc/verify.hip passes to reject() at the commit the fixture was recorded at
SENTENCES = [
    "Failed to extract Merkle root", "Failed to extract last codeword", "No FRI roots extracted", "last codeword is not well formed",
    "last codeword too small", "re-evaluated codeword does not match original!",
    "last codeword does not correspond to polynomial of low enough degree", "Failed to extract triple values", "Expected triple of values",
    "colinearity check failure", "Failed to extract path for aa", "Failed to extract path for bb", "Failed to extract path for cc",
    "merkle authentication path verification fails for aa", "merkle authentication path verification fails for bb",
    "merkle authentication path verification fails for cc", "last codeword: expected four values per element of the last domain",
    "last codeword: a coordinate is not canonical", "proof of work: failed to extract the nonce",
    "proof of work: the nonce record must hold exactly one value", "proof of work", "triple: a coordinate is not canonical",
    "column openings: wrong length", "column openings: malformed row", "column openings: the weighted sum is not the codeword value",
    "column openings: malformed path", "column openings: authentication path does not verify", "air openings: wrong length",
    "air openings: malformed row", "air openings: malformed path", "air openings: authentication path does not verify",
    "air openings: an opened value is not canonical", "air openings: the composition of the opened rows is not the codeword value",
    "perm openings: wrong length", "perm openings: malformed row", "perm openings: malformed path",
    "perm openings: authentication path does not verify", "perm openings: an opened value is not canonical",
    "perm openings: the composition of the opened rows is not the codeword value",
]
# sentences no well-formed request reaches, with the reason (none is known: the list is here for the day one appears)
UNREACHABLE = {}


# ---------------------------------------------------------------------------------------------- the raw calls
def _verdict(eng, status, acc, used=None, npv=None, pi=None, pv=None, per=1):
    why = eng.L.smi_last_error(eng.h).decode() if (status == 0 and acc.value != 1) or status <= -50 else ""
    out = {"status": status, "accept": acc.value, "reason": why, "consumed": None if used is None else used.value,
           "n_pv": None if npv is None else npv.value, "pv": None}
    if npv is not None and npv.value != SENTINEL:
        out["pv"] = zlib.crc32(pi[:npv.value].tobytes() + pv[:per * npv.value].tobytes())
    return out


def call_fri(eng, fn, cfg, proof, prior=b"", bits=0):
    """fn: fri_verify | fri_verify_fs | fri_verify_ext | fri_verify_ext_pow"""
    n = 2 * int(cfg.num_colinearity_tests) + 2
    per = 4 if "ext" in fn else 1
    pi, pv = np.zeros(n, dtype=np.uint64), np.zeros(per * n, dtype=np.uint64)
    acc, npv, used = C.c_int(SENTINEL), C.c_size_t(SENTINEL), C.c_size_t(SENTINEL)
    tr = bytes(prior)
    if fn == "fri_verify":
        assert not tr
        st = eng.L.smi_fri_verify(eng.h, C.byref(cfg), proof, len(proof), C.byref(acc), pi.ctypes.data, pv.ctypes.data, C.byref(npv))
        return _verdict(eng, st, acc, None, npv, pi, pv)
    args = (eng.h, C.byref(cfg), tr if tr else None, len(tr), proof, len(proof), C.byref(acc), pi.ctypes.data, pv.ctypes.data, C.byref(npv),
            C.byref(used))
    if fn == "fri_verify_ext_pow":
        st = eng.L.smi_fri_verify_ext_pow(*args, bits)
    else:
        st = getattr(eng.L, "smi_" + fn)(*args)
    return _verdict(eng, st, acc, used, npv, pi, pv, per)


def call_air(eng, fn, flat, proof, roots, W, log_n, lb, t, bits=0, open_columns=1):
    """fn: stark_verify | air_verify | air_verify_rows | air_verify_ext | air_verify_ext_pow | air_verify_perm; flat: the
    flattened AIR (None for stark_verify); roots: bytes"""
    from stark_rs_amd import _lib
    cfg = _lib.StarkCfg(log_n, lb, W, 0 if fn in ("stark_verify", "air_verify") else 1, 1, eng.g, t, open_columns)
    rb = np.frombuffer(bytes(roots), dtype=np.uint8).copy()
    acc = C.c_int(SENTINEL)
    if fn == "stark_verify":
        st = eng.L.smi_stark_verify(eng.h, C.byref(cfg), rb.ctypes.data, proof, len(proof), C.byref(acc))
    elif fn == "air_verify_perm":
        st = eng.L.smi_air_verify_perm(eng.h, C.byref(cfg), C.byref(flat), C.byref(flat.perm), rb.ctypes.data, proof, len(proof), C.byref(acc), bits)
    elif fn == "air_verify_ext_pow":
        st = eng.L.smi_air_verify_ext_pow(eng.h, C.byref(cfg), C.byref(flat), rb.ctypes.data, proof, len(proof), C.byref(acc), bits)
    else:
        st = getattr(eng.L, "smi_" + fn)(eng.h, C.byref(cfg), C.byref(flat), rb.ctypes.data, proof, len(proof), C.byref(acc))
    return _verdict(eng, st, acc)


# ---------------------------------------------------------------------------------------------- records and mutations
def records(b):
    """a well-formed stream -> [(offset, tag, count, payload offset)]"""
    out, i = [], 0
    while i < len(b):
        tag = b[i]
        if tag == 0:
            out.append((i, 0, 1, i + 1))
            i += 33
        else:
            assert tag in (2, 3), (i, tag)
            cnt = int.from_bytes(b[i + 1:i + 9], "little")
            out.append((i, tag, cnt, i + 9))
            i += 9 + cnt * (8 if tag == 2 else 32)
    assert i == len(b)
    return out


def labels(R, t, grind, sections):
    """the name of every record of a proof in stream order: root<r>, last, nonce, r<r>.triple<s>, r<r>.path<s>.<aa|bb|cc>, then
    per opening section v its sec<v>.row<q> and sec<v>.path<q>; sections = [(rows, paths)]"""
    out = ["root%d" % r for r in range(R)] + ["last"] + (["nonce"] if grind else [])
    for r in range(R - 1):
        out += ["r%d.triple%d" % (r, s) for s in range(t)]
        out += ["r%d.path%d.%s" % (r, s, w) for s in range(t) for w in ("aa", "bb", "cc")]
    for v, (m_rows, m_paths) in enumerate(sections):
        out += ["sec%d.row%d" % (v, q) for q in range(m_rows)] + ["sec%d.path%d" % (v, q) for q in range(m_paths)]
    return out


def _kind(label):
    """the kind a record is an example of: its label without the test / position number"""
    head, _, tail = label.partition(".")
    if label.startswith("root") or label in ("last", "nonce"):
        return "root" if label.startswith("root") else label
    if tail.startswith("triple"):
        return head + ".triple"
    if head.startswith("sec"):
        return head + "." + tail.rstrip("0123456789")
    return head + ".path." + tail.rsplit(".", 1)[1]


class Stream:
    def __init__(self, proof, names, p):
        self.b, self.p = bytes(proof), p
        self.recs = records(self.b)
        assert len(self.recs) == len(names), (len(self.recs), len(names))
        self.at = dict(zip(names, self.recs))
        self.names = names

    def edit(self, b, op, name):
        """one defect: trunc (cut in front of the record) | tag | count | flip | plusp, applied to the bytearray b"""
        off, tag, cnt, pay = self.at[name]
        if op == "trunc":
            del b[off:]
        elif op == "tag":
            b[off] = {0: 2, 2: 3, 3: 2}[tag]
        elif op == "count":
            b[off + 1:off + 9] = U64(cnt - 1)
        elif op == "flip":
            b[pay] ^= 1
        elif op == "flip2":                     # a later value / digest of the record
            b[pay + (8 if tag == 2 else 32)] ^= 1
        elif op == "plusp":
            b[pay:pay + 8] = U64(int.from_bytes(b[pay:pay + 8], "little") + self.p)
        else:
            raise ValueError(op)

    def mutated(self, *edits):
        """edits in the order given, except that cuts run last (offsets stay valid)"""
        b = bytearray(self.b)
        for op, name in sorted(edits, key=lambda e: e[0] == "trunc"):
            if name in self.at and self.at[name][0] < len(b):
                self.edit(b, op, name)
        return bytes(b)

    def examples(self):
        """one record of every kind: the second of its kind where there is one (not the first test, not the first root)"""
        seen = {}
        for name in self.names:
            seen.setdefault(_kind(name), []).append(name)
        return {k: v[min(1, len(v) - 1)] for k, v in seen.items()}

    def single_mutations(self):
        yield "ok", self.b
        for name in self.names:
            yield "trunc@" + name, self.mutated(("trunc", name))
        yield "trunc@end-1", self.b[:-1]
        yield "one byte more", self.b + b"\x00"
        for kind, name in self.examples().items():
            tag = self.at[name][1]
            ops = ["tag", "flip"] + (["count"] if tag else []) + (["plusp"] if tag == 2 else [])
            for op in ops:
                yield "%s:%s" % (op, name), self.mutated((op, name))

    def pair(self, *edits):
        return "pair:" + " + ".join("%s:%s" % e for e in edits), self.mutated(*edits)


def fri_pairs(s, R):
    """defects in two places: the one checked first sits later in the stream, and the reverse"""
    out = [s.pair(("flip", "r0.path0.aa"), ("trunc", "r0.path2.aa")), s.pair(("flip", "r0.path1.bb"), ("flip", "r0.path0.cc")),
           s.pair(("flip", "r0.path2.cc"), ("tag", "r0.path1.aa")), s.pair(("flip", "r0.path0.bb"), ("count", "r0.path1.cc")),
           s.pair(("count", "r0.triple1"), ("flip", "r0.triple0")), s.pair(("plusp", "r0.triple0"), ("tag", "r0.triple1")),
           s.pair(("flip", "r0.triple2"), ("flip", "r0.path0.aa")), s.pair(("flip", "last"), ("tag", "root1")),
           s.pair(("flip", "root0"), ("trunc", "last")), s.pair(("flip", "last"), ("trunc", "r0.triple0")),
           s.pair(("plusp", "last"), ("count", "r0.triple0"))]
    if R > 2:
        out += [s.pair(("flip", "r1.path0.aa"), ("trunc", "r1.path1.cc")), s.pair(("flip", "r1.triple0"), ("flip", "r0.path2.cc")),
                s.pair(("flip", "r0.path2.cc"), ("trunc", "r1.triple0"))]
    if "nonce" in s.at:
        out += [s.pair(("flip", "nonce"), ("flip", "last")), s.pair(("flip", "nonce"), ("tag", "r0.triple0")),
                s.pair(("count", "nonce"), ("flip", "r0.path0.aa"))]
    return out


def opening_pairs(s, n_sections, last_path):
    out = [s.pair(("tag", last_path), ("flip", "sec0.row0")), s.pair(("tag", "sec0.row2"), ("trunc", last_path)),
           s.pair(("flip", "r0.path0.aa"), ("tag", "sec0.row0")), s.pair(("count", "sec0.path1"), ("flip", "sec0.path0")),
           s.pair(("plusp", "sec0.row1"), ("tag", "sec0.path3")), s.pair(("flip2", "sec0.row1"), ("flip", "sec0.row0")),
           s.pair(("count", "sec0.row3"), ("flip", "sec0.row0"))]
    if n_sections == 2:
        out += [s.pair(("tag", "sec1.path0"), ("flip", "sec0.path0")), s.pair(("tag", "sec1.row0"), ("flip", "sec0.row0")),
                s.pair(("flip", "sec1.path0"), ("flip", "sec0.path1")), s.pair(("plusp", "sec1.row0"), ("flip", "sec0.path2")),
                s.pair(("count", "sec1.row1"), ("tag", "sec0.path1"))]
    return out


# ---------------------------------------------------------------------------------------------- the cases
def _dev_cols(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr.astype(np.uint32)).reshape(-1).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr()


def _rounds(eng, cfg):
    return int(eng.fri_num_rounds(cfg))


def _forged_last(o, proof, R, vals):
    """the proof with its last root and last codeword replaced by `vals` and the root of their leaves"""
    recs = records(proof)
    arr = np.array(vals, dtype=np.uint64)
    root = bytes(o.merkle_commit(o.leaf_hashes(arr))) if len(vals) and len(vals) & (len(vals) - 1) == 0 else bytes(32)
    return proof[:33 * (R - 1)] + b"\x00" + root + b"\x02" + U64(len(vals)) + arr.tobytes() + proof[recs[R + 1][0]:]


def fri_case(eng, o, p, g, ext, N, E, t, prior, bits):
    """-> (name, [(mutation, fn, verdict thunk)])"""
    name = "%s N=%d E=%d t=%d prior=%d%s p=%d" % ("ext" if ext else "base", N, E, t, len(prior), "" if bits is None else " bits=%d" % bits, p)
    omega, offset = o.ff_prim_nth_root_g(N, p, g), g
    cfg = eng.fri_cfg(omega, offset, N, E, t)
    if ext:
        rng = np.random.default_rng(N + t)
        cw = np.stack([np.asarray(o.fast_coset_ntt(rng.integers(0, p, N // E, dtype=np.uint64), N, omega, offset, p), dtype=np.uint64) for _ in range(4)])
        keep, d_in = _dev_cols(cw)
        proof = eng.dev_fri_prove_ext(cfg, d_in, N, transcript=prior, grind_bits=bits)[0]
        del keep
    else:
        cw = o.fast_coset_ntt(o.splitmix64(11 + N, N // E) % np.uint64(p), N, omega, offset, p)
        proof = eng.fri_prove(cfg, cw, prior)[0]
    R = _rounds(eng, cfg)
    s = Stream(proof, labels(R, t, bits is not None, []), p)
    own = (["fri_verify_ext_pow"] if bits is not None else ["fri_verify_ext"]) if ext else (["fri_verify_fs"] + ([] if prior else ["fri_verify"]))
    b = 0 if bits is None else bits
    runs = []
    for mut, bad in list(s.single_mutations()) + fri_pairs(s, R):
        for fn in own:
            runs.append((mut, fn, lambda fn=fn, bad=bad: call_fri(eng, fn, cfg, bad, prior, b)))
    # other parameters, other transcripts, the other variants' verifiers
    from stark_rs_amd._lib import FriCfg
    others = {"cfg:E*2": FriCfg(omega, offset, N, 2 * E, t), "cfg:t+1": FriCfg(omega, offset, N, E, t + 1),
              "cfg:offset+1": FriCfg(omega, offset + 1, N, E, t), "cfg:no rounds": FriCfg(omega, offset, N, E, N // 4),
              "cfg:E=2": FriCfg(omega, offset, N, 2, t), "cfg:N=3N/2": FriCfg(omega, offset, 3 * N // 2, E, t)}
    for mut, c2 in others.items():
        for fn in own:
            runs.append((mut, fn, lambda fn=fn, c2=c2: call_fri(eng, fn, c2, proof, prior, b)))
    c0 = others["cfg:no rounds"]
    for fn in own:
        runs.append(("cfg:no rounds, from the last codeword", fn, lambda fn=fn: call_fri(eng, fn, c0, proof[s.at["last"][0]:], prior, b)))
        runs.append(("prior + one byte", fn if fn != "fri_verify" else "fri_verify_fs",
                     lambda fn=fn: call_fri(eng, fn if fn != "fri_verify" else "fri_verify_fs", cfg, proof, prior + b"x", b)))
    for fn in ("fri_verify_fs", "fri_verify_ext", "fri_verify_ext_pow"):
        if fn not in own:
            runs.append(("other verifier", fn, lambda fn=fn: call_fri(eng, fn, cfg, proof, prior, 0)))
    if bits is not None:
        nonce = int.from_bytes(proof[s.at["nonce"][3]:s.at["nonce"][3] + 8], "little")
        bad = bytearray(proof)
        bad[s.at["nonce"][3]:s.at["nonce"][3] + 8] = U64(nonce + 1)
        runs.append(("nonce + 1", own[0], lambda bad=bytes(bad): call_fri(eng, own[0], cfg, bad, prior, bits)))
        bad = proof[:s.at["nonce"][0]] + proof[s.at["nonce"][0] + 17:]
        runs.append(("nonce record missing", own[0], lambda bad=bad: call_fri(eng, own[0], cfg, bad, prior, bits)))
        for b2 in (0, bits + 16, 33):
            runs.append(("bits=%d demanded" % b2, own[0], lambda b2=b2: call_fri(eng, own[0], cfg, proof, prior, b2)))
    if not ext:
        n_last = s.at["last"][2]
        last = [int.from_bytes(proof[s.at["last"][3] + 8 * i:s.at["last"][3] + 8 * i + 8], "little") for i in range(n_last)]
        forged = {"last: no values": [], "last: two zeros": [0, 0], "last: three zeros": [0, 0, 0], "last: twice the length, zeros": [0] * (2 * n_last),
                  "last: half the length, zeros": [0] * (n_last // 2), "last: value + p committed": [last[0] + p] + last[1:],
                  "last: the same values committed again": last}
        for mut, vals in forged.items():
            bad = _forged_last(o, proof, R, vals)
            for fn in own:
                runs.append((mut, fn, lambda fn=fn, bad=bad: call_fri(eng, fn, cfg, bad, prior, 0)))
    return name, runs


def small_airs(n, p, name=None):
    """-> {name: (air builder taking the value of the first boundary point's offset, columns, log_blowup)}: K = 0 at W = 2,
    the Fibonacci pair (K = 2), the switch with its periodic selector (K = 2), and W = 3 with K = 2 (air_rows.wide)"""
    from stark_rs_amd.mirror import Air
    rng = np.random.default_rng(5)
    flat = [[int(x) for x in rng.integers(0, p, n)] for _ in range(2)]

    def k0(d=0):
        return Air(2).boundary(0, 0, (flat[0][0] + d) % p).boundary(1, n - 1, flat[1][n - 1])

    def fib(d=0):
        air, _ = ac.make("fib", n, p)
        air.boundaries[0] = (air.boundaries[0][0], air.boundaries[0][1], (air.boundaries[0][2] + d) % p)
        return air

    def switch(d=0):
        air, _ = ap.make("switch", n, p)
        air.boundaries[0] = (air.boundaries[0][0], air.boundaries[0][1], (air.boundaries[0][2] + d) % p)
        return air
    def wide3(d=0):
        air, _ = ar.wide(3, 2, p, n)
        air.boundaries[0] = (air.boundaries[0][0], air.boundaries[0][1], (air.boundaries[0][2] + d) % p)
        return air
    if name == "wide3":
        return wide3, ar.wide(3, 2, p, n)[1], 2
    return {"k0": (k0, flat, 2), "fib": (fib, ac.make("fib", n, p)[1], 3), "switch": (switch, ap.make("switch", n, p)[1], 3)}


AIR_FNS = {"cols": "air_verify", "rows": "air_verify_rows", "ext": "air_verify_ext", "extpow": "air_verify_ext_pow"}


def _upload(eng, cols):
    v = np.ascontiguousarray(np.asarray(cols, dtype=np.uint64)).reshape(-1)
    d = eng.dev_alloc(4 * v.size)
    eng.dev_upload(v, d)
    return d


def air_case(eng, o, p, g, variant, air_name, log_n, t, bits=4):
    make, cols, lb = small_airs(1 << log_n, p, "wide3") if air_name == "wide3" else small_airs(1 << log_n, p)[air_name]
    air, W, K = make(), len(cols), len(make().constraints)
    name = "air %s %s log_n=%d lb=%d t=%d p=%d" % (variant, air_name, log_n, lb, t, p)
    d = _upload(eng, cols)
    res = eng.dev_air_prove(air, d, W, log_n, lb, t, row_leaves=variant != "cols", ext=variant in ("ext", "extpow"),
                            grind_bits=bits if variant == "extpow" else None)
    eng.sync()
    eng.dev_free(d)
    proof, roots = res["proof"], res["column_roots"].tobytes()
    _d, E = eng.air_plan(air, W, log_n, lb)
    N = 1 << (log_n + lb)
    R = _rounds(eng, eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t))
    m = (4 if K else 2) * t
    s = Stream(proof, labels(R, t, variant == "extpow", [(m, m * (W if variant == "cols" else 1))]), p)
    flat, flat2, fn = air.flatten(p), make(1).flatten(p), AIR_FNS[variant]
    verify = lambda bad, f=flat, fn=fn, r=roots, b=bits: call_air(eng, fn, f, bad, r, W, log_n, lb, t, b)
    runs = []
    for mut, bad in list(s.single_mutations()) + fri_pairs(s, R)[:6] + opening_pairs(s, 1, s.names[-1]):
        runs.append((mut, fn, lambda bad=bad: verify(bad)))
    runs.append(("another boundary value", fn, lambda: verify(proof, f=flat2)))
    runs.append(("another boundary value + flip:sec0.row0", fn, lambda: verify(s.mutated(("flip", "sec0.row0")), f=flat2)))
    wrong = bytearray(roots)
    wrong[5] ^= 1
    runs.append(("wrong root", fn, lambda: verify(proof, r=bytes(wrong))))
    if variant == "extpow":
        runs.append(("bits + 16 demanded", fn, lambda: verify(proof, b=bits + 16)))
        runs.append(("bits 33 demanded", fn, lambda: verify(proof, b=33)))
        runs.append(("pair:flip:nonce + tag:sec0.row0", fn, lambda: verify(s.mutated(("flip", "nonce"), ("tag", "sec0.row0")))))
    for v2, fn2 in AIR_FNS.items():                                         # the other variants' verifiers
        if fn2 != fn:
            r2 = roots[:32] * W if v2 == "cols" else roots[:32]
            runs.append(("other verifier", fn2, lambda fn2=fn2, r2=r2: call_air(eng, fn2, flat, proof, r2, W, log_n, lb, t, bits)))
    runs.append(("other verifier", "stark_verify", lambda: call_air(eng, "stark_verify", None, proof, roots[:32] * W, W, log_n, lb, t)))
    return name, runs


def stark_case(eng, o, p, g, log_n=4, lb=2, W=3, t=3):
    name = "stark open_columns log_n=%d lb=%d W=%d t=%d p=%d" % (log_n, lb, W, t, p)
    n = 1 << log_n
    cols = np.stack([o.splitmix64(0x5354524B00 + c, n) % np.uint64(p) for c in range(W)])
    d = _upload(eng, cols)
    res = eng.dev_stark_prove(d, W, log_n, lb, t, open_columns=True)
    eng.sync()
    eng.dev_free(d)
    proof, roots = res["proof"], res["column_roots"].tobytes()
    N = 1 << (log_n + lb)
    R = _rounds(eng, eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, 1 << lb, t))
    s = Stream(proof, labels(R, t, False, [(2 * t, 2 * t * W)]), p)
    verify = lambda bad, r=roots, oc=1, w=W: call_air(eng, "stark_verify", None, bad, r, w, log_n, lb, t, open_columns=oc)
    runs = [(mut, "stark_verify", lambda bad=bad: verify(bad)) for mut, bad in
            list(s.single_mutations()) + fri_pairs(s, R)[:6] + opening_pairs(s, 1, s.names[-1])]
    runs.append(("roots rotated", "stark_verify", lambda: verify(proof, r=roots[32:] + roots[:32])))
    runs.append(("open_columns = 0", "stark_verify", lambda: verify(proof, oc=0)))
    runs.append(("no columns", "stark_verify", lambda: verify(proof, w=0)))
    from stark_rs_amd.mirror import Air
    flat = Air(W).flatten(p)
    runs.append(("other verifier", "air_verify", lambda: call_air(eng, "air_verify", flat, proof, roots, W, log_n, lb, t)))
    return name, runs


def rows_plus_p_case(eng, o, p, g, log_n=4, t=3):
    """a row-committed proof from the oracle's primitives whose tree commits to column 1 with p added in the upper half of
    the domain: every path verifies, so the canonical check is reached -- and, with another boundary value, its place
    between the compositions of the two sides of a test"""
    make, cols, lb = small_airs(1 << log_n, p)["fib"]
    air, W, K = make(), 2, 2
    name = "air rows fib, column 1 + p committed in the upper half, log_n=%d lb=%d t=%d p=%d" % (log_n, lb, t, p)
    N, B = 1 << (log_n + lb), 1 << lb
    _d, E = eng.air_plan(air, W, log_n, lb)
    lde = ac.lde(o, cols, p, g, log_n, lb, 1, g)
    shown = [np.asarray(c, dtype=np.uint64).copy() for c in lde]
    shown[1][N // 2:] += np.uint64(p)
    nodes = o.merkle_new(ar.row_leaves(o, shown))
    root = bytes(nodes[-1])
    prior, wts = ar.transcript(o, W, K, root)
    cw = ac.codeword_poly_route(o, air, cols, wts, p, g, log_n, lb, 1, g)[0]
    _, wN = ac.roots_of_unity(o, p, g, log_n, lb)
    fri, top = tc.prove(o, o.fri_cfg(wN, g, N, E, t, p), cw, prior)
    proof = fri + ar.openings_bytes(o, shown, top, N, B, True, nodes)
    flat, flat2 = air.flatten(p), make(1).flatten(p)
    runs = [("as committed", "air_verify_rows", lambda: call_air(eng, "air_verify_rows", flat, proof, root, W, log_n, lb, t)),
            ("another boundary value", "air_verify_rows", lambda: call_air(eng, "air_verify_rows", flat2, proof, root, W, log_n, lb, t))]
    return name, runs


def perm_case(eng, o, p, g, log_n=8, t=8, bits=0, lb=3):
    name = "perm cubic log_n=%d lb=%d t=%d bits=%d p=%d" % (log_n, lb, t, bits, p)
    n = 1 << log_n

    def make():
        air, cols = pm.cubic(n, p)
        return pm.with_permutation(air, cols, 1, p)
    air, cols = make()
    W, K = len(cols), len(air.constraints)
    d = _upload(eng, cols)
    res = eng.dev_air_prove(air, d, W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=bits)
    eng.sync()
    eng.dev_free(d)
    proof, roots = res["proof"], res["column_roots"].tobytes()
    _d, E = eng.air_plan(air, W, log_n, lb)
    N = 1 << (log_n + lb)
    R = _rounds(eng, eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t))
    s = Stream(proof, labels(R, t, True, [(4 * t, 4 * t), (4 * t, 4 * t)]), p)
    flat = air.flatten(p)
    other = make()[0]
    other.perm = ([1], [W - 1])
    flat2 = other.flatten(p)
    fn = "air_verify_perm"
    verify = lambda bad, f=flat, r=roots, b=bits: call_air(eng, fn, f, bad, r, W, log_n, lb, t, b)
    runs = []
    for mut, bad in list(s.single_mutations()) + fri_pairs(s, R)[:6] + opening_pairs(s, 2, s.names[-1]):
        runs.append((mut, fn, lambda bad=bad: verify(bad)))
    runs.append(("a swapped column", fn, lambda: verify(proof, f=flat2)))
    runs.append(("a swapped column + flip:sec1.row0", fn, lambda: verify(s.mutated(("flip", "sec1.row0")), f=flat2)))
    runs.append(("bits + 16 demanded", fn, lambda: verify(proof, b=bits + 16)))
    wrong = bytearray(roots)
    wrong[40] ^= 1
    runs.append(("wrong root_2", fn, lambda: verify(proof, r=bytes(wrong))))
    plain = make()[0]
    plain.perm = None
    fp = plain.flatten(p)
    for fn2 in ("air_verify_ext_pow", "air_verify_ext", "air_verify_rows"):
        runs.append(("other verifier", fn2, lambda fn2=fn2: call_air(eng, fn2, fp, proof, roots[:32], W, log_n, lb, t, bits)))
    left, right = air.perm
    for mut, kw in (("z coordinate 3 + p committed", dict(z_plus_p=3)), ("trace column 1 + p committed", dict(trace_plus_p=1))):
        tam = pm.prove(o, air, left, right, cols, p, g, log_n, lb, t, 1, g, E, bits, **kw)
        runs.append((mut, fn, lambda tam=tam: verify(tam["proof"], r=tam["roots"])))
        runs.append((mut + ", a swapped column", fn, lambda tam=tam: verify(tam["proof"], f=flat2, r=tam["roots"])))
    return name, runs


def all_cases(engines, o):
    """-> [(case name, [(mutation, function, thunk -> verdict)])] in a fixed order"""
    out = []
    (p0, g0), (p1, g1) = ac.PRIMES
    shapes = [(64, 4, 3), (128, 4, 4)]
    for i, (N, E, t) in enumerate(shapes):
        p, g = ac.PRIMES[i]
        for prior in (b"", bytes(range(37))):
            out.append(fri_case(engines[p], o, p, g, False, N, E, t, prior, None))
            out.append(fri_case(engines[p], o, p, g, True, N, E, t, prior, None))
        out.append(fri_case(engines[p], o, p, g, True, N, E, t, bytes(range(37)) if i else b"", 6))
    out.append(stark_case(engines[p0], o, p0, g0))
    for i, (variant, air_name) in enumerate((v, a) for a in ("k0", "fib", "switch") for v in AIR_FNS):
        p, g = ac.PRIMES[i % 2]
        out.append(air_case(engines[p], o, p, g, variant, air_name, 4, 3))
    out.append(rows_plus_p_case(engines[p0], o, p0, g0))
    out.append(perm_case(engines[p1], o, p1, g1))
    for i, variant in enumerate(AIR_FNS):                                   # W = 3, four opened rows: three trees, three-wide rows
        p, g = ac.PRIMES[(i + 1) % 2]
        out.append(air_case(engines[p], o, p, g, variant, "wide3", 4, 3))
    return out


def run_all(engines, o):
    """-> {case: [[mutation, function, status, accept, reason, consumed, n_pv, pv], ...]}"""
    table = {}
    for name, runs in all_cases(engines, o):
        rows = []
        for mut, fn, thunk in runs:
            v = thunk()
            rows.append([mut, fn, v["status"], v["accept"], v["reason"], v["consumed"], v["n_pv"], v["pv"]])
        assert name not in table
        table[name] = rows
    return table


# ---------------------------------------------------------------------------------------------- the fixture file
# The table is stored packed: the mutation names, the function names and the (status, accept, sentence) triples once each,
# and per case a flat list of integers: name, function, triple a row, and for the FRI functions (which have these outputs)
# consumed, n_pv, pv as well, with -1 for "not an output of this function".  pack and unpack are inverse to each other.
def pack(table):
    names = sorted({r[0] for rows in table.values() for r in rows})
    fns = sorted({r[1] for rows in table.values() for r in rows})
    triples = sorted({tuple(r[2:5]) for rows in table.values() for r in rows})
    ni, fi, ti = ({x: i for i, x in enumerate(xs)} for xs in (names, fns, triples))
    cases = {case: [x for r in rows for x in [ni[r[0]], fi[r[1]], ti[tuple(r[2:5])]] +
                    ([-1 if v is None else v for v in r[5:8]] if r[1].startswith("fri") else [])] for case, rows in table.items()}
    return {"names": names, "functions": fns, "verdicts": [list(t) for t in triples], "cases": cases}


def unpack(packed):
    names, fns, triples = packed["names"], packed["functions"], packed["verdicts"]
    out = {}
    for case, f in packed["cases"].items():
        rows, k = [], 0
        while k < len(f):
            fri = fns[f[k + 1]].startswith("fri")
            rows.append([names[f[k]], fns[f[k + 1]]] + list(triples[f[k + 2]]) + ([None if v == -1 else v for v in f[k + 3:k + 6]] if fri else [None] * 3))
            k += 6 if fri else 3
        out[case] = rows
    return out


def dump(table, path):
    import json
    p = pack(table)

    def wrap(xs):                                                   # whole items, lines of up to 158 characters
        lines, line = [], " "
        for i, x in enumerate(xs):
            item = (" " if isinstance(x, str) else "") + json.dumps(x, separators=(",", ":")) + ("," if i + 1 < len(xs) else "")
            if len(line) + len(item) > 158 and line != " ":
                lines.append(line)
                line = " "
            line += item
        return "\n".join(lines + [line])
    parts = ['"%s": [\n%s\n ]' % (k, wrap(p[k])) for k in ("names", "functions", "verdicts")]
    parts.append('"cases": {\n' + ",\n".join(' %s: [\n%s\n ]' % (json.dumps(c), wrap(f)) for c, f in p["cases"].items()) + "\n}")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(parts) + "\n}\n")


def load(path):
    import json
    return unpack(json.load(open(path)))
