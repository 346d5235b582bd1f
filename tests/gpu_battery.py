"""One parity battery for every Merkle and FRI launch plan, independent of the SMI_* tuning knobs (which a process reads
once): the same items, against the same oracle expectations, whatever plan the knobs of the running process choose.

  expected(oracle, out_dir)       CPU oracle only: inputs and expected outputs, written as files under out_dir
  run(engines, exp_dir, report)   GPU only, no oracle: every item through the C ABI entry that reaches it, every stored
                                  level and every proof byte compared, kernel launches recorded per item

Not a test module: imported by tests/test_gpu_plans.py (default knobs, in-process) and started by it as
`python tests/gpu_battery.py EXP_DIR REPORT.json` in a fresh child per non-default knob setting.  Exit status: 0 all items
equal, 1 a mismatch, 2 an item raised."""
import json
import os
import sys
import time

import numpy as np

P, G = 998244353, 3
P2, G2 = 469762049, 3
MAX_LOG = 21
ELEM_LOGS = list(range(0, MAX_LOG + 1))
DIGEST_LOGS = list(range(1, MAX_LOG + 1))
ROW4_LOGS = list(range(0, MAX_LOG + 1))
ROW_WIDTHS_AT_20 = (1, 3, 5)
# Under TOP_BLOCKS=1024 two subtree steps first appear above 2^21 leaves -- the K=2 step over digests and the row-leaf
# step (tests/test_launch_plans.py derives both from the planner): the smallest trees that take them, checked by
# their root and N_OPENINGS openings instead of every level
EXTRA_TREES = {"Dx22": ("D", 22, 0), "Rx22": ("R", 22, 4)}
TOP_LOG = 22
N_OPENINGS = 64
PRIOR = bytes((7 * i + 1) & 255 for i in range(37))   # 37 bytes: Fiat-Shamir phase 5 (not a whole number of 32-byte chunks)
STARK = dict(logn=17, lb=3, W=4, t=8)                  # N = 2^20 on the second prime
LDE = dict(logn=20, lb=3, W=3)
PROVES = {   # name: (log len, expansion, t, offset, prior)
    "prove_a": (21, 8, 8, 5, b""),
    "prove_b": (14, 8, 16, 3, b""),
    "prove_b_prior": (14, 8, 16, 3, PRIOR),
    "prove_c": (12, 4, 4, 3, b""),
}


def tree_input(base, n, p):
    """the first n of the base values (base: (W, >= n) or (>= n,)), p - 1 at index 0 and at the last index"""
    a = np.array(base[..., :n], dtype=np.uint64)
    a[..., 0] = p - 1
    a[..., n - 1] = p - 1
    return a


def tree_items(extras=True):
    """name -> (leaf kind 'E' | 'D' | 'R', log n, row width, full: every level is compared)"""
    items = {}
    for l in ELEM_LOGS:
        items["E%02d" % l] = ("E", l, 0, True)
    for l in DIGEST_LOGS:
        items["D%02d" % l] = ("D", l, 0, True)
    for l in ROW4_LOGS:
        items["R4_%02d" % l] = ("R", l, 4, True)
    for w in ROW_WIDTHS_AT_20:
        items["R%d_20" % w] = ("R", 20, w, True)
    if extras:
        for name, (kind, l, w) in EXTRA_TREES.items():
            items[name] = (kind, l, w, False)
    return items


def level_start(n, lvl):
    """index of level lvl's first node among the 2n - 1 nodes stored level after level"""
    return 2 * (n - (n >> lvl))


def _opening_indices(n, seed):
    rng = np.random.default_rng(seed)
    idx = [0, n - 1] + [int(v) for v in rng.integers(0, n, N_OPENINGS - 2)]
    return idx


# ------------------------------------------------------------------------------------------------ expectations
def expected(o, out_dir, extras=True, log=None):
    """Everything run() compares with, from the oracle alone.  Returns the manifest (also written as manifest.json)."""
    import transcript_compose as tc
    say = log or (lambda *_: None)
    os.makedirs(out_dir, exist_ok=True)
    save = lambda name, arr: np.save(os.path.join(out_dir, name), np.ascontiguousarray(arr))
    man = {"trees": {}, "proves": {}, "stark": {}, "lde": {}}
    t0 = time.time()

    top_log = TOP_LOG if extras else MAX_LOG
    base_e = o.splitmix64(0xE1E3, 1 << top_log) % np.uint64(P)
    base_r = np.stack([o.splitmix64(0x520000 + c, 1 << top_log) % np.uint64(P) for c in range(5)])
    save("base_e.npy", base_e)
    save("base_r.npy", base_r)

    def trees(kinds):
        for name, (kind, l, w, full) in tree_items(extras).items():
            if kind not in kinds:
                continue
            n = 1 << l
            if kind == "D" and full:       # the digests are the leaf hashes of the same elements: the element tree's nodes
                man["trees"][name] = {"kind": kind, "logn": l, "W": 0, "full": True, "file": "tree_E%02d.npy" % l}
                continue
            if kind == "R":
                leaves = o.row_hashes(tree_input(base_r[:w], n, P))
            else:
                leaves = o.leaf_hashes_batched(tree_input(base_e, n, P))
            nodes = o.merkle_new(leaves)
            ent = {"kind": kind, "logn": l, "W": w, "full": full}
            if full:
                ent["file"] = "tree_%s.npy" % name
                save(ent["file"], nodes)
            else:
                idx = _opening_indices(n, l)
                paths = [o.merkle_open(nodes, n, i) for i in idx]
                root = bytes(nodes[-1])
                for i, path in zip(idx, paths):
                    assert o.merkle_verify(bytes(leaves[i]), i, path, root), (name, i)
                ent.update(root=root.hex(), indices=idx, file="open_%s.npy" % name)
                save(ent["file"], np.frombuffer(b"".join(b"".join(p) for p in paths), dtype=np.uint8).reshape(len(idx), l, 32))
            man["trees"][name] = ent
            say("tree %s %.1fs" % (name, time.time() - t0))

    def proves():
        for name, (l, exp, t, offset, prior) in PROVES.items():
            n = 1 << l
            omega = o.ff_prim_nth_root(n)
            cw = o.fast_coset_ntt(o.splitmix64(77 + l, n // exp) % np.uint64(P), n, omega, offset)
            cfg = o.fri_cfg(omega, offset, n, exp, t)
            proof, top = tc.prove(o, cfg, cw, prior) if prior else o.fri_prove(cfg, cw)
            save(name + "_cw.npy", cw)
            with open(os.path.join(out_dir, name + ".bin"), "wb") as f:
                f.write(proof)
            man["proves"][name] = {"logn": l, "expansion": exp, "t": t, "offset": offset, "omega": omega, "prior": prior.hex(),
                                   "top": [int(v) for v in top]}
            say("%s %.1fs" % (name, time.time() - t0))

    def stark():
        # the build-defined prove, composed as tests/test_gpu_pipeline.py::test_stark_prove_composition does
        logn, lb, W, t = STARK["logn"], STARK["lb"], STARK["W"], STARK["t"]
        n, N = 1 << logn, 1 << (logn + lb)
        cols = np.stack([o.splitmix64(0x5354524B00 + c, n) % np.uint64(P2) for c in range(W)])
        w, Wn = o.ff_prim_nth_root_g(n, P2, G2), o.ff_prim_nth_root_g(N, P2, G2)
        lde = np.stack([o.fast_coset_ntt(o.fast_intt(cols[c], w, 1, P2), N, Wn, G2, P2) for c in range(W)])
        trees = [o.merkle_new(o.leaf_hashes_batched(lde[c])) for c in range(W)]
        cfg = o.fri_cfg(Wn, G2, N, 1 << lb, t, P2)
        # lde < 2^29 and weights < 2^29: the sum of W = 4 products stays below 2^64
        combine = lambda weights: sum(lde[c] * np.uint64(weights[c]) for c in range(W)) % np.uint64(P2)
        fs, weights = o.FiatShamir(), []
        for c in range(W):
            fs.absorb(bytes(trees[c][-1]))
            weights.append(fs.challenge() % P2)
        proof, top = o.fri_prove(cfg, combine(weights))
        # smi_stark_cfg.open_columns: rows at a and a + N/2 per test, then per (test, column) MerkleTree::open at both
        u64 = lambda v: int(v).to_bytes(8, "little")
        half, opened = N // 2, bytearray()
        for s in top:
            for i in (s % half, s % half + half):
                opened += b"\x02" + u64(W) + b"".join(u64(col[i]) for col in lde)
        for s in top:
            for c in range(W):
                for i in (s % half, s % half + half):
                    path = o.merkle_open(trees[c], N, i)
                    opened += b"\x03" + u64(len(path)) + b"".join(path)
        row_root = bytes(o.merkle_new(o.row_hashes(lde))[-1])
        row_weights = [int.from_bytes(o.hash_from_bytes(row_root + c.to_bytes(8, "little"))[:8], "little") % P2 for c in range(W)]
        row_proof, row_top = o.fri_prove(cfg, combine(row_weights))
        save("stark_cols.npy", cols)
        for fname, blob in (("stark_columns.bin", proof), ("stark_opened.bin", proof + bytes(opened)), ("stark_rows.bin", row_proof)):
            with open(os.path.join(out_dir, fname), "wb") as f:
                f.write(blob)
        man["stark"] = dict(STARK, column_roots=[bytes(tr[-1]).hex() for tr in trees], top=[int(v) for v in top],
                            row_root=row_root.hex(), row_top=[int(v) for v in row_top])
        say("stark %.1fs" % (time.time() - t0))

    def lde():
        logn, lb, W = LDE["logn"], LDE["lb"], LDE["W"]
        n, N = 1 << logn, 1 << (logn + lb)
        cols = np.stack([tree_input(o.splitmix64(0x4C4445 + c, n) % np.uint64(P), n, P) for c in range(W)])
        w, Wn = o.ff_prim_nth_root(n), o.ff_prim_nth_root(N)
        out = np.stack([o.fast_coset_ntt(o.fast_intt(cols[c], w, 1), N, Wn, G).astype(np.uint32) for c in range(W)])
        save("lde_in.npy", cols)
        save("lde_out.npy", out)
        man["lde"] = dict(LDE)
        say("lde %.1fs" % (time.time() - t0))

    # five independent jobs side by side: the oracle's C calls release the interpreter lock, and the only state they share
    # is the message of a panic, which none of these calls raises
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(5) as pool:
        for job in [pool.submit(f) for f in (stark, lambda: trees("ED"), lambda: trees("R"), proves, lde)]:
            job.result()
    man["trees"] = {name: man["trees"][name] for name in tree_items(extras)}

    man["oracle_seconds"] = round(time.time() - t0, 1)
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(man, f)
    return man


# ----------------------------------------------------------------------------------------------------- GPU half
def _first_diff(a, b):
    a, b = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    if len(a) != len(b):
        return min(len(a), len(b))
    d = np.flatnonzero(a != b)
    return int(d[0]) if len(d) else None


def _digests(eng, d_ptr, count):
    """count 32-byte digests at d_ptr (the download is of u32 words widened to u64)"""
    return eng.dev_download(d_ptr, 8 * count).astype(np.uint32).view(np.uint8).reshape(count, 32)


class _Runner:
    def __init__(self, engines, exp_dir):
        self.eng, self.eng2, self.dir = engines["ref"], engines["p2"], exp_dir
        self.items = {}

    def load(self, name):
        return np.load(os.path.join(self.dir, name), mmap_mode="r")

    def blob(self, name):
        with open(os.path.join(self.dir, name), "rb") as f:
            return f.read()

    def item(self, name, eng, fn):
        """fn() -> (ok, where) bracketed by the context's launch profile"""
        if self.only is not None and name not in self.only:
            return
        t0 = time.time()
        eng.profile(True)
        try:
            ok, where = fn()
            rec = {"ok": bool(ok), "where": where}
        except Exception as e:   # a status from the ABI is a failed item; the engine is still usable
            rec = {"ok": False, "where": None, "error": "%s: %s" % (type(e).__name__, e)}
        rec["launches"] = {k: v["launches"] for k, v in eng.profile_read().items()}
        eng.profile(False)
        rec["seconds"] = round(time.time() - t0, 3)
        self.items[name] = rec

    def tree(self, ent, base_e, base_r, d_in, d_nodes):
        eng, kind, n, w = self.eng, ent["kind"], 1 << ent["logn"], ent["W"]
        if kind == "R":
            eng.dev_upload(tree_input(base_r[:w], n, P).reshape(-1), d_in)
            eng.dev_merkle_build_rows(d_in, w, n, n, d_nodes)
        else:
            eng.dev_upload(tree_input(base_e, n, P), d_in)
            if kind == "E":
                eng.dev_merkle_build(d_in, n, d_nodes)
            else:
                eng.dev_hash_leaves(d_in, n, d_nodes)
                eng.dev_merkle_from_digests(n, d_nodes)
        if ent["full"]:
            got, want = _digests(eng, d_nodes, 2 * n - 1), self.load(ent["file"])
            bad = np.flatnonzero((got != want).any(axis=1))
            if not len(bad):
                return True, None
            node = int(bad[0])
            lvl = max(l for l in range(ent["logn"] + 1) if level_start(n, l) <= node)
            return False, {"level": lvl, "index": node - level_start(n, lvl), "differing_nodes": int(len(bad))}
        # the root and N_OPENINGS authentication paths read out of the stored levels, against the oracle's
        if bytes(_digests(eng, d_nodes + 32 * (2 * n - 2), 1)[0]).hex() != ent["root"]:
            return False, {"level": ent["logn"], "index": 0}
        want = self.load(ent["file"])
        for k, i in enumerate(ent["indices"]):
            for lvl in range(ent["logn"]):
                sib = (i >> lvl) ^ 1
                if not np.array_equal(_digests(eng, d_nodes + 32 * (level_start(n, lvl) + sib), 1)[0], want[k, lvl]):
                    return False, {"level": lvl, "index": sib, "opening": i}
        return True, None

    def prove(self, name, ent, misaligned):
        eng = self.eng
        n = 1 << ent["logn"]
        cw, want = self.load(name + "_cw.npy"), self.blob(name + ".bin")
        cfg = eng.fri_cfg(ent["omega"], ent["offset"], n, ent["expansion"], ent["t"])
        d = eng.dev_alloc((n + 4) * 4)
        at = d + 4 if misaligned else d     # only 4-byte aligned: the four-at-a-time leaf source must not be used on it
        try:
            eng.dev_upload(cw, at)
            got, top = eng.dev_fri_prove(cfg, at, n, bytes.fromhex(ent["prior"]))
        finally:
            eng.dev_free(d)
        if list(top) != ent["top"]:
            return False, {"top_indices": list(top)}
        at = _first_diff(got, want)
        return at is None, (None if at is None else {"byte": at})

    def stark(self, man, variant):
        """smi_dev_stark_prove, the single-GPU entry that builds several trees in one set of launches (launch_merkle_batch,
        grid.y = W).  The ABI hands out no node of those trees: what it does hand out is compared -- the W roots, and with
        open_columns the authentication paths of every column at the sampled rows -- with the oracle's four trees."""
        eng, cols = self.eng2, self.load("stark_cols.npy")
        d = eng.dev_alloc(cols.size * 4)
        try:
            eng.dev_upload(np.array(cols).reshape(-1), d)
            res = eng.dev_stark_prove(d, man["W"], man["logn"], man["lb"], man["t"], row_leaves=variant == "rows",
                                      open_columns=variant == "opened")
        finally:
            eng.dev_free(d)
        roots = [bytes(r).hex() for r in res["column_roots"]]
        want_roots = [man["row_root"]] if variant == "rows" else man["column_roots"]
        if roots != want_roots:
            return False, {"column_roots": [c for c in range(len(want_roots)) if roots[c] != want_roots[c]]}
        if res["top_indices"] != (man["row_top"] if variant == "rows" else man["top"]):
            return False, {"top_indices": res["top_indices"]}
        at = _first_diff(res["proof"], self.blob("stark_%s.bin" % variant))
        return at is None, (None if at is None else {"byte": at})

    def lde(self, man, two_pass):
        eng, cols, want = self.eng, self.load("lde_in.npy"), self.load("lde_out.npy")
        W, n, N = man["W"], 1 << man["logn"], 1 << (man["logn"] + man["lb"])
        d_in, d_out = eng.dev_alloc(W * n * 4), eng.dev_alloc(W * N * 4)
        try:
            eng.lde_two_pass(two_pass)
            eng.dev_upload(np.array(cols).reshape(-1), d_in)
            eng.dev_lde(d_in, W, man["logn"], man["lb"], d_out, 1, G)
            for c in range(W):
                got = eng.dev_download(d_out + 4 * c * N, N)
                bad = np.flatnonzero(got != want[c])
                if len(bad):
                    return False, {"column": c, "index": int(bad[0]), "differing": int(len(bad))}
        finally:
            eng.lde_two_pass(False)
            eng.dev_free(d_in)
            eng.dev_free(d_out)
        return True, None


def run(engines, exp_dir, report=None, extras=True, only=None):
    """engines: {"ref": Engine(P, G), "p2": Engine(P2, G2)}.  -> the report (written to `report` as JSON when given):
    per item ok, where it first differs, launches per kernel name; the SMI_* variables of this process; wall seconds.
    only: a set of item names to run instead of all."""
    t0 = time.time()
    with open(os.path.join(exp_dir, "manifest.json")) as f:
        man = json.load(f)
    r = _Runner(engines, exp_dir)
    r.only = None if only is None else set(only)
    eng = r.eng
    base_e, base_r = r.load("base_e.npy"), r.load("base_r.npy")
    top_log = max(e["logn"] for name, e in man["trees"].items() if extras or e["full"])
    d_in = eng.dev_alloc((5 << top_log) * 4)
    d_nodes = eng.dev_alloc((2 << top_log) * 32)
    for name, ent in man["trees"].items():
        if ent["full"] or extras:
            r.item(name, eng, lambda: r.tree(ent, base_e, base_r, d_in, d_nodes))
    eng.dev_free(d_in)
    eng.dev_free(d_nodes)
    for name, ent in man["proves"].items():
        r.item(name, eng, lambda: r.prove(name, ent, False))
    r.item("prove_a_misaligned", eng, lambda: r.prove("prove_a", man["proves"]["prove_a"], True))
    for variant in ("columns", "opened", "rows"):
        r.item("stark_" + variant, r.eng2, lambda: r.stark(man["stark"], variant))
    for two_pass in (False, True):
        r.item("lde_two_pass" if two_pass else "lde", eng, lambda: r.lde(man["lde"], two_pass))
    out = {"items": r.items, "env": {k: v for k, v in os.environ.items() if k.startswith("SMI_")},
           "ok": all(i["ok"] for i in r.items.values()), "seconds": round(time.time() - t0, 2)}
    if report:
        with open(report, "w") as f:
            json.dump(out, f, indent=1)
    return out


def main(argv):
    if len(argv) < 3:
        print("usage: gpu_battery.py EXPECTATION_DIR REPORT.json [--no-extras] [--only=ITEM,ITEM,...]", file=sys.stderr)
        return 2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import stark_rs_amd as s
    engines = {"ref": s.Engine(P, G, 0), "p2": s.Engine(P2, G2, 0)}
    try:
        only = [a[len("--only="):].split(",") for a in argv[3:] if a.startswith("--only=")]
        out = run(engines, argv[1], argv[2], extras="--no-extras" not in argv[3:], only=only[0] if only else None)
    finally:
        for e in engines.values():
            e.close()
    for name, it in out["items"].items():
        if not it["ok"]:
            print("MISMATCH", name, it.get("where"), it.get("error", ""))
    print("battery: %d items, %s, %.1f s" % (len(out["items"]), "all equal" if out["ok"] else "FAILED", out["seconds"]))
    if any("error" in it for it in out["items"].values()):
        return 2
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
