#!/usr/bin/env python3
"""Development tool (GPU box): this build against a build of the parent commit, for the change that routed the plain argument
list through the operand list's kernels and gave the four two-tree provers one body ("Where a new two-tree variant
plugs in").

    python3 tools/two_tree_ab.py --parent-lib <the parent commit's libstarkmi.so> [--out profiles/two_tree_prover_ab.log]

The parent's library is loaded through SMI_LIB, as tools/shared_lookup_time.py's session did.  Every measurement runs in a fresh
child process per library (this file with --child), each under `timeout`; the libraries alternate, and the first step that
fails ends the run.
(a) equality: smi_dev_air_prove_perm, _lookup, _args and _xargs at log_n = 8, t = 8, grind_bits = 8 on both primes: proof,
    roots, top_indices and closes byte for byte.
(b) time at n = 2^22, W = 6, B = 8, t = 32, grind_bits = 16 on the second prime: the plain list [permutation m = 2, lookup m = 2]
    through smi_dev_air_prove_args, the same list through smi_dev_air_prove_xargs, a single permutation, a single lookup; nine
    timed calls after three warm-ups per library and prover; wall time and every stage as median (min .. max); and the
    smi_ctx_profile medians of the plain list's block launch and compose launch (the parent's args_block_kernel and
    air_args_compose_kernel, this build's xargs_block_kernel and air_xargs_compose_kernel).  Accepted when this build's
    median is at most the parent's median plus the parent's own min-max spread.
(c) the 4-byte path of the plain column build (the columns' base one word off 16 bytes) at n = 2^22: a recorded cost, no gate.
(d) bench.py --steps 20 --warmup 5, three runs a library, alternating."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--log-n", type=int, default=22)
ap.add_argument("--skip-bench", action="store_true")
ap.add_argument("--child", choices=["equal", "time", "fallback"], default=None)
ap.add_argument("--json", default=None, help="(child) where the figures go")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
med = statistics.median


def mmm(v):
    return f"median {med(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f})"


# ---------------------------------------------------------------------------------------------- the children
def airs(s, np, n, p, seed):
    """-> (cols, {prover: Air}): columns 2, 3 hold the rows of columns 0, 1 in another order, column 4 is all ones"""
    from stark_rs_amd.mirror import Air
    rng = np.random.default_rng(seed)
    tab = np.stack([rng.permutation(n).astype(np.int64), rng.integers(0, p, n, dtype=np.int64)])
    order = rng.permutation(n)
    cols = np.stack([tab[0], tab[1], tab[0][order], tab[1][order], np.ones(n, dtype=np.int64), rng.integers(0, p, n, dtype=np.int64)])
    W = len(cols)
    made = {"args": Air(W).add_permutation([2, 3], [0, 1]).add_lookup([2, 3], [0, 1], 4),
            "xargs": Air(W).add_permutation([2, 3], [0, 1]).add_lookup([2, 3], [0, 1], 4),
            "perm": Air(W).permutation([2, 3], [0, 1]),
            "lookup": Air(W).lookup([2, 3], [0, 1], 4)}
    made["xargs"].xargs_always = True
    for a in made.values():
        a.boundary(0, 0, int(cols[0][0]))
    return cols, made


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import stark_rs_amd as s
    dev = torch.device("cuda:0")
    kw = dict(row_leaves=True, ext=True, timed=True, check=False)
    out = {}
    if args.child == "equal":
        log_n, lb, t, bits = 8, 3, 8, 8
        for p, g in ((s.P_REF, s.G_REF), (s.P2, s.G2)):
            eng = s.Engine(p, g, 0)
            cols, made = airs(s, np, 1 << log_n, p, 3)
            trace = torch.from_numpy(cols.astype(np.int32).reshape(-1)).to(dev)
            for name, air in made.items():
                r = eng.dev_air_prove(air, trace.data_ptr(), len(cols), log_n, lb, t, grind_bits=bits, **kw)
                out[f"{name} p={p}"] = dict(proof=bytes(r["proof"]).hex(), roots=r["column_roots"].tobytes().hex(),
                                            top_indices=[int(x) for x in r["top_indices"]], closes=r["closes"])
            eng.close()
    else:
        p, g = s.P2, s.G2
        eng = s.Engine(p, g, 0)
        log_n, lb, t, bits = args.log_n, 3, 32, 16
        n, N = 1 << log_n, 1 << (log_n + lb)
        cols, made = airs(s, np, n, p, 1)
        W = len(cols)
        trace = torch.from_numpy(cols.astype(np.int32).reshape(-1)).to(dev)
        tp = trace.data_ptr()
        ch = [int(x) for x in np.random.default_rng(2).integers(1 << 62, (1 << 64) - 1, 8, dtype=np.uint64)]

        def profiled(fn, stem):
            """-> (the label whose name holds `stem`, its total_ms over the timed calls)"""
            for _ in range(3):
                fn()
            eng.sync()
            eng.profile(True)
            eng.profile_read()
            ms, label = [], None
            for _ in range(args.reps):
                fn()
                got = eng.profile_read()
                (label,) = [k for k in got if stem in k]
                ms.append(got[label]["total_ms"])
            eng.profile(False)
            return label, ms

        if args.child == "fallback":
            c = torch.empty(8 * n + 4, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            assert c.data_ptr() % 16 == 0
            label, ms = profiled(lambda: eng.dev_args_columns(made["args"], tp, W, log_n, ch, c.data_ptr() + 4), "args_block_kernel")
            out = dict(label=label, ms=ms)
        else:
            for i in range(3 + args.reps):
                for name, air in made.items():
                    eng.sync()
                    t0 = time.perf_counter()
                    r = eng.dev_air_prove(air, tp, W, log_n, lb, t, grind_bits=bits, **kw)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert r["closes"] in (True, [True, True])
                    if i >= 3:
                        rec = out.setdefault("prove " + name, dict(wall=[], stages={k: [] for k in r["stage_ms"]}))
                        rec["wall"].append(dt)
                        for k, v in r["stage_ms"].items():
                            rec["stages"][k].append(v)
            c = torch.empty(8 * n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            label, ms = profiled(lambda: eng.dev_args_columns(made["args"], tp, W, log_n, ch, c.data_ptr()), "args_block_kernel")
            out["block launch"] = dict(label=label, ms=ms)
            lde = torch.empty(W * N, dtype=torch.int32, device=dev)
            cl = torch.empty(8 * N, dtype=torch.int32, device=dev)
            cw = torch.empty(4 * N, dtype=torch.int32, device=dev)
            eng.dev_lde(tp, W, log_n, lb, lde.data_ptr())
            eng.dev_lde(c.data_ptr(), 8, log_n, lb, cl.data_ptr())
            wts = torch.from_numpy(np.random.default_rng(3).integers(1 << 62, (1 << 64) - 1, 4 * (W + 1 + 4), dtype=np.uint64).view(np.int64)).to(dev)
            torch.cuda.synchronize()
            label, ms = profiled(lambda: eng.dev_air_compose_args(made["args"], lde.data_ptr(), cl.data_ptr(), W, log_n, lb, ch, wts.data_ptr(), cw.data_ptr()),
                                 "args_compose_kernel")
            out["compose launch"] = dict(label=label, ms=ms)
        eng.close()
    with open(args.json, "w") as f:
        json.dump(out, f)


# ---------------------------------------------------------------------------------------------- the driver
LINES = []
TMP = tempfile.mkdtemp(prefix="two_tree_ab_")   # where the children leave their figures


def say(text):
    print(text, flush=True)
    LINES.append(text)


def finish(code):
    dst = args.out or os.path.join(ROOT, "profiles", "two_tree_prover_ab.log")
    with open(dst, "w") as f:
        f.write("\n".join(LINES) + "\n")
    sys.exit(code)


def step(cmd, lib, limit):
    """one GPU step in a process of its own under `timeout`; a failure ends the run"""
    env = dict(os.environ)
    env.pop("SMI_LIB", None)
    if lib:
        env["SMI_LIB"] = lib
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        say(f"FAILED (exit {r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        finish(1)
    return r.stdout


def run_child(what, lib, tag, limit=300):
    path = os.path.join(TMP, f"two_tree_ab_{what}_{tag}.json")
    step([sys.executable, os.path.abspath(__file__), "--root", ROOT, "--child", what, "--json", path, "--reps", str(args.reps), "--log-n", str(args.log_n)], lib, limit)
    with open(path) as f:
        return json.load(f)


def gate(what, new, old):
    """-> accepted?  this build's median against the parent's median plus the parent's own min-max spread"""
    spread, d = max(old) - min(old), med(new) - med(old)
    ok = d <= spread
    say(f"  {what}: this build - parent = {d:+.4f} ms; the parent's own min-max spread is {spread:.4f} ms -> "
        + ("accepted" if ok else "SLOWER than the parent by more than its spread"))
    return ok


def driver():
    parent = os.path.abspath(args.parent_lib)
    both = (("parent", parent), ("this build", None))
    ok = True
    say("(a) equality: the four provers at log_n = 8, t = 8, grind_bits = 8, both primes")
    eq = {tag: run_child("equal", lib, tag.split()[0]) for tag, lib in both}
    for key in eq["parent"]:
        same = [f for f in ("proof", "roots", "top_indices", "closes") if eq["parent"][key][f] == eq["this build"][key][f]]
        say(f"  {key:28s}: proof {len(eq['parent'][key]['proof']) // 2} bytes; equal: {', '.join(same)}" + ("" if len(same) == 4 else "  <- DIFFERS"))
        ok = ok and len(same) == 4
    say(f"(b) time: n = 2^{args.log_n}, W = 6, B = 8, t = 32, grind_bits = 16, the second prime; {args.reps} timed calls after 3 warm-ups")
    tm = {tag: run_child("time", lib, tag.split()[0]) for tag, lib in both}
    for key in tm["parent"]:
        for tag, _lib in both:
            rec = tm[tag][key]
            if "wall" in rec:
                say(f"  {tag:10s} {key:14s} wall {mmm(rec['wall'])}")
                say("             stages " + "; ".join(f"{k} {med(v):.3f} ({min(v):.3f} .. {max(v):.3f})" for k, v in rec["stages"].items()))
            else:
                say(f"  {tag:10s} {key:14s} {rec['label']:26s} {mmm(rec['ms'])}")
        ok = gate(key, tm["this build"][key].get("wall") or tm["this build"][key]["ms"], tm["parent"][key].get("wall") or tm["parent"][key]["ms"]) and ok
    say(f"(c) the 4-byte path of the plain column build, the columns' base one word off 16 bytes, n = 2^{args.log_n} (a recorded cost, no gate)")
    fb = {tag: run_child("fallback", lib, tag.split()[0]) for tag, lib in both}
    for tag, _lib in both:
        say(f"  {tag:10s} {fb[tag]['label']:26s} {mmm(fb[tag]['ms'])}")
    a, b = fb["parent"]["ms"], fb["this build"]["ms"]
    say(f"  this build / parent = {med(b) / med(a):.4f}; the difference of the medians is {med(b) - med(a):+.4f} ms, the parent's own min-max spread {max(a) - min(a):.4f} ms")
    if not args.skip_bench:
        say("(d) bench.py --gpus 1 --steps 20 --warmup 5, three runs a library, alternating")
        vals = {tag: [] for tag, _lib in both}
        for _ in range(3):
            for tag, lib in both:
                res = json.loads(step([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], lib, 300).strip().splitlines()[-1])
                key = "value" if "value" in res else next(k for k, v in res.items() if isinstance(v, (int, float)))
                vals[tag].append(res[key])
                say(f"  {tag:10s} {key} = {res[key]}" + (f" {res['unit']}" if "unit" in res else ""))
        lo = {tag: (min(v), max(v)) for tag, v in vals.items()}
        over = lo["parent"][0] <= lo["this build"][1] and lo["this build"][0] <= lo["parent"][1]
        say(f"  ranges: parent {lo['parent'][0]} .. {lo['parent'][1]}, this build {lo['this build'][0]} .. {lo['this build'][1]} -> " + ("they overlap" if over else "they do NOT overlap"))
    say("result: " + ("accepted" if ok else "NOT accepted"))
    finish(0 if ok else 1)


if args.child:
    child()
elif args.parent_lib:
    driver()
else:
    ap.error("--parent-lib or --child")
