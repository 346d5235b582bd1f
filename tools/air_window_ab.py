#!/usr/bin/env python3
"""Development tool (GPU box): the measurements of the transition-window change (include/stark_mi.h, "AIR: transition
windows"), by the method of tools/two_tree_ab.py -- fresh child processes (this file with --child), each under `timeout`, the
two libraries alternating, the first step that fails ends the run.

    python3 tools/air_window_ab.py --parent-lib <the parent commit's libstarkmi.so> [--out profiles/air_window_time.log]

(a) no regression for two-row AIRs: four mimc lanes (tests/air_periodic.py lanes) at n = 2^20, B = 8, t = 32, 16 grinding bits
    through smi_dev_air_prove_deep_fold4; nine timed calls after three warm-ups per library; wall time and every stage as
    median (min .. max), and the smi_ctx_profile medians of air_compose_ext_kernel, deep_eval_kernel and deep_compose_kernel.
    Accepted when this build's median is at most the parent's median plus the parent's own min-max spread.
(b) bench.py --steps 20 --warmup 5, three runs a library, alternating; the ranges must overlap.
(c) what the window buys (this build only): `sq` in one column with S = 3 against its two-column two-row form, `tap4` against
    its three-column form (tests/window_compose.py), n = 2^20, B = 8, t = 32, coset leaves: wall, stages, proof bytes.  No
    threshold."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ap_ = argparse.ArgumentParser()
ap_.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap_.add_argument("--parent-lib", default=None)
ap_.add_argument("--out", default=None)
ap_.add_argument("--reps", type=int, default=9)
ap_.add_argument("--log-n", type=int, default=20)
ap_.add_argument("--skip-bench", action="store_true")
ap_.add_argument("--child", choices=["ab", "buys"], default=None)
ap_.add_argument("--json", default=None, help="(child) where the figures go")
args = ap_.parse_args()
ROOT = os.path.abspath(args.root)
med = statistics.median
# label -> the kernel names it sums (smi_ctx_profile): the codeword launch is deep_compose_kernel or, under a window, its twin
KERNELS = {"air_compose_ext_kernel": ("air_compose_ext_kernel",), "deep_eval_kernel": ("deep_eval_kernel",),
           "deep_compose_kernel": ("deep_compose_kernel", "deep_compose_window_kernel")}


def mmm(v):
    return f"median {med(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f})"


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import stark_rs_amd as s
    dev = torch.device("cuda:0")
    p, g = s.P2, s.G2
    eng = s.Engine(p, g, 0)
    log_n, lb, t, bits = args.log_n, 3, 32, 16
    n = 1 << log_n
    kw = dict(row_leaves=True, ext=True, deep=True, coset_leaves=True, timed=True, check=False, grind_bits=bits)
    out = {}

    def timed(air, cols, label):
        trace = torch.from_numpy(np.asarray(cols, dtype=np.int64).astype(np.int32).reshape(-1)).to(dev)
        W = len(cols)
        rec = out.setdefault(label, dict(wall=[], stages={}, kernels={k: [] for k in KERNELS}, proof_bytes=0, W=W))
        for i in range(3 + args.reps):
            if i == 3:
                eng.sync()
                eng.profile(True)
                eng.profile_read()
            eng.sync()
            t0 = time.perf_counter()
            r = eng.dev_air_prove(air, trace.data_ptr(), W, log_n, lb, t, **kw)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= 3:
                got = eng.profile_read()
                rec["wall"].append(dt)
                for k, v in r["stage_ms"].items():
                    rec["stages"].setdefault(k, []).append(v)
                for k in KERNELS:
                    rec["kernels"][k].append(sum(v["total_ms"] for name, v in got.items() if name in KERNELS[k]))
        eng.profile(False)
        rec["proof_bytes"] = len(r["proof"])
        ok, why = eng.air_verify(air, r["proof"], r["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True, deep=True, coset_leaves=True,
                                 grind_bits=bits)
        assert ok, why

    if args.child == "ab":
        import air_periodic as ap
        air = ap.lanes([64, 64, 64, 64], p)
        ks = [[v % p for v in per] for per in air.periodics]
        cols = []
        for c in range(4):
            x = [c + 2]
            for r in range(n - 1):
                x.append(pow(x[-1] + ks[c][r % 64], 3, p))
            cols.append(x)
        x = [2]   # lane 0 also reads the next row of lane 1's constants: its trace follows its own rule
        for r in range(n - 1):
            x.append((pow(x[-1] + ks[0][r % 64], 3, p) - 7 * ks[1][(r + 1) % 64] * x[-1]) % p)
        cols[0] = x
        timed(air, cols, "mimc x 4")
    else:
        import window_compose as wc
        for name in ("sq", "tap4"):
            air, cols = wc.make(name, n, p)
            timed(air, cols, f"{name}: one column, S = {air.window}")
            air2, cols2 = wc.two_row_form(name, n, p)
            timed(air2, cols2, f"{name}: {len(cols2)} columns, S = 2")
    eng.close()
    json.dump(out, open(args.json, "w"))


def run_child(kind, lib, limit):
    env = dict(os.environ)
    if lib:
        env["SMI_LIB"] = lib
    else:
        env.pop("SMI_LIB", None)
    with tempfile.NamedTemporaryFile(suffix=".json") as f:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--root", ROOT, "--child", kind, "--json", f.name,
               "--reps", str(args.reps), "--log-n", str(args.log_n)]
        r = subprocess.run(cmd, env=env)
        if r.returncode:
            sys.exit(f"child {kind} ({lib or 'this build'}) ended with status {r.returncode}")
        return json.load(open(f.name))


def bench(lib):
    env = dict(os.environ)
    if lib:
        env["SMI_LIB"] = lib
    else:
        env.pop("SMI_LIB", None)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                       env=env, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"bench.py ended with status {r.returncode}: {r.stderr[-400:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def main():
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say(f"transition windows: this build against the parent commit's library ({args.parent_lib}); n = 2^{args.log_n}, B = 8, t = 32, 16 grinding bits,")
    say(f"coset leaves (smi_dev_air_prove_deep_fold4); {args.reps} timed calls after 3 warm-ups, fresh process per library.")
    say()
    say("(a) two-row AIR, four mimc lanes")
    res = {}
    for who, lib in (("parent", args.parent_lib), ("this build", None)):
        res[who] = run_child("ab", lib, 300)["mimc x 4"]
    for who in ("parent", "this build"):
        r = res[who]
        say(f"  {who:10s} wall   {mmm(r['wall'])}   proof {r['proof_bytes']} bytes")
        for k, v in r["stages"].items():
            say(f"  {who:10s}   stage {k:9s} {mmm(v)}")
        for k, v in r["kernels"].items():
            say(f"  {who:10s}   {k:24s} {mmm(v)}")
    pw, nw = res["parent"]["wall"], res["this build"]["wall"]
    ok = med(nw) <= med(pw) + (max(pw) - min(pw))
    say(f"  rule: this build's median {med(nw):.4f} <= parent's median {med(pw):.4f} + its spread {max(pw) - min(pw):.4f}: {'holds' if ok else 'FAILS'}")
    for k in KERNELS:
        pk, nk = res["parent"]["kernels"][k], res["this build"]["kernels"][k]
        ok_k = med(nk) <= med(pk) + (max(pk) - min(pk))
        say(f"  rule, {k}: {med(nk):.4f} <= {med(pk):.4f} + {max(pk) - min(pk):.4f}: {'holds' if ok_k else 'FAILS'}")
    if not args.skip_bench:
        say()
        say("(b) bench.py --gpus 1 --steps 20 --warmup 5, alternating")
        vals = {"parent": [], "this build": []}
        for _ in range(3):
            for who, lib in (("parent", args.parent_lib), ("this build", None)):
                b = bench(lib)
                key = "value" if "value" in b else sorted(k for k, v in b.items() if isinstance(v, (int, float)))[0]
                vals[who].append(b[key])
                say(f"  {who:10s} {key} = {b[key]}  {b.get('unit', '')}")
        lo = max(min(vals["parent"]), min(vals["this build"]))
        hi = min(max(vals["parent"]), max(vals["this build"]))
        say(f"  ranges: parent {min(vals['parent'])} .. {max(vals['parent'])}, this build {min(vals['this build'])} .. {max(vals['this build'])}: "
            f"{'overlap' if lo <= hi else 'DO NOT OVERLAP'}")
    say()
    say("(c) what the window buys (this build)")
    buys = run_child("buys", None, 600)
    for label, r in buys.items():
        say(f"  {label:28s} wall {mmm(r['wall'])}   proof {r['proof_bytes']} bytes")
        say("      stages " + "  ".join(f"{k} {med(v):.3f}" for k, v in r["stages"].items()))
        say("      kernels " + "  ".join(f"{k} {med(v):.4f}" for k, v in r["kernels"].items()))
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    child() if args.child else main()
