#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's argument-list subsection.

    python3 tools/args_time.py [--out profiles/args_time.log]

At n = 2^22, W = 6, B = 8 on the second prime, the list [permutation m = 2, lookup m = 2] over one trace: columns 2, 3 hold
the rows of columns 0, 1 in another order, so that both statements hold with every multiplicity one.  The plain list runs the
operand list's kernels (xargs_block_kernel, air_xargs_compose_kernel), so those are the labels read.  HIP-event medians of
REPS runs after three warm-up runs, with min and max; each new path and its yardstick alternate in one process.  The
yardsticks are the existing kernels, never the code under test.
columns: the three launches of smi_dev_args_columns against smi_dev_perm_column then smi_dev_lookup_column (six launches).
compose: the list's air_xargs_compose_kernel against air_perm_compose_kernel and air_lookup_compose_kernel back to back, and against a
         device-to-device copy of its own bytes: 9 trace columns, two auxiliary columns twice, the codeword read and written.
prove  : smi_dev_air_prove_args against smi_dev_air_prove_perm plus smi_dev_air_prove_lookup on the same trace, grind_bits =
         16, t = 32: wall time and the six stages."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--log-n", type=int, default=22)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import stark_rs_amd as s  # noqa: E402
from stark_rs_amd.mirror import Air  # noqa: E402

p, g = s.P2, s.G2
eng = s.Engine(p, g, 0)
dev = torch.device("cuda:0")
rng = np.random.default_rng(1)
log_n, lb, W, t, bits = args.log_n, 3, 6, 32, 16
n, N = 1 << log_n, 1 << (log_n + lb)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def mmm(v):
    return f"median {statistics.median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f})"


def alternate(runs):
    """runs: {label: (fn, kernel names)} -> {label: {kernel: [ms per rep], "sum": [...]}}; the labels alternate rep by rep"""
    for fn, _names in runs.values():
        for _ in range(3):
            fn()
    eng.sync()
    eng.profile(True)
    eng.profile_read()
    out = {label: {k: [] for k in names + ("sum",)} for label, (_fn, names) in runs.items()}
    for _ in range(args.reps):
        for label, (fn, names) in runs.items():
            fn()
            got = eng.profile_read()
            for k in names:
                out[label][k].append(got[k]["total_ms"])
            out[label]["sum"].append(sum(got[k]["total_ms"] for k in names))
    eng.profile(False)
    return out


def copy_times(nbytes):
    a = torch.empty(nbytes // 8, dtype=torch.int32, device=dev)   # nbytes / 2 read + nbytes / 2 written
    b = torch.empty_like(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for i in range(3 + args.reps):
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            out.append(e0.elapsed_time(e1))
    return out


def show(title, res):
    say(title)
    for label, per in res.items():
        for k, v in per.items():
            say(f"  {label:9s} {k:26s} {mmm(v)}")


tab = np.stack([rng.permutation(n).astype(np.int64), rng.integers(0, p, n, dtype=np.int64)])
order = rng.permutation(n)
cols = np.stack([tab[0], tab[1], tab[0][order], tab[1][order], np.ones(n, dtype=np.int64), rng.integers(0, p, n, dtype=np.int64)])
trace = torch.from_numpy(cols.astype(np.int32).reshape(-1)).to(dev)
both = Air(W).add_permutation([2, 3], [0, 1]).add_lookup([2, 3], [0, 1], 4)
perm = Air(W).permutation([2, 3], [0, 1])
look = Air(W).lookup([2, 3], [0, 1], 4)
for a in (both, perm, look):
    a.boundary(0, 0, int(cols[0][0]))
ch = [int(x) for x in rng.integers(1 << 62, (1 << 64) - 1, 8, dtype=np.uint64)]
tp = trace.data_ptr()

# ---- the columns: three launches against six
c2 = torch.empty(8 * n, dtype=torch.int32, device=dev)
z1 = torch.empty(4 * n, dtype=torch.int32, device=dev)
s1 = torch.empty(4 * n, dtype=torch.int32, device=dev)
torch.cuda.synchronize()


def pair_columns():
    eng.dev_perm_column(perm, tp, W, log_n, ch, z1.data_ptr())
    eng.dev_lookup_column(look, tp, W, log_n, ch, s1.data_ptr())


assert eng.dev_args_columns(both, tp, W, log_n, ch, c2.data_ptr()) == [True, True]
pair_columns()
eng.sync()
assert torch.equal(c2[:4 * n], z1) and torch.equal(c2[4 * n:], s1)
res = alternate({"args": (lambda: eng.dev_args_columns(both, tp, W, log_n, ch, c2.data_ptr()),
                          ("xargs_block_kernel", "args_scan_kernel", "args_propagate_kernel")),
                 "pair": (pair_columns, ("perm_block_kernel", "perm_scan_kernel", "perm_propagate_kernel", "lookup_block_kernel", "lookup_scan_kernel",
                                         "lookup_propagate_kernel"))})
show(f"columns n=2^{log_n} [perm m=2, lookup m=2]", res)
col_res = res

# ---- the auxiliary quotients: one launch against two, and a copy of its bytes
lde = torch.empty(W * N, dtype=torch.int32, device=dev)
cl = torch.empty(8 * N, dtype=torch.int32, device=dev)
cw = torch.empty(4 * N, dtype=torch.int32, device=dev)
cw2 = torch.empty(4 * N, dtype=torch.int32, device=dev)
eng.dev_lde(tp, W, log_n, lb, lde.data_ptr())
eng.dev_lde(c2.data_ptr(), 8, log_n, lb, cl.data_ptr())
wts = torch.from_numpy(rng.integers(1 << 62, (1 << 64) - 1, 4 * (W + 4), dtype=np.uint64).view(np.int64)).to(dev)
wts_l = torch.cat([wts[:4 * W], wts[4 * (W + 2):]])   # the lookup's own two weights behind the main ones
torch.cuda.synchronize()


def pair_compose():
    eng.dev_air_compose_perm(perm, lde.data_ptr(), cl.data_ptr(), W, log_n, lb, ch, wts.data_ptr(), cw2.data_ptr())
    eng.dev_air_compose_lookup(look, lde.data_ptr(), cl.data_ptr() + 4 * 4 * N, W, log_n, lb, ch, wts_l.data_ptr(), cw2.data_ptr())


res = alternate({"args": (lambda: eng.dev_air_compose_args(both, lde.data_ptr(), cl.data_ptr(), W, log_n, lb, ch, wts.data_ptr(), cw.data_ptr()),
                          ("air_xargs_compose_kernel",)),
                 "pair": (pair_compose, ("air_perm_compose_kernel", "air_lookup_compose_kernel"))})
show(f"compose N=2^{log_n + lb}", res)
nbytes = (4 * 9 + 32 * 2 + 32) * N
say(f"  copy of the fused launch's {nbytes} bytes: {mmm(copy_times(nbytes))}")
cmp_res = res
del lde, cl, cw, cw2, c2, z1, s1
torch.cuda.empty_cache()

# ---- the proves, alternating
kw = dict(row_leaves=True, ext=True, grind_bits=bits, timed=True, check=False)
wall = {"args": [], "perm": [], "lookup": []}
stages = {k: [] for k in wall}
for i in range(3 + args.reps):
    for name, a in (("args", both), ("perm", perm), ("lookup", look)):
        eng.sync()
        t0 = time.perf_counter()
        r = eng.dev_air_prove(a, tp, W, log_n, lb, t, **kw)
        dt = (time.perf_counter() - t0) * 1e3
        assert r["closes"] in (True, [True, True])
        if i >= 3:
            wall[name].append(dt)
            stages[name].append(r["stage_ms"])
for name in wall:
    st = {k: statistics.median(x[k] for x in stages[name]) for k in stages[name][0]}
    say(f"prove {name:7s} n=2^{log_n} W={W} t={t} bits={bits}: {mmm(wall[name])}; stages " + ", ".join(f"{k} {v:.3f}" for k, v in st.items()))
two = [a + b for a, b in zip(wall["perm"], wall["lookup"])]
say(f"prove perm + lookup, rep by rep: {mmm(two)}")


def verdict(what, new, old):
    spread = max(old) - min(old)
    d = statistics.median(new) - statistics.median(old)
    say(f"{what}: new - yardstick = {d:+.4f} ms; the yardstick's own min-max spread is {spread:.4f} ms -> "
        + ("SLOWER than the yardstick by more than its spread" if d > spread else "not slower than the yardstick beyond its spread"))


verdict("columns", col_res["args"]["sum"], col_res["pair"]["sum"])
verdict("compose", cmp_res["args"]["sum"], cmp_res["pair"]["sum"])
verdict("prove", wall["args"], two)
eng.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
