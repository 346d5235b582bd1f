#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's subsection "Argument list with selectors and periodic members".

    python3 tools/xargs_time.py [--out profiles/xargs_time.log]

At n = 2^22, W = 9, B = 8 on the second prime.  HIP-event kernel times through smi_ctx_profile: medians of REPS launches after
three warm-up launches, with min and max; nothing is pinned; the paths that are compared alternate in one process.
(a) the plain list [permutation m = 2, lookup m = 2] through its own entry points and the same list handed over as an operand
    list (mirror.Air.xargs_always): both run xargs_block_kernel and air_xargs_compose_kernel, and the outputs are compared
    first.  The plain list once had kernels of its own; they went when it was routed here, and the comparison of the two
    pairs of kernels, against the parent commit's library, is on record in profiles/two_tree_prover_ab.log
    (tools/two_tree_ab.py).
(b) the list [permutation m = 2 with a selector on either side, lookup m = 1 into a periodic table of 256 entries with a
    selector] through the same kernels, the compose launch beside a device-to-device copy of the bytes it moves."""
import argparse
import os
import statistics
import sys

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
log_n, lb, W = args.log_n, 3, 9
n, N = 1 << log_n, 1 << (log_n + lb)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def mmm(v):
    return f"median {statistics.median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f})"


def alternate(runs):
    """runs: {label: (fn, kernel names)} -> {label: {kernel: [ms per rep]}}; the labels alternate rep by rep"""
    for fn, _names in runs.values():
        for _ in range(3):
            fn()
    eng.sync()
    eng.profile(True)
    eng.profile_read()
    out = {label: {k: [] for k in names} for label, (_fn, names) in runs.items()}
    for _ in range(args.reps):
        for label, (fn, names) in runs.items():
            fn()
            got = eng.profile_read()
            for k in names:
                out[label][k].append(got[k]["total_ms"])
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


table = rng.permutation(256).astype(np.int64)
tab = np.stack([rng.permutation(n).astype(np.int64), rng.integers(0, p, n, dtype=np.int64)])
order = rng.permutation(n)
bits = rng.integers(0, 2, n, dtype=np.int64)
right = np.zeros(n, dtype=np.int64)
right[order] = bits   # the right side selects the rows of the table that the selected left rows hold
cols = np.stack([tab[0], tab[1], tab[0][order], tab[1][order], np.ones(n, dtype=np.int64), bits, right, table[rng.integers(0, 256, n)],
                 rng.integers(0, p, n, dtype=np.int64)])
trace = torch.from_numpy(cols.astype(np.int32).reshape(-1)).to(dev)
tp = trace.data_ptr()
plain = Air(W).add_permutation([2, 3], [0, 1]).add_lookup([2, 3], [0, 1], 4)
new = Air(W).add_permutation([2, 3], [0, 1]).add_lookup([2, 3], [0, 1], 4)
new.xargs_always = True
sel = Air(W)
j = sel.periodic([int(v) for v in table])
sel.add_permutation([2, 3], [0, 1], left_sel=5, right_sel=6).add_lookup([7], [("per", j)], 4, sel=5)
ch = [int(x) for x in rng.integers(1 << 62, (1 << 64) - 1, 8, dtype=np.uint64)]

# ---- the columns
c_plain = torch.empty(8 * n, dtype=torch.int32, device=dev)
c_new = torch.empty(8 * n, dtype=torch.int32, device=dev)
c_sel = torch.empty(8 * n, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
assert eng.dev_args_columns(plain, tp, W, log_n, ch, c_plain.data_ptr()) == [True, True]
assert eng.dev_args_columns(new, tp, W, log_n, ch, c_new.data_ptr()) == [True, True]
eng.dev_args_columns(sel, tp, W, log_n, ch, c_sel.data_ptr())
eng.sync()
assert torch.equal(c_plain, c_new)
res = alternate({"plain": (lambda: eng.dev_args_columns(plain, tp, W, log_n, ch, c_plain.data_ptr()), ("xargs_block_kernel",)),
                 "operand": (lambda: eng.dev_args_columns(new, tp, W, log_n, ch, c_new.data_ptr()), ("xargs_block_kernel",)),
                 "selected": (lambda: eng.dev_args_columns(sel, tp, W, log_n, ch, c_sel.data_ptr()), ("xargs_block_kernel",))})
show(f"(a), (b) column build, block launch, n=2^{log_n}", res)

# ---- the auxiliary quotients
lde = torch.empty(W * N, dtype=torch.int32, device=dev)
cl = torch.empty(8 * N, dtype=torch.int32, device=dev)
cls = torch.empty(8 * N, dtype=torch.int32, device=dev)
cw = [torch.empty(4 * N, dtype=torch.int32, device=dev) for _ in range(3)]
eng.dev_lde(tp, W, log_n, lb, lde.data_ptr())
eng.dev_lde(c_plain.data_ptr(), 8, log_n, lb, cl.data_ptr())
eng.dev_lde(c_sel.data_ptr(), 8, log_n, lb, cls.data_ptr())
wts = torch.from_numpy(rng.integers(1 << 62, (1 << 64) - 1, 4 * (W + 4), dtype=np.uint64).view(np.int64)).to(dev)
torch.cuda.synchronize()
run = lambda air, c, out: eng.dev_air_compose_args(air, lde.data_ptr(), c.data_ptr(), W, log_n, lb, ch, wts.data_ptr(), out.data_ptr())
run(plain, cl, cw[0])
run(new, cl, cw[1])
eng.sync()
assert torch.equal(cw[0], cw[1])
res = alternate({"plain": (lambda: run(plain, cl, cw[0]), ("air_xargs_compose_kernel",)),
                 "operand": (lambda: run(new, cl, cw[1]), ("air_xargs_compose_kernel",)),
                 "selected": (lambda: run(sel, cls, cw[2]), ("air_xargs_compose_kernel",))})
show(f"(a), (b) compose launch, N=2^{log_n + lb}", res)
# (b) reads per point: the permutation's 4 members and 2 selectors, the lookup's 1 trace member, its multiplicity and its
# selector (the periodic table stays in cache): 9 column words; two auxiliary columns twice; the codeword read and written
nbytes = (4 * 9 + 32 * 2 + 32) * N
say(f"  copy of the selected list's {nbytes} bytes: {mmm(copy_times(nbytes))}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
