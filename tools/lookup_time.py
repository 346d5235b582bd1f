#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's lookup-argument subsection.

    python3 tools/lookup_time.py [--out profiles/lookup_time.log]

At n = 2^22, W = 5, m = 2, B = 8 on the second prime; HIP-event medians of REPS launches after three warm-up launches.
helper : the two launches of smi_dev_lookup_multiplicities (lookup_insert_kernel, lookup_count_kernel; smi_ctx_profile)
         against an in-run device-to-device copy of the bytes they must move at the least: the 2m tuple columns read, the
         8 n bytes of the table written and read back, 4 n of multiplicities written.  The accesses are random: the copy is
         a floor, not a target.
column : the three launches of smi_dev_lookup_column (lookup_block_kernel, lookup_scan_kernel, lookup_propagate_kernel)
         and their sum against a copy of 4 (2m + 1) n bytes read and 16 n written.
compose: air_lookup_compose_kernel against a copy of its bytes: 2m + 1 columns, s twice, the codeword read and written.
prove  : smi_dev_air_prove_lookup with its six stages beside smi_dev_air_prove_perm on the same shape (a lookup column that is
         a shuffled copy of the table, every multiplicity one: both statements hold), grind_bits = 16, t = 32: median wall
         time of REPS calls each, interleaved."""
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
log_n, lb, W, t, bits, m = args.log_n, 3, 5, 32, 16, 2
n, N = 1 << log_n, 1 << (log_n + lb)
lines = []


def say(text):
    print(text)
    lines.append(text)


def copy_ms(nbytes):
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
    return statistics.median(out)


def kernel_medians(fn, names):
    for _ in range(3):
        fn()
    eng.sync()
    eng.profile(True)
    eng.profile_read()
    out = {k: [] for k in names}
    for _ in range(args.reps):
        fn()
        got = eng.profile_read()
        for k in names:
            out[k].append(got[k]["total_ms"])
    eng.profile(False)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def report(title, names, med, floor_bytes, unit, count):
    total = sum(med[k][0] for k in names)
    cp = copy_ms(floor_bytes)
    say(title)
    for k in names:
        say(f"  {k:26s} median {med[k][0]:.4f} ms  (min {med[k][1]:.4f}, max {med[k][2]:.4f})")
    say(f"  sum {total:.4f} ms; copy of {floor_bytes} bytes {cp:.4f} ms; ratio {total / cp:.2f}; "
        f"{floor_bytes / total / 1e6:.1f} GB/s of the floor bytes; {count / total / 1e6:.2f} G {unit}/s")


# the table: a shuffled range beside a random member; the lookups: a shuffled copy of it (every multiplicity one)
tab = np.stack([rng.permutation(n).astype(np.int64), rng.integers(0, p, n, dtype=np.int64)])
order = rng.permutation(n)
cols = np.stack([tab[0][order], tab[1][order], tab[0], tab[1], np.zeros(n, dtype=np.int64)])
trace = torch.from_numpy(cols.astype(np.int32).reshape(-1)).to(dev)
air = Air(W).lookup([0, 1], [2, 3], 4)
air.boundary(0, 0, int(cols[0][0]))
twin = Air(W).permutation([0, 1], [2, 3])
twin.boundary(0, 0, int(cols[0][0]))
ch = [int(x) for x in rng.integers(1 << 62, (1 << 64) - 1, 8, dtype=np.uint64)]
d_mult = trace.data_ptr() + 4 * 4 * n
torch.cuda.synchronize()

# ---- the helper, into the trace's own multiplicity column
names = ("lookup_insert_kernel", "lookup_count_kernel")
med = kernel_medians(lambda: eng.dev_lookup_multiplicities(air, trace.data_ptr(), W, log_n, d_mult), names)
assert bool((trace[4 * n:] == 1).all())
report(f"helper n=2^{log_n} m={m} (a shuffled copy: no two lanes share a counter)", names, med, (4 * 2 * m + 16 + 4) * n, "rows", n)
# the contention case: every lookup is table row 0
hot = trace.clone()
hot[:n] = int(tab[0][0])
hot[n:2 * n] = int(tab[1][0])
torch.cuda.synchronize()
med = kernel_medians(lambda: eng.dev_lookup_multiplicities(air, hot.data_ptr(), W, log_n, hot.data_ptr() + 4 * 4 * n), names)
assert int(hot[4 * n]) == n
report(f"helper n=2^{log_n} m={m} (all lookups hit one row: one counter takes every atomic add)", names, med, (4 * 2 * m + 16 + 4) * n, "rows", n)
del hot

# ---- the column
sc = torch.empty(4 * n, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
names = ("lookup_block_kernel", "lookup_scan_kernel", "lookup_propagate_kernel")
closes = eng.dev_lookup_column(air, trace.data_ptr(), W, log_n, ch, sc.data_ptr())
med = kernel_medians(lambda: eng.dev_lookup_column(air, trace.data_ptr(), W, log_n, ch, sc.data_ptr()), names)
report(f"column n=2^{log_n} m={m} closes={closes}", names, med, (4 * (2 * m + 1) + 16) * n, "rows", n)

# ---- the auxiliary quotients
lde = torch.empty(W * N, dtype=torch.int32, device=dev)
sl = torch.empty(4 * N, dtype=torch.int32, device=dev)
cw = torch.empty(4 * N, dtype=torch.int32, device=dev)
eng.dev_lde(trace.data_ptr(), W, log_n, lb, lde.data_ptr())
eng.dev_lde(sc.data_ptr(), 4, log_n, lb, sl.data_ptr())
wts = torch.from_numpy(rng.integers(1 << 62, (1 << 64) - 1, 4 * (W + 2), dtype=np.uint64).view(np.int64)).to(dev)
torch.cuda.synchronize()
names = ("air_lookup_compose_kernel", "air_compose_ext_kernel")
med = kernel_medians(lambda: eng.dev_air_compose_lookup(air, lde.data_ptr(), sl.data_ptr(), W, log_n, lb, ch, wts.data_ptr(), cw.data_ptr()), names)
report(f"compose N=2^{log_n + lb}", names[:1], med, (4 * (2 * m + 1) + 32 + 32) * N, "points", N)
say(f"  air_compose_ext_kernel (the launch before it, same call) median {med['air_compose_ext_kernel'][0]:.4f} ms")
del lde, sl, cw, sc
torch.cuda.empty_cache()

# ---- the prove, interleaved with the permutation prove on the same trace
kw = dict(row_leaves=True, ext=True, grind_bits=bits, timed=True, check=False)
wall = {"lookup": [], "perm": []}
stages = {"lookup": [], "perm": []}
for i in range(3 + args.reps):
    for name, a in (("lookup", air), ("perm", twin)):
        eng.sync()
        t0 = time.perf_counter()
        res = eng.dev_air_prove(a, trace.data_ptr(), W, log_n, lb, t, **kw)
        dt = (time.perf_counter() - t0) * 1e3
        assert res["closes"]
        if i >= 3:
            wall[name].append(dt)
            stages[name].append(res["stage_ms"])
for name in ("lookup", "perm"):
    st = {k: statistics.median(x[k] for x in stages[name]) for k in stages[name][0]}
    say(f"prove {name:8s} n=2^{log_n} W={W} t={t} bits={bits}: median {statistics.median(wall[name]):.2f} ms "
        f"(min {min(wall[name]):.2f}, max {max(wall[name]):.2f}); stages " + ", ".join(f"{k} {v:.3f}" for k, v in st.items()))
eng.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
