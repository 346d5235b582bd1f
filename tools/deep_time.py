#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's out-of-domain sampling subsection.

    python3 tools/deep_time.py                # prove with out-of-domain sampling beside smi_dev_air_prove_ext_pow

Every line is printed and, at the end, written to --out (default profiles/deep_time.log under --root).

At n = 2^20, W = 4 (four MiMC lanes x' = (x + k)^3, k of period 64), B = 8, t = 32 on the second prime, grind_bits = 16.
prove  : smi_dev_air_prove_deep with its seven stages beside smi_dev_air_prove_ext_pow for the same AIR on one trace: median
         wall time and median stage_ms of REPS calls each, interleaved, after three warm-up calls; the two proof lengths; both
         proofs verified once.
kernels: HIP-event medians (smi_ctx_profile) of deep_compose_kernel, deep_eval_kernel and deep_eval_combine_kernel inside
         those proves; deep_compose_kernel against an in-run device-to-device copy of its 4 (W + 4 D) + 16 bytes a point."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
LINES = []


def print(*a):   # noqa: A001  every line goes to the log as well
    LINES.append(" ".join(str(x) for x in a))
    sys.stdout.write(LINES[-1] + "\n")


sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import stark_rs_amd as s  # noqa: E402
from stark_rs_amd.mirror import Air  # noqa: E402

p, g = s.P2, s.G2
eng = s.Engine(p, g, 0)
dev = torch.device("cuda:0")
rng = np.random.default_rng(1)
log_n, lb, W, t, bits = args.log_n, 3, 4, 32, 16
n, N = 1 << log_n, 1 << (log_n + lb)

ks = [int(v) for v in rng.integers(1, p, 64)]
air = Air(W)
k = air.periodic(ks)
x = np.array([3, 5, 7, 11], dtype=object)
rows = [x.copy()]
for r in range(n - 1):
    x = (x + ks[r % 64]) ** 3 % p
    rows.append(x)
cols = np.array(rows, dtype=np.int64).T.copy()
for c in range(W):
    air.transition({("next", c): 1, ("cur", c, 3): -1, (("cur", c, 2), ("per", k)): -3, (("cur", c), ("per", k, 2)): -3, ("per", k, 3): -1})
    air.boundary(c, 0, int(cols[c][0])).boundary(c, n - 1, int(cols[c][n - 1]))
trace = torch.from_numpy(cols.astype(np.int32)).to(dev)
torch.cuda.synchronize()
d, D = eng.air_plan_deep(air, W, log_n, lb)
_d, E = eng.air_plan(air, W, log_n, lb)
print(f"n=2^{log_n} W={W} B={1 << lb} t={t} bits={bits}: degree {d}, D={D} segments; ext_pow runs FRI at E={E}, deep at E={1 << lb}")


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


MODES = {"deep": dict(row_leaves=True, ext=True, deep=True, grind_bits=bits, timed=True, check=False),
         "ext_pow": dict(row_leaves=True, ext=True, grind_bits=bits, timed=True, check=False)}
wall = {m: [] for m in MODES}
stages = {m: [] for m in MODES}
last = {}
for i in range(3 + args.reps):
    for m, kw in MODES.items():
        eng.sync()
        t0 = time.perf_counter()
        res = eng.dev_air_prove(air, trace.data_ptr(), W, log_n, lb, t, **kw)
        dt = (time.perf_counter() - t0) * 1e3
        last[m] = res
        if i >= 3:
            wall[m].append(dt)
            stages[m].append(res["stage_ms"])
for m in MODES:
    st = {key: statistics.median(v[key] for v in stages[m]) for key in stages[m][0]}
    print(f"prove {m:8s}: median {statistics.median(wall[m]):.2f} ms (min {min(wall[m]):.2f}, max {max(wall[m]):.2f}); proof {len(last[m]['proof'])} bytes; stages "
          + ", ".join(f"{key} {v:.3f}" for key, v in st.items()))
ok, why = eng.air_verify(air, last["deep"]["proof"], last["deep"]["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True, deep=True, grind_bits=bits)
ok2, why2 = eng.air_verify(air, last["ext_pow"]["proof"], last["ext_pow"]["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=bits)
print(f"verify: deep {ok} {why!r}; ext_pow {ok2} {why2!r}; layout length {eng.air_plan_deep(air, W, log_n, lb, num_colinearity_tests=t)[2]}")

# ---- the kernels of the deep prove
names = ("deep_compose_kernel", "deep_eval_kernel", "deep_eval_combine_kernel")
eng.sync()
eng.profile(True)
eng.profile_read()
got = {key: [] for key in names}
for _ in range(args.reps):
    eng.dev_air_prove(air, trace.data_ptr(), W, log_n, lb, t, **MODES["deep"])
    rd = eng.profile_read()
    for key in names:
        got[key].append((rd[key]["total_ms"], rd[key]["launches"]))
eng.profile(False)
for key in names:
    ms = [v[0] for v in got[key]]
    print(f"  {key:26s} median {statistics.median(ms):.4f} ms over {got[key][0][1]} launches a prove (min {min(ms):.4f}, max {max(ms):.4f})")
per_point = 4 * (W + 4 * D) + 16
cp = copy_ms(per_point * N)
cm = statistics.median(v[0] for v in got["deep_compose_kernel"])
print(f"  deep_compose_kernel: {per_point} bytes a point, {per_point * N} bytes; copy of as many bytes {cp:.4f} ms; ratio {cm / cp:.2f}; "
      f"{per_point * N / cm / 1e6:.1f} GB/s; {N / cm / 1e6:.2f} G points/s")
eng.close()
out = args.out or os.path.join(os.path.abspath(args.root), "profiles", "deep_time.log")
with open(out, "w") as fh:
    fh.write("\n".join(LINES) + "\n")
