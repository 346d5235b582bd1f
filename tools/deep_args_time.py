#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's subsection on out-of-domain sampling with an argument list.

    python3 tools/deep_args_time.py           # deep_args beside the list prover of the same build

Every line is printed and, at the end, written to --out (default profiles/deep_args_time.log under --root).

At n = 2^20, t = 32, grind_bits = 16 on the second prime, for README.md's nine-column list (a permutation of two columns and two
lookups into one table column), the multiplicities filled once beforehand.
prove  : smi_dev_air_prove_deep_xargs at B = 8 with its eight stages beside smi_dev_air_prove_xargs at B = 8 on one trace, and
         smi_dev_air_prove_deep_xargs at B = 4, where the list prover cannot run: median wall time and median stage_ms of REPS
         calls each, interleaved, after three warm-up calls; the proof lengths; every proof verified once.
kernel : deep_compose_args_kernel at (W, A, D) = (9, 3, 2) beside its twin deep_compose_kernel at (W + 4 A, D) = (21, 2) -- the
         same bytes and the same multiply count -- on random columns at N = 2^23: BATCHES medians of REPS launches each
         (HIP events, smi_ctx_profile), interleaved, each against an in-run device-to-device copy of as many bytes; the spread
         is the twin's own largest minus smallest batch median."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--batches", type=int, default=5)
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
log_n, W, t, bits = args.log_n, 9, 32, 16
n = 1 << log_n

vm = Air(9).add_permutation([0, 1], [2, 3]).add_lookup([4], [5], 6).add_lookup([7], [5], 8)
vm.xargs_always = True   # the superset form: smi_dev_air_prove_xargs, the prover deep_args is set beside
order = rng.permutation(n)
c0, c1 = rng.integers(0, p, n), rng.integers(0, p, n)
table = rng.permutation(4 * n)[:n]
cols = np.stack([c0, c1, c0[order], c1[order], table[rng.integers(0, n, n)], table, np.zeros(n, dtype=np.int64),
                 table[rng.integers(0, max(1, n // 4), n)], np.zeros(n, dtype=np.int64)]).astype(np.int64)
trace = torch.from_numpy(cols.astype(np.int32)).to(dev)
torch.cuda.synchronize()
for a in (1, 2):
    eng.dev_args_multiplicities(vm, a, trace.data_ptr(), W, log_n, trace.data_ptr() + 4 * ((6 if a == 1 else 8) << log_n))
d, D = eng.air_plan_deep_args(vm, W, log_n, 3)
_d, E = eng.air_plan(vm, W, log_n, 3)
print(f"n=2^{log_n} W={W} A=3 t={t} bits={bits}: degree {d}, D={D} segments; the list prover runs FRI at E={E} (B=8), deep_args at E=B")


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


common = dict(row_leaves=True, ext=True, grind_bits=bits, timed=True, check=False)
MODES = {"deep_args B=8": (3, dict(common, deep_args=True)), "xargs B=8": (3, dict(common)), "deep_args B=4": (2, dict(common, deep_args=True))}
wall = {m: [] for m in MODES}
stages = {m: [] for m in MODES}
last = {}
for i in range(3 + args.reps):
    for m, (lb, kw) in MODES.items():
        eng.sync()
        t0 = time.perf_counter()
        res = eng.dev_air_prove(vm, trace.data_ptr(), W, log_n, lb, t, **kw)
        dt = (time.perf_counter() - t0) * 1e3
        last[m] = res
        if i >= 3:
            wall[m].append(dt)
            stages[m].append(res["stage_ms"])
for m, (lb, kw) in MODES.items():
    st = {key: statistics.median(v[key] for v in stages[m]) for key in stages[m][0]}
    print(f"prove {m:14s}: median {statistics.median(wall[m]):.2f} ms (min {min(wall[m]):.2f}, max {max(wall[m]):.2f}); proof {len(last[m]['proof'])} bytes; "
          f"closes {last[m]['closes']}; stages " + ", ".join(f"{key} {v:.3f}" for key, v in st.items()))
for m, (lb, kw) in MODES.items():
    ok, why = eng.air_verify(vm, last[m]["proof"], last[m]["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=bits,
                             deep_args=kw.get("deep_args", False))
    print(f"verify {m}: {ok} {why!r}")
try:
    eng.air_plan(vm, W, log_n, 2)
    print("the list prover plans B=4: unexpected")
except s.StarkMiError as e:
    print(f"the list prover at B=4: refused ({e})")
print(f"layout lengths: B=8 {eng.air_plan_deep_args(vm, W, log_n, 3, num_colinearity_tests=t)[2]}, B=4 {eng.air_plan_deep_args(vm, W, log_n, 2, num_colinearity_tests=t)[2]}")

# ---- the kernel beside its twin
A, lb = 3, 3
N = 1 << (log_n + lb)
Wt = W + 4 * A
big = torch.from_numpy(rng.integers(0, p, (Wt + 4 * D) * N, dtype=np.int32)).to(dev)   # trace | aux coordinates | segments
out = torch.empty(4 * N, dtype=torch.int32, device=dev)
base = big.data_ptr()
z = [int(v) for v in rng.integers(1, p, 4)]
cnt = 4 * (2 * W + 2 * A + D)
ood_a, ch_a = [int(v) for v in rng.integers(0, p, cnt)], [int(v) for v in rng.integers(1 << 62, (1 << 63), cnt)]
cnt_t = 4 * (2 * Wt + D)
ood_t, ch_t = [int(v) for v in rng.integers(0, p, cnt_t)], [int(v) for v in rng.integers(1 << 62, (1 << 63), cnt_t)]
torch.cuda.synchronize()


def run_args():
    eng.dev_deep_compose_args(base, base + 4 * W * N, base + 4 * Wt * N, W, A, D, log_n, lb, z, ood_a, ch_a, out.data_ptr())


def run_twin():
    eng.dev_deep_compose(base, base + 4 * Wt * N, Wt, D, log_n, lb, z, ood_t, ch_t, out.data_ptr())


KERNELS = {"deep_compose_args_kernel": run_args, "deep_compose_kernel": run_twin}
for fn in KERNELS.values():
    for _ in range(3):
        fn()
eng.sync()
eng.profile(True)
eng.profile_read()
med = {k: [] for k in KERNELS}
for b in range(args.batches):
    for k, fn in KERNELS.items():
        ms = []
        for _ in range(args.reps):
            fn()
            rd = eng.profile_read()
            ms.append(rd[k]["total_ms"])
        med[k].append(statistics.median(ms))
eng.profile(False)
per_point = 4 * (W + 4 * A + 4 * D) + 16
cp = copy_ms(per_point * N)
print(f"kernel yardstick at N=2^{log_n + lb}: {per_point} bytes a point, {per_point * N} bytes; copy of as many bytes {cp:.4f} ms")
for k in KERNELS:
    shape = f"(W, A, D) = ({W}, {A}, {D})" if k.endswith("args_kernel") else f"(W, D) = ({Wt}, {D})"
    print(f"  {k:26s} {shape}: batch medians {', '.join(f'{v:.4f}' for v in med[k])} ms; median {statistics.median(med[k]):.4f} ms; "
          f"ratio to the copy {statistics.median(med[k]) / cp:.3f}; {per_point * N / statistics.median(med[k]) / 1e6:.1f} GB/s")
twin = med["deep_compose_kernel"]
spread = (max(twin) - min(twin)) / cp
excess = (statistics.median(med["deep_compose_args_kernel"]) - statistics.median(twin)) / cp
print(f"  the twin's run-to-run spread of batch medians: {spread:.3f} of a copy; deep_compose_args_kernel's ratio exceeds the twin's by {excess:+.3f}: "
      + ("within the spread" if excess <= spread else "MORE than the spread"))
eng.close()
dst = args.out or os.path.join(os.path.abspath(args.root), "profiles", "deep_args_time.log")
with open(dst, "w") as fh:
    fh.write("\n".join(LINES) + "\n")
