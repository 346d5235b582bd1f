#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's permutation-argument subsection.

    python3 tools/perm_time.py                # column build, auxiliary quotients, prove

At n = 2^22, W = 4, m = 2, B = 8 on the second prime; HIP-event medians of REPS launches after three warm-up launches.
column : the three launches of smi_dev_perm_column (perm_block_kernel, perm_scan_kernel, perm_propagate_kernel; smi_ctx_profile)
         and their sum, against an in-run device-to-device copy of the bytes the build must move: 4 * 2m * n read and 16 n
         written.
compose: air_perm_compose_kernel against a copy of its bytes: 2m columns, z twice, the codeword read and written.
prove  : smi_dev_air_prove_perm with its six stages beside smi_dev_air_prove_ext_pow for the same AIR without the
         permutation, on one trace, grind_bits = 16, t = 32: median wall time of REPS calls each, interleaved."""
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
args = ap.parse_args()
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
KERNELS = ("perm_block_kernel", "perm_scan_kernel", "perm_propagate_kernel")


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


src = rng.integers(0, p, (2, n), dtype=np.int64)
order = rng.permutation(n)
cols = np.stack([src[0], src[1], src[0][order], src[1][order]])
trace = torch.from_numpy(cols.astype(np.int32)).to(dev)
air = Air(W).permutation([0, 1], [2, 3])
air.boundary(0, 0, int(cols[0][0]))
plain = Air(W)
plain.boundary(0, 0, int(cols[0][0]))
ch = [int(x) for x in rng.integers(1 << 62, (1 << 64) - 1, 8, dtype=np.uint64)]
m = 2

# ---- the column
z = torch.empty(4 * n, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
closes = eng.dev_perm_column(air, trace.data_ptr(), W, log_n, ch, z.data_ptr())
med = kernel_medians(lambda: eng.dev_perm_column(air, trace.data_ptr(), W, log_n, ch, z.data_ptr()), KERNELS)
total = sum(med[k][0] for k in KERNELS)
floor_bytes = (4 * 2 * m + 16) * n
cp = copy_ms(floor_bytes)
print(f"column n=2^{log_n} m={m} closes={closes}")
for k in KERNELS:
    print(f"  {k:24s} median {med[k][0]:.4f} ms  (min {med[k][1]:.4f}, max {med[k][2]:.4f})")
print(f"  sum of the three launches {total:.4f} ms; copy of {floor_bytes} bytes {cp:.4f} ms; ratio {total / cp:.2f}; "
      f"{floor_bytes / total / 1e6:.1f} GB/s of the floor bytes; {n / total / 1e6:.2f} G rows/s")

# ---- the auxiliary quotients
lde = torch.empty(W * N, dtype=torch.int32, device=dev)
zl = torch.empty(4 * N, dtype=torch.int32, device=dev)
cw = torch.empty(4 * N, dtype=torch.int32, device=dev)
eng.dev_lde(trace.data_ptr(), W, log_n, lb, lde.data_ptr())
eng.dev_lde(z.data_ptr(), 4, log_n, lb, zl.data_ptr())
wts = torch.from_numpy(rng.integers(1 << 62, (1 << 64) - 1, 4 * (W + 2), dtype=np.uint64).view(np.int64)).to(dev)
torch.cuda.synchronize()
names = ("air_perm_compose_kernel", "air_compose_ext_kernel")
med = kernel_medians(lambda: eng.dev_air_compose_perm(air, lde.data_ptr(), zl.data_ptr(), W, log_n, lb, ch, wts.data_ptr(), cw.data_ptr()), names)
aux_bytes = (4 * 2 * m + 32 + 32) * N
cp = copy_ms(aux_bytes)
k = "air_perm_compose_kernel"
print(f"compose N=2^{log_n + lb}")
print(f"  {k} median {med[k][0]:.4f} ms (min {med[k][1]:.4f}, max {med[k][2]:.4f}); copy of {aux_bytes} bytes {cp:.4f} ms; ratio {med[k][0] / cp:.2f}; "
      f"{aux_bytes / med[k][0] / 1e6:.1f} GB/s; {N / med[k][0] / 1e6:.2f} G points/s")
print(f"  air_compose_ext_kernel (the launch before it, same call) median {med['air_compose_ext_kernel'][0]:.4f} ms")
del lde, zl, cw, z
torch.cuda.empty_cache()

# ---- the prove, interleaved with the extension prove of the same AIR without the permutation
kw = dict(row_leaves=True, ext=True, grind_bits=bits, timed=True, check=False)
wall = {"perm": [], "ext_pow": []}
stages = {"perm": [], "ext_pow": []}
for i in range(3 + args.reps):
    for name, a in (("perm", air), ("ext_pow", plain)):
        eng.sync()
        t0 = time.perf_counter()
        res = eng.dev_air_prove(a, trace.data_ptr(), W, log_n, lb, t, **kw)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= 3:
            wall[name].append(dt)
            stages[name].append(res["stage_ms"])
for name in ("perm", "ext_pow"):
    st = {k: statistics.median(x[k] for x in stages[name]) for k in stages[name][0]}
    print(f"prove {name:8s} n=2^{log_n} W={W} t={t} bits={bits}: median {statistics.median(wall[name]):.2f} ms "
          f"(min {min(wall[name]):.2f}, max {max(wall[name]):.2f}); stages " + ", ".join(f"{k} {v:.3f}" for k, v in st.items()))
eng.close()
