#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's subsection on zero-knowledge DEEP proofs.

    python3 tools/zk_time.py

Every line is printed and, at the end, written to --out (default profiles/zk_time.log under --root).

prove  : four MiMC lanes x' = (x + k)^3 (k of period 64) at n = 2^20, B = 8, t = 32, grind_bits = 16, the second prime -- the
         shape of profiles/deep_fold4_time.log with the closing boundary points on the last real row n - k_t - 1.  The
         zero-knowledge prove (zk=seed) and smi_dev_air_prove_deep_fold4 alternate in one process: three warm-up calls each,
         then --reps calls each; per call the sum of stage_ms (HIP events on the prover's stream) and the wall time; medians
         with min .. max, the median of every stage, the proof bytes against the layouts, every last proof verified once, the
         ratio, and the extended columns and tree columns each variant moves.
kernel : random_fill_kernel and zk_segments_kernel at the sizes of that prove (k_t = 264, k_s = 129): one salt column of
         N = 2^23 residues, the 4 n coefficients of the mask polynomial, the 4 k_t randomiser rows, and a split with D = 2
         (h_len = 2 n, D' = 3); their own bracketed times (smi_ctx_profile) beside an in-run device-to-device copy: of a buffer
         as large as the output (random_fill), of as many bytes as the kernel reads and writes (zk_segments)."""
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
    sys.stdout.flush()


sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import stark_rs_amd as s  # noqa: E402

p, g = s.P2, s.G2
eng = s.Engine(p, g, 0)
dev = torch.device("cuda:0")
log_n, lb, t, W = args.log_n, 3, 32, 4
n, N = 1 << log_n, 1 << (log_n + lb)
kt, ks = 8 * t + 8, 4 * t + 1
med = statistics.median
span = lambda v: f"{med(v):.4f} ms ({min(v):.4f} .. {max(v):.4f})"
stream = torch.cuda.Stream()
SEED = bytes(range(32))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for i in range(3 + args.reps):
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        if i >= 3:
            out.append(e0.elapsed_time(e1))
    return out


def bracketed(fn, name):
    for _ in range(3):
        fn()
    eng.profile(True)
    eng.profile_read()
    out = []
    for _ in range(args.reps):
        fn()
        out.append(eng.profile_read()[name]["total_ms"])
    eng.profile(False)
    return out


# ---- the prove beside the non-hiding prove of the same shape
from stark_rs_amd.mirror import Air  # noqa: E402
bits = 16
rng = np.random.default_rng(1)
kc = [int(v) for v in rng.integers(1, p, 64)]
mimc = Air(4)
k = mimc.periodic(kc)
x = np.array([3, 5, 7, 11], dtype=object)
rows = [x.copy()]
for r in range(n - 1):
    x = (x + kc[r % 64]) ** 3 % p
    rows.append(x)
mcols = np.array(rows, dtype=np.int64).T.copy()
for c in range(4):
    mimc.transition({("next", c): 1, ("cur", c, 3): -1, (("cur", c, 2), ("per", k)): -3, (("cur", c), ("per", k, 2)): -3, ("per", k, 3): -1})
    mimc.boundary(c, 0, int(mcols[c][0])).boundary(c, n - kt - 1, int(mcols[c][n - kt - 1]))
mtrace = torch.from_numpy(mcols.astype(np.int32)).to(dev)
ztrace = mtrace.clone()   # the zero-knowledge prove overwrites its last k_t rows
torch.cuda.synchronize()
common = dict(row_leaves=True, ext=True, grind_bits=bits, timed=True, check=False, deep=True, coset_leaves=True)
modes = {"zero-knowledge": dict(common, zk=SEED), "deep fold4": common}
ev, wall, stages, last = ({m: [] for m in modes} for _ in range(4))
for i in range(3 + args.reps):
    for m, kw in modes.items():
        eng.sync()
        t0 = time.perf_counter()
        res = eng.dev_air_prove(mimc, (ztrace if "zk" in kw else mtrace).data_ptr(), W, log_n, lb, t, **kw)
        dt = (time.perf_counter() - t0) * 1e3
        last[m] = res
        if i >= 3:
            wall[m].append(dt)
            ev[m].append(sum(res["stage_ms"].values()))
            stages[m].append(res["stage_ms"])
d_, Dz, _kt, _ks = eng.air_plan_deep_zk(mimc, W, log_n, lb, t)
_d0, D0 = eng.air_plan_deep(mimc, W, log_n, lb)
want = {"zero-knowledge": eng.air_deep_zk_layout(mimc, W, log_n, lb, t)[1], "deep fold4": eng.air_deep_fold4_layout(mimc, W, log_n, lb, t)[1]}
print(f"mimc x4: n=2^{log_n} W={W} B={1 << lb} t={t} bits={bits}; k_t = {kt}, k_s = {ks}; D = {D0} -> D' = {Dz}; modulus {p}")
for m in modes:
    st = {name: statistics.median(v[name] for v in stages[m]) for name in stages[m][0]}
    nbytes = len(last[m]["proof"])
    ok, why = eng.air_verify(mimc, last[m]["proof"], last[m]["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=bits, deep=True,
                             coset_leaves=True, zk=(m == "zero-knowledge"))
    print(f"  {m:15s}: stages' sum {med(ev[m]):.3f} ms ({min(ev[m]):.3f} .. {max(ev[m]):.3f}); wall {med(wall[m]):.3f} ms ({min(wall[m]):.3f} .. {max(wall[m]):.3f}); "
          f"proof {nbytes} bytes ({'=' if nbytes == want[m] else '!='} layout {want[m]}); verified {ok} {why!r}")
    print("    stages " + ", ".join(f"{name} {v:.3f}" for name, v in st.items()))
za, zb = med(ev["zero-knowledge"]), med(ev["deep fold4"])
ext_zk, ext_0 = W + 1 + 4 * Dz + 4, W + 4 * D0                       # columns extended to N (the derived AIR's periodic column among them)
tree_zk, tree_0 = W + 1 + 4 * Dz + 5, W + 4 * D0
print(f"  zero-knowledge / deep fold4: stages' sum {za / zb:.3f}, wall {med(wall['zero-knowledge']) / med(wall['deep fold4']):.3f}, "
      f"bytes {len(last['zero-knowledge']['proof']) / len(last['deep fold4']['proof']):.3f}")
print(f"  columns of N words extended: {ext_zk} against {ext_0}; hashed into the two trees: {tree_zk} against {tree_0}; read by the DEEP compose "
      f"launch: {W + 4 * Dz} against {W + 4 * D0}; at 4 bytes x N = {4 * N} bytes a column and pass")
del last

eng.set_stream(stream.cuda_stream)   # the library's launches and the events below share one stream
print(f"the kernels at n = 2^{log_n}, B = {1 << lb}, t = {t}: k_t = {kt}, k_s = {ks}; modulus {p}")
for what, count in (("a salt column, N residues", N), ("a mask polynomial, 4 n coefficients", 4 * n), ("the randomiser rows, W k_t residues", W * kt)):
    buf = torch.empty(count, dtype=torch.int32, device=dev)
    a_, b_ = torch.empty(max(count, 4), dtype=torch.int32, device=dev), torch.empty(max(count, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    k = bracketed(lambda: eng.dev_random_fill(SEED, 1, buf.data_ptr(), count), "random_fill_kernel")
    cp = timed(lambda: b_.copy_(a_))
    hashes = (count + 3) // 4
    print(f"random_fill_kernel, {what} ({count}): {span(k)}; a device copy of a buffer of its {4 * count} bytes {span(cp)}; "
          f"{9 * hashes / med(k) / 1e6:.1f} G mixes/s, {count / med(k) / 1e6:.2f} G residues/s")
    del buf, a_, b_

D, h_len = 2, 2 * n
Dp = -(-h_len // (n - ks))
hc = torch.randint(0, p, (4, N), dtype=torch.int32, device=dev)
rho = torch.randint(0, p, (4 * (Dp - 1) * ks,), dtype=torch.int32, device=dev)
moved = 4 * (4 * h_len + 4 * Dp * n)
a_, b_ = torch.empty(moved // 8, dtype=torch.int32, device=dev), torch.empty(moved // 8, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
for what, lead in (("16-byte accesses", 0), ("4-byte accesses (bases one word off)", 1)):
    hsrc = hc.data_ptr() + 4 * lead
    out = torch.empty(4 * Dp * n + 4, dtype=torch.int32, device=dev)
    d_out = out.data_ptr() + 4 * lead
    torch.cuda.synchronize()
    k = bracketed(lambda: eng.dev_zk_segments(hsrc, h_len, log_n, ks, Dp, rho.data_ptr(), d_out, h_stride=N - (4 if lead else 0)), "zk_segments_kernel")
    cp = timed(lambda: b_.copy_(a_))
    print(f"zk_segments_kernel, D = {D} -> D' = {Dp}, {what}: {span(k)}; a copy of the {moved} bytes it reads and writes {span(cp)}, "
          f"{med(k) / med(cp):.2f} copies")
eng.close()
dst = args.out or os.path.join(os.path.abspath(args.root), "profiles", "zk_time.log")
with open(dst, "w") as fh:
    fh.write("\n".join(LINES) + "\n")
