#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's subsection on next-row operands in argument lists.

    python3 tools/next_row_time.py

Every line is printed and, at the end, written to --out (default profiles/next_row_members_time.log under --root).

The 9-column `vm` list of README.md (one permutation of two columns, two lookups into one table column) at n = 2^20, B = 8,
t = 32, grind_bits = 16, the second prime, coset leaves (deep_args=True, coset_leaves=True), extended by ONE lookup whose
tuple has one next-row member: (c9[r], c9[r + 1]) is a row of the public table (per 0, per 1) on every row but the last.

  next-row   W = 11: c9 the column, c10 the multiplicities; the lookup reads [c9, next c9].
  copy col   W = 12: the same statement the only way a list could say it before -- c11 holds the rotated copy
             c11[r] = c9[r + 1], bound by the transition constraint next(c9) - c11 = 0 on every row but the last (a periodic
             selector); the lookup reads [c9, c11].  This runs unchanged on the parent commit: it is the baseline.

The two proves alternate in one process: three warm-up calls each, then --reps calls each; per call the sum of stage_ms (HIP
events on the prover's stream); medians with min .. max, the median of every stage, the proof bytes against the layouts, every
last proof verified once.  Then the kernels: smi_dev_xargs_columns and smi_dev_air_compose_xargs on the next-row list and on
the same list with the flag removed (the instantiations every other list launches), bracketed by the context's profile
events, --reps launches each after three warm-ups, alternating."""
import argparse
import os
import statistics
import sys

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
from stark_rs_amd.mirror import Air  # noqa: E402

p, g = s.P2, s.G2
eng = s.Engine(p, g, 0)
dev = torch.device("cuda:0")
log_n, lb, t, bits = args.log_n, 3, 32, 16
n, N = 1 << log_n, 1 << (args.log_n + 3)
med = statistics.median
rng = np.random.default_rng(7)
STEP = 64   # the public table: (v, succ(v)) for a cycle of 64 values


def base_cols(W):
    cols = np.zeros((W, n), dtype=np.int64)
    c0, c1 = rng.integers(0, p, n), rng.integers(0, p, n)
    order = rng.permutation(n)
    table = rng.permutation(4 * n)[:n]
    cols[0], cols[1], cols[2], cols[3] = c0, c1, c0[order], c1[order]
    cols[4], cols[5] = table[rng.integers(0, n, n)], table
    cols[7] = table[rng.integers(0, n // 4, n)]
    return cols


def vm(W):
    air = Air(W)
    air.add_permutation([0, 1], [2, 3])
    air.add_lookup([4], [5], 6)
    air.add_lookup([7], [5], 8)
    return air


cycle = [int(v) for v in np.random.default_rng(11).permutation(1 << 20)[:STEP]]
walk = np.array([cycle[r % STEP] for r in range(n)], dtype=np.int64)   # c9[r + 1] is the successor of c9[r]; row n - 1 is deselected
live = [1] * (n - 1) + [0]

nx = vm(11)
tv, ts = nx.periodic(cycle), nx.periodic(cycle[1:] + cycle[:1])
lv = nx.periodic(live)
nx.add_lookup([9, ("next", 9)], [("per", tv), ("per", ts)], 10, sel=("per", lv))
plain = vm(11)                                                           # the same list with the flag removed: the plain instantiations
for per in (cycle, cycle[1:] + cycle[:1], live):
    plain.periodic(per)
plain.add_lookup([9, 9], [("per", 0), ("per", 1)], 10, sel=("per", 2))

cp = vm(12)
tv, ts = cp.periodic(cycle), cp.periodic(cycle[1:] + cycle[:1])
lv = cp.periodic(live)
cp.transition({(("per", lv), ("next", 9)): 1, (("per", lv), ("cur", 11)): -1})   # live (c9' - c11) = 0
cp.add_lookup([9, 11], [("per", tv), ("per", ts)], 10, sel=("per", lv))

rng = np.random.default_rng(7)
a_cols = base_cols(11)
a_cols[9] = walk
rng = np.random.default_rng(7)
b_cols = base_cols(12)
b_cols[9], b_cols[11] = walk, np.roll(walk, -1)
traces = {"next-row": torch.from_numpy(a_cols.astype(np.int32)).to(dev), "copy col": torch.from_numpy(b_cols.astype(np.int32)).to(dev)}
airs, widths = {"next-row": nx, "copy col": cp}, {"next-row": 11, "copy col": 12}
torch.cuda.synchronize()
for m in airs:
    for a, mc in ((1, 6), (2, 8), (3, 10)):                               # the multiplicity columns, counted on the device
        eng.dev_args_multiplicities(airs[m], a, traces[m].data_ptr(), widths[m], log_n, traces[m].data_ptr() + 4 * mc * n)
kw = dict(row_leaves=True, ext=True, grind_bits=bits, timed=True, check=False, deep_args=True, coset_leaves=True)
ev, stages, last = ({m: [] for m in airs} for _ in range(3))
for i in range(3 + args.reps):
    for m in airs:
        eng.sync()
        res = eng.dev_air_prove(airs[m], traces[m].data_ptr(), widths[m], log_n, lb, t, **kw)
        last[m] = res
        if i >= 3:
            ev[m].append(sum(res["stage_ms"].values()))
            stages[m].append(res["stage_ms"])
print(f"n=2^{log_n} B={1 << lb} t={t} bits={bits}, coset leaves, deep_args; A=4; modulus {p}; {args.reps} timed calls each after 3 warm-ups, alternating")
for m in airs:
    W = widths[m]
    st = {name: med(v[name] for v in stages[m]) for name in stages[m][0]}
    nbytes, want = len(last[m]["proof"]), eng.air_deep_args_fold4_layout(airs[m], W, log_n, lb, t)[1]
    ok, why = eng.air_verify(airs[m], last[m]["proof"], last[m]["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=bits, deep_args=True,
                             coset_leaves=True)
    print(f"  {m:9s} W={W} K={len(airs[m].constraints)}: stages' sum {med(ev[m]):.3f} ms ({min(ev[m]):.3f} .. {max(ev[m]):.3f}); proof {nbytes} bytes "
          f"({'=' if nbytes == want else '!='} layout {want}); closes {last[m]['closes']}; verified {ok} {why!r}")
    print("    stages " + ", ".join(f"{name} {v:.3f}" for name, v in st.items()))
za, zb = med(ev["next-row"]), med(ev["copy col"])
print(f"  next-row / copy col: stages' sum {za / zb:.3f}, bytes {len(last['next-row']['proof']) / len(last['copy col']['proof']):.3f}")

# ---- the kernels: the NEXT instantiation against the plain one on the same list with the flag removed
ch = [int(x) for x in np.random.default_rng(3).integers(1, 1 << 62, 8)]
A, W = 4, 11
d_c = torch.zeros(4 * A * n, dtype=torch.int32, device=dev)
lde = torch.randint(0, p, (W, N), dtype=torch.int32, device=dev)         # the compose launches work point by point
cl = torch.randint(0, p, (4 * A, N), dtype=torch.int32, device=dev)
out = torch.zeros(4 * N, dtype=torch.int32, device=dev)
wch = torch.from_numpy(np.random.default_rng(5).integers(1 << 62, (1 << 63) - 1, 4 * (W + 2 * A), dtype=np.int64)).to(dev)
torch.cuda.synchronize()
times = {}
eng.profile(True)
for i in range(3 + args.reps):
    for name, air in (("next-row", nx), ("flag removed", plain)):
        eng.profile_read()
        eng.dev_args_columns(air, traces["next-row"].data_ptr(), W, log_n, ch, d_c.data_ptr())
        eng.dev_air_compose_args(air, lde.data_ptr(), cl.data_ptr(), W, log_n, lb, ch, wch.data_ptr(), out.data_ptr())
        for k, v in eng.profile_read().items():
            if i >= 3 and ("xargs_block" in k or "xargs_compose" in k):
                times.setdefault((name, k), []).append(v["total_ms"] / v["launches"])
eng.profile(False)
print("  kernels on the next-row list and on the same list with the flag removed (profile events, ms per launch):")
for (name, k), v in sorted(times.items(), key=lambda kv: kv[0][1]):
    print(f"    {name:12s} {k:40s} median {med(v):.4f} ({min(v):.4f} .. {max(v):.4f})")
eng.close()
dst = args.out or os.path.join(os.path.abspath(args.root), "profiles", "next_row_members_time.log")
with open(dst, "w") as fh:
    fh.write("\n".join(LINES) + "\n")
