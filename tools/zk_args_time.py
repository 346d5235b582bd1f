#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's subsection on zero-knowledge DEEP proofs with an argument list.

    python3 tools/zk_args_time.py

Every line is printed and, at the end, written to --out (default profiles/zk_args_time.log under --root).

The 9-column `vm` list of README.md (one permutation of two columns, two lookups into one table column) at n = 2^20, B = 8,
t = 32, grind_bits = 16, the second prime.  The zero-knowledge list prove (deep_args=True, coset_leaves=True, zk=seed) and the
plain coset-leaf list prove (smi_dev_air_prove_deep_xargs_fold4) alternate in one process: three warm-up calls each, then
--reps calls each; per call the sum of stage_ms (HIP events on the prover's stream) and the wall time; medians with min ..
max, the median of every stage, the proof bytes against the layouts, every last proof verified once, and the two ratios.
The zk trace's arguments hold over the n_a = n - k_t active rows (its multiplicities are counted there by
smi_dev_xargs_multiplicities_rows), the plain trace's over all n rows.

    SMI_LIB=<the parent commit's libstarkmi.so> python3 tools/zk_args_time.py --plain-only --label parent --append

times the plain list prove alone on another build of the library (one without the zero-knowledge list variant) and appends
its two lines to the log: run it before and after the full run, in one session, to show that the plain prove did not move."""
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
ap.add_argument("--plain-only", action="store_true", help="the plain coset-leaf list prove alone (for a build loaded through SMI_LIB)")
ap.add_argument("--label", default="this build")
ap.add_argument("--append", action="store_true", help="append to --out instead of writing it")
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
log_n, lb, t, W, bits = args.log_n, 3, 32, 9, 16
n = 1 << log_n
kt = 8 * t + 16
na = n - kt
med = statistics.median
SEED = bytes(range(32))


def vm_trace(rows):
    """the list holds over the first `rows` rows; the rows behind hold values that are in no table"""
    rng = np.random.default_rng(7)
    cols = np.zeros((W, n), dtype=np.int64)
    cols[:, rows:] = p - 1 - rng.integers(0, 7, (W, n - rows))
    c0, c1 = rng.integers(0, p, rows), rng.integers(0, p, rows)
    order = rng.permutation(rows)
    table = rng.permutation(4 * n)[:rows]
    cols[0, :rows], cols[1, :rows], cols[2, :rows], cols[3, :rows] = c0, c1, c0[order], c1[order]
    cols[4, :rows], cols[5, :rows] = table[rng.integers(0, rows, rows)], table
    cols[7, :rows] = table[rng.integers(0, max(1, rows // 4), rows)]
    return torch.from_numpy(cols.astype(np.int32)).to(dev)


vm = Air(W)
vm.add_permutation([0, 1], [2, 3])
vm.add_lookup([4], [5], 6)
vm.add_lookup([7], [5], 8)
ztrace, mtrace = vm_trace(na), vm_trace(n)
torch.cuda.synchronize()
for a, mc in ((1, 6), (2, 8)):                                # the multiplicity columns, counted on the device
    if not args.plain_only:
        eng.dev_xargs_multiplicities_rows(vm, a, ztrace.data_ptr(), W, log_n, na, ztrace.data_ptr() + 4 * mc * n)
    eng.dev_args_multiplicities(vm, a, mtrace.data_ptr(), W, log_n, mtrace.data_ptr() + 4 * mc * n)
common = dict(row_leaves=True, ext=True, grind_bits=bits, timed=True, check=False, deep_args=True, coset_leaves=True)
modes = {"zero-knowledge list": dict(common, zk=SEED), "deep list fold4": common}
if args.plain_only:
    del modes["zero-knowledge list"]
ev, wall, stages, last = ({m: [] for m in modes} for _ in range(4))
for i in range(3 + args.reps):
    for m, kw in modes.items():
        eng.sync()
        t0 = time.perf_counter()
        res = eng.dev_air_prove(vm, (ztrace if "zk" in kw else mtrace).data_ptr(), W, log_n, lb, t, **kw)
        dt = (time.perf_counter() - t0) * 1e3
        last[m] = res
        if i >= 3:
            wall[m].append(dt)
            ev[m].append(sum(res["stage_ms"].values()))
            stages[m].append(res["stage_ms"])
_d0, D0 = eng.air_plan_deep_args(vm, W, log_n, lb)
want = {"deep list fold4": eng.air_deep_args_fold4_layout(vm, W, log_n, lb, t)[1]}
if args.plain_only:
    print(f"{args.label}: the plain list prove alone, n=2^{log_n} W={W} A=3 B={1 << lb} t={t} bits={bits}; D = {D0}; modulus {p}")
else:
    dz, Dz, _kt, ks = eng.air_plan_deep_zk_args(vm, W, log_n, lb, t)
    Dzk = 1
    while Dzk < dz - 1:
        Dzk <<= 1
    want["zero-knowledge list"] = eng.air_deep_zk_args_layout(vm, W, log_n, lb, t)[1]
    print(f"{args.label}: vm list: n=2^{log_n} W={W} A=3 B={1 << lb} t={t} bits={bits}; k_t = {kt}, k_s = {ks}; zk plan d = {dz}, D = {Dzk} -> D' = {Dz} "
          f"(the plain list plan: D = {D0}); modulus {p}")
for m in modes:
    st = {name: statistics.median(v[name] for v in stages[m]) for name in stages[m][0]}
    nbytes = len(last[m]["proof"])
    ok, why = eng.air_verify(vm, last[m]["proof"], last[m]["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=bits, deep_args=True,
                             coset_leaves=True, zk=(m == "zero-knowledge list"))
    print(f"  {m:19s}: stages' sum {med(ev[m]):.3f} ms ({min(ev[m]):.3f} .. {max(ev[m]):.3f}); wall {med(wall[m]):.3f} ms ({min(wall[m]):.3f} .. {max(wall[m]):.3f}); "
          f"proof {nbytes} bytes ({'=' if nbytes == want[m] else '!='} layout {want[m]}); closes {last[m]['closes']}; verified {ok} {why!r}")
    print("    stages " + ", ".join(f"{name} {v:.3f}" for name, v in st.items()))
if args.plain_only:
    eng.close()
    dst = args.out or os.path.join(os.path.abspath(args.root), "profiles", "zk_args_time.log")
    with open(dst, "a" if args.append else "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    sys.exit(0)
za, zb = med(ev["zero-knowledge list"]), med(ev["deep list fold4"])
print(f"  zero-knowledge list / deep list fold4: stages' sum {za / zb:.3f}, wall {med(wall['zero-knowledge list']) / med(wall['deep list fold4']):.3f}, "
      f"bytes {len(last['zero-knowledge list']['proof']) / len(last['deep list fold4']['proof']):.3f}")
print(f"  columns of N words hashed into the three trees: {W + 1} + {4 * 3 + 1} + {4 * Dz + 5} against {W} + {4 * 3} + {4 * D0}")
eng.close()
dst = args.out or os.path.join(os.path.abspath(args.root), "profiles", "zk_args_time.log")
with open(dst, "a" if args.append else "w") as fh:
    fh.write("\n".join(LINES) + "\n")
