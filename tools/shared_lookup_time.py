#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's subsection on shared-table lookups.

    python3 tools/shared_lookup_time.py

Every line is printed and, at the end, written to --out (default profiles/shared_lookup_time.log under --root).

The 9-column `vm` list of README.md (one permutation of two columns, two lookups into one table column, each with a
multiplicity column of its own) against the same statement with the two lookups merged into ONE shared lookup of J = 2, which
needs 8 columns: n = 2^20, B = 8, t = 32, grind_bits = 16, the second prime.  Per prover -- the coset-leaf list prove
(smi_dev_air_prove_deep_xargs_fold4) and the zero-knowledge list prove (smi_dev_air_prove_deep_zk_xargs) -- the two lists
alternate in one process: three warm-up calls each, then --reps calls each; per call the sum of stage_ms (HIP events on the
prover's stream) and the wall time; medians with min .. max, the median of every stage, the proof bytes against the layouts,
D and D' of each list, every last proof verified once, and one line saying which list is faster.

    SMI_LIB=<the parent commit's libstarkmi.so> python3 tools/shared_lookup_time.py --unchanged-only --label parent --append

times the 9-column list alone on another build of the library (one without shared lookups) and appends its lines to the log:
run it before and after `--unchanged-only --label "this build"` in one session, so that the parent's own run-to-run spread is
on record beside this build's figure for a list that has no shared lookup."""
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
ap.add_argument("--unchanged-only", action="store_true", help="the 9-column list alone (also for a build loaded through SMI_LIB)")
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
log_n, lb, t, bits = args.log_n, 3, 32, 16
n = 1 << log_n
kt = 8 * t + 16
na = n - kt
med = statistics.median
SEED = bytes(range(32))


def cells(rows):
    """the statement's cells over the first `rows` rows (the rows behind hold values that are in no table): the permutation's
    four columns, the table, and the two looked-up columns"""
    rng = np.random.default_rng(7)
    tail = lambda: p - 1 - rng.integers(0, 7, n - rows)
    c0, c1 = rng.integers(0, p, rows), rng.integers(0, p, rows)
    order = rng.permutation(rows)
    table = rng.permutation(4 * n)[:rows]
    look_a, look_b = table[rng.integers(0, rows, rows)], table[rng.integers(0, max(1, rows // 4), rows)]
    return [np.concatenate([v, tail()]) for v in (c0, c1, c0[order], c1[order], look_a, table, look_b)]


def nine(rows):
    """README's list: columns 6 and 8 are the two multiplicity columns"""
    c = cells(rows)
    z = np.zeros(n, dtype=np.int64)
    air = Air(9).add_permutation([0, 1], [2, 3]).add_lookup([4], [5], 6).add_lookup([7], [5], 8)
    return air, torch.from_numpy(np.stack(c[:6] + [z, c[6], z]).astype(np.int32)).to(dev), [(1, 6), (2, 8)]


def shared(rows):
    """the same statement with ONE lookup argument of two tuples: column 7 is the multiplicity column of both"""
    c = cells(rows)
    air = Air(8).add_permutation([0, 1], [2, 3]).add_lookups([[4], [6]], [5], 7)
    return air, torch.from_numpy(np.stack(c + [np.zeros(n, dtype=np.int64)]).astype(np.int32)).to(dev), [(1, 7)]


lists = {"nine columns, two lookups": nine}
if not args.unchanged_only:
    lists["eight columns, one shared lookup"] = shared
common = dict(row_leaves=True, ext=True, grind_bits=bits, timed=True, check=False, deep_args=True, coset_leaves=True)
provers = {"deep_xargs_fold4": (common, n), "deep_zk_xargs": (dict(common, zk=SEED), na)}
print(f"{args.label}: n=2^{log_n} B={1 << lb} t={t} bits={bits}; k_t = {kt}; modulus {p}; {args.reps} timed calls a list after 3 warm-ups, the lists alternating")
for prover, (kw, rows) in provers.items():
    zk = "zk" in kw
    made = {}
    for name, make in lists.items():
        air, trace, mults = make(rows)
        torch.cuda.synchronize()
        for a, mc in mults:                                   # the multiplicity columns, counted on the device
            if zk:
                eng.dev_xargs_multiplicities_rows(air, a, trace.data_ptr(), air.n_cols, log_n, rows, trace.data_ptr() + 4 * mc * n)
            else:
                eng.dev_args_multiplicities(air, a, trace.data_ptr(), air.n_cols, log_n, trace.data_ptr() + 4 * mc * n)
        made[name] = (air, trace)
    ev, wall, stages, last = ({m: [] for m in lists} for _ in range(4))
    for i in range(3 + args.reps):
        for name, (air, trace) in made.items():
            eng.sync()
            t0 = time.perf_counter()
            res = eng.dev_air_prove(air, trace.data_ptr(), air.n_cols, log_n, lb, t, **kw)
            dt = (time.perf_counter() - t0) * 1e3
            last[name] = res
            if i >= 3:
                wall[name].append(dt)
                ev[name].append(sum(res["stage_ms"].values()))
                stages[name].append(res["stage_ms"])
    print(f"{prover}:")
    for name, (air, trace) in made.items():
        W, A = air.n_cols, len(air.args)
        if zk:
            d, Dp, _kt, _ks = eng.air_plan_deep_zk_args(air, W, log_n, lb, t)
            D = 1
            while D < d - 1:
                D <<= 1
            want, plan = eng.air_deep_zk_args_layout(air, W, log_n, lb, t)[1], f"d = {d}, D = {D}, D' = {Dp}"
            hashed = f"{W + 1} + {4 * A + 1} + {4 * Dp + 5}"
        else:
            d, D = eng.air_plan_deep_args(air, W, log_n, lb)
            want, plan = eng.air_deep_args_fold4_layout(air, W, log_n, lb, t)[1], f"d = {d}, D = {D}"
            hashed = f"{W} + {4 * A} + {4 * D}"
        st = {k: med(v[k] for v in stages[name]) for k in stages[name][0]}
        nbytes = len(last[name]["proof"])
        ok, why = eng.air_verify(air, last[name]["proof"], last[name]["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=bits,
                                 deep_args=True, coset_leaves=True, zk=zk)
        print(f"  {name:32s}: W = {W}, A = {A}, {plan}; columns of N words hashed into the three trees {hashed}")
        print(f"    stages' sum {med(ev[name]):.3f} ms ({min(ev[name]):.3f} .. {max(ev[name]):.3f}); wall {med(wall[name]):.3f} ms "
              f"({min(wall[name]):.3f} .. {max(wall[name]):.3f}); proof {nbytes} bytes ({'=' if nbytes == want else '!='} layout {want}); "
              f"closes {last[name]['closes']}; verified {ok} {why!r}")
        print("    stages " + ", ".join(f"{k} {v:.3f}" for k, v in st.items()))
    if len(made) == 2:
        a, b = list(made)
        ra, rb = med(ev[a]), med(ev[b])
        print(f"  {prover}: the list with {'one shared lookup' if rb < ra else 'two lookups'} is faster: stages' sum {rb:.3f} ms shared against {ra:.3f} ms "
              f"(x {rb / ra:.3f}), wall x {med(wall[b]) / med(wall[a]):.3f}, proof bytes x {len(last[b]['proof']) / len(last[a]['proof']):.3f}")
    del made
    torch.cuda.empty_cache()
eng.close()
dst = args.out or os.path.join(os.path.abspath(args.root), "profiles", "shared_lookup_time.log")
with open(dst, "a" if args.append else "w") as fh:
    fh.write("\n".join(LINES) + "\n")
