#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's subsection on out-of-domain sampling over coset leaves.

    python3 tools/deep_fold4_time.py          # the coset-leaf DEEP provers beside the folding-2 DEEP provers of the same build

Every line is printed and, at the end, written to --out (default profiles/deep_fold4_time.log under --root).

The shapes of profiles/deep_time.log and profiles/deep_args_time.log: the second prime, t = 32, grind_bits = 16;
  plain : four MiMC lanes x' = (x + k)^3 (k of period 64) at n = 2^20, B = 8;
  list  : README.md's nine-column list (a permutation of two columns and two lookups into one table column) at n = 2^20,
          at B = 8 and at B = 4, the multiplicities filled once beforehand.
prove  : per shape the new variant (coset_leaves=True) and the variant it stands beside, alternating in one process: three
         warm-up calls each, then REPS calls each; per call the sum of stage_ms (HIP events on the prover's stream) and the
         wall time; medians with min .. max, the median of every stage, the proof bytes against the layout functions, and every
         last proof verified once.
kernel : coset_leaf_hash_kernel beside row_hash_wide_kernel over the same buffers of 2^23 points a column, at W = 4 and
         W = 21 (W = 4 goes to the fused row path of the Merkle kernels, which has no kernel of its own to bracket: the row
         tree is then timed whole): the kernels' own bracketed times (smi_ctx_profile), the whole trees by HIP events, each
         against an in-run device-to-device copy of the coset kernel's floor bytes 4 V n + 32 q."""
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
from stark_rs_amd.mirror import Air  # noqa: E402

p, g = s.P2, s.G2
eng = s.Engine(p, g, 0)
dev = torch.device("cuda:0")
rng = np.random.default_rng(1)
log_n, t, bits = args.log_n, 32, 16
n = 1 << log_n
med = statistics.median
span = lambda v: f"{med(v):.3f} ms ({min(v):.3f} .. {max(v):.3f})"

# ---- the two statements
ks = [int(v) for v in rng.integers(1, p, 64)]
mimc = Air(4)
k = mimc.periodic(ks)
x = np.array([3, 5, 7, 11], dtype=object)
rows = [x.copy()]
for r in range(n - 1):
    x = (x + ks[r % 64]) ** 3 % p
    rows.append(x)
mcols = np.array(rows, dtype=np.int64).T.copy()
for c in range(4):
    mimc.transition({("next", c): 1, ("cur", c, 3): -1, (("cur", c, 2), ("per", k)): -3, (("cur", c), ("per", k, 2)): -3, ("per", k, 3): -1})
    mimc.boundary(c, 0, int(mcols[c][0])).boundary(c, n - 1, int(mcols[c][n - 1]))
mtrace = torch.from_numpy(mcols.astype(np.int32)).to(dev)

vm = Air(9).add_permutation([0, 1], [2, 3]).add_lookup([4], [5], 6).add_lookup([7], [5], 8)
order = rng.permutation(n)
c0, c1 = rng.integers(0, p, n), rng.integers(0, p, n)
table = rng.permutation(4 * n)[:n]
lcols = np.stack([c0, c1, c0[order], c1[order], table[rng.integers(0, n, n)], table, np.zeros(n, dtype=np.int64),
                  table[rng.integers(0, max(1, n // 4), n)], np.zeros(n, dtype=np.int64)]).astype(np.int64)
ltrace = torch.from_numpy(lcols.astype(np.int32)).to(dev)
torch.cuda.synchronize()
for a in (1, 2):
    eng.dev_args_multiplicities(vm, a, ltrace.data_ptr(), 9, log_n, ltrace.data_ptr() + 4 * ((6 if a == 1 else 8) << log_n))

common = dict(row_leaves=True, ext=True, grind_bits=bits, timed=True, check=False)
SHAPES = [("mimc x4 B=8", mimc, mtrace, 4, 3, "deep"), ("nine-column list B=8", vm, ltrace, 9, 3, "deep_args"), ("nine-column list B=4", vm, ltrace, 9, 2, "deep_args")]
for label, air, trace, W, lb, key in SHAPES:
    modes = {"coset leaves, fold 4": dict(common, coset_leaves=True, **{key: True}), "row leaves, fold 2": dict(common, **{key: True})}
    ev, wall, stages, last = ({m: [] for m in modes} for _ in range(4))
    for i in range(3 + args.reps):
        for m, kw in modes.items():
            eng.sync()
            t0 = time.perf_counter()
            res = eng.dev_air_prove(air, trace.data_ptr(), W, log_n, lb, t, **kw)
            dt = (time.perf_counter() - t0) * 1e3
            last[m] = res
            if i >= 3:
                wall[m].append(dt)
                ev[m].append(sum(res["stage_ms"].values()))
                stages[m].append(res["stage_ms"])
    if key == "deep":
        want = {"coset leaves, fold 4": eng.air_deep_fold4_layout(air, W, log_n, lb, t)[1], "row leaves, fold 2": eng.air_plan_deep(air, W, log_n, lb, num_colinearity_tests=t)[2]}
    else:
        want = {"coset leaves, fold 4": eng.air_deep_args_fold4_layout(air, W, log_n, lb, t)[1],
                "row leaves, fold 2": eng.air_plan_deep_args(air, W, log_n, lb, num_colinearity_tests=t)[2]}
    print(f"{label}: n=2^{log_n} W={W} t={t} bits={bits}")
    for m, kw in modes.items():
        st = {name: med(v[name] for v in stages[m]) for name in stages[m][0]}
        nbytes = len(last[m]["proof"])
        ok, why = eng.air_verify(air, last[m]["proof"], last[m]["column_roots"], W, log_n, lb, t, row_leaves=True, ext=True, grind_bits=bits,
                                 coset_leaves=kw.get("coset_leaves", False), **{key: True})
        print(f"  {m:22s}: stages' sum {span(ev[m])}; wall {span(wall[m])}; proof {nbytes} bytes "
              f"({'=' if nbytes == want[m] else '!='} layout {want[m]}); verified {ok} {why!r}")
        print("    stages " + ", ".join(f"{name} {v:.3f}" for name, v in st.items()))
    a, b = (med(ev[m]) for m in modes)
    sa, sb = ({name: med(v[name] for v in stages[m]) for name in stages[m][0]} for m in modes)
    worst = max(sa, key=lambda name: sa[name] - sb[name])
    print(f"  coset leaves / row leaves: time {a / b:.3f}, bytes {len(last['coset leaves, fold 4']['proof']) / len(last['row leaves, fold 2']['proof']):.3f}; "
          f"the stage that gains least (or loses most): {worst} {sa[worst] - sb[worst]:+.3f} ms")
    del last

# ---- the leaf kernel beside the wide-row kernel
stream = torch.cuda.Stream()
eng.set_stream(stream.cuda_stream)   # the library's launches and the events below share one stream


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
    eng.profile(True)
    eng.profile_read()
    out = []
    for _ in range(args.reps):
        fn()
        rd = eng.profile_read().get(name)
        if rd:
            out.append(rd["total_ms"])
    eng.profile(False)
    return out


N = 1 << 23
q = N // 4
for V in (4, 21):
    cols = torch.randint(0, p, (V, N), dtype=torch.int32, device=dev)
    nodes = torch.empty((2 * N, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cosets = lambda: eng.dev_merkle_build_cosets(cols.data_ptr(), V, N, N, nodes.data_ptr())
    rows_ = lambda: eng.dev_merkle_build_rows(cols.data_ptr(), V, N, N, nodes.data_ptr())
    floor = 4 * V * N + 32 * q
    a_, b_ = torch.empty(floor // 8, dtype=torch.int32, device=dev), torch.empty(floor // 8, dtype=torch.int32, device=dev)
    cp = med(timed(lambda: b_.copy_(a_)))
    tc, tr_ = timed(cosets), timed(rows_)
    kc, kr = bracketed(cosets, "coset_leaf_hash_kernel"), bracketed(rows_, "row_hash_wide_kernel")
    print(f"leaf kernels at 2^23 points a column, V = {V}: the coset kernel's floor {floor} bytes, a copy of as many {cp:.4f} ms")
    print(f"  coset tree (q = 2^21 leaves of {4 * V} values): whole {span(tc)}; coset_leaf_hash_kernel {span(kc)}, {med(kc) / cp:.2f} copies, "
          f"{(V + 8) * q / med(kc) / 1e6:.1f} G mixes/s")
    print(f"  row tree   (2^23 leaves of {V} values): whole {span(tr_)}" + (f"; row_hash_wide_kernel {span(kr)}, {med(kr) / cp:.2f} copies of the coset floor, "
          f"{((V + 3) // 4 + 8) * N / med(kr) / 1e6:.1f} G mixes/s" if kr else "; leaves hashed by the fused row path of the Merkle kernels"))
    print(f"  whole tree, cosets / rows: {med(tc) / med(tr_):.3f}")
    del cols, nodes, a_, b_
eng.close()
dst = args.out or os.path.join(os.path.abspath(args.root), "profiles", "deep_fold4_time.log")
with open(dst, "w") as fh:
    fh.write("\n".join(LINES) + "\n")
