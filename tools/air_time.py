#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's AIR section.

    python3 tools/air_time.py                 # compose kernel times + prove medians on this build
    python3 tools/air_time.py --stark-only    # only smi_dev_stark_prove(open_columns = 1): what a build without the
                                              # AIR entry points can run (set --root to that build's tree)
    rocprofv3 --kernel-trace --output-format csv --pmc SQ_INSTS_VALU SQ_WAVES -d OUT -o air -- python3 tools/air_time.py --single
                                              # VALU instructions per wave of each AIR's launch, in a run of its own

compose: HIP-event time of air_compose_kernel (smi_ctx_profile) at (W = 4, n = 2^22, B = 8) for the empty, fib-like,
mixer AIRs and at (W = 64, n = 2^18) for a 32-constraint AIR; median of REPS launches after 3 warm-up launches;
achieved bytes/s of 4 (W + 1) N against an in-run device-to-device copy moving the same bytes.
prove: median wall time of nine smi_dev_air_prove(empty) / smi_dev_stark_prove(open_columns = 1) calls on one trace.
periodic: four lanes x' = (x + k)^3 at (n = 2^22, B = 8), (a) the constants as periodic columns (W = 4, Q = 4, period 64 and
period n) and (b) as four more trace columns (W = 8, Q = 0): compose kernel time, prove wall time and stages.  --no-periodic
leaves (a) out: what a library without periodic columns (SMI_LIB) can run.
rows: smi_dev_air_prove_rows beside smi_dev_air_prove on the same trace -- empty and mixer at (W = 4, n = 2^22) and the
32-constraint AIR at (W = 64, n = 2^18): median of nine calls, the five stages and the proof length of both.  --no-rows leaves
them out: what a library without the row-committed entry points can run.
ext (--ext-only: nothing else): the quartic-extension legs.  air_compose_ext_kernel beside FOUR launches of
air_compose_kernel (what a caller without it does for four weight vectors) on the same columns, against a device copy of
4 (W + 4) N bytes; fri_fold_ext_kernel at 2^25 elements against a device copy of its 48 bytes per output element;
smi_dev_air_prove_ext(mixer) beside smi_dev_air_prove_rows(mixer) on one trace, median of nine with the stages.
--no-ext leaves them out (a build without the entry points skips them by itself).
--single-ext: one air_compose_ext_kernel launch per AIR, the run to put under `rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES`."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--stark-only", action="store_true")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--single", action="store_true", help="one launch per AIR at (W = 4, n = 2^22) and nothing else: the run to put under "
                "`rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_WAVES` (the k-th air_compose_kernel dispatch is the k-th AIR printed)")
ap.add_argument("--no-periodic", action="store_true", help="skip the legs that need periodic columns")
ap.add_argument("--no-stark", action="store_true", help="skip smi_dev_stark_prove")
ap.add_argument("--no-rows", action="store_true", help="skip the smi_dev_air_prove_rows legs")
ap.add_argument("--ext-only", action="store_true", help="only the quartic-extension legs")
ap.add_argument("--no-ext", action="store_true", help="skip the quartic-extension legs: what a library without them can run")
ap.add_argument("--single-ext", action="store_true", help="--single for air_compose_ext_kernel")
ap.add_argument("--rows-only", action="store_true", help="only the column-tree / row-tree prove pairs")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import stark_rs_amd as s  # noqa: E402

p, g = s.P2, s.G2
eng = s.Engine(p, g, 0)
dev = torch.device("cuda:0")
rng = np.random.default_rng(1)


def rand_cols(W, n):
    return torch.from_numpy(rng.integers(0, p, (W, n), dtype=np.int64).astype(np.int32)).to(dev)


def median_kernel_ms(fn, name):
    for _ in range(3):
        fn()
    eng.sync()
    eng.profile(True)
    eng.profile_read()
    out = []
    for _ in range(args.reps):
        fn()
        out.append(eng.profile_read()[name]["total_ms"])
    eng.profile(False)
    return statistics.median(out), min(out), max(out)


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


def airs(W, n):
    from stark_rs_amd.mirror import Air
    empty = Air(W)
    fib = Air(W)
    fib.transition({("next", 0): 1, ("cur", 1): -1}).transition({("next", 1): 1, ("cur", 0): -1, ("cur", 1): -1})
    fib.boundary(0, 0, 1).boundary(1, 0, 1).boundary(0, n - 1, 5)
    def transitions(air):
        air.transition({("next", 0): 1, (("cur", 0), ("cur", 1)): -1, ("cur", 2): -1})
        air.transition({("next", 1): 1, (("cur", 0, 2), ("cur", 2)): -1, ("cur", 1): -3})
        return air.transition({("next", 2): 1, ("cur", 2): -1, (): -1})
    mixer = transitions(Air(W))
    mixer.boundary(0, 0, 5).boundary(1, 0, 11).boundary(2, 0, 0).boundary(2, n - 1, n - 1).boundary(0, n - 1, 9)
    only_t = transitions(Air(W))
    only_b = Air(W)
    only_b.boundaries = list(mixer.boundaries)
    return [("empty", empty), ("fib", fib), ("mixer", mixer), ("mixer, transitions only", only_t), ("mixer, boundaries only", only_b)]


def wide(W, K, n):
    from stark_rs_amd.mirror import Air
    air = Air(W)
    for k in range(K):
        air.transition({("next", k % W): 1, (("cur", (k + 1) % W), ("cur", (3 * k + 2) % W)): -(k + 1), ("cur", (5 * k) % W, 2): 7, (): k})
    for c in range(0, W, 4):
        air.boundary(c, 0, 1).boundary(c, n - 1 - c, 2)
    return air


def lanes(periods):
    """len(periods) lanes x' = (x + k)^3 with lane c's constants in periodic column c"""
    from stark_rs_amd.mirror import Air
    air = Air(len(periods))
    for c, P in enumerate(periods):
        air.periodic([int(v) for v in rng.integers(0, p, P)])
        air.transition({("next", c): 1, ("cur", c, 3): -1, (("cur", c, 2), ("per", c)): -3, (("cur", c), ("per", c, 2)): -3, ("per", c, 3): -1})
    return air


def ext_legs():
    for W, log_n, lb, cases in [(4, 22, 3, None), (64, 18, 3, "wide")]:
        n, N = 1 << log_n, 1 << (log_n + lb)
        lde, out4, out = rand_cols(W, N), torch.empty((4, N), dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        nbytes = 4 * (W + 4) * N
        cms = copy_ms(nbytes)
        print(f"ext W={W} n=2^{log_n} B={1 << lb}: 4(W+4)N = {nbytes / 1e9:.3f} GB; device copy of the same bytes {cms:.3f} ms = {nbytes / cms / 1e9:.2f} TB/s", flush=True)
        for name, air in (airs(W, n)[:3] if cases is None else [("empty", airs(W, n)[0][1]), ("32 constraints", wide(W, 32, n))]):
            K = len(air.constraints)
            ch = torch.from_numpy(rng.integers(0, 1 << 62, 4 * (W + K), dtype=np.int64)).to(dev)
            vecs = [ch[e::4].contiguous() for e in range(4)]
            flat = air.flatten(p)
            torch.cuda.synchronize()
            med, lo, hi = median_kernel_ms(lambda: eng.dev_air_compose_ext(flat, lde.data_ptr(), W, log_n, lb, ch.data_ptr(), out4.data_ptr()),
                                           "air_compose_ext_kernel")

            def four():
                for e in range(4):
                    eng.dev_air_compose(flat, lde.data_ptr(), W, log_n, lb, vecs[e].data_ptr(), out.data_ptr())
            med4, lo4, hi4 = median_kernel_ms(four, "air_compose_kernel")
            print(f"  compose_ext {name:16s}: median {med:7.3f} ms (min {lo:.3f}, max {hi:.3f})  {nbytes / med / 1e9:5.2f} TB/s = {100 * cms / med:5.1f} % of the copy;"
                  f"  four air_compose_kernel launches {med4:7.3f} ms (min {lo4:.3f}, max {hi4:.3f}): x{med4 / med:.2f}", flush=True)
        del lde, out4, out
    L = 1 << 25
    cw, nxt = rand_cols(4, L), torch.empty((4, L // 2), dtype=torch.int32, device=dev)
    al = torch.from_numpy(rng.integers(0, 1 << 62, 4, dtype=np.int64)).to(dev)
    omega = pow(g, (p - 1) // L, p)
    torch.cuda.synchronize()
    med, lo, hi = median_kernel_ms(lambda: eng.dev_fri_fold_ext(cw.data_ptr(), L, L, al.data_ptr(), g, omega, nxt.data_ptr()), "fri_fold_ext_kernel")
    nbytes = 48 * (L // 2)
    cms = copy_ms(nbytes)
    print(f"fri_fold_ext_kernel 2^25 elements: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})  {nbytes / med / 1e9:.2f} TB/s; device copy of the same "
          f"{nbytes / 1e9:.3f} GB {cms:.3f} ms = {nbytes / cms / 1e9:.2f} TB/s: {100 * cms / med:.1f} % of the copy", flush=True)
    del cw, nxt
    W, log_n, lb, t = 4, 22, 3, 32
    trace = rand_cols(W, 1 << log_n)
    flat = airs(W, 1 << log_n)[2][1].flatten(p)
    torch.cuda.synchronize()
    for variant, kw in (("rows", dict(row_leaves=True)), ("ext", dict(row_leaves=True, ext=True)), ("rows", dict(row_leaves=True)), ("ext", dict(row_leaves=True, ext=True))):
        runs = wall(lambda: eng.dev_air_prove(flat, trace.data_ptr(), W, log_n, lb, t, timed=True, check=False, **kw))
        med = runs[4]
        print(f"air_prove[{variant:4s}] mixer, any trace W={W} n=2^{log_n}: median {med[0]:.3f} ms (min {runs[0][0]:.3f}, max {runs[-1][0]:.3f})  "
              f"stages {({k: round(v, 3) for k, v in med[1]['stage_ms'].items()})}  proof {len(med[1]['proof'])} bytes", flush=True)


def wall(fn):
    for _ in range(2):
        fn()
    runs = []
    for _ in range(9):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        runs.append((1e3 * (time.perf_counter() - t0), res))
    runs.sort(key=lambda x: x[0])
    return runs


if args.ext_only:
    ext_legs()
    eng.close()
    sys.exit(0)

if args.single or args.single_ext:
    W, log_n, lb = 4, 22, 3
    N = 1 << (log_n + lb)
    lde, out = rand_cols(W, N), torch.empty((4 if args.single_ext else 1) * N, dtype=torch.int32, device=dev)
    for k, (name, air) in enumerate(airs(W, 1 << log_n)):
        wts = torch.from_numpy(rng.integers(0, 1 << 62, (4 if args.single_ext else 1) * (W + len(air.constraints)), dtype=np.int64)).to(dev)
        torch.cuda.synchronize()
        compose = eng.dev_air_compose_ext if args.single_ext else eng.dev_air_compose
        compose(air.flatten(p), lde.data_ptr(), W, log_n, lb, wts.data_ptr(), out.data_ptr())
        eng.sync()
        print(f"dispatch {k}: {name}  ({N} points)", flush=True)
    eng.close()
    sys.exit(0)

if not args.stark_only and not args.rows_only:
    for W, log_n, lb, cases in [(4, 22, 3, None), (64, 18, 3, "wide")]:
        n, N = 1 << log_n, 1 << (log_n + lb)
        lde, out = rand_cols(W, N), torch.empty(N, dtype=torch.int32, device=dev)
        nbytes = 4 * (W + 1) * N
        cms = copy_ms(nbytes)
        print(f"W={W} n=2^{log_n} B={1 << lb}: 4(W+1)N = {nbytes / 1e9:.3f} GB; device copy of the same bytes {cms:.3f} ms = {nbytes / cms / 1e9:.2f} TB/s", flush=True)
        for name, air in (airs(W, n) if cases is None else [("empty", airs(W, n)[0][1]), ("32 constraints", wide(W, 32, n))]):
            K = len(air.constraints)
            wts = torch.from_numpy(rng.integers(0, 1 << 62, W + K, dtype=np.int64)).to(dev)
            flat = air.flatten(p)
            torch.cuda.synchronize()
            med, lo, hi = median_kernel_ms(lambda: eng.dev_air_compose(flat, lde.data_ptr(), W, log_n, lb, wts.data_ptr(), out.data_ptr()),
                                           "air_compose_kernel")
            print(f"  compose {name:26s}: median {med:7.3f} ms (min {lo:.3f}, max {hi:.3f}; {args.reps} launches)  {nbytes / med / 1e9:5.2f} TB/s"
                  f" = {100 * cms / med:5.1f} % of the copy", flush=True)
        del lde, out

W, log_n, lb, t = 4, 22, 3, 32
trace = rand_cols(W, 1 << log_n)
torch.cuda.synchronize()


def prove_pair(label, flat, tr, Wl, ln):
    """column trees and, unless --no-rows, the row tree: the same statement on the same trace, one after the other"""
    for variant in ("columns",) + (() if args.no_rows else ("rows",)):
        runs = wall(lambda: eng.dev_air_prove(flat, tr.data_ptr(), Wl, ln, lb, t, timed=True, check=False, **({"row_leaves": True} if variant == "rows" else {})))
        med = runs[4]
        print(f"air_prove[{variant:7s}] {label:26s} W={Wl} n=2^{ln}: median {med[0]:.3f} ms (min {runs[0][0]:.3f}, max {runs[-1][0]:.3f})  "
              f"stages {({k: round(v, 3) for k, v in med[1]['stage_ms'].items()})}  proof {len(med[1]['proof'])} bytes", flush=True)


def pair_legs():
    from stark_rs_amd.mirror import Air
    prove_pair("empty", Air(W).flatten(p), trace, W, log_n)
    prove_pair("mixer, any trace", airs(W, 1 << log_n)[2][1].flatten(p), trace, W, log_n)
    wide_trace = rand_cols(64, 1 << 18)
    torch.cuda.synchronize()
    prove_pair("32 constraints", wide(64, 32, 1 << 18).flatten(p), wide_trace, 64, 18)


if args.rows_only:
    pair_legs()
    eng.close()
    sys.exit(0)

if not args.no_stark:
    runs = wall(lambda: eng.dev_stark_prove(trace.data_ptr(), W, log_n, lb, t, timed=True, open_columns=True))
    print(f"stark_prove(open_columns=1) W=4 n=2^22: median {runs[4][0]:.3f} ms  all {[round(r[0], 3) for r in runs]}  stages {runs[4][1]['stage_ms']}", flush=True)
if not args.stark_only:
    from stark_rs_amd.mirror import Air
    flat = Air(W).flatten(p)
    runs = wall(lambda: eng.dev_air_prove(flat, trace.data_ptr(), W, log_n, lb, t, timed=True, check=False))
    print(f"air_prove(empty)            W=4 n=2^22: median {runs[4][0]:.3f} ms  all {[round(r[0], 3) for r in runs]}  stages {runs[4][1]['stage_ms']}", flush=True)
    name, mixer = airs(W, 1 << log_n)[2]
    flat = mixer.flatten(p)
    runs = wall(lambda: eng.dev_air_prove(flat, trace.data_ptr(), W, log_n, lb, t, timed=True, check=False))
    print(f"air_prove(mixer, any trace) W=4 n=2^22: median {runs[4][0]:.3f} ms  all {[round(r[0], 3) for r in runs]}  stages {runs[4][1]['stage_ms']}", flush=True)

if not args.stark_only:
    # periodic columns against the same constants committed as trace columns
    n, N = 1 << log_n, 1 << (log_n + lb)
    legs = [] if args.no_periodic else [("(a) W=4 Q=4 period 64", lanes([64] * 4), None), ("(a') W=4 Q=4 period n", lanes([n] * 4), None)]
    a64 = lanes([64] * 4)
    legs.append(("(b) W=8 Q=0, constants committed", a64.with_periodic_as_trace(),
                 torch.from_numpy(np.stack([np.resize(np.array(v, dtype=np.int64), n) for v in a64.periodics]).astype(np.int32)).to(dev)))
    for name, air, extra in legs:
        Wl, K = air.n_cols, len(air.constraints)
        flat = air.flatten(p)
        tr = trace if extra is None else torch.cat([trace, extra]).contiguous()
        lde, out = torch.empty((Wl, N), dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        wts = torch.from_numpy(rng.integers(0, 1 << 62, Wl + K, dtype=np.int64)).to(dev)
        torch.cuda.synchronize()
        eng.dev_lde(tr.data_ptr(), Wl, log_n, lb, lde.data_ptr())
        med, lo, hi = median_kernel_ms(lambda: eng.dev_air_compose(flat, lde.data_ptr(), Wl, log_n, lb, wts.data_ptr(), out.data_ptr()),
                                       "air_compose_kernel")
        nbytes = 4 * (Wl + 1) * N
        print(f"  compose {name:34s}: median {med:7.3f} ms (min {lo:.3f}, max {hi:.3f})  4(W+1)N = {nbytes / 1e9:.3f} GB  {nbytes / med / 1e9:5.2f} TB/s", flush=True)
        del lde, out
        runs = wall(lambda: eng.dev_air_prove(flat, tr.data_ptr(), Wl, log_n, lb, t, timed=True, check=False))
        print(f"air_prove {name:34s}: median {runs[4][0]:.3f} ms  all {[round(r[0], 3) for r in runs]}  stages {runs[4][1]['stage_ms']}", flush=True)
if not args.stark_only and not args.no_rows:
    pair_legs()
if not args.stark_only and not args.no_ext:
    if hasattr(eng, "dev_air_compose_ext"):
        ext_legs()
    else:
        print("ext legs skipped: this build has no quartic-extension entry points (--no-ext says so up front)", flush=True)
eng.close()
