#!/usr/bin/env python3
"""Development tool (GPU box): the leaf launch of a row tree over more than four columns, and the whole tree.

    python3 tools/row_hash_time.py                      # this build
    SMI_LIB=/path/to/another/libstarkmi.so python3 tools/row_hash_time.py --tag parent

For W in {5, 8, 16, 64} with n chosen so that the columns hold about 0.5 GB: HIP-event times (median of --reps calls
after 3 warm-up calls) of smi_dev_merkle_build_rows (leaf launch + tree) and of smi_dev_merkle_from_digests over the same
digests (the tree alone); their difference is the leaf launch whatever the build calls its kernel.  Where the build
names the kernel in smi_ctx_profile (row_hash_wide_kernel) its own bracketed time is printed next to the difference.
Two floors from the same run: a device-to-device copy that moves 4 W n + 32 n bytes, and (ceil(W/4) + 8) n mixes at
the rate smi_ctx_mix_probe returns.  One JSON line per width."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--tag", default="this")
ap.add_argument("--shapes", default="5:24,8:24,16:23,64:21", help="W:log2(n) pairs")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import stark_rs_amd as s  # noqa: E402

p, g = s.P2, s.G2
eng = s.Engine(p, g, 0)
dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
eng.set_stream(stream.cuda_stream)   # the library's launches and the events below share one stream


def timed(fn):
    """median, min, max of the HIP-event time of fn, bracketed on the stream it runs on"""
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
    return statistics.median(out), min(out), max(out)


def copy_ms(nbytes):
    a = torch.empty(nbytes // 8, dtype=torch.int32, device=dev)   # nbytes / 2 read + nbytes / 2 written
    b = torch.empty_like(a)
    return timed(lambda: b.copy_(a))[0]


mix_rate = eng.mix_probe()
print(json.dumps({"tag": args.tag, "lib": os.environ.get("SMI_LIB", "default"), "mix_probe_per_s": mix_rate}), flush=True)
for spec in args.shapes.split(","):
    W, logn = (int(x) for x in spec.split(":"))
    n = 1 << logn
    cols = torch.randint(0, p, (W, n), dtype=torch.int32, device=dev)
    nodes = torch.empty((2 * n, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    whole = timed(lambda: eng.dev_merkle_build_rows(cols.data_ptr(), W, n, n, nodes.data_ptr()))
    tree = timed(lambda: eng.dev_merkle_from_digests(n, nodes.data_ptr()))
    rec = {"tag": args.tag, "W": W, "log_n": logn, "column_gb": 4 * W * n / 1e9,
           "tree_with_leaves_ms": whole, "tree_alone_ms": tree, "leaf_ms_by_difference": whole[0] - tree[0]}
    eng.profile(True)
    eng.profile_read()
    own = []
    for _ in range(args.reps):
        eng.dev_merkle_build_rows(cols.data_ptr(), W, n, n, nodes.data_ptr())
        k = eng.profile_read().get("row_hash_wide_kernel")
        if k:
            own.append(k["total_ms"])
    eng.profile(False)
    if own:
        rec["leaf_ms_bracketed"] = (statistics.median(own), min(own), max(own))
    nbytes, mixes = 4 * W * n + 32 * n, ((W + 3) // 4 + 8) * n
    rec["floor_copy_ms"] = copy_ms(nbytes)
    rec["floor_mix_ms"] = 1e3 * mixes / mix_rate
    print(json.dumps(rec), flush=True)
    del cols, nodes
eng.close()
