#!/usr/bin/env python3
"""Development tool (GPU box): median wall time of smi_poly_zerofier, smi_poly_eval_points (n coefficients) and
smi_poly_interpolate_points on n random distinct points of 998244353, n = 2^12, 2^16, 2^20 -- host buffers in and out,
the context's stream synchronised before and after each call; REPS runs (default 7) after a warm-up of the same shape --
and the launches of one call (smi_ctx_profile, separate run).  Prints one line per size and one JSON line.
    python3 tools/poly_tree_time.py [log_n ...]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stark_rs_amd as s  # noqa: E402

logs = [int(a) for a in sys.argv[1:]] or [12, 16, 20]
reps = max(5, int(os.environ.get("REPS", "7")))
p, g = s.P_REF, s.G_REF
e = s.Engine(p, g, 0)
rng = np.random.default_rng(1)
result = {"p": p, "reps": reps, "sizes": {}}
for L in logs:
    n = 1 << L
    dom = np.unique(rng.integers(0, p, n + n // 8, dtype=np.uint64))[:n]
    rng.shuffle(dom)
    f = rng.integers(0, p, n, dtype=np.uint64)
    vals = rng.integers(0, p, n, dtype=np.uint64)
    calls = {"zerofier": lambda: e.poly_zerofier(dom), "eval_points": lambda: e.poly_eval_points(f, dom),
             "interpolate_points": lambda: e.poly_interpolate_points(dom, vals)}
    row = {}
    for name, fn in calls.items():
        fn()   # warm-up of the same shape: staging buffers, scale tables
        walls = []
        for _ in range(reps):
            e.sync()
            t0 = time.perf_counter()
            fn()
            e.sync()
            walls.append(1e3 * (time.perf_counter() - t0))
        e.profile_read()
        e.profile(True)
        fn()
        launches = sum(r["launches"] for r in e.profile_read().values())
        e.profile(False)
        row[name] = {"median_ms": round(statistics.median(walls), 3), "min_ms": round(min(walls), 3),
                     "max_ms": round(max(walls), 3), "launches": launches}
        print(f"2^{L} {name:19s} median {statistics.median(walls):8.3f} ms  min {min(walls):8.3f}  max {max(walls):8.3f}  "
              f"launches {launches}  ({reps} runs)", flush=True)
    result["sizes"][str(n)] = row
e.close()
print(json.dumps(result))
