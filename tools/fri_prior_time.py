#!/usr/bin/env python3
"""Development tool (GPU box): median wall time of Fri::prove over a 2^L-point device codeword (blowup 8, t = 32) with
a caller's transcript of 0, 64 (phase 0: the fused path from another seed) and 37 bytes (phase 5: a phase-aware round
after every tree, no fused tail) -- smi_dev_fri_prove / smi_dev_fri_prove_fs.   python3 tools/fri_prior_time.py [L]"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import stark_rs_amd as s  # noqa: E402

L = int(sys.argv[1]) if len(sys.argv) > 1 else 23
reps = int(os.environ.get("REPS", "9"))
p, g = s.P_REF, s.G_REF
e = s.Engine(p, g, 0)
n = 1 << L
omega = e.prim_nth_root(n)
coeffs = np.random.default_rng(1).integers(0, p, n // 8, dtype=np.int64).astype(np.uint64)
cw = e.coset_ntt(coeffs, L, 3)
x = torch.from_numpy(np.asarray(cw, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
cfg = e.fri_cfg(omega, 3, n, 8, 32)
rng = np.random.default_rng(2)
for prior_len in (0, 64, 37):
    prior = rng.integers(0, 256, prior_len, dtype=np.uint8).tobytes()
    for _ in range(3):
        e.dev_fri_prove(cfg, x.data_ptr(), n, prior)
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.dev_fri_prove(cfg, x.data_ptr(), n, prior)
        walls.append(1e3 * (time.perf_counter() - t0))
    print(f"2^{L} fri_prove prior {prior_len:3d} B (phase {prior_len % 32:2d}): median {statistics.median(walls):7.3f} ms  "
          f"min {min(walls):.3f}  max {max(walls):.3f}  ({reps} runs)", flush=True)
e.close()
