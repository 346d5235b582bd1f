#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's "Fold by 4" subsection, written to profiles/fold4_time.log.

    python3 tools/fold4_time.py [--log profiles/fold4_time.log]

The fold: fri_fold4_ext_kernel at 2^25 elements beside its yardstick, the two fri_fold_ext_kernel launches it replaces (2^25
under alpha, then 2^24 under alpha^2 on the squared domain), and beside a device copy of its 80 * 2^23 bytes.  HIP-event
times (smi_ctx_profile), median of 9 after 3 warm-ups with min and max; the two paths alternate launch by launch in one
process, on the second project prime.  The outputs of the two paths are compared once, exactly."""
import argparse
import os
import statistics
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--log", default=None)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import stark_rs_amd as s  # noqa: E402

p, g = s.P2, s.G2
eng = s.Engine(p, g, 0)
dev = torch.device("cuda:0")
rng = np.random.default_rng(1)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def ext_sq(a):
    """a * a in F_p[X] / (X^4 - g) on Python ints"""
    prod = [0] * 7
    for i, x in enumerate(a):
        for j, y in enumerate(a):
            prod[i + j] += x * y
    return [(prod[k] + g * (prod[k + 4] if k < 3 else 0)) % p for k in range(4)]


def stats(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


L = 1 << 25
cw = torch.from_numpy(rng.integers(0, p, (4, L), dtype=np.int64).astype(np.int32)).to(dev)
mid = torch.empty((4, L // 2), dtype=torch.int32, device=dev)
out2 = torch.empty((4, L // 4), dtype=torch.int32, device=dev)
out4 = torch.empty((4, L // 4), dtype=torch.int32, device=dev)
alpha = [int(v) for v in rng.integers(0, 1 << 62, 4, dtype=np.int64)]
al1 = torch.tensor(alpha, dtype=torch.int64, device=dev)
al2 = torch.tensor(ext_sq([a % p for a in alpha]), dtype=torch.int64, device=dev)
omega = pow(g, (p - 1) // L, p)
torch.cuda.synchronize()


def fold4():
    eng.dev_fri_fold4_ext(cw.data_ptr(), L, L, al1.data_ptr(), g, omega, out4.data_ptr())


def pair():
    eng.dev_fri_fold_ext(cw.data_ptr(), L, L, al1.data_ptr(), g, omega, mid.data_ptr())
    eng.dev_fri_fold_ext(mid.data_ptr(), L // 2, L // 2, al2.data_ptr(), g * g % p, omega * omega % p, out2.data_ptr())


for _ in range(3):
    fold4()
    pair()
eng.sync()
assert torch.equal(out4, out2), "the fold by 4 and the two folds by 2 disagree"
eng.profile(True)
eng.profile_read()
t4, t2 = [], []
for _ in range(args.reps):
    fold4()
    t4.append(eng.profile_read()["fri_fold4_ext_kernel"]["total_ms"])
    pair()
    t2.append(eng.profile_read()["fri_fold_ext_kernel"]["total_ms"])
eng.profile(False)

nbytes = 80 * (L // 4)
a = torch.empty(nbytes // 8, dtype=torch.int32, device=dev)   # nbytes / 2 read + nbytes / 2 written
b = torch.empty_like(a)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
tc = []
for i in range(3 + args.reps):
    e0.record()
    b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    if i >= 3:
        tc.append(e0.elapsed_time(e1))

m4, m2, mc = statistics.median(t4), statistics.median(t2), statistics.median(tc)
say(f"p = {p}, 2^25 elements, {args.reps} alternating launches after 3 warm-ups; outputs of the two paths equal")
say(f"fri_fold4_ext_kernel (one launch, {nbytes / 1e9:.3f} GB):            {stats(t4)}  {nbytes / m4 / 1e9:.2f} TB/s")
say(f"fri_fold_ext_kernel x 2 (2^25 then 2^24, {144 * (L // 4) / 1e9:.3f} GB):  {stats(t2)}  {144 * (L // 4) / m2 / 1e9:.2f} TB/s")
say(f"device copy of {nbytes / 1e9:.3f} GB:                               {stats(tc)}  {nbytes / mc / 1e9:.2f} TB/s")
say(f"fold4 / pair = {m4 / m2:.3f};  copy / fold4 = {mc / m4:.3f}")
del cw, mid, out2, out4, a, b

# ---- the prove: air_prove[ext], W = 4, n = 2^22, blowup 8, t = 32, grind_bits 16, folding 4 beside folding 2
from stark_rs_amd.mirror import Air  # noqa: E402

W, log_n, lb, t, bits = 4, 22, 3, 32, 16
n, N = 1 << log_n, 1 << (log_n + lb)
air = Air(W)   # the mixer of tools/air_time.py on any trace (check=False): three transitions, five boundary points
air.transition({("next", 0): 1, (("cur", 0), ("cur", 1)): -1, ("cur", 2): -1})
air.transition({("next", 1): 1, (("cur", 0, 2), ("cur", 2)): -1, ("cur", 1): -3})
air.transition({("next", 2): 1, ("cur", 2): -1, (): -1})
air.boundary(0, 0, 5).boundary(1, 0, 11).boundary(2, 0, 0).boundary(2, n - 1, n - 1).boundary(0, n - 1, 9)
flat = air.flatten(p)
K = 3
trace = torch.from_numpy(rng.integers(0, p, (W, n), dtype=np.int64).astype(np.int32)).to(dev)
torch.cuda.synchronize()
_deg, E = eng.air_plan(flat, W, log_n, lb)


def rounds(length, e, tests):
    r = 0
    while length > e and 4 * tests < length:
        length //= 2
        r += 1
    return r


def header_len(folding):
    """the byte formulas of include/stark_mi.h"""
    R2, logN = rounds(N, E, t), log_n + lb
    if folding == 2:
        last = N >> (R2 - 1)
        fri = 33 * R2 + 9 + 32 * last + 17
        for r in range(R2 - 1):
            d = logN - r
            fri += t * (9 + 96) + t * (2 * (9 + 32 * d) + 9 + 32 * (d - 1))
        return fri, fri + t * 4 * (9 + 8 * W) + t * 4 * (9 + 32 * logN)
    F = (R2 - 1) // 2
    last = N >> (2 * F)
    fri = 33 * (F + 1) + 9 + 32 * last + 17
    for r in range(F):
        fri += t * (9 + 128) + t * (9 + 32 * (logN - 2 * r - 2))
    return fri, fri + t * 8 * (9 + 8 * W) + t * 8 * (9 + 32 * logN)


def prove(folding):
    return eng.dev_air_prove(flat, trace.data_ptr(), W, log_n, lb, t, timed=True, check=False, row_leaves=True, ext=True, grind_bits=bits,
                             folding=folding)


runs = {2: [], 4: []}
for i in range(3 + args.reps):
    for folding in (2, 4):
        res = prove(folding)
        if i >= 3:
            runs[folding].append(res)
say(f"air_prove[ext] mixer, any trace, W={W} n=2^{log_n} B={1 << lb} t={t} grind_bits={bits}, FRI at E={E}; HIP-event stage times, "
    f"{args.reps} alternating proves after 3 warm-ups")
for folding in (2, 4):
    tot = [sum(r["stage_ms"].values()) for r in runs[folding]]
    stages = {k: statistics.median([r["stage_ms"][k] for r in runs[folding]]) for k in runs[folding][0]["stage_ms"]}
    fri_ms = [r["stage_ms"]["fri"] for r in runs[folding]]
    nbytes = len(runs[folding][0]["proof"])
    want_fri, want = header_len(folding)
    assert nbytes == want, (folding, nbytes, want)
    say(f"  folding={folding}: stages total {stats(tot)};  fri {stats(fri_ms)};  median stages {({k: round(v, 3) for k, v in stages.items()})}")
    say(f"             proof {nbytes} bytes = the header's formula (FRI part {want_fri}, openings {want - want_fri})")
eng.close()
if args.log:
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
