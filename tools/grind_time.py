#!/usr/bin/env python3
"""Development tool (GPU box): the numbers of DESIGN.md's "Grinding" subsection.  One JSON line per leg.

    python3 tools/grind_time.py               # both legs
    python3 tools/grind_time.py --rate-only
    python3 tools/grind_time.py --prove-only

rate: smi_dev_grind at bits = 32 with max_tries = 2^28 on a transcript at phase 0 (9 mixes a nonce) and one at phase 28 (10
mixes), chosen so that the call returns SMI_ERR_GRIND_EXHAUSTED: no nonce below the cap is valid, every lane runs to the
cap, the work is fixed.  HIP-event time of grind_kernel alone (smi_ctx_profile), median of nine calls after three;
nonces/s and its share of the floor tries * (9 or 10) / mixes_per_s with mixes_per_s from smi_ctx_mix_probe in this
process.
prove: smi_dev_air_prove_ext (unchanged code) beside smi_dev_air_prove_ext_pow at 0, 16, 20 and 24 bits on one trace at
the headline shape (mixer, W = 4, n = 2^22, B = 8, t = 32): wall times interleaved in one session, median of nine after
two warm-up rounds, the `fri` stage, the nonce found and (nonce + 1) / rate beside the added time."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--log-tries", type=int, default=28)
ap.add_argument("--rate-only", action="store_true")
ap.add_argument("--prove-only", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import stark_rs_amd as s  # noqa: E402

p, g = s.P2, s.G2
eng = s.Engine(p, g, 0)
dev = torch.device("cuda:0")
mix_rate = eng.mix_probe()
print(json.dumps({"leg": "mix_probe", "mixes_per_s": mix_rate}), flush=True)


def exhausted(t, bits, tries):
    try:
        eng.grind(t, bits, tries)
    except s.StarkMiError as e:
        if e.status != -55:
            raise
        return True
    return False


def rate_leg(length):
    tries, bits = 1 << args.log_tries, 32
    rng = np.random.default_rng(length)
    while True:   # 15 in 16 transcripts have no valid nonce below 2^28 at 32 bits
        t = bytes(rng.integers(0, 256, length, dtype=np.uint8))
        if exhausted(t, bits, tries):
            break
    for _ in range(2):
        exhausted(t, bits, tries)
    eng.profile(True)
    eng.profile_read()
    ms = []
    for _ in range(args.reps):
        assert exhausted(t, bits, tries)
        ms.append(eng.profile_read()["grind_kernel"]["total_ms"])
    eng.profile(False)
    med, mixes = statistics.median(ms), 9 if length % 32 <= 24 else 10
    rate = tries / (med * 1e-3)
    floor_ms = 1e3 * tries * mixes / mix_rate
    print(json.dumps({"leg": "rate", "phase": length % 32, "transcript_len": length, "mixes_per_nonce": mixes, "tries": tries,
                      "kernel_ms": {"median": med, "min": min(ms), "max": max(ms)}, "nonces_per_s": rate, "mixes_per_s": rate * mixes,
                      "floor_ms": floor_ms, "share_of_mix_floor": floor_ms / med}), flush=True)
    return rate


def prove_leg(rate9):
    from stark_rs_amd.mirror import Air
    W, log_n, lb, t = 4, 22, 3, 32
    n, N = 1 << log_n, 1 << (log_n + lb)
    air = Air(W)
    air.transition({("next", 0): 1, (("cur", 0), ("cur", 1)): -1, ("cur", 2): -1})
    air.transition({("next", 1): 1, (("cur", 0, 2), ("cur", 2)): -1, ("cur", 1): -3})
    air.transition({("next", 2): 1, ("cur", 2): -1, (): -1})
    air.boundary(0, 0, 5).boundary(1, 0, 11).boundary(2, 0, 0).boundary(2, n - 1, n - 1).boundary(0, n - 1, 9)
    flat = air.flatten(p)
    _d, E = eng.air_plan(flat, W, log_n, lb)
    trace = torch.from_numpy(np.random.default_rng(1).integers(0, p, (W, n), dtype=np.int64).astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    R = eng.fri_num_rounds(eng.fri_cfg(pow(g, (p - 1) // N, p), g, N, E, t))
    at = 33 * R + 9 + 32 * (N >> (R - 1))            # the nonce record, behind the roots and the last codeword
    variants = [None, 0, 16, 20, 24]
    wall, fri, nonce = {v: [] for v in variants}, {v: [] for v in variants}, {}
    for rnd in range(2 + args.reps):                 # interleaved: every variant once per round
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = eng.dev_air_prove(flat, trace.data_ptr(), W, log_n, lb, t, timed=True, check=False, row_leaves=True, ext=True, grind_bits=v)
            dt = 1e3 * (time.perf_counter() - t0)
            if rnd >= 2:
                wall[v].append(dt)
                fri[v].append(res["stage_ms"]["fri"])
            if v is not None:
                nonce[v] = int.from_bytes(res["proof"][at + 9:at + 17], "little")
    base = statistics.median(wall[None])
    for v in variants:
        rec = {"leg": "prove", "grind_bits": v, "wall_ms": {"median": statistics.median(wall[v]), "min": min(wall[v]), "max": max(wall[v])},
               "fri_stage_ms_median": statistics.median(fri[v])}
        if v is not None:
            rec.update({"nonce": nonce[v], "added_wall_ms": statistics.median(wall[v]) - base,
                        "added_fri_ms": statistics.median(fri[v]) - statistics.median(fri[None]),
                        "nonce_plus_1_over_rate_ms": 1e3 * (nonce[v] + 1) / rate9})
        print(json.dumps(rec), flush=True)


rate9 = None
if not args.prove_only:
    rate9 = rate_leg(64)      # phase 0
    rate_leg(60)              # phase 28
if not args.rate_only:
    if rate9 is None:
        rate9 = mix_rate / 9
    prove_leg(rate9)
eng.close()
