#!/usr/bin/env python3
"""bench.py -- the headline measurement (contract in the task statement, section 4).

Metric (BASELINE.json): NTT field-elements/s on the 2^22-row trace at blowup 8 (+ prove time).
Workload at every N: each rank holds its own 4-column x 2^22-row synthetic trace resident in HBM
(u32 residues of the second prime 469762049 = 7*2^26+1, because the reference prime
998244353 has no 2^25 domain -- SURVEY F2/H1).  One step = the batched low-degree extension of
that trace: 4 inverse NTTs of 2^22 points + 4 coset NTTs of 2^25 points.  Columns are independent
units, so ranks share no data-path collective (weak scaling); value = NTT points transformed by
all ranks per second.  A plain run measures only that; with --full the same JSON line also reports:
  * roofline    -- the dominant kernel's achieved HBM GB/s from HIP events around every launch
                   in the timed region (algorithmic bytes: 8 B per point per pass), and
                   the same launch as a pure copy with the pass's access pattern (pattern_copy);
  * cpu_baseline-- the op-for-op CPU oracle of the reference path on a bounded sample (rank 0);
  * prove_ms    -- end-to-end build-defined prove (LDE + 4 column commits + combine + Fri::prove)
                   of the same trace, with per-stage HIP-event times; prove_row_leaves_ms: the same
                   with one row-leaf tree instead of the four column trees (a build-defined variant);
  * ntt_2p20    -- BASELINE configs[1]: 2^20-point forward+inverse on the reference prime;
                   cfg3_2p20x4_blowup8: configs[2], LDE + Merkle commit of a 2^20 x 4 trace on it;
  * four_step   -- (N > 1) one 2^26-point NTT sharded over the N GPUs with the RCCL all-to-all.
--dump-outputs DIR writes a seeded sample of the last timed step's extension (float64 .npy) for comparing builds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

LOG_ROWS, LOG_BLOWUP, N_COLS, N_TESTS = 22, 3, 4, 32
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: 8 TB/s spec (6.29 TB/s measured copy ceiling)


def splitmix64(seed, n):
    with np.errstate(over="ignore"):
        i = np.arange(1, n + 1, dtype=np.uint64)
        z = np.uint64(seed) + i * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def cpu_baseline():
    """The reference's own CPU algorithms (oracle = op-for-op port; Rust toolchain absent) on a
    bounded sample of the same path: Lagrange interpolate_domain at n = 2^8 and 2^10 + power-sum
    eval_domain, the n^3 / N*d fit through the measured points extrapolated (and labelled so) to the
    sizes of BASELINE's configs, the oracle's radix-2 restatement as the fair algorithmic baseline,
    and the commit side (MerkleTree::new, fold_codeword) -- SURVEY 8(d), BASELINE.md section 3."""
    from oracle import oracle as o
    o.build()
    p = o.P_REF
    n, N = 1 << 10, 1 << 13
    w, W = o.ff_prim_nth_root(n), o.ff_prim_nth_root(N)
    n_cols = 2                          # two of the workload's columns: ~11 s of CPU work
    dom = [o.ff_exp(w, k) for k in range(n)]
    dom_big = [o.ff_mul(3, o.ff_exp(W, k)) for k in range(N)]
    t_int = t_ev = 0.0
    for c in range(n_cols):
        vals = splitmix64(0x5354524B00 + c, n) % np.uint64(p)
        t0 = time.perf_counter()
        coeffs = o.poly_interpolate_domain(dom, vals)
        t1 = time.perf_counter()
        o.poly_eval_domain(coeffs, dom_big)
        t2 = time.perf_counter()
        t_int += t1 - t0
        t_ev += t2 - t1
    # the second measured point of interpolate_domain (n = 2^8; repeated to get above timer noise) and of
    # eval_domain (d = 2^8, N = 2^11): the exponents of the fit come from the two points, not from the model
    n8, N8 = 1 << 8, 1 << 11
    w8, W8 = o.ff_prim_nth_root(n8), o.ff_prim_nth_root(N8)
    dom8 = [o.ff_exp(w8, k) for k in range(n8)]
    dom8_big = [o.ff_mul(3, o.ff_exp(W8, k)) for k in range(N8)]
    vals8 = splitmix64(0x5354524B00, n8) % np.uint64(p)
    reps8 = 4
    t0 = time.perf_counter()
    for _ in range(reps8):
        c8 = o.poly_interpolate_domain(dom8, vals8)
    t1 = time.perf_counter()
    for _ in range(reps8):
        o.poly_eval_domain(c8, dom8_big)
    t2 = time.perf_counter()
    t_int8, t_ev8 = (t1 - t0) / reps8, (t2 - t1) / reps8
    t_int10, t_ev10 = t_int / n_cols, t_ev / n_cols
    import math
    exp_int = math.log(t_int10 / t_int8) / math.log(n / n8)                   # ~3 for the O(n^3) Lagrange form
    exp_ev = math.log(t_ev10 / t_ev8) / math.log((n * N) / (n8 * N8))         # ~1 in N*d
    def extrap(log_rows, log_blowup=3):       # model: t_int ~ n^3, t_ev ~ N*d, anchored at the 2^10 point
        nn, NN = 1 << log_rows, 1 << (log_rows + log_blowup)
        ti = t_int10 * (nn / n) ** 3
        te = t_ev10 * (nn * NN) / (n * N)
        return {"rows": f"2^{log_rows}", "interpolate_domain_s": ti, "eval_domain_s": te,
                "field_elements_per_s": (nn + NN) / (ti + te), "years": (ti + te) / 3.156e7, "extrapolated": True}
    # the fair algorithmic baseline: the oracle's radix-2 restatement, same arithmetic, 1 thread
    big = splitmix64(2, 1 << 20) % np.uint64(p)
    w20, w23 = o.ff_prim_nth_root(1 << 20), o.ff_prim_nth_root(1 << 23)
    t3 = time.perf_counter()
    c20 = o.fast_intt(big, w20, 1)
    o.fast_coset_ntt(c20, 1 << 23, w23, 3)
    t4 = time.perf_counter()
    # ... and on all host cores: independent columns, one per thread (the C oracle runs outside the GIL)
    from concurrent.futures import ThreadPoolExecutor
    n_thr = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
    col_job = lambda c: o.fast_coset_ntt(o.fast_intt(splitmix64(100 + c, 1 << 20) % np.uint64(p), w20, 1), 1 << 23, w23, 3)[0]
    t8 = time.perf_counter()
    with ThreadPoolExecutor(n_thr) as ex:
        list(ex.map(col_job, range(n_thr)))
    t9 = time.perf_counter()
    # the commit side of the path on the CPU: MerkleTree::new over 2^18 digests and one fold of a
    # 2^18-element codeword (the reference's per-element exp + two xgcd inversions)
    m = 1 << 18
    digests = np.frombuffer(splitmix64(5, 4 * m).tobytes(), dtype=np.uint8).reshape(m, 32)
    t5 = time.perf_counter()
    o.merkle_new(digests)
    t6 = time.perf_counter()
    cw = splitmix64(6, m) % np.uint64(p)
    wm = o.ff_prim_nth_root(m)
    o.fri_fold_codeword(o.fri_cfg(wm, 3, m, 8, 32), cw, 0x0123456789ABCDEF, 3, wm)
    t7 = time.perf_counter()
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {
        "cpu_model": model, "host_cores": os.cpu_count(), "threads_used": 1,
        "merkle_node_hashes_per_s": (m - 1) / (t6 - t5), "merkle_mixes_per_s": 10.0 * (m - 1) / (t6 - t5),
        "fold_elements_per_s": (m // 2) / (t7 - t6),
        "commit_sample": f"oracle MerkleTree::new over 2^18 digests ({t6 - t5:.2f}s), Fri::fold_codeword of 2^18 elements ({t7 - t6:.2f}s), 1 thread",
        "value": n_cols * (n + N) / (t_int + t_ev), "unit": "field-elements/s", "cores": 1, "kind": "port",
        "sample": f"LDE of {n_cols} columns of 2^10 rows at blowup 8: oracle interpolate_domain n=2^10 ({t_int:.2f}s) + eval_domain "
                  f"d=2^10,N=2^13 ({t_ev:.2f}s), single thread, same u128 % p arithmetic and O(n^3)/O(N*d) algorithms as the reference",
        # the two measured sizes of SURVEY 8(d) and what the fit through them says about the configs' sizes
        "measured": {"interpolate_domain_s": {"2^8": t_int8, "2^10": t_int10}, "eval_domain_s": {"d=2^8,N=2^11": t_ev8, "d=2^10,N=2^13": t_ev10},
                     "fitted_exponent_interpolate_in_n": exp_int, "fitted_exponent_eval_in_N_times_d": exp_ev},
        "extrapolation": {"model": "interpolate_domain ~ n^3 (src/univariate/interpolate.rs:21-42), eval_domain ~ N*d (eval.rs:6-21), "
                                   "anchored at the measured 2^10 point; EXTRAPOLATED, not measured -- the reference algorithm is intractable there",
                          "cfg2_cfg3_2^20_rows": extrap(20), "headline_2^22_rows": extrap(22)},
        "fast_ntt_value": ((1 << 20) + (1 << 23)) / (t4 - t3),
        "fast_ntt_sample": f"oracle radix-2 iNTT 2^20 + coset NTT 2^23, 1 thread ({t4 - t3:.2f}s)",
        "fast_ntt_all_cores_value": n_thr * ((1 << 20) + (1 << 23)) / (t9 - t8), "fast_ntt_all_cores": n_thr,
    }


def hash_roofline(kernels, ceiling_mix_per_s, stage_ms, n_leaves, n_trees, pmc_name="merkle_sub_kernel<leaves> K=2"):
    """The prove's own roofline (Merkle "reported against both HBM and VALU").  `kernels` = event-bracketed
    per-kernel times of ONE prove (smi_ctx_profile), alg_mixes / alg_bytes as the library accounts them (9 mix_state per
    8-byte leaf, 10 per node; 4 B read per leaf, 32 B written per digest); `ceiling_mix_per_s` = smi_ctx_mix_probe in
    this run (the bare permutation, two hashes per lane: the integer-VALU ceiling of this formulation at the clock the
    chip holds under that load); `stage_ms` = the un-instrumented prove's stage times (events between the stages only).
    Bracketing every launch lets the chip clock higher than in the plain prove, so the dominant kernel's duration is
    scaled to the plain prove's clock the way `roofline` does it for the LDE: x (stage sum / bracketed kernel sum)."""
    hashk = {k: v for k, v in kernels.items() if v.get("alg_mixes", 0) > 0}
    if not hashk or not ceiling_mix_per_s:
        return None
    dom_name, dom = max(hashk.items(), key=lambda kv: kv[1]["total_ms"])
    bracketed_sum = sum(v["total_ms"] for v in kernels.values())
    plain_sum = sum(stage_ms.values())
    scale = max(1.0, plain_sum / bracketed_sum) if bracketed_sum > 0 else 1.0
    dom_ms = dom["total_ms"] * scale
    out = {
        "bound": "valu", "kernel": dom_name, "unit": "mix_state/s",
        "achieved": dom["alg_mixes"] / (dom_ms * 1e-3), "peak": ceiling_mix_per_s,
        "frac": dom["alg_mixes"] / (dom_ms * 1e-3) / ceiling_mix_per_s,
        "peak_source": "smi_ctx_mix_probe in this run: bare mix_state loop, two hashes per lane, 40 workgroups per CU, no memory traffic",
        "launches_per_prove": dom["launches"], "kernel_ms_per_prove": dom_ms, "kernel_ms_per_prove_bracketed": dom["total_ms"],
        "mixes_per_prove_in_kernel": dom["alg_mixes"],
        "hbm": {"alg_bytes_per_prove_in_kernel": dom["alg_bytes"], "achieved": dom["alg_bytes"] / (dom_ms * 1e-3) / 1e9,
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": dom["alg_bytes"] / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
        "share_of_prove_kernel_time": dom["total_ms"] / bracketed_sum if bracketed_sum else None,
    }
    # whole prove and its commit stage against the same two ceilings, on the un-instrumented clock
    tot_mixes = sum(v["alg_mixes"] for v in hashk.values())
    out["whole_prove"] = {"mixes": tot_mixes, "ms": plain_sum, "achieved": tot_mixes / (plain_sum * 1e-3),
                          "frac": tot_mixes / (plain_sum * 1e-3) / ceiling_mix_per_s,
                          "hash_kernel_share_of_kernel_time": sum(v["total_ms"] for v in hashk.values()) / bracketed_sum}
    if "commit" in stage_ms and stage_ms["commit"] > 0:
        cm = n_trees * (19.0 * n_leaves - 10.0)                      # N*9 + (N-1)*10 per tree
        cb = n_trees * 68.0 * n_leaves                               # ... and ~68 N bytes per tree
        out["commit"] = {"mixes": cm, "ms": stage_ms["commit"], "achieved": cm / (stage_ms["commit"] * 1e-3),
                         "frac": cm / (stage_ms["commit"] * 1e-3) / ceiling_mix_per_s,
                         "hbm_achieved": cb / (stage_ms["commit"] * 1e-3) / 1e9, "hbm_frac": cb / (stage_ms["commit"] * 1e-3) / 1e9 / HBM_PEAK_GBS}
    # VALU instructions per thread of the dominant kernel: SQ_INSTS_VALU / SQ_WAVES from the committed rocprofv3 --pmc
    # summary (tools/profile_prove_valu.sh), beside what its mixes alone cost in this formulation
    try:
        import glob
        files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_prove_pmc.json")))
        if files:
            pm = json.load(open(files[-1]))
            e = pm.get(pmc_name) or pm.get(dom_name)
            if e:
                out["valu_instr_per_thread"] = e["valu_insts_per_wave"]
                out["valu_instr_source"] = os.path.relpath(files[-1], ROOT) + " (rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES, earlier run)"
                out["valu_instr_of_the_mixes_alone"] = 56 * 88 + 10 * 102   # 4 leaves + 2 nodes two per state (88 per mix), 1 node alone (102)
    except Exception:
        pass
    out["kernels"] = {k: {"launches": v["launches"], "ms_per_prove_bracketed": v["total_ms"], "mixes": v["alg_mixes"],
                          "Gmix_per_s_bracketed": v["alg_mixes"] / (v["total_ms"] * 1e-3) / 1e9 if v["total_ms"] else None}
                      for k, v in hashk.items()}
    return out


DUMP_ROWS, DUMP_SEED = 1 << 20, 0x5354524B   # --dump-outputs: 2^20 of the 2^25 extended rows, 40 MB in all


def dump_outputs(dirname, lde, rank=0):
    """What the timed step hands its caller -- the extended trace, (N_COLS, N) u32 residues on the device -- as float64
    .npy files (exact: every residue is below 2^29): the same seeded sample of rows of every column (the first and last
    row always among them), the row indices, and per column the sums of the low and high 16 bits of every residue
    (exact in float64, they cover the rows outside the sample).  Rank r > 0 adds the suffix _rank<r>."""
    import torch
    n_rows = lde.shape[1]
    rows = np.random.default_rng(DUMP_SEED).choice(n_rows - 2, DUMP_ROWS - 2, replace=False) + 1
    rows = np.sort(np.concatenate([[0, n_rows - 1], rows]))
    sample = lde[:, torch.from_numpy(rows).to(lde.device)].cpu().numpy().view(np.uint32).astype(np.float64)
    sums = np.zeros((lde.shape[0], 2), dtype=np.float64)
    for c in range(lde.shape[0]):
        col = lde[c].to(torch.int64)
        sums[c] = [float((col & 0xFFFF).sum().item()), float((col >> 16).sum().item())]
    sfx = f"_rank{rank}" if rank else ""
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, f"lde_sample{sfx}.npy"), sample)
    np.save(os.path.join(dirname, f"lde_sample_rows{sfx}.npy"), rows.astype(np.float64))
    np.save(os.path.join(dirname, f"lde_column_sums{sfx}.npy"), sums)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # Defaults: a timed region of more than a second.  A 20-step region (15 ms) from an idle GPU is over before the chip has
    # settled -- measured r03: 0.783 ms per step over 20 steps after 3 warm-ups, 0.697 ms over 1 500 back-to-back steps -- so
    # the headline is the sustained figure (whatever --steps / --warmup are: see `preconditioning` below) and the cold
    # burst is reported beside it with --full (`burst`), as is `sustained` (>= 1 s of steps) after a short --steps.
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    # A plain run measures the headline only: set-up, pre-conditioning, W warm-up steps, K timed steps, the result line.
    # Every other leg (burst, sustained, roofline and copy-only twins, prove, 2^20 configs, multi-GPU legs, CPU baseline)
    # runs with --full.
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beyond the headline: burst, sustained, roofline, prove, 2^20 configs, "
                         "multi-GPU legs and the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip prove / 2^20 / four-step / cpu legs")
    ap.add_argument("--in-loop-only", action="store_true",
                    help="skip the pre-conditioning, and with --full the burst, the sustained figure, the pass that brackets "
                         "every launch and the copy-only twins, so that a profiler attached to this run sees the kernels "
                         "only as they run in the loop (tools/profile.sh)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write a fixed sample of the last step's extension as DIR/*.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    # `python bench.py --gpus N` (N > 1) outside a launcher: start one rank per GPU ourselves, as a
    # child process, BEFORE anything in this process touches the GPU (no exec after HIP init), and
    # relay the ranks' output (rank 0 prints the JSON line).  Under torch.distributed.run the
    # launcher's WORLD_SIZE must agree with --gpus, so a one-GPU number can never be recorded as an
    # N-GPU result.
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__),
               "--gpus", str(args.gpus), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        if args.full:
            cmd.append("--full")
        if args.no_extras:
            cmd.append("--no-extras")
        if args.in_loop_only:
            cmd.append("--in-loop-only")
        if args.dump_outputs:
            cmd += ["--dump-outputs", os.path.abspath(args.dump_outputs)]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.call(cmd, env=env))
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world_env}: refusing to mislabel the run", file=sys.stderr)
        sys.exit(2)

    import torch
    import torch.distributed as dist
    import stark_rs_amd as s

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # Rehearsal knobs (one-GPU box): SMI_BENCH_BACKEND=gloo and SMI_BENCH_DEVICE=0 run N ranks on one
    # card to exercise the distributed control flow; SMI_BENCH_FORCE_DIST=1 runs the multi-GPU legs on
    # a one-rank RCCL group (launched through torch.distributed.run).  The driver's runs use none.
    distributed = world > 1 or os.environ.get("SMI_BENCH_FORCE_DIST") == "1"
    backend = os.environ.get("SMI_BENCH_BACKEND", "nccl")
    if "SMI_BENCH_DEVICE" in os.environ:
        local_rank = int(os.environ["SMI_BENCH_DEVICE"])
    if distributed:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist.init_process_group(backend)
    else:
        torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")

    def barrier():
        if distributed:
            dist.barrier()

    eng = s.Engine(s.P2, s.G2, local_rank)
    p = s.P2
    n, N = 1 << LOG_ROWS, 1 << (LOG_ROWS + LOG_BLOWUP)

    # synthetic trace, column c of rank r seeded 0x5354524B00 + 4r + c, resident in HBM
    host = np.concatenate([(splitmix64(0x5354524B00 + N_COLS * rank + c, n) % np.uint64(p)).astype(np.uint32)
                           for c in range(N_COLS)])
    trace = torch.from_numpy(host.view(np.int32)).to(dev)
    out = torch.empty(N_COLS * N, dtype=torch.int32, device=dev)

    def step():
        eng.dev_lde(trace.data_ptr(), N_COLS, LOG_ROWS, LOG_BLOWUP, out.data_ptr())

    # burst: what rounds 1 and 2 reported as the headline -- 20 steps after 3 warm-up steps on a GPU that was idle until
    # then (clocks still ramping); kept for continuity, never the headline
    burst = None
    if args.full and not args.in_loop_only:
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        tb = time.perf_counter()
        for _ in range(20):
            step()
        torch.cuda.synchronize()
        burst = {"steps": 20, "warmup": 3, "ms_per_step": 1e3 * (time.perf_counter() - tb) / 20, "note": "rank-local, from an idle GPU"}
    # Pre-conditioning, reported as such (`preconditioning`): a GPU that has just left idle needs ~35 ms of work before it
    # holds its clocks (profiles/r03_b_lde_warmup_trend.txt: the first 50 steps average 737 us, every later bucket 680-688),
    # and the driver calls this script with --steps 20 --warmup 5, i.e. a 15 ms region inside that transient.  So the same
    # step runs untimed for a quarter of a second BEFORE the contract's W warm-up steps: the K timed steps then measure the
    # state a prover that is busy actually runs in, whatever W and K are.  The cold figure is `burst` (with --full).
    precond = None
    if not args.in_loop_only:
        tpc = time.perf_counter()
        n_pc = 0
        while time.perf_counter() - tpc < 0.25:
            for _ in range(50):
                step()
            torch.cuda.synchronize()
            n_pc += 50
        precond = {"steps": n_pc, "seconds": time.perf_counter() - tpc,
                   "note": "untimed, before the W warm-up steps: brings the GPU from idle to its sustained clocks; `burst` (--full) is the cold figure"}
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    # headline: exactly K un-instrumented steps between barrier + synchronize on both sides
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    if distributed:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out.view(N_COLS, N), rank)

    points_per_step = N_COLS * (n + N)                      # transform sizes summed over the batch
    value = world * points_per_step * args.steps / elapsed
    result = {
        "metric": "ntt_field_elements_per_sec", "value": value, "unit": "field-elements/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u32", "data": "synthetic",
        "config": {"workload": "lde_2^22rows_x4cols_blowup8 (4 iNTT 2^22 + 4 coset NTT 2^25 per GPU per step)",
                   "prime": p, "points_per_step_per_gpu": points_per_step, "parallelism": f"columns x{world} (no collective)"},
    }
    if not args.full:
        if precond is not None:
            result["preconditioning"] = precond
        if rank == 0:
            print(json.dumps(result), flush=True)
        eng.close()
        if distributed:
            dist.destroy_process_group()
        return

    # sustained: when the caller asked for a short region (--steps below ~1 s of work), also time at least a second of
    # back-to-back steps, the same way, and report it beside the headline
    sustained = None
    if not args.in_loop_only and elapsed < 0.9:
        n_sus = max(200, int(1.2 / max(elapsed / args.steps, 1e-6)))
        barrier()
        torch.cuda.synchronize()
        ts = time.perf_counter()
        for _ in range(n_sus):
            step()
        torch.cuda.synchronize()
        barrier()
        t_sus = time.perf_counter() - ts
        if distributed:
            tt = torch.tensor([t_sus], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            t_sus = float(tt.item())
        sustained = {"steps": n_sus, "seconds": t_sus, "ms_per_step": 1e3 * t_sus / n_sus,
                     "value": world * N_COLS * (n + N) * n_sus / t_sus,
                     "ratio_to_headline_ms_per_step": (t_sus / n_sus) / (elapsed / args.steps)}
    # roofline: a second set of steps with a HIP-event bracket around every launch (on the
    # engine's stream), outside the headline timing
    prof_steps = max(5, min(args.steps, 20))
    all_steps = 2 if args.in_loop_only else prof_steps      # --in-loop-only: just enough to name the dominant kernel
    eng.profile(True)
    step()                      # the first bracketed launch of a process pays for the event pool (140-205 us on a 37 us kernel in
    torch.cuda.synchronize()    # the --in-loop-only runs of r03, which skewed every share taken from two steps): discarded
    eng.profile_read()
    for _ in range(all_steps):
        step()
    torch.cuda.synchronize()
    kernels = eng.profile_read()
    eng.profile(False)

    # roofline of the dominant kernel (largest total time in the timed region).  An event pair around a launch perturbs
    # what it measures: the kernel no longer runs back to back with its neighbours and the chip clocks higher (DESIGN.md
    # section 3 item 8 -- the 2^25 x 4 second pass: 249 us with every launch bracketed, 243 us with only its own launches
    # bracketed, 285 us in the plain loop by rocprofv3's trace, where the kernels abut and their durations add up to the
    # step time).  `achieved` / `frac` therefore use the bracketed duration scaled to the headline's own clock:
    # x (un-instrumented ms_per_step / sum of the bracketed durations of a step), never below the measured bracket.
    dom_name, dom = max(kernels.items(), key=lambda kv: kv[1]["total_ms"])
    bracketed_ms = dom["total_ms"] / dom["launches"]
    bytes_per_launch = dom["alg_bytes"] / dom["launches"]
    eng.profile_only(dom_name)
    eng.profile(True)
    for _ in range(prof_steps):
        step()
    torch.cuda.synchronize()
    alone = eng.profile_read().get(dom_name)
    eng.profile(False)
    eng.profile_only(None)
    alone_ms = alone["total_ms"] / alone["launches"] if alone and alone["launches"] else None
    # the same for every other kernel of the step, one at a time: each then suffers the same perturbation (one event pair in a
    # loop of otherwise abutting launches), so their RATIOS are the in-loop ratios; see avg_launch_ms_alone_share below
    alone_all = {dom_name: alone_ms}
    if not args.in_loop_only and alone_ms:
        for name in kernels:
            if name == dom_name:
                continue
            eng.profile_only(name)
            eng.profile(True)
            for _ in range(prof_steps):
                step()
            torch.cuda.synchronize()
            rec = eng.profile_read().get(name)
            eng.profile(False)
            eng.profile_only(None)
            alone_all[name] = rec["total_ms"] / rec["launches"] * (rec["launches"] / prof_steps) if rec and rec["launches"] else None
    alone_step_ms = sum(alone_all.values()) if all(v is not None for v in alone_all.values()) and len(alone_all) == len(kernels) else None
    bracketed_step_ms = sum(k["total_ms"] for k in kernels.values()) / all_steps
    # In the loop the kernels of a step abut (rocprofv3 trace: no gap) and their durations add up to the step time, so the
    # dominant kernel's in-loop duration is its share of the bracketed step x the un-instrumented ms_per_step.  The scale goes
    # both ways: in r02's 20-step bursts the bracketed launches ran at a higher clock than the loop (scale > 1); in the
    # sustained state the event pairs cost the bracketed launches a few percent instead (r03: 257 us bracketed, 237-241 us by
    # the trace of the same loop), scale < 1.
    share_ms = bracketed_ms * (1e3 * elapsed / args.steps) / bracketed_step_ms
    # ... and the shares are taken from the one-kernel-at-a-time measurements where there are any: with EVERY launch bracketed
    # the second pass gains more from the pauses than its neighbours do, and its share came out 2 % low against rocprofv3's
    # trace of the same command (r03, final tree: 236.8 us against 241.6); measured one at a time, every kernel carries the
    # same single event pair and the shares are the loop's (240.8 us, profiles/r03_final_driver_command2_*).
    avg_ms = alone_ms * (1e3 * elapsed / args.steps) / alone_step_ms if alone_step_ms else share_ms
    achieved = bytes_per_launch / (avg_ms * 1e-3) / 1e9
    # HBM traffic per launch from the PMC passes of tools/profile.sh (rocprofv3 --pmc FETCH_SIZE /
    # WRITE_SIZE in separate runs, gfx950 correction applied there): a measured file committed under
    # profiles/, not something this run can collect itself; null when the file has no entry for
    # the dominant kernel of this run.
    traffic = step_traffic = None
    pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(pmc_path):
        try:
            pmc = json.load(open(pmc_path))
            traffic = pmc.get(dom_name, {}).get("hbm_bytes_per_launch")
            per = [pmc.get(k, {}).get("hbm_bytes_per_launch") for k in kernels]
            if all(x is not None for x in per):     # every launch of a step: launches per step x bytes per launch
                step_traffic = sum(x * v["launches"] / all_steps for x, v in zip(per, kernels.values()))
        except Exception:
            traffic = step_traffic = None
    # What HBM delivers for each pass's own access pattern: the copy-only twin of every pass kernel
    # (same tiles, loads and store addresses, no arithmetic), timed the same way.
    probes = {}
    if not args.in_loop_only:
        eng.copy_probe(True)
        eng.profile(True)
        for _ in range(5):
            step()
        probes = eng.profile_read()
        eng.profile(False)
        eng.copy_probe(False)
    def twin(k):      # name of the kernel a copy-only twin stands for
        if k.startswith("lde_copy_probe_a"):
            return k.replace("lde_copy_probe_a", "lde_a_kernel")
        if k == "lde_copy_probe_b":
            return "lde_b_kernel"
        cols = k.replace("ntt_copy_probe", "ntt_pass_cols_kernel")   # the pass ran as the column-sharing kernel (csrc/ntt.hip)
        return cols if cols in kernels else k.replace("ntt_copy_probe", "ntt_pass_kernel")
    probe_ms = {twin(k): v["total_ms"] / v["launches"] for k, v in probes.items()}
    ntt_ms = sum(k["total_ms"] for k in kernels.values()) / all_steps
    roofline = {"bound": "hbm", "kernel": dom_name, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": "profiles/pmc_traffic.json (rocprofv3 --pmc, earlier run of the same command)",
                "avg_launch_ms": avg_ms,
                "avg_launch_ms_note": ("its share of the step, every kernel of the step bracketed by events alone in turn, x un-instrumented ms_per_step (kernels abut in the loop)"
                                       if alone_step_ms else "share of the event-bracketed step x un-instrumented ms_per_step (kernels abut in the loop)"),
                "avg_launch_ms_every_launch_bracketed": bracketed_ms, "avg_launch_ms_only_this_kernel_bracketed": alone_ms,
                "avg_launch_ms_share_of_all_bracketed_step": share_ms,
                "alg_bytes_per_launch": bytes_per_launch,
                # whole-LDE view: SURVEY 8(d) (12+4B)*n*4 cols algorithmic bytes over the step's kernel time
                "step_alg_bytes": (12 + 4 * (1 << LOG_BLOWUP)) * n * N_COLS,
                # one clock for both: the headline's un-instrumented ms_per_step (step_frac = step_achieved / peak)
                "step_achieved": (12 + 4 * (1 << LOG_BLOWUP)) * n * N_COLS / (elapsed / args.steps) / 1e9,
                "step_frac": (12 + 4 * (1 << LOG_BLOWUP)) * n * N_COLS / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
                # the same bytes over the sum of the event-bracketed kernel durations of a step (a higher clock, see kernels_note)
                "step_achieved_bracketed_kernel_sum": (12 + 4 * (1 << LOG_BLOWUP)) * n * N_COLS / (ntt_ms * 1e-3) / 1e9,
                "step_traffic": step_traffic,
                # the same launch as a pure copy (no arithmetic): the ceiling of this access pattern
                "pattern_copy_GBps": (bytes_per_launch / (probe_ms[dom_name] * 1e-3) / 1e9) if dom_name in probe_ms else None,
                "frac_of_pattern_copy": (probe_ms[dom_name] / bracketed_ms) if dom_name in probe_ms else None,   # both bracketed
                "kernels_note": "per-kernel times with every launch bracketed by events (shorter than in the loop)",
                "kernels": {k: {"launches": v["launches"], "avg_ms": v["total_ms"] / v["launches"],
                                "GBps": v["alg_bytes"] / (v["total_ms"] * 1e-3) / 1e9,
                                "copy_only_ms": probe_ms.get(k)} for k, v in kernels.items()}}

    result["roofline"] = roofline
    if sustained is not None:
        result["sustained"] = sustained
    if burst is not None:
        result["burst"] = burst
    if precond is not None:
        result["preconditioning"] = precond

    # The headline line must survive anything the extra legs do: a watchdog thread prints what has
    # been measured so far and exits NON-ZERO if an extra (e.g. a collective on a flaky peer) hangs;
    # `stage` names the leg that was in flight.
    import threading
    lock = threading.Lock()
    stage = {"name": "start"}

    class Locked(dict):              # the main thread's writes and the watchdog's snapshot never interleave
        def __setitem__(self, k, v):
            with lock:
                dict.__setitem__(self, k, v)
    result = Locked(result)

    def enter(name):
        with lock:
            stage["name"] = name

    def _bail():
        with lock:
            snap = dict(result)
            snap["extras_timeout"] = True
            snap["extras_timeout_stage"] = stage["name"]
        if rank == 0:
            print(json.dumps(snap, default=str), flush=True)
        os._exit(3)

    class SelfCheckFailed(Exception):
        pass
    selfcheck_failed = False

    watchdog = threading.Timer(420.0, _bail)
    watchdog.daemon = True
    watchdog.start()

    if not args.no_extras:
        # ---- end-to-end prove of the same trace (build-defined composition)
        enter("prove")
        try:
            for _ in range(2):   # warm-up: the first call sizes the device arena, the second allocates it
                eng.dev_stark_prove(trace.data_ptr(), N_COLS, LOG_ROWS, LOG_BLOWUP, N_TESTS)
            # nine timed proves, each between its own synchronisations; prove_ms = the median's wall time (host call to
            # proof bytes on the host), stage times from the same prove
            runs = []
            for _ in range(9):
                barrier()
                torch.cuda.synchronize()
                tp = time.perf_counter()
                res_k = eng.dev_stark_prove(trace.data_ptr(), N_COLS, LOG_ROWS, LOG_BLOWUP, N_TESTS, timed=True)
                runs.append((1e3 * (time.perf_counter() - tp), res_k))
            runs.sort(key=lambda x: x[0])
            prove_ms, res = runs[len(runs) // 2]
            result["prove_ms_all"] = [x[0] for x in runs]
            if distributed:
                tt = torch.tensor([prove_ms], dtype=torch.float64, device=dev)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                prove_ms = float(tt.item())
            result["prove_ms"] = prove_ms                       # every rank proves its own trace (weak scaling)
            result["proofs_per_s"] = world * 1e3 / prove_ms
            result["prove_stage_ms"] = res["stage_ms"]
            result["prove_proof_bytes"] = len(res["proof"])
            # the prove on its own roofline: integer VALU (in-run ceiling of the bare permutation) and HBM
            enter("prove_roofline")
            ceiling = eng.mix_probe(512)
            eng.profile(True)
            eng.dev_stark_prove(trace.data_ptr(), N_COLS, LOG_ROWS, LOG_BLOWUP, N_TESTS)
            pk = eng.profile_read()
            eng.profile(False)
            result["prove_roofline"] = hash_roofline(pk, ceiling, res["stage_ms"], N, N_COLS)
        except Exception as e:  # reported, never hidden
            result["prove_error"] = str(e)
        # build-defined variant: one tree over the rows of the extended trace instead
        # of one per column -- four columns are one 32-byte chunk, so the commit costs a quarter
        enter("prove_row_leaves")
        try:
            eng.dev_stark_prove(trace.data_ptr(), N_COLS, LOG_ROWS, LOG_BLOWUP, N_TESTS, row_leaves=True)
            torch.cuda.synchronize()
            tp = time.perf_counter()
            res = eng.dev_stark_prove(trace.data_ptr(), N_COLS, LOG_ROWS, LOG_BLOWUP, N_TESTS, timed=True, row_leaves=True)
            result["prove_row_leaves_ms"] = 1e3 * (time.perf_counter() - tp)
            result["prove_row_leaves_stage_ms"] = res["stage_ms"]
        except Exception as e:
            result["prove_row_leaves_error"] = str(e)

        # ---- BASELINE configs[1]: 2^20-point forward + inverse on the reference prime
        enter("ntt_2p20 / cfg3")
        if rank == 0:
            e1 = s.Engine(s.P_REF, s.G_REF, local_rank)
            x = torch.from_numpy((splitmix64(2, 1 << 20) % np.uint64(s.P_REF)).astype(np.uint32).view(np.int32)).to(dev)
            y = torch.empty_like(x)
            for _ in range(5):
                e1.dev_ntt(x.data_ptr(), y.data_ptr(), 20, inverse=True)
                e1.dev_ntt(y.data_ptr(), x.data_ptr(), 20)
            torch.cuda.synchronize()
            reps = 200
            t1 = time.perf_counter()
            for _ in range(reps):
                e1.dev_ntt(x.data_ptr(), y.data_ptr(), 20, inverse=True)
                e1.dev_ntt(y.data_ptr(), x.data_ptr(), 20)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            us20 = 1e6 * dt / (2 * reps)
            result["ntt_2p20"] = {"field_elements_per_s": 2 * reps * (1 << 20) / dt, "us_per_transform": us20, "prime": s.P_REF,
                                  # 8 n algorithmic bytes per transform; two launches of ~7 us each: latency, not bandwidth
                                  "alg_bytes_per_transform": 8 << 20, "achieved_GBps": (8 << 20) / (us20 * 1e-6) / 1e9,
                                  "frac": (8 << 20) / (us20 * 1e-6) / 1e9 / HBM_PEAK_GBS, "bound_note": "launch latency (two passes of one wave of workgroups each)"}
            # ---- BASELINE configs[2]: 2^20-row x 4-column trace, LDE at blowup 8 + Merkle commit, on the
            # reference prime (N = 2^23 is its largest domain); the stage times of the prove over it
            try:
                tr = torch.from_numpy(np.concatenate([(splitmix64(0x5354524B00 + c, 1 << 20) % np.uint64(s.P_REF)).astype(np.uint32)
                                                      for c in range(N_COLS)]).view(np.int32)).to(dev)
                for _ in range(2):
                    e1.dev_stark_prove(tr.data_ptr(), N_COLS, 20, LOG_BLOWUP, N_TESTS)
                r3 = e1.dev_stark_prove(tr.data_ptr(), N_COLS, 20, LOG_BLOWUP, N_TESTS, timed=True)
                c3 = {"prime": s.P_REF, "lde_ms": r3["stage_ms"]["lde"], "commit_ms": r3["stage_ms"]["commit"],
                      "prove_ms": sum(r3["stage_ms"].values())}
                n3 = 1 << 20
                lde_bytes3 = (12 + 4 * (1 << LOG_BLOWUP)) * n3 * N_COLS                       # (12 + 4B) n per column
                c3["lde_frac"] = lde_bytes3 / (c3["lde_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
                ceil3 = e1.mix_probe(512)
                e1.profile(True)
                e1.dev_stark_prove(tr.data_ptr(), N_COLS, 20, LOG_BLOWUP, N_TESTS)
                pk3 = e1.profile_read()
                e1.profile(False)
                hr3 = hash_roofline(pk3, ceil3, r3["stage_ms"], n3 << LOG_BLOWUP, N_COLS)
                if hr3:
                    c3["commit_frac_valu"] = hr3["commit"]["frac"]
                    c3["commit_frac_hbm"] = hr3["commit"]["hbm_frac"]
                    c3["prove_roofline"] = {k: hr3[k] for k in ("kernel", "achieved", "peak", "frac", "unit", "hbm", "whole_prove", "commit")}
                result["cfg3_2p20x4_blowup8"] = c3
            except Exception as e:
                result["cfg3_error"] = str(e)
            e1.close()

        # ---- one codeword / one trace over the N GPUs through the native multi-GPU entry points
        # (smi_mgpu_*: round loop, kernels and RCCL collectives inside libstarkmi.so)
        enter("mgpu fri / prove")
        if distributed:
          try:
            from stark_rs_amd.mgpu import HipMem, HostCollectives, MultiGpu
            logN = LOG_ROWS + LOG_BLOWUP
            blk = (1 << logN) // world
            # blocks below 2^18 elements are gathered: from there a round is hash latency, not throughput
            host, mg, why = None, None, ""
            if backend == "nccl" or os.environ.get("SMI_BENCH_TRY_RCCL"):
                try:
                    mg = MultiGpu(eng, rank, world, min_block=1 << 18)
                except Exception as e:
                    why = f"{type(e).__name__}: {e}"
                ok = torch.tensor([1 if mg is not None else 0], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
                dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                if not int(ok.item()) and mg is not None:
                    mg.close()
                    mg = None
            if mg is None:
                # rehearsal backend, or the in-library RCCL communicator could not be created on some rank: the same
                # prover over the host shim (staged through host memory -- slow, and labelled as such below)
                grp = dist.new_group(backend="gloo") if backend == "nccl" else None
                host = HostCollectives(rank, world, HipMem(), group=grp)
                mg = MultiGpu(eng, rank, world, host=host, min_block=1 << 18)
                if why or backend == "nccl":
                    result["mgpu_rccl_unavailable"] = why or "communicator failed on another rank"
            omega = eng.prim_nth_root(1 << logN)
            coll_kind = "rccl (in-library)" if host is None else "host shim (staged through host memory)"
            result["mgpu_collectives"] = coll_kind
            # Self-checks before anything is timed (the first multi-GPU run on real links must not report numbers for
            # wrong results): each compares a multi-GPU entry point with the single-GPU one on the same input, on every
            # rank; a mismatch on ANY rank is recorded, every rank skips the multi-GPU legs, the headline line is still
            # printed and the process exits non-zero at the end (never os._exit in the middle of a collective sequence).
            checks = {}
            # (1) Fri::prove of a 2^20-point codeword: sharded proof == single-GPU proof, byte for byte
            chk_n = 1 << 20
            chk = (splitmix64(11, chk_n) % np.uint64(p)).astype(np.uint32)
            cfg_c = eng.fri_cfg(eng.prim_nth_root(chk_n), s.G2, chk_n, 1 << LOG_BLOWUP, N_TESTS)
            d_part = torch.from_numpy(chk[rank * (chk_n // world):(rank + 1) * (chk_n // world)].view(np.int32).copy()).to(dev)
            got, got_top = mg.fri_prove(cfg_c, d_part.data_ptr(), chk_n // world)
            d_all = torch.from_numpy(chk.view(np.int32).copy()).to(dev)
            want = eng.dev_fri_prove(cfg_c, d_all.data_ptr(), chk_n)
            checks["fri_prove_2p20"] = bytes(want[0]) == got and list(want[1]) == got_top
            # (2) the sharded extension of a 2^18 x 4 trace: this rank's block of every column == the same block of smi_dev_lde
            ln_c, n_c = 18, 1 << 18
            N_c = n_c << LOG_BLOWUP
            tr_c = torch.from_numpy(np.concatenate([(splitmix64(21 + c, n_c) % np.uint64(p)).astype(np.uint32) for c in range(N_COLS)]).view(np.int32)).to(dev)
            ref_c = torch.empty(N_COLS * N_c, dtype=torch.int32, device=dev)
            eng.dev_lde(tr_c.data_ptr(), N_COLS, ln_c, LOG_BLOWUP, ref_c.data_ptr())
            blk_c = N_c // world
            got_c = torch.empty(N_COLS * blk_c, dtype=torch.int32, device=dev)
            mg.lde(tr_c.data_ptr(), N_COLS, ln_c, LOG_BLOWUP, got_c.data_ptr())
            torch.cuda.synchronize()
            checks["lde_2p18x4"] = bool(torch.equal(got_c.view(N_COLS, blk_c), ref_c.view(N_COLS, N_c)[:, rank * blk_c:(rank + 1) * blk_c]))
            # (3) one 2^22-point transform over the ranks == smi_dev_ntt of the same input (natural order, this rank's block)
            L_c = 22
            x_c = (splitmix64(31, 1 << L_c) % np.uint64(p)).astype(np.uint32)
            r0 = 1 << mg.ntt_first_digit(L_c)
            B_c = (1 << L_c) // r0
            strip_c = torch.from_numpy(np.ascontiguousarray(x_c.reshape(r0, B_c)[:, rank * (B_c // world):(rank + 1) * (B_c // world)]).reshape(-1).view(np.int32)).to(dev)
            out_c = torch.empty((1 << L_c) // world, dtype=torch.int32, device=dev)
            mg.ntt(strip_c.data_ptr(), out_c.data_ptr(), L_c, offset=s.G2, natural=True)
            full_c = torch.from_numpy(x_c.view(np.int32).copy()).to(dev)
            want_c = torch.empty_like(full_c)
            eng.dev_ntt(full_c.data_ptr(), want_c.data_ptr(), L_c, offset=s.G2)
            torch.cuda.synchronize()
            per_c = (1 << L_c) // world
            checks["ntt_2p22_natural_block"] = bool(torch.equal(out_c, want_c[rank * per_c:(rank + 1) * per_c]))
            del tr_c, ref_c, got_c, strip_c, out_c, full_c, want_c, d_all, d_part
            ok_all = torch.tensor([1 if all(checks.values()) else 0], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(ok_all, op=dist.ReduceOp.MIN)
            if not int(ok_all.item()):
                bad = [k for k, v in checks.items() if not v]
                result["mgpu_selfcheck"] = "MISMATCH" + (f" on this rank: {bad}" if bad else " on another rank")
                print(f"bench.py: rank {rank}: multi-GPU self-check failed: {bad or 'another rank'}", file=sys.stderr, flush=True)
                mg.close()
                raise SelfCheckFailed()
            result["mgpu_selfcheck"] = ("every rank: sharded Fri::prove of a 2^20 codeword == single-GPU proof bytes; smi_mgpu_lde 2^18 x 4 block == "
                                        "smi_dev_lde; smi_mgpu_ntt 2^22 natural-order block == smi_dev_ntt")
            # BASELINE configs[3]: ONE 2^26-point transform over the N GPUs (strong scaling): pass 0 on column
            # strips, one all-to-all over xGMI, the remaining passes (smi_mgpu_ntt)
            enter("four_step_2p26")
            L26 = 26
            strip = torch.from_numpy((splitmix64(4 + rank, (1 << L26) // world) % np.uint64(p)).astype(np.uint32).view(np.int32)).to(dev)
            work, out26 = torch.empty_like(strip), torch.empty_like(strip)
            work.copy_(strip)
            mg.ntt(work.data_ptr(), out26.data_ptr(), L26)
            torch.cuda.synchronize()
            barrier()
            reps, dt = 10, 0.0
            for _ in range(reps):
                work.copy_(strip)                 # the transform clobbers its strip; the refill is outside the clock
                torch.cuda.synchronize()
                barrier()
                t1 = time.perf_counter()
                mg.ntt(work.data_ptr(), out26.data_ptr(), L26)
                torch.cuda.synchronize()
                barrier()
                dt += time.perf_counter() - t1
            tt = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            result["four_step_2p26"] = {"field_elements_per_s": reps * (1 << L26) / float(tt.item()),
                                        "ms_per_transform": 1e3 * float(tt.item()) / reps, "scaling": "strong",
                                        "path": "pass pipeline + one all-to-all (smi_mgpu_ntt)", "collectives": coll_kind}
            del strip, work, out26
            enter("mgpu fri / prove")
            # Fri::prove of one 2^25-point codeword
            block = torch.from_numpy((splitmix64(9 + rank, blk) % np.uint64(p)).astype(np.uint32).view(np.int32)).to(dev)
            cfg25 = eng.fri_cfg(omega, s.G2, 1 << logN, 1 << LOG_BLOWUP, N_TESTS)
            mg.fri_prove(cfg25, block.data_ptr(), blk)
            torch.cuda.synchronize()
            barrier()
            t1 = time.perf_counter()
            proof, _top = mg.fri_prove(cfg25, block.data_ptr(), blk)
            torch.cuda.synchronize()
            barrier()
            dt = time.perf_counter() - t1
            tt = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            result["sharded_fri_prove_2p25_ms"] = 1e3 * float(tt.item())
            result["sharded_fri_prove_bytes"] = len(proof)
            result["sharded_fri_prove_collectives"] = coll_kind
            # BASELINE configs[4]: the full prove of ONE 2^22 x 4 trace over the N GPUs (strong scaling):
            # extension sharded by (column, coset) units, column trees and FRI by blocks of leaves
            one = torch.from_numpy(np.concatenate([(splitmix64(0x5354524B00 + c, n) % np.uint64(p)).astype(np.uint32)
                                                   for c in range(N_COLS)]).view(np.int32)).to(dev)
            for _ in range(2):
                mg.stark_prove(one.data_ptr(), N_COLS, LOG_ROWS, LOG_BLOWUP, N_TESTS)
            torch.cuda.synchronize()
            barrier()
            t1 = time.perf_counter()
            _roots, sproof, _top = mg.stark_prove(one.data_ptr(), N_COLS, LOG_ROWS, LOG_BLOWUP, N_TESTS)
            torch.cuda.synchronize()
            barrier()
            dt = time.perf_counter() - t1
            tt = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            result["sharded_prove_2p22x4_ms"] = {"value": 1e3 * float(tt.item()), "scaling": "strong", "proof_bytes": len(sproof),
                                                 "collectives": coll_kind}
            mg.close()
          except SelfCheckFailed:
            selfcheck_failed = True
          except Exception as e:
            import traceback
            result["sharded_fri_error"] = f"{type(e).__name__}: {e} | {traceback.format_exc(limit=3)}"

        # the CPU path beside the GPU numbers, at any world size: rank 0's host cores, one thread (the other ranks
        # wait for it at the process group's teardown)
        enter("cpu_baseline")
        watchdog.cancel()          # the GPU legs are over: the CPU leg cannot hang on a peer, and its ~15 s must not count against them
        if rank == 0:
            try:
                result["cpu_baseline"] = cpu_baseline()
            except Exception as e:
                result["cpu_baseline_error"] = f"{type(e).__name__}: {e}"

    watchdog.cancel()
    if rank == 0:
        print(json.dumps(result), flush=True)
    eng.close()
    if distributed:
        dist.destroy_process_group()
    if selfcheck_failed:
        sys.exit(4)


if __name__ == "__main__":
    main()
