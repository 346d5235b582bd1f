"""CPU: the host-side arithmetic of bench.py that needs no GPU -- the prove's roofline block from per-kernel records,
the launcher's refusal to mislabel a run, its options, --dump-outputs on a host tensor, and the synthetic-input
generator against the oracle's.  One GPU test: a plain run's line and dump against the oracle."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_splitmix64_is_the_surveys_generator(oracle):
    b = _bench()
    for seed in (1, 2, 0x5354524B00, 2 ** 63 + 5):
        assert np.array_equal(b.splitmix64(seed, 1000), oracle.splitmix64(seed, 1000))


def test_hash_roofline_block_from_kernel_records():
    b = _bench()
    N, W = 1 << 25, 4
    # one prove: the leaf kernel of the column trees and of the first FRI rounds, the digest levels, the chunk kernel, an NTT pass
    kernels = {
        "merkle_sub_kernel<leaves>": {"launches": 7, "total_ms": 8.4, "alg_bytes": 1.2e10, "alg_mixes": 3.3e9},
        "merkle_sub_kernel<digests>": {"launches": 9, "total_ms": 1.45, "alg_bytes": 1.0e9, "alg_mixes": 4.7e8},
        "merkle_top_kernel": {"launches": 34, "total_ms": 0.8, "alg_bytes": 1e8, "alg_mixes": 4.9e7},
        "ntt_pass_kernel<8,5,last>": {"launches": 1, "total_ms": 0.23, "alg_bytes": 1.07e9, "alg_mixes": 0.0},
    }
    stage = {"lde": 0.72, "commit": 6.6, "combine": 0.02, "fri": 4.25}
    r = b.hash_roofline(kernels, 4.7e11, stage, N, W)
    assert r["kernel"] == "merkle_sub_kernel<leaves>" and r["bound"] == "valu" and r["unit"] == "mix_state/s"
    scale = sum(stage.values()) / sum(k["total_ms"] for k in kernels.values())           # the plain prove's clock
    assert abs(r["kernel_ms_per_prove"] - 8.4 * max(1.0, scale)) < 1e-9
    assert abs(r["frac"] - 3.3e9 / (r["kernel_ms_per_prove"] * 1e-3) / 4.7e11) < 1e-12
    assert abs(r["hbm"]["frac"] - 1.2e10 / (r["kernel_ms_per_prove"] * 1e-3) / 1e9 / b.HBM_PEAK_GBS) < 1e-12
    # N*9 + (N-1)*10 mix_state per tree, ~68 N bytes per tree
    assert r["commit"]["mixes"] == W * (19.0 * N - 10.0)
    assert abs(r["commit"]["hbm_frac"] - W * 68.0 * N / 6.6e-3 / 1e9 / b.HBM_PEAK_GBS) < 1e-12
    assert abs(r["whole_prove"]["mixes"] - (3.3e9 + 4.7e8 + 4.9e7)) < 1
    assert set(r["kernels"]) == {"merkle_sub_kernel<leaves>", "merkle_sub_kernel<digests>", "merkle_top_kernel"}
    json.dumps(r)                                                                          # the block goes into the JSON line
    assert b.hash_roofline({"ntt": {"launches": 1, "total_ms": 1.0, "alg_bytes": 1.0, "alg_mixes": 0.0}}, 4.7e11, stage, N, W) is None
    assert b.hash_roofline(kernels, 0.0, stage, N, W) is None


def test_bench_refuses_a_world_size_that_disagrees_with_gpus():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0"],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "refusing to mislabel" in out.stderr


def test_bench_rejects_a_step_count_below_one():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0", "--warmup", "0"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps" in out.stderr


def test_bench_offers_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout


def test_dump_outputs_writes_a_fixed_exact_sample(tmp_path, monkeypatch):
    """--dump-outputs on a host tensor: the same seeded rows every time (first and last included), float64 values equal to
    the u32 residues, exact per-column bit sums, rank suffixes, well under the 64 MB budget at the real size."""
    import torch
    b = _bench()
    assert (b.N_COLS + 1) * b.DUMP_ROWS * 8 + b.N_COLS * 2 * 8 <= 64 << 20       # sample + rows + sums, float64
    monkeypatch.setattr(b, "DUMP_ROWS", 64)
    n = 1 << 12
    host = (b.splitmix64(7, 4 * n) % np.uint64(469762049)).astype(np.uint32).reshape(4, n)
    lde = torch.from_numpy(host.view(np.int32))
    b.dump_outputs(str(tmp_path / "a"), lde)
    b.dump_outputs(str(tmp_path / "b"), lde, rank=1)
    rows = np.load(tmp_path / "a" / "lde_sample_rows.npy")
    sample = np.load(tmp_path / "a" / "lde_sample.npy")
    sums = np.load(tmp_path / "a" / "lde_column_sums.npy")
    assert rows.dtype == sample.dtype == sums.dtype == np.float64
    r = rows.astype(np.int64)
    assert len(r) == 64 and len(np.unique(r)) == 64 and r[0] == 0 and r[-1] == n - 1 and np.all(np.diff(r) > 0)
    assert np.array_equal(sample, host[:, r].astype(np.float64))
    h = host.astype(np.int64)
    assert np.array_equal(sums, np.stack([(h & 0xFFFF).sum(1), (h >> 16).sum(1)], 1).astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "b" / "lde_sample_rows_rank1.npy"), rows)
    assert np.array_equal(np.load(tmp_path / "b" / "lde_sample_rank1.npy"), sample)


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_extension(oracle, tmp_path):
    """A plain run: the headline keys, K timed steps, none of the --full legs; its dump is the oracle's extension of the
    synthetic trace (column 0 at the sampled rows) and its column sums."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["metric"] == "ntt_field_elements_per_sec" and r["unit"] == "field-elements/s" and r["higher_is_better"] is True
    assert r["dtype"] == "u32" and r["steps"] == 7 and r["warmup"] == 2 and r["ms_per_step"] > 0
    assert abs(r["value"] - r["config"]["points_per_step_per_gpu"] / (r["ms_per_step"] * 1e-3)) <= 1e-9 * r["value"]
    assert not {"roofline", "burst", "sustained", "prove_ms", "cpu_baseline"} & set(r)
    o = oracle
    P2, G2, logn, lb = 469762049, 3, 22, 3
    n, N = 1 << logn, 1 << (logn + lb)
    col0 = o.splitmix64(0x5354524B00, n) % np.uint64(P2)
    lde0 = o.fast_coset_ntt(o.fast_intt(col0, o.ff_prim_nth_root_g(n, P2, G2), 1, P2), N, o.ff_prim_nth_root_g(N, P2, G2), G2, P2)
    rows = np.load(tmp_path / "lde_sample_rows.npy").astype(np.int64)
    sample = np.load(tmp_path / "lde_sample.npy")
    assert sample.shape == (4, len(rows)) and np.array_equal(sample[0], lde0[rows].astype(np.float64))
    sums = np.load(tmp_path / "lde_column_sums.npy")
    l0 = lde0.astype(np.int64)
    assert sums[0, 0] == float((l0 & 0xFFFF).sum()) and sums[0, 1] == float((l0 >> 16).sum())
