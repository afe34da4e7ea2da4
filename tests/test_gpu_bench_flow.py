"""The multi-process bench flow (what the driver launches for N > 1): two ranks on this box's single GPU
over gloo — barrier, timed steps with the bucketed gradient all-reduce, profile pass on every rank, one
JSON line from rank 0.  (A collective executed by rank 0 only used to dead-lock this flow.)
Also: `bench.py --gpus 2` WITHOUT a torchrun environment must start the two ranks itself, a world size that
differs from --gpus must fail, and strong scaling must shard a fixed total."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _line(res):
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _clean_env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(kw)
    return env


def test_two_rank_bench_line(gpu_device):
    env = _clean_env(NMRGNN_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29533", BENCH,
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--graphs", "16"]
    d = _line(subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240))
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert "roofline" in d and "cpu_baseline" not in d
    assert d["config"]["backend"] == "gloo" and d["config"]["atoms_total"] == 2 * 16 * 256
    assert d["rank_ms_per_step"]["max"] >= d["rank_ms_per_step"]["min"] > 0 and d["allreduce_exposed_ms"] >= 0


def test_gpus_flag_without_torchrun_starts_the_ranks_itself(gpu_device):
    """`python bench.py --gpus 2` (no torchrun): re-executes under torch.distributed.run with 2 ranks; strong scaling
    over a fixed total of 24 graphs -> 12 per rank"""
    env = _clean_env(NMRGNN_DIST_BACKEND="gloo")
    cmd = [sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1", "--scaling", "strong",
           "--total-graphs", "24", "--no-profile"]
    d = _line(subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240))
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert d["config"]["atoms_total"] == 24 * 256 and d["config"]["atoms_this_rank"] == 12 * 256


def test_four_rank_strong_scaling_form(gpu_device):
    """the form the driver launches on an 8-GPU node (BASELINE configs[3]: `--gpus 8 --scaling strong --total-graphs 4096`
    under torch.distributed.run) with FOUR ranks sharing the box's one GPU over gloo (four ranks plus this process: at most
    six processes may hold one GPU open), with a small uneven total so that the run stays short: shard sizes, one JSON
    line, exit code 0, every rank through barrier / timed steps / profile pass / destroy"""
    env = _clean_env(NMRGNN_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4",
           "--master-addr", "127.0.0.1", "--master-port", "29536", BENCH,
           "--gpus", "4", "--steps", "2", "--warmup", "1", "--scaling", "strong", "--total-graphs", "102"]
    d = _line(subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600))
    assert d["n_gpus"] == 4 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["atoms_total"] == 102 * 256
    # parallel.shard_range(102, 0, 4): the first 102 % 4 = 2 ranks hold 26 graphs, the others 25
    assert d["config"]["atoms_this_rank"] == 26 * 256
    assert d["config"]["world_size"] == 4 and d["config"]["backend"] == "gloo"
    assert d["config"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert d["rank_ms_per_step"]["max"] >= d["rank_ms_per_step"]["min"] > 0


def test_world_size_mismatch_is_an_error(gpu_device):
    env = _clean_env(NMRGNN_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29534", BENCH,
           "--gpus", "4", "--steps", "1", "--warmup", "0", "--graphs", "4"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode != 0
    assert "WORLD_SIZE=2" in res.stderr


def test_nccl_is_required_unless_overridden(gpu_device):
    """two ranks on ONE GPU cannot form an RCCL communicator: without the explicit gloo override the bench refuses"""
    env = _clean_env()
    env.pop("NMRGNN_DIST_BACKEND", None)
    res = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0", "--graphs", "4"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    import torch
    if torch.cuda.device_count() < 2:
        assert res.returncode != 0


def test_single_rank_bench_line_has_all_fields(gpu_device):
    res = subprocess.run([sys.executable, BENCH, "--steps", "2", "--warmup", "1", "--graphs", "16",
                          "--no-cpu-baseline"], cwd=ROOT, env=_clean_env(), capture_output=True, text=True, timeout=600)
    d = _line(res)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "ms_per_step_hipevent_median", "preprocess_ms",
              "inference", "fp32_mfma_only", "f256", "configs4"):
        assert k in d, k
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(d["roofline"])
    assert "error" not in d["f256"] and "error" not in d["configs4"], (d["f256"], d["configs4"])
    assert d["f256"]["value"] > 0 and d["configs4"]["knn16_padded_50_frames_per_call"]["value"] > 0


def test_dump_outputs_hold_the_last_timed_step(gpu_device, tmp_path):
    """--dump-outputs DIR: the loss, parameters and gradients of the LAST timed step as float .npy files (under 64 MB).
    The same arguments give the same inputs and the engine is bitwise reproducible, so warmup 1 + 2 timed steps and
    warmup 2 + 1 timed step end on the same third optimiser step and dump the same arrays; a run one step shorter differs."""
    import numpy as np

    def run(tag, warmup, steps):
        out = tmp_path / tag
        res = subprocess.run([sys.executable, BENCH, "--steps", str(steps), "--warmup", str(warmup), "--graphs", "16",
                              "--no-cpu-baseline", "--no-profile", "--no-extras", "--dump-outputs", str(out)],
                             cwd=ROOT, env=_clean_env(), capture_output=True, text=True, timeout=240)
        d = _line(res)
        assert d["steps"] == steps and d["ms_per_step"] > 0
        arrs = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
        assert all(f.endswith(".npy") for f in os.listdir(out))
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert d["dump_outputs"]["arrays"] == len(arrs)
        assert float(arrs["loss"][0]) == d["loss"]
        return arrs

    a = run("a", 1, 2)
    names = [k for k in a if k.startswith("param.")]
    assert names and sorted("grad." + k[6:] for k in names) == sorted(k for k in a if k.startswith("grad."))
    assert any(np.abs(a[k]).max() > 0 for k in a if k.startswith("grad."))
    c = run("c", 2, 1)
    assert sorted(a) == sorted(c)
    for k in a:
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
    short = run("short", 1, 1)
    assert short["loss"][0] != a["loss"][0]
    assert any(not np.array_equal(short[k], a[k]) for k in names)
