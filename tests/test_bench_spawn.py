"""bench.py honours --gpus N by itself (the driver's invocation form): without a launcher it re-launches under
torch.distributed.run with N ranks, rendezvous on 127.0.0.1, and rank 0 prints ONE JSON line with n_gpus = N.
--dry-run keeps the launcher / barrier / max-over-ranks / JSON plumbing and skips the GPU work, so this runs on CPU (gloo)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_gpus_2_spawns_two_ranks():
    r = run(["--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1", "--batch", "4"])
    assert r["n_gpus"] == 2 and r["steps"] == 3 and r["warmup"] == 1
    assert r["config"]["global_batch"] == 8 and r["scaling"] == "weak"
    assert r["value"] > 0 and r["ms_per_step"] > 0
    assert r["ranks"]["world_size_seen_by_backend"] == 2 and r["ranks"]["ms_per_step_min"] <= r["ranks"]["ms_per_step_max"]
    assert abs(r["ranks"]["ms_per_step_max"] - r["ms_per_step"]) < 1e-2          # the line's time is the slowest rank's


def test_single_rank_default():
    r = run(["--dry-run", "--steps", "2", "--warmup", "0"])
    assert r["n_gpus"] == 1


@pytest.mark.gpu
def test_gpus_2_with_real_kernels_on_one_gpu():
    """The N-rank path on hardware: `bench.py --gpus 2` respawns under torch.distributed.run, both ranks rendezvous (gloo: a 1-GPU box has no second
    device for RCCL) and run the real detector on cuda:0 (--share-gpu), frames sharded by rank, barrier-bracketed timed loop, max over ranks, ONE JSON
    line from rank 0 -- plus one DDP + SyncBN training step (2 x 1 frame) through the same process group.  The short N > 1 form: no Waymo / uniform legs."""
    r = run(["--gpus", "2", "--backend", "gloo", "--share-gpu", "--batch", "2", "--steps", "2", "--warmup", "1", "--full"],
            {"PNX_BENCH_TRAIN_FRAMES": "1", "PNX_BENCH_TRAIN_STEPS": "1", "PNX_BENCH_TRAIN_WARMUP": "1", "MIOPEN_FIND_MODE": "2"}, timeout=900)
    assert r["n_gpus"] == 2 and r["steps"] == 2 and r["config"]["global_batch"] == 4 and r["config"]["parallelism"] == "frame-sharded replicas x2"
    assert r["ranks"]["world_size_seen_by_backend"] == 2 and r["ranks"]["ms_per_step_min"] <= r["ranks"]["ms_per_step_max"]
    assert abs(r["ms_per_step"] - r["ranks"]["ms_per_step_max"]) < 1e-2               # value uses the slowest rank
    assert r["value"] > 0 and r["roofline"]["frac"] > 0 and r["detections_last_step"] > 0
    assert "value_uniform" not in r and "value_c4" not in r                           # short form
    assert r["value_train"] > 0 and r["train"]["loss_finite"] and "DDP" in r["train"]["step"]
    # one MIOpen mode per line, the same at every N: the N = 2 line says which, and what an efficiency is computed from
    assert r["ranks"]["miopen"]["train"].startswith("immediate") and r["train"]["miopen"].startswith("immediate") and r["ranks"]["miopen"]["inference"].startswith("find")
    assert r["efficiency_basis"]["train"] == "value_train(N) / (N x value_train(1))" and r["efficiency_basis"]["frames_per_gpu_per_step"] == {"inference": 2, "train": 1}


@pytest.mark.gpu
def test_dump_outputs_holds_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the detections of the timed loop's last step as .npy files (float32 / float64), whose rows add up to the line's count."""
    import numpy as np

    r = run(["--batch", "2", "--steps", "3", "--warmup", "1", "--no-extras", "--no-back-to-back", "--dump-outputs", str(tmp_path)],
            {"PNX_NO_MIOPEN_BENCH": "1"}, timeout=900)
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    names = ("box3d_lidar", "scores", "label_preds", "frame_counts")
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(k + ".npy" for k in names)
    d = {k: np.load(tmp_path / (k + ".npy")) for k in names}
    n = int(d["frame_counts"].sum())
    assert d["frame_counts"].shape == (2,) and d["frame_counts"].dtype == np.float64 and n == r["detections_last_step"] > 0
    assert d["box3d_lidar"].shape == (n, 9) and d["box3d_lidar"].dtype == np.float32 and np.isfinite(d["box3d_lidar"]).all()
    assert d["scores"].shape == (n,) and d["scores"].dtype == np.float32 and np.isfinite(d["scores"]).all()
    assert d["label_preds"].shape == (n,) and d["label_preds"].dtype == np.float64 and np.array_equal(d["label_preds"], np.round(d["label_preds"]))


@pytest.mark.gpu
def test_plain_run_is_the_timed_loop_only():
    """Without --full the run is set-up, warm-up, the timed steps and the line: none of the legs that take runs of their own."""
    r = run(["--batch", "2", "--steps", "2", "--warmup", "1"], {"PNX_NO_MIOPEN_BENCH": "1"}, timeout=900)
    assert r["value"] > 0 and r["ms_per_step"] > 0 and r["unit"] == "frames/s" and r["higher_is_better"] and r["dtype"] == "bf16"
    assert r["roofline"]["frac"] > 0 and r["roofline"]["back_to_back"] is None and r["cpu_baseline"] is None and r["detections_last_step"] > 0
    legs = ("value_uniform", "value_with_h2d_merge", "value_c4", "value_c5", "value_train", "value_train_fp32", "sections_us", "nms_us", "roofline_backbone")
    assert not [k for k in legs if k in r]


@pytest.mark.gpu
def test_gpus_2_over_rccl_when_two_devices_are_visible():
    """The same line over RCCL (backend nccl, one rank per GPU): runs wherever >= 2 devices are visible -- the boxes this repository is developed on have
    one, so there it skips and the gloo form above is what exercises the N-rank path."""
    torch = pytest.importorskip("torch")
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (RCCL refuses two ranks on one device)")
    r = run(["--gpus", "2", "--backend", "nccl", "--batch", "2", "--steps", "2", "--warmup", "1", "--full"],
            {"PNX_BENCH_TRAIN_FRAMES": "1", "PNX_BENCH_TRAIN_STEPS": "1", "PNX_BENCH_TRAIN_WARMUP": "1", "MIOPEN_FIND_MODE": "2", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}, timeout=1200)
    assert r["n_gpus"] == 2 and r["ranks"]["backend"] == "nccl" and r["ranks"]["world_size_seen_by_backend"] == 2
    assert r["value"] > 0 and r["value_train"] > 0 and r["train"]["loss_finite"]
    assert r["ranks"]["miopen"]["train"].startswith("immediate")
