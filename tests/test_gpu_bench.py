"""bench.py's N > 1 code path on ONE GPU: two ranks launched the way the driver launches them (torch.distributed.run), sharing
the device through the SPVO_BENCH_SHARED_GPU test hook (gloo process group, the C ABI's file transport for the pose gather --
RCCL refuses two ranks on one device).  Exercises what a multi-GPU run adds to the step loop: per-rank streams, the batched pose
all-gather inside the timed region, barrier, max-over-ranks timing, rank 0's single JSON line."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_share_one_gpu():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, SPVO_BENCH_SHARED_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "40", "--warmup", "5", "--no-cpu-baseline", "--no-extras"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # rank 0 prints ONE JSON line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 40 and out["scaling"] == "weak" and out["value"] > 0
    assert abs(out["value"] - 2 * 40 / (out["ms_per_step"] * 40 / 1e3)) < 0.02 * out["value"]   # whole-job rate = all ranks' frames / max time
    assert "file transport" in out["config"]["pose_gather"]
    assert out["config"]["streams"] == 2


def test_gpus_flag_spawns_the_ranks_itself():
    """`python bench.py --gpus 2` with no launcher and no WORLD_SIZE: bench.py starts the two ranks itself (fresh child
    interpreters, started before anything touches the GPU) and rank 0 prints the one JSON line with n_gpus = 2."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SPVO_BENCH_SHARED_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", "--repeats", "3", "--no-cpu-baseline", "--no-extras"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 20 and out["repeats"] == 3 and out["value"] > 0
    assert out["ms_per_step_min"] <= out["ms_per_step"] <= out["ms_per_step_max"]
    assert out["config"]["streams"] == 2


def test_headline_workload_needs_no_host_driven_nms_continuation():
    """bench.py's headline workload (seeded VGG weights at 360x1176: denser heat maps than the trained graphs') through the pipelined
    loop: every heat map's suppression settles inside the launches enqueued with the submission (three round launches + the
    finishing kernel).  A continuation by the host (spvo_detect_wait -> nms_settle) waits behind everything queued on the tail
    stream; with three round launches alone it ran on 7 % of the frames and cost the headline 6 %."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "60", "--warmup", "10", "--repeats", "2", "--full", "--no-cpu-baseline", "--no-extras"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["nms_host_continuations"] == {"timed_region": 0, "timed_steps": 120}
    assert out["roofline"]["frac"] > 0.3 and out["value"] > 0


def test_plain_run_times_the_steps_once_and_dumps_the_same_outputs_every_time(tmp_path):
    """A plain `bench.py --steps N --warmup W` times exactly N steps in one block, leaves out what only --full measures, and with
    --dump-outputs writes what the last timed step computed as float .npy files: identical from run to run (seeded inputs)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    dumps = []
    for run in range(2):
        d = tmp_path / f"out{run}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 30 and out["repeats"] == 1 and out["value"] > 0 and out["dtype"] == "f32" and out["higher_is_better"] is True
        assert abs(out["value"] - 1e3 / out["ms_per_step"]) < 0.01 * out["value"]
        for moved in ("roofline", "stages_ms", "nms_host_continuations", "cpu_baseline", "host_interface", "other_configs", "ate"):
            assert moved not in out, moved
        files = sorted(p.name for p in d.iterdir())
        assert files == sorted(f"{n}.npy" for n in ("pose", "solver_outcome", "keypoints_left", "keypoints_right", "pnp_inliers", "stereo_matches", "temporal_matches"))
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert arrays["solver_outcome.npy"][0] == 1 and arrays["keypoints_left.npy"].shape[1] == 2 and len(arrays["stereo_matches.npy"]) > 0
        dumps.append(arrays)
    for f, a in dumps[0].items():
        assert np.array_equal(a, dumps[1][f]), f
