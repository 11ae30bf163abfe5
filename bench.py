#!/usr/bin/env python3
"""bench.py -- stereo frames/s of the MI355X-native SuperPoint stereo-VO front end.

One "step" = one stereoCallback of the reference (visual_odometry_node.cpp:150-262):
addStereoImagePair (preprocess + VGG SuperPoint fp32 + post-processing of BOTH images),
matchDescriptors x2, solveStereoOdometry -> one 6-DoF relative pose, driven through the
C++ host mirror of FeatureFrontEnd over the C ABI (include/spvo.h).

Workload (BASELINE.json configs[1]): VGG SuperPoint fp32 (seeded synthetic weights with the
reference's exact 1 300 865-parameter layout: the real ones are missing from the reference
tree), 1241x376 KITTI-sized synthetic stereo pairs, network size 360x1176 (the reference's
largest), reference launch-file parameters.  Input images are resident in HBM before the timed
region.  N GPUs = N independent stereo streams, one rank per GPU (weak scaling); the only
collective is the all-gather of the 7-double poses over RCCL (batches of 64 frames, off the critical path).

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times exactly --steps steps in one block and prints the line
(--dump-outputs DIR: and writes what the last timed step computed); --full adds the repeated blocks, the per-kernel and roofline
figures, the informational legs and the CPU baseline.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "superpoint-stereo-visual-odometry_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def _early_cpu_limit(argv):
    """`--cpus N`: restrict the process to N CPUs before numpy / torch / HIP create their helper threads (they inherit the mask)."""
    for k, a in enumerate(argv):
        n = a.split("=", 1)[1] if a.startswith("--cpus=") else (argv[k + 1] if a == "--cpus" and k + 1 < len(argv) else None)
        if n and int(n) > 0 and hasattr(os, "sched_setaffinity"):
            os.sched_setaffinity(0, set(sorted(os.sched_getaffinity(0))[:int(n)]))


if __name__ == "__main__":
    _early_cpu_limit(sys.argv[1:])
    # The HIP runtime deals a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  A front end has three streams; the
    # FP16 / INT8 legs (BASELINE configs 3 and 5) run with a second tail stream (spvo_set_tuning "tail_streams" = 2), which only pays with a
    # queue of its own -- so this process asks for eight, as a deployment of those engines would in its launch file.  The
    # headline's engine keeps one tail stream; with it the queue count changes nothing measurable.  Read by the
    # runtime when it initialises: set before torch is imported.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402

NET_H, NET_W = 360, 1176
SEQ_LEN = 8
FP32_MFMA_PEAK_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
F16_MFMA_PEAK_TFLOPS = 2500.0   # same guide, "Peak BF16/FP16 MFMA ~2.5 PF dense" (the FP16 engines of config 3)
HBM_PEAK_GBPS = 8000.0           # same guide, "HBM3E ~8 TB/s"
I8_MFMA_PEAK_TOPS = 5000.0      # same guide, MFMA table: I8 32x32x32 = the cycles of the BF16 form at 2x the K (the INT8 engines of config 5)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def usable_cpus():
    """CPUs this process may really use: the affinity mask, cut to the cgroup's CPU quota (a container with `cpu.max` = 16 CPUs
    on a 256-thread host runs 128 OpenMP threads 6x SLOWER than 16: measured, tools/cpu_scaling.py)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(frames, P_l, P_r, weights_path, order, budget_s=25.0, ate_frames=None, ate_weights=None):
    """The CPU restatement of the whole stereoCallback (oracle/cpu: plain C++17 + OpenMP, `-O3 -march=native` rebuilt on THIS
    machine) timed on the host cores: a bounded sample of the same workload -- 5 warm-up frames, then up to 50 timed frames
    (fewer when 25 s of CPU time are used up first), medians per stage in the reference's latency-CSV columns
    (visual_odometry_node.cpp:246-258).  A reported baseline, kind "port": the reference's own CPU path (OpenCV ORB) needs
    OpenCV, which neither this image nor the GPU box has."""
    import oracle  # noqa: F401
    from oracle import cpu_backend
    lib, arch = None, "x86-64-v3 (prebuilt)"
    try:
        lib = cpu_backend.build("native", out=os.path.join(tempfile.mkdtemp(prefix="spvo_cpu_"), "libspvo_cpu_native.so"))
        arch = "native"
    except Exception:   # no compiler on this machine: the library built by __graft_entry__.build()
        pass
    cpu = cpu_backend.CpuBackend(lib, net_height=NET_H, net_width=NET_W, num_threads=usable_cpus())
    cpu.load_weights(weights_path)
    cpu.frontend_reset("KNN", True, 2.0, 0.25, 4)
    rows, t_start, k = [], time.time(), 0
    warm = 5
    per_frame = []    # EVERY frame from the reset on (warm-ups included): what the GPU pass over the same frame indices is compared with
    while True:
        L, R = frames[order[k % len(order)]]
        r = cpu.frontend_step(L, R, P_l, P_r)
        per_frame.append((r.pnp_ok, r.accepted, r.refined, r.lm_iterations, r.n_inliers, r.n_stereo, r.n_kp_l, *r.q[:], *r.t[:]))
        if k >= warm:
            rows.append((r.t_detect_ms, r.t_match_ms, r.t_solve_ms, r.t_total_ms, r.n_inliers, r.refined, r.accepted, r.pnp_ok, r.lm_iterations, r.n_stereo, r.n_kp_l))
        k += 1
        if len(rows) >= 50 or (len(rows) >= 10 and time.time() - t_start > budget_s):
            break
    a = np.array(rows, np.float64)
    med = np.median(a[:, :4], axis=0)
    threads = cpu.threads
    # BASELINE config 1: the reference's classic front end (ORB / ORB / BF / KNN at the native resolution,
    # launch/visual_odometry_classic.launch) on the same host cores.  The reference takes ORB from OpenCV, which this machine does
    # not have: oracle/cpu/orb_cpu.inc restates it from the published algorithm with the reference's parameters (one documented
    # deviation: the 256 test pairs are seeded, OpenCV's are a learned table).  Reported, never optimised against.
    orb = None
    try:
        cpu.frontend_reset_classic("KNN", True, 2.0, 4)
        orows, k = [], 0
        while len(orows) < 50:
            L, R = frames[k % len(frames)]                  # frames 0..7 cyclically: seven real steps and one jump back per cycle
            r = cpu.frontend_step(L, R, P_l, P_r)
            if k >= 5:
                orows.append((r.t_detect_ms, r.t_match_ms, r.t_solve_ms, r.t_total_ms, r.n_kp_l, r.n_stereo, r.n_temporal, r.n_inliers))
            k += 1
        o = np.array(orows, np.float64)
        om = np.median(o[:, :4], axis=0)
        orb = {"value": round(1e3 / float(om[3]), 2), "unit": "stereo frames/s", "cores": int(threads), "kind": "port",
               "stage_median_ms": {"detect": round(float(om[0]), 2), "match": round(float(om[1]), 2), "solve": round(float(om[2]), 2), "total": round(float(om[3]), 2)},
               "keypoints_per_image": int(np.median(o[:, 4])), "stereo_matches": int(np.median(o[:, 5])), "temporal_matches": int(np.median(o[:, 6])),
               "pnp_inliers": int(np.median(o[:, 7])),
               "sample": "50 stereo frames after 5 warm-ups, ORB 2000 features / 8 levels / scale 1.2 / FAST 20 (feature_detection_classic.cpp:13-24) at "
                         "376x1241, Hamming BF + KNN 0.8, same solver; published for the reference itself: 11.6 FPS on a Ryzen 5 3600 (VO/README.md:32)"}
    except Exception as exc:
        orb = {"error": repr(exc)}
    cpu.close()
    ate_cpu = None
    if ate_frames is not None and ate_weights:   # the ATE sequence (trained sp_squeeze graph) end to end on the CPU: its own features, matcher, solver
        try:
            cpu2 = cpu_backend.CpuBackend(lib, net_height=NET_H, net_width=NET_W, num_threads=usable_cpus())
            cpu2.load_weights(ate_weights)
            cpu2.frontend_reset("KNN", True, 2.0, 0.25, 4)
            ate_cpu = []
            for L, R in ate_frames:
                r = cpu2.frontend_step(L, R, P_l, P_r)
                ate_cpu.append((r.pnp_ok, r.accepted, r.refined, r.lm_iterations, r.n_inliers, r.n_stereo, r.n_kp_l, *r.q[:], *r.t[:]))
            cpu2.close()
        except Exception as exc:
            ate_cpu = repr(exc)
    return {"_per_frame": np.array(per_frame, np.float64), "_ate_cpu": ate_cpu,
            "value": round(1e3 / float(med[3]), 3), "unit": "stereo frames/s", "cores": int(threads), "kind": "port",
            "cpu_model": cpu_model(), "host_cpus": os.cpu_count(), "cpu_quota": usable_cpus(),
            "stage_median_ms": {"detect": round(float(med[0]), 2), "match": round(float(med[1]), 2), "solve": round(float(med[2]), 2), "total": round(float(med[3]), 2)},
            "solver_stats": {"pnp_ok_rate": round(float(a[:, 7].mean()), 3), "accepted_rate": round(float(a[:, 6].mean()), 3), "refined_rate": round(float(a[:, 5].mean()), 3),
                             "mean_lm_iterations": round(float(a[:, 8].mean()), 2), "mean_pnp_inliers": round(float(a[:, 4].mean()), 1),
                             "mean_stereo_matches": round(float(a[:, 9].mean()), 1), "mean_keypoints_left": round(float(a[:, 10].mean()), 1),
                             "note": "the same fields as the headline's solver_stats, but NOT the same frames: these are the sample's frames 5.. after a reset (frame_count <= 10 "
                                     "accepts everything, base.cpp:251), the headline's are thousands of frames of the ping-pong cycle with the gate armed; the like-for-like "
                                     "comparison is `solver_stats_same_frames` below"},
            "latency_ms": {"p50": round(float(np.median(a[:, 3])), 3), "p99": round(float(np.sort(a[:, 3])[min(len(a) - 1, int(0.99 * len(a)))]), 3),
                           "definition": "t_total per frame (one pair at a time: the reference's latency column, visual_odometry_node.cpp:246-258)"},
            "config1_orb_front_end": orb,
            "sample": f"{len(rows)} stereo frames after {warm} warm-ups through oracle/cpu (C++17 + OpenMP restatement of the whole step: "
                      f"crop/resize, VGG fp32 direct convolution, softmax/NMS, descriptor sampling, brute-force L2 matching, triangulation, "
                      f"RANSAC, LM), g++ -O3 -march={arch}, {threads} OpenMP threads (= the CPUs this process may use: affinity mask and cgroup quota); "
                      f"median of per-frame totals"}


def cached_stream(synth, tex, seed):
    """The synthetic stereo stream of one rank, rendered once per seed and machine (8 ranks launched back to back for N = 1, 2, 4, 8
    would otherwise each spend seconds in the renderer before their first step)."""
    path = os.path.join(tempfile.gettempdir(), f"spvo_synth_{SEQ_LEN}_{seed}.npz")
    try:
        z = np.load(path)
        frames = [(z["L"][k], z["R"][k]) for k in range(SEQ_LEN)]
        return frames, None, z["P_l"], z["P_r"]   # (the ground-truth ego-motion is not needed for timing)
    except Exception:   # not rendered yet (or an unreadable file): render and publish atomically
        frames, poses, P_l, P_r = synth.stereo_sequence(SEQ_LEN, tex, seed=seed)
        tmp = f"{path}.{os.getpid()}.tmp.npz"
        try:
            np.savez(tmp, L=np.stack([f[0] for f in frames]), R=np.stack([f[1] for f in frames]), P_l=P_l, P_r=P_r)
            os.replace(tmp, path)
        except OSError:
            pass
        return frames, poses, P_l, P_r


ATE_FRAMES = 40      # the untimed trajectory pass (`ate` in the JSON line): a monotone synthetic sequence with exact ground truth
ATE_SEED = 100
_OUTCOME_COLS = ("pnp_ok", "accepted", "refined", "lm_iterations", "pnp_inliers", "stereo_matches", "keypoints_left")


def cached_ate_sequence(synth, tex):
    """ATE_FRAMES synthetic stereo frames with their ground-truth poses, rendered once per machine (0.2 s per frame)"""
    path = os.path.join(tempfile.gettempdir(), f"spvo_synth_ate_{ATE_FRAMES}_{ATE_SEED}.npz")
    try:
        z = np.load(path)
        return [(z["L"][k], z["R"][k]) for k in range(ATE_FRAMES)], [(z["Rw"][k], z["tw"][k]) for k in range(ATE_FRAMES)]
    except Exception:
        frames, poses, _, _ = synth.stereo_sequence(ATE_FRAMES, tex, seed=ATE_SEED)
        tmp = f"{path}.{os.getpid()}.tmp.npz"
        try:
            np.savez(tmp, L=np.stack([f[0] for f in frames]), R=np.stack([f[1] for f in frames]), Rw=np.stack([p[0] for p in poses]), tw=np.stack([p[1] for p in poses]))
            os.replace(tmp, path)
        except OSError:
            pass
        return frames, poses


def _quat_to_rot(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def integrate_steps(steps):
    """camera centres in the first camera's frame from cam0_curr_T_cam0_prev steps (R or q, t), as visual_odometry_node.cpp:118-127 chains them"""
    T = np.eye(4)
    out = [np.zeros(3)]
    for r, t in steps:
        S = np.eye(4)
        S[:3, :3] = r if np.ndim(r) == 2 else _quat_to_rot(r)
        S[:3, 3] = t
        T = T @ np.linalg.inv(S)
        out.append(T[:3, 3].copy())
    return np.array(out)


def ate_rmse(a, b):
    e = np.linalg.norm(a - b, axis=1)
    return float(np.sqrt(np.mean(e ** 2))), float(e.max())


def gpu_sequence(host, models_dir, prefix, seq, P_l, P_r):
    """the unchanged node's call sequence (addStereoImagePair on host images, matchDescriptors x 2, solveStereoOdometry) over `seq` on a fresh front
    end of the FP32 engine `prefix`: one row per frame = _OUTCOME_COLS + q (xyzw) + t of cam0_curr_T_cam0_prev (identity on the first frame)"""
    fe = host.FrontEnd(models_dir, prefix=prefix, selector="KNN", cross_check=True, batch=2, height=NET_H, width=NET_W, conf_thresh=0.015, dist_thresh=4,
                       border_remove=4, stereo_threshold=2.0, min_disparity=0.25, refinement_degree=4, precision="FP32")
    if not fe.engine_loaded:
        raise RuntimeError("engine load failed: " + fe.last_error)
    rows = []
    for L, R in seq:
        res = fe.step(L, R, P_l, P_r)
        f = fe.last_solve() if res is not None else dict(pnp_ok=0, accepted=0, refined=0, lm_iterations=0)
        q, t = res if res is not None else ((0, 0, 0, 1), (0, 0, 0))
        rows.append((f["pnp_ok"], f["accepted"], f["refined"], f["lm_iterations"], len(fe.inliers("pnp")) if res is not None else 0,
                     len(fe.matches(host.CURR_LEFT_CURR_RIGHT)[0]), len(fe.keypoints(host.CURR_LEFT)), *q, *t))
    fe.close()
    return np.array(rows, np.float64)


def dump_outputs(directory, fe, host, pose):
    """--dump-outputs: what the last timed step handed to its caller -- its pose and the solver's outcome -- and what the front end holds for
    that frame: the keypoints of both images, the stereo and the temporal matches (query, train, distance) and the PnP inliers, as
    float32 / float64 .npy files.  The inputs are seeded, so two builds can be compared file by file.  (The descriptors of the device path
    stay in the context's slots: the host deque holds n x 0 headers.)"""
    os.makedirs(directory, exist_ok=True)
    q, t = pose if pose is not None else ((0, 0, 0, 1), (0, 0, 0))
    flags = fe.last_solve()
    arrays = {"pose": np.concatenate([np.asarray(q, np.float64), np.asarray(t, np.float64)]),   # q (x, y, z, w), t of cam0_curr_T_cam0_prev
              "solver_outcome": np.array([pose is not None, flags["pnp_ok"], flags["accepted"], flags["refined"], flags["lm_iterations"]], np.float64),
              "keypoints_left": fe.keypoints(host.CURR_LEFT), "keypoints_right": fe.keypoints(host.CURR_RIGHT),
              "pnp_inliers": fe.inliers("pnp").astype(np.float64)}
    for name, kind in (("stereo_matches", host.CURR_LEFT_CURR_RIGHT), ("temporal_matches", host.CURR_LEFT_PREV_LEFT)):
        qi, ti, d = fe.matches(kind)
        arrays[name] = np.stack([qi.astype(np.float64), ti.astype(np.float64), d.astype(np.float64)], axis=1)
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), a)


def outcome_stats(a):
    return {"pnp_ok_rate": round(float(a[:, 0].mean()), 3), "accepted_rate": round(float(a[:, 1].mean()), 3), "refined_rate": round(float(a[:, 2].mean()), 3),
            "mean_lm_iterations": round(float(a[:, 3].mean()), 2), "mean_pnp_inliers": round(float(a[:, 4].mean()), 1),
            "mean_stereo_matches": round(float(a[:, 5].mean()), 1), "mean_keypoints_left": round(float(a[:, 6].mean()), 1)}


def pin_to_gpu_numa_node(torch, local_rank):
    """Best effort: run this rank's host thread on the cores of the NUMA node its GPU hangs off (one process per GPU: the launch
    loop then never crosses sockets to reach its device)."""
    try:
        pr = torch.cuda.get_device_properties(local_rank)
        bdf = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
        node = int(open(f"/sys/bus/pci/devices/{bdf}/numa_node").read())
        if node < 0:
            return None
        cpus = set()
        for part in open(f"/sys/devices/system/node/node{node}/cpulist").read().strip().split(","):
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
        cpus &= os.sched_getaffinity(0)
        if cpus:
            os.sched_setaffinity(0, cpus)
        return node
    except Exception:
        return None


def spawn_ranks(n, cmd=None, deadline_s=None, grace_s=5.0, poll_s=0.1):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script (or of `cmd`, a test hook), one per GPU,
    exactly as `python -m torch.distributed.run --nnodes=1 --nproc-per-node N` would (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*
    in the environment).  The children are fresh interpreters started BEFORE this process has touched the GPU or imported
    torch (never re-exec a process that has initialised HIP); rank 0 inherits stdout and prints the one JSON line.

    The children are POLLED: the first rank that exits non-zero (out of memory, RCCL initialisation, a crash) has its siblings
    terminated -- SIGTERM, then SIGKILL after `grace_s` -- instead of leaving them in `dist.barrier()` / `ncclAllGather` until
    somebody's timeout; the launcher then returns that rank's exit code with the tail of its stderr on ours.  `deadline_s`
    (default: SPVO_BENCH_RANK_DEADLINE or 1500 s) bounds the whole job the same way."""
    import signal
    import socket
    import subprocess
    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = str(sk.getsockname()[1])
    if deadline_s is None:
        deadline_s = float(os.environ.get("SPVO_BENCH_RANK_DEADLINE", "1500"))
    cmd = list(cmd) if cmd else [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    logdir = tempfile.mkdtemp(prefix="spvo_ranks_")
    procs, logs = [], []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        # rank 0 writes to OUR stdout and stderr as it goes (the JSON line, progress and [spvo] diagnostics of a long job are visible live);
        # the other ranks' stderr is captured and shown only if one of them fails
        logs.append(None if r == 0 else open(os.path.join(logdir, f"rank{r}.stderr"), "w+b"))
        procs.append(subprocess.Popen(cmd, env=env, stdout=None if r == 0 else subprocess.DEVNULL, stderr=logs[-1]))

    def tail(r, nbytes=3000):
        if logs[r] is None:
            return "(rank 0 wrote to this process's stderr: see above)"
        logs[r].flush()
        logs[r].seek(0, os.SEEK_END)
        size = logs[r].tell()
        logs[r].seek(max(0, size - nbytes))
        return logs[r].read().decode("utf-8", "replace")

    def stop_all():   # our own children only, by their exact pids (they stay in this process group: whoever kills the group gets them too)
        alive = [pr for pr in procs if pr.poll() is None]
        for pr in alive:
            pr.terminate()
        t_end = time.time() + grace_s
        while time.time() < t_end and any(pr.poll() is None for pr in alive):
            time.sleep(poll_s)
        for pr in alive:
            if pr.poll() is None:
                pr.kill()
                pr.wait()

    class Stopped(Exception):
        pass

    def on_signal(signum, _frame):   # the launcher itself is being stopped: take the ranks along
        raise Stopped(signum)
    old = {sg: signal.signal(sg, on_signal) for sg in (signal.SIGTERM, signal.SIGINT)}

    t0 = time.time()
    rc, failed = 0, None
    try:
        while True:
            codes = [pr.poll() for pr in procs]
            bad = [r for r, c in enumerate(codes) if c not in (None, 0)]
            if bad:
                failed, rc = bad[0], abs(codes[bad[0]]) or 1
                break
            if all(c == 0 for c in codes):
                break
            if time.time() - t0 > deadline_s:
                failed, rc = -1, 124
                break
            time.sleep(poll_s)
        if failed is not None:
            stop_all()
            if failed >= 0:
                sys.stderr.write(f"bench.py: rank {failed} of {n} exited with code {rc}; the other ranks were terminated.  Its stderr ends:\n{tail(failed)}\n")
            else:
                sys.stderr.write(f"bench.py: the {n} ranks did not finish within {deadline_s:.0f} s and were terminated.\n")
        return rc
    except Stopped as st:
        stop_all()
        return 128 + int(st.args[0])
    finally:   # every path, the stopped one included: handlers back, log files closed, the temporary directory gone
        for sg, h in old.items():
            signal.signal(sg, h)
        for f in logs:
            if f is not None:
                f.close()
        import shutil
        shutil.rmtree(logdir, ignore_errors=True)


def repeats_for(first_elapsed, target_s=1.0):
    """How often a timed block of K steps is repeated: so that the blocks add up to about `target_s` seconds (the driver's 20 steps
    are an 18 ms block: one sample of that says little), at least 5, at most 200."""
    return int(min(200, max(5, -(-target_s // max(first_elapsed, 1e-4)))))


def spread(times, steps):
    """median / min / max of the per-block times as a dict fragment"""
    a = np.sort(np.asarray(times, np.float64))
    med = float(np.median(a))
    return med, {"repeats": int(a.size), "ms_per_step_min": round(1e3 * float(a[0]) / steps, 4), "ms_per_step_max": round(1e3 * float(a[-1]) / steps, 4),
                 "spread_pct": round(100.0 * float(a[-1] - a[0]) / med, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=0, help="timed blocks of --steps steps (default 0: one block; with --full as many as make about one second, 5..200); "
                                                            "the line reports the median block")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline figure: repeated timed blocks, per-kernel events in the timed region, the "
                                                         "stage / roofline pass, the informational legs and the CPU baseline with the trajectory check")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step computed (pose, solver outcome, "
                                                                         "keypoints, matches, PnP inliers) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(with --full) skip the CPU baseline and the trajectory check")
    ap.add_argument("--no-extras", action="store_true", help="(with --full) skip the informational legs (split mode, host images, trained graph, classic front end, other configs)")
    ap.add_argument("--legs", default="split,host,trained,classic,configs", help="(with --full) informational legs to run after the headline (comma list of split, host, trained, classic, configs)")
    ap.add_argument("--no-profile", action="store_true", help="(with --full) do not record per-kernel HIP events in the timed region")
    ap.add_argument("--no-pipeline", action="store_true", help="do not hand the next stereo pairs over early")
    ap.add_argument("--sync-solve", action="store_true", help="solve inside the step (solveStereoOdometry in one piece) instead of handing every frame's solve over and "
                                                              "collecting its pose during the next step (solveStereoOdometrySubmit / Collect: the default whenever pairs are handed over "
                                                              "ahead; neutral on the fp32 headline, +20..40 %% where the host and the solver bound the step: FP16 / INT8 engines)")
    ap.add_argument("--net-size", default="360x1176", help="network input HxW: 360x1176 (the reference's, default = the headline workload) or 376x1240 (native, SURVEY.md section 8)")
    ap.add_argument("--precision", default="FP32", choices=["FP32", "FP16", "INT8"],
                    help="FP32 = the headline workload (BASELINE config 2); FP16 = the half-precision engine of config 3 (use with --net-size 192x640); "
                         "INT8 = post-training-quantised engine, calibrated on the device on the bench's own frames (config 5)")
    ap.add_argument("--graph", default="vgg", choices=["vgg", "sp_mbv1", "sp_mbv2", "sp_squeeze"],
                    help="network: vgg (seeded, the headline) or one of the reference's ONNX graphs (tests/golden/<graph>.spvw)")
    ap.add_argument("--max-keypoints", type=int, default=1000, help="keypoint cap per image (reference: 1000; config 5: 2048)")
    ap.add_argument("--match-fp8", action="store_true", help="fp8 (e4m3) shortlist GEMM in the matcher, exact fp32 re-rank (config 5)")
    ap.add_argument("--fp32-split", action="store_true",
                    help="evaluate the FP32 engine on the bf16 matrix pipe (3 bf16 pieces per operand, 6 partial products, fp32 accumulation; "
                         "spvo_set_fp32_split) -- opt-in, not the headline")
    ap.add_argument("--config", type=int, default=0, choices=[0, 2, 3, 5],
                    help="BASELINE.json config shortcut: 2 = default; 3 = FP16 192x640; 5 = sp_mbv1 INT8, 2048 keypoints, fp8 shortlist")
    ap.add_argument("--dump-ops", action="store_true", help="(with --full) add per-layer network times to the JSON line")
    ap.add_argument("--py-loop", action="store_true", help="drive the timed steps from Python, one front-end call at a time, instead of handing blocks of stereoCallbacks to the host "
                                                             "library's C loop (spvo_host_run_device_block): what the interpreter costs per step, for A/B")
    ap.add_argument("--cpus", type=int, default=0, help="restrict this process to that many CPUs (os.sched_setaffinity, BEFORE anything touches the GPU): what one rank of an "
                                                          "8-rank job gets of the GPU box's 16-CPU quota is 2 -- the host-budget check of DESIGN.md section 6")
    ap.add_argument("--depth", type=int, default=4, choices=[1, 2, 3, 4], help="stereo pairs handed over ahead of the one being solved; at 4 the front end pairs trunks (two stereo pairs per set of network launches: spvo_set_trunk_pairing)")
    args = ap.parse_args()
    if args.config == 3:
        args.precision, args.net_size = "FP16", "192x640"
    elif args.config == 5:
        args.precision, args.graph, args.max_keypoints, args.match_fp8 = "INT8", "sp_mbv1", 2048, True
    headline = args.precision == "FP32" and args.graph == "vgg" and args.max_keypoints == 1000 and not args.match_fp8 and not args.fp32_split
    profile = args.full and not args.no_profile     # per-kernel events in the timed region + the stage pass behind it
    extras = args.full and headline and not args.no_extras
    global NET_H, NET_W
    NET_H, NET_W = (int(v) for v in args.net_size.lower().split("x"))

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:   # no launcher: be one (before anything touches the GPU)
        sys.exit(spawn_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("SPVO_QUIET", "1")    # the seeded (untrained) weights make the reference's gating message fire on every frame
    if args.fp32_split:
        if args.precision != "FP32":
            raise SystemExit("--fp32-split applies to FP32 engines")

    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU path")
    # Test hook: SPVO_BENCH_SHARED_GPU=1 lets several ranks share the visible GPU(s) over the gloo backend, so the N > 1
    # code path (pose gather, barrier, max-over-ranks timing) can be exercised on a one-GPU box.  RCCL refuses two ranks
    # on one device; a real run uses one GPU per rank and backend "nccl" (= RCCL).
    shared = os.environ.get("SPVO_BENCH_SHARED_GPU") == "1"
    if shared:
        local_rank = local_rank % torch.cuda.device_count()
    elif local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} needs GPU {local_rank}, {torch.cuda.device_count()} visible (one rank per GPU; --gpus {args.gpus})")
    torch.cuda.set_device(local_rank)
    # Test hook: SPVO_BENCH_FORCE_DIST=1 runs the collective path (RCCL process group, pose all-gather, barrier, max-reduce) in a
    # single-rank job too, so that it can be exercised on a one-GPU box.
    dist_on = world > 1 or os.environ.get("SPVO_BENCH_FORCE_DIST") == "1"
    if dist_on and "RANK" not in os.environ:
        os.environ.update({"RANK": "0", "WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": os.environ.get("MASTER_PORT", "29533")})
    if dist_on:
        import datetime
        # a peer that died leaves a collective waiting: bound that wait (the launcher -- spawn_ranks or torch.distributed.run -- stops the
        # job as soon as it sees the dead rank; this is the backstop)
        dist_timeout = datetime.timedelta(seconds=int(os.environ.get("SPVO_BENCH_DIST_TIMEOUT", "300")))
        if shared:
            dist.init_process_group("gloo", timeout=dist_timeout)
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=dist_timeout)

    if world > 1:   # several ranks share the host: an equal share of the CPUs this job may really use (cgroup quota, not the host's core count)
        torch.set_num_threads(max(1, usable_cpus() // world))
    from spvo import capi, host, posegather, synth, weights
    # device, keypoint cap and fp8 shortlist of the front ends created below: the host class's setters (setDevice, setMaxKeypoints,
    # setMatchFp8), not environment variables
    host.set_options(device=local_rank, max_keypoints=args.max_keypoints, match_fp8=1 if args.match_fp8 else 0)
    small_engine = args.precision in ("FP16", "INT8")
    if small_engine and int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) >= 8:
        capi.set_tuning("tail_streams", 2)   # (BASELINE configs 3 / 5 as this script's own workload: as in the `other_configs` legs below)
    keep2_main = args.precision == "FP16"    # engines whose frame is shorter than the solver's chain (config 3); config 5's INT8 trunk paces its loop: no gain, one frame more latency
    if keep2_main:
        capi.set_tuning("solve_keep", 2)     # two solves stay pending behind every submit: a frame's last solver kernel goes out with the next frame's hypotheses
    capi.tuning_from_env()   # SPVO_TUNE_<NAME>=<int>: diagnostic switches for A/B runs of this script (the library itself never reads the environment)
    if args.fp32_split:
        capi.set_tuning("fp32_split", 1)   # engines loaded from here on run in split mode (the library reads no environment variable for it)

    plan = weights.vgg_plan(seed=0) if args.graph == "vgg" else weights.load(os.path.join(ROOT, "tests", "golden", args.graph + ".spvw"))
    n_params = int(sum(op.weight.size + op.bias.size for op in plan.ops if op.weight is not None))
    tmp = tempfile.mkdtemp(prefix=f"spvo_bench_{rank}_")
    os.makedirs(os.path.join(tmp, "laptop"))

    # every rank renders its own stream (different seed = different ego-motion); sample-image texture
    tex = os.path.join(ROOT, "tests", "golden", "images", "0000000000.png")
    frames, poses, P_l, P_r = cached_stream(synth, tex, posegather.stream_seed(rank))
    if os.environ.get("SPVO_BENCH_BURN"):   # diagnostic: seconds of host arithmetic before the loop (what rendering the stream does on a cold cache)
        t_b = time.time()
        while time.time() - t_b < float(os.environ["SPVO_BENCH_BURN"]):
            np.random.rand(512, 512) @ np.random.rand(512, 512)
    if world > 1 and os.environ.get("SPVO_BENCH_NO_PIN") != "1":   # several ranks share the host: keep each on the cores next to its GPU
        pin_to_gpu_numa_node(torch, local_rank)
    if args.precision == "INT8":       # activation scales from the fp32 engine of the same plan on this stream's own frames (on the device)
        from spvo import quant
        calib = [quant.calibration_inputs(plan, frames[k], NET_H, NET_W) for k in (0, SEQ_LEN // 2, SEQ_LEN - 1)]
        plan.act_scales = quant.calibrate(plan, calib, NET_H, NET_W)
    plan.precision = args.precision
    engine_path = os.path.join(tmp, "laptop", weights.engine_name("superpoint_pretrained", 2, NET_H, NET_W, args.precision))
    weights.save(plan, engine_path)
    d_frames = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in frames]
    rows, cols = frames[0][0].shape
    order = list(range(SEQ_LEN)) + list(range(SEQ_LEN - 2, 0, -1))       # ping-pong: every step is a real motion
    # one device buffer per POSITION of the cycle: the front end recognises an announced pair by its pointers, and with more than two pairs
    # handed over ahead the ping-pong order shows the same frame twice inside the window (6, 7, 6)
    cycles = {}

    def cycle_buffers(seq):
        key = tuple(seq)
        if key not in cycles:
            distinct = len(set(seq)) == len(seq)
            cycles[key] = [d_frames[f] if distinct else tuple(t.clone() for t in d_frames[f]) for f in seq]
        return cycles[key]

    fe = host.FrontEnd(tmp, prefix="superpoint_pretrained", selector="KNN", cross_check=True, batch=2,
                       height=NET_H, width=NET_W, conf_thresh=0.015, dist_thresh=4, border_remove=4,
                       stereo_threshold=2.0, min_disparity=0.25, refinement_degree=4, precision=args.precision)
    if not fe.engine_loaded:
        raise SystemExit("engine load failed: " + fe.last_error)
    ctx = fe.context()
    # shared-GPU test hook: RCCL refuses two ranks on one device, so the C ABI's file transport carries the poses there
    pg = posegather.PoseGather(torch.device("cpu") if shared else torch.device("cuda", local_rank), force=dist_on)

    deferred = not (args.no_pipeline or args.sync_solve)

    def step(i, order=order):
        cyc = cycle_buffers(order)
        dl, dr = cyc[i % len(cyc)]
        ahead = [None] * 4                                                  # the next pairs are already in HBM
        for d in range(0 if args.no_pipeline else args.depth):
            nl, nr = cyc[(i + 1 + d) % len(cyc)]
            ahead[d] = (nl.data_ptr(), nr.data_ptr())
        # with pairs handed over ahead the solve is handed over too: the pose of frame i is collected in step i + 1 (or by
        # fe.finish_solve() after the last step), so the solver's latency is never between two hand-overs of images
        res = fe.step_device(dl.data_ptr(), dr.data_ptr(), rows, cols, dl.stride(0), P_l, P_r, ahead[0], ahead[1], deferred_solve=deferred, next3_pair=ahead[2], next4_pair=ahead[3])
        if dist_on:                                                       # pose staged; RCCL all-gather per 64 frames on a side stream
            pg.gather_async(*(res if res is not None else (None, None)))
            if (i + 1) % 1024 == 0:
                pg.collect()
        return res

    ptr_cache = {}

    def run_frames(first, n, order=order, depth=None, records=None):
        """n stereoCallbacks starting at frame index `first`: through the host library's C loop in sub-blocks of at most 64 frames (the
        poses of a sub-block go to the pose gather as they did per step), or -- with --py-loop -- one Python call per front-end call.
        Appends the frames' records (pose, first-call -> pose latency, solver outcome) to `records` when given.  Returns the last pose
        the caller received, (q, t), or None."""
        depth = (0 if args.no_pipeline else args.depth) if depth is None else depth
        got = None
        if args.py_loop:
            for i in range(first, first + n):
                res = step(i, order)
                got = res if res is not None else got
            return got
        key = tuple(order)
        if key not in ptr_cache:
            cyc = cycle_buffers(order)
            ptr_cache[key] = ([c[0].data_ptr() for c in cyc], [c[1].data_ptr() for c in cyc], cyc[0][0].stride(0))
        pl, pr, stride = ptr_cache[key]
        done = 0
        while done < n:
            m = min(64, n - done)
            rec = fe.run_device_block(pl, pr, rows, cols, stride, P_l, P_r, first + done, m, depth, deferred and depth > 0)
            if dist_on:
                for r in rec:
                    pg.gather_async(*((r["q"], r["t"]) if r["has_pose"] else (None, None)))
            if records is not None:
                records.append(rec)
            got = (rec["q"][-1], rec["t"][-1]) if rec["has_pose"][-1] else got
            done += m
        return got

    def barrier():
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()

    # The step loop is Python; the collector of the interpreter is not part of the workload.  A generation-2 pass over the
    # ~10^5 objects that importing torch leaves behind costs tens of milliseconds, and whether one falls into a 200-step timed
    # region depends on the allocation history of the process: 880 stereo frames/s from a cold start against 1070 after the
    # stream had been rendered in-process (tools/bench_variance.sh, tools/host_breakdown.py).  Everything alive now is frozen
    # out of the collector's reach and the collector is off while steps are timed.
    import gc
    gc.collect()
    gc.freeze()
    gc.disable()
    run_frames(0, args.warmup)
    if dist_on:
        pg.collect()
    # Inside the timed region only the dominant kernel (conv1b = stage "conv:1") is bracketed by HIP events on the
    # context's stream: two event records per step.  Timing every stage costs 2 records per kernel and 7 % of the
    # throughput, so the stage breakdown comes from a separate, untimed pass below.
    if profile:
        ctx.profile_only("conv:1" if args.graph == "vgg" else "detect")
        ctx.profile_enable(True)
        ctx.profile_reset()
    # A timed block = EXACTLY args.steps steps between two barriers (+ device synchronisation).  A plain run times one block (or
    # --repeats); with --full the block is repeated -- a block of 20 steps lasts 18 ms, one such sample is thin -- and `value` is the
    # MEDIAN block (max over ranks per block); the number of repeats follows from the first block's duration and is the same on every rank.
    cursor = [args.warmup]
    last_pose = [None]      # the pose the last timed step handed to its caller (--dump-outputs)
    timed_records = []
    local_times = []        # THIS rank's block times (the line's `value` uses the max over ranks per block; `per_rank_fps` shows the ranks apart)
    pg.reset_timing()

    def timed_block():
        barrier()
        t0 = time.perf_counter()
        got = run_frames(cursor[0], args.steps, records=timed_records)
        last = fe.finish_solve()                                            # the last step's pose (deferred solve): inside the timed region (the C loop collects it itself)
        last_pose[0] = last if last is not None else got
        if dist_on and last is not None:
            pg.gather_async(*last)
        if dist_on:
            gathered = pg.collect()                                         # every pose of every rank has arrived: inside the timed region
            assert gathered.shape[1:] == (world, 7)
        t_own = time.perf_counter() - t0                                    # this rank's frames and its share of the collectives, before it waits for the slowest rank
        barrier()
        cursor[0] += args.steps
        local_times.append(t_own)
        return time.perf_counter() - t0

    def over_ranks(ts):
        if not dist_on:
            return list(ts)
        t = torch.tensor(list(ts), dtype=torch.float64, device="cpu" if shared else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return [float(v) for v in t.tolist()]

    block_times = over_ranks([timed_block()])
    n_rep = args.repeats if args.repeats > 0 else (repeats_for(block_times[0]) if args.full else 1)
    block_times += over_ranks([timed_block() for _ in range(n_rep - 1)])
    if args.dump_outputs and rank == 0:   # before anything else runs on this front end
        dump_outputs(args.dump_outputs, fe, host, last_pose[0])
    elapsed, headline_spread = spread(block_times, args.steps)
    gather_timing = pg.timing()
    rank_fps = [args.steps / float(np.median(local_times))]
    rank_gather_ms = [gather_timing.get("mean_ms", 0.0)]
    rank_init_ms = [pg.init_ms]
    if dist_on:   # every rank's own rate, collective cost and communicator set-up time, gathered OUTSIDE the timed region
        t = torch.tensor([rank_fps[0], rank_gather_ms[0], rank_init_ms[0]], dtype=torch.float64, device="cpu" if shared else "cuda")
        allr = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allr, t)
        rank_fps, rank_gather_ms, rank_init_ms = ([float(a[i]) for a in allr] for i in range(3))
    prof, prof_all = {}, {}
    if profile:
        prof = ctx.profile()
        ctx.profile_only(None)
        ctx.profile_reset()
        n_extra = min(max(args.steps, 50), 100)
        run_frames(cursor[0], n_extra)
        fe.finish_solve()
        barrier()
        prof_all = ctx.profile()
        ctx.profile_enable(False)

    def frame_summary(records):
        """latency and solver statistics of the frames of the timed blocks (C loop records).  Latency: from the first call that handed a
        pair over (its announcement, `depth` frames ahead of its turn, or addStereoImagePair itself) to its pose in the caller's hands --
        the reference's t_total (visual_odometry_node.cpp:246-258) plus what look-ahead and the deferred solve add."""
        if not records:
            return {}
        r = np.concatenate(records)
        r = r[r["has_pose"] == 1]
        if r.size == 0:
            return {}
        lat = np.sort(r["latency_ms"])
        return {"latency_ms": {"p50": round(float(lat[lat.size // 2]), 3), "p99": round(float(lat[min(lat.size - 1, int(0.99 * lat.size))]), 3),
                               "mean": round(float(lat.mean()), 3), "frames": int(lat.size),
                               "definition": "first call that hands the pair over (announcement or addStereoImagePair) -> its pose returned; the reference's t_total when depth = 0"},
                "solver_stats": {"pnp_ok_rate": round(float(r["pnp_ok"].mean()), 3), "accepted_rate": round(float(r["accepted"].mean()), 3),
                                 "refined_rate": round(float(r["refined"].mean()), 3), "mean_lm_iterations": round(float(r["lm_iterations"].mean()), 2),
                                 "mean_pnp_inliers": round(float(r["pnp_inliers"].mean()), 1), "mean_stereo_matches": round(float(r["stereo_matches"].mean()), 1),
                                 "mean_keypoints_left": round(float(r["keypoints_left"].mean()), 1)}}

    def leg_frames(order_=order, start=args.warmup, depth=None):
        """an extra (informational) leg on device images, timed like the headline through the same C loop: barrier-bracketed blocks of at least
        100 frames (each block's barriers drain the pipeline), the median block; returns (time scaled to args.steps steps, spread fields, frame summary)"""
        n = max(args.steps, 100)
        cur = [start]
        recs = []

        def block():
            barrier()
            t1 = time.perf_counter()
            run_frames(cur[0], n, order_, depth, recs)
            fe.finish_solve()
            barrier()
            cur[0] += n
            return time.perf_counter() - t1
        t_probe = block()
        if t_probe < 0.05:      # short steps (the small engines: 0.15 - 0.27 ms): blocks of at least ~50 ms, so that the fill and drain of the
            n = min(1000, -(-int(n * 0.05 / t_probe) // 50) * 50)   # four-deep pipeline and the host's jitter stay a small part of a block
            recs.clear()
            t_probe = block()
        ts = [t_probe]
        ts += [block() for _ in range((args.repeats if args.repeats > 0 else repeats_for(ts[0], 0.6)) - 1)]
        e, sp = spread(ts, n)
        return e * args.steps / n, {**sp, "steps_per_block": n}, frame_summary(recs)

    def leg(step_fn, finish, start=args.warmup):
        """an extra (informational) leg timed like the headline: barrier-bracketed blocks, the median block.  Its blocks are at least
        100 steps long whatever --steps says (each block's barriers drain the pipeline: at the driver's 20 steps that costs a
        look-ahead leg 10 % and says nothing about the path); the leg reports `steps_per_block`.  Returned: the median block's time
        scaled to args.steps steps (so that args.steps / time is the leg's frame rate) and the spread fields."""
        n = max(args.steps, 100)
        cur = [start]

        def block():
            barrier()
            t1 = time.perf_counter()
            for i in range(cur[0], cur[0] + n):
                step_fn(i)
            finish()
            barrier()
            cur[0] += n
            return time.perf_counter() - t1
        ts = [block()]
        ts += [block() for _ in range((args.repeats if args.repeats > 0 else repeats_for(ts[0], 0.6)) - 1)]
        e, sp = spread(ts, n)
        return e * args.steps / n, {**sp, "steps_per_block": n}

    legs = set(args.legs.split(","))
    if rank == 0:
        total_frames = args.steps * world
        out = {
            "metric": "stereo frames/sec (1241x376 KITTI)", "value": round(total_frames / elapsed, 2), "unit": "stereo frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 4),
            **headline_spread, "timing": "median of `repeats` timed blocks of `steps` steps each (barrier + synchronize on both sides, max over ranks per block)",
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32 as 3 x bf16 (split operands, fp32 accumulate)" if args.fp32_split else {"FP32": "f32", "FP16": "f16", "INT8": "i8"}[args.precision], "data": "synthetic",
            "config": {"workload": (f"SuperPoint VGG {args.precision.lower()} (seeded synthetic weights, {n_params} params)" if args.graph == "vgg" else
                                    f"SuperPoint {args.graph} {args.precision.lower()} (the reference's TRAINED ONNX graph, re-packed as tests/golden/{args.graph}.spvw, {n_params} params)")
                                   + f", 1241x376 stereo pairs, net {NET_H}x{NET_W}, {args.max_keypoints} kp cap, "
                                   + ("fp8 shortlist + exact re-rank, " if args.match_fp8 else "")
                                   + "BF+KNN 0.8, P3P-style RANSAC 500 it, LM refinement degree 4; one stereo stream per GPU, RCCL all-gather of poses",
                       "net_size": [NET_H, NET_W], "input_size": [rows, cols], "streams": world,
                       "host_cpus_allowed": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
                       "hw_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "4")),   # the HIP runtime's queue count this process asked for (used by the FP16 / INT8 legs' second tail stream)
                       "tail_streams": capi.get_tuning("tail_streams", 1),
                       "solves_kept_pending": capi.get_tuning("solve_keep", 1),   # behind every submit of the block loop (2: a frame's last solver kernel goes out in one launch with the next frame's hypotheses)
                       "hand_over": ("images of the next %d pairs handed over ahead (prefetchStereoImagePairDevice)" % args.depth + ("; with four ahead the front end pairs trunks: a pair whose network would only queue waits for its successor and the two run through every layer in one launch (spvo_set_trunk_pairing)" if args.depth >= 4 else "") if not args.no_pipeline else "one pair at a time")
                                    + ("; each frame's solve handed over too, its pose collected during the next step (solveStereoOdometrySubmit / Collect), the last one before the closing barrier" if deferred else ""),
                       "pose_gather": {"local": "single stream, no collective", "c:rccl": "spvo_pose_allgather_n (C ABI, RCCL), one collective per 64 frames",
                                       "c:host": "spvo_pose_allgather_n (C ABI, file transport: test hook)",
                                       "torch": "torch.distributed all_gather (RCCL), one collective per 64 frames"}.get(pg.transport, pg.transport)
                                      + (" -- " + pg.transport_note if pg.transport_note else "")},
        }
        out.update(frame_summary(timed_records))
        # the ranks apart (one entry per rank; N = 1: one entry): each rank's own frame rate over its median block BEFORE the closing barrier, what a batched pose
        # collective costs its calling thread, and the one-off communicator creation (ncclCommInitRank + bootstrap), which is outside every timed region
        out["per_rank_fps"] = {"min": round(min(rank_fps), 2), "median": round(float(np.median(rank_fps)), 2), "max": round(max(rank_fps), 2), "ranks": [round(v, 2) for v in rank_fps],
                               "definition": "steps / this rank's median block time, measured before the block's closing barrier (value = all ranks' steps / max over ranks)"}
        out["pose_gather_ms"] = {**gather_timing, "per_rank_mean_ms": [round(v, 4) for v in rank_gather_ms],
                                 "definition": "host wall time of one spvo_pose_allgather_n (all ranks' poses of <= 64 frames, RCCL) inside the timed region, rank 0's distribution + every rank's mean"}
        out["comm_init_ms"] = {"per_rank": [round(v, 1) for v in rank_init_ms], "where": "communicator creation (spvo_comm_create = ncclCommInitRank, id broadcast through torch.distributed) before warm-up: not in the timed region"}
        out["step_loop"] = ("one Python call per front-end call (--py-loop)" if args.py_loop else
                            "blocks of stereoCallbacks handed to the host library's C loop (host/harness_capi.cpp: spvo_host_run_device_block), as the reference's C++ node runs them")
        dom = prof.get("conv:1") if args.graph == "vgg" and args.precision != "INT8" else None
        if args.fp32_split:
            out["config"]["workload"] = out["config"]["workload"].replace(" fp32 ", " fp32 [split mode: bf16x3 operands, 6 partial products] ")     # conv1b: 43 % of all CNN FLOPs
        if dom and dom["calls"]:
            avg_ms = dom["total_ms"] / dom["calls"]
            achieved = dom["flops"] / (avg_ms * 1e-3) / 1e12
            traffic = None                                                 # HBM bytes per launch from the committed PMC pass
            # The kernel family the engine runs conv1b on, and the multiply-adds its matrix instructions execute per multiply-add
            # of the direct convolution, come from the library (spvo_profile_stage_kernel): Winograd F(4x4,3x3) executes 36
            # multiplies per 4x4 outputs and channel pair instead of the direct method's 144 (1/4), F(2x2,3x3) 16 instead of 36
            # (4/9), the split mode six bf16 partial products per fp32 product (x6).  `achieved` / `frac` count what the matrix
            # pipe EXECUTES per launch; the layer's ALGORITHMIC rate (direct 3x3 convolution) is reported
            # beside it under its own name and never enters `frac` (it exceeds the peak: that is the point of Winograd).
            kfam, kfactor = ctx.stage_kernel("conv:1")
            # ... quoted only when the counter file was collected on THESE kernel sources: tools/collect_profiles_r06.sh stamps every
            # profiles/r06_*.json with the hash of csrc/ (tools/csrc_hash.py); a stamp that differs from the sources the running library
            # was built from gives `traffic: null, traffic_stale: true` instead of a number nobody re-measured
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            from csrc_hash import csrc_sha16
            src_tag = csrc_sha16(ROOT)
            pmc_file = {"conv_wino4_kernel": "r06_pmc.json"}.get(kfam)
            pmc = os.path.join(ROOT, "profiles", pmc_file) if pmc_file else None
            traffic_stale = None
            if pmc and os.path.exists(pmc) and (NET_H, NET_W) == (360, 1176):
                pj = json.load(open(pmc))
                traffic_stale = pj.get("csrc_sha16") != src_tag
                if not traffic_stale:
                    traffic = (pj.get(kfam) or {}).get("traffic_bytes_per_launch")
                    if traffic:   # the counter pass ran launches of TWO images; with trunk pairing the timed launches average more (per image the same)
                        traffic = int(traffic * dom["flops"] / (2.0 * 2 * NET_H * NET_W * 64 * 64 * 9))
            peak = FP32_MFMA_PEAK_TFLOPS if args.precision == "FP32" and not args.fp32_split else F16_MFMA_PEAK_TFLOPS
            kdesc = {"conv_wino4_kernel": "<POOL,RELU,TAG=1> (Winograd F(4x4,3x3), fp32)", "conv_wino2_kernel": "<POOL,RELU,TAG=1> (Winograd F(2x2,3x3), fp32)",
                     "conv_wino_kernel": "<POOL,RELU,TAG=1> (Winograd F(2x2,3x3), fp32)", "conv_wino64_kernel": "<POOL,RELU,TAG=1> (Winograd F(2x2,3x3), filters in registers, fp32)"}.get(kfam, "<KS=3,...,POOL,RELU>")
            counted = {0.25: " (Winograd F(4x4,3x3): 1/4 of the direct convolution's)", 4.0 / 9.0: " (Winograd F(2x2,3x3): 4/9 of the direct convolution's)",
                       6.0: " (split mode: six bf16 partial products per fp32 product)"}.get(kfactor, "")
            algorithmic = achieved
            executed_per_launch = dom["flops"] * kfactor
            achieved = executed_per_launch / (avg_ms * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": kfam + kdesc + " instance of op 1 = conv1b 64->64 @" + f"{NET_H}x{NET_W}, " + ("2 or 4 images per launch (trunk pairing: flops and time are the means over the timed launches)" if args.depth >= 4 and not args.no_pipeline else "2 images"),
                               "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                               "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_stale": traffic_stale, "csrc_sha16": src_tag,
                               "traffic_source": ("profiles/" + os.path.basename(pmc) + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes; FETCH_SIZE x 2 as the guide prescribes for gfx950; same csrc_sha16)") if traffic else None,
                               "avg_kernel_ms": round(avg_ms, 5), "flops_per_launch": executed_per_launch,
                               "flops_counted": "executed on the matrix pipe" + counted,
                               "algorithmic_flops_per_launch": dom["flops"], "algorithmic_tflops": round(algorithmic, 2),
                               "algorithmic_frac_of_peak": round(algorithmic / peak, 4)}
            if kfactor == 0.25:   # the same launch priced as round 2's kernel was: what fraction of the peak an F(2x2,3x3) kernel would need to be this fast
                out["roofline"]["frac_if_counted_as_f2x2"] = round(algorithmic * (4.0 / 9.0) / peak, 4)
        # NMS: round launches are enqueued with the submission; a heat map whose decisions are still open after them is continued by
        # the HOST (spvo_detect_wait), synchronously behind everything queued on the tail stream -- in the pipelined loop that is a
        # stall of more than a trunk.  Counted over the timed blocks: 0 is what the default of four launches is chosen for.
        if profile:
            out["nms_host_continuations"] = {"timed_region": int(prof.get("nms_redo", {}).get("calls", 0)), "timed_steps": args.steps * len(block_times)}
        any_stage = next((v for k, v in prof_all.items() if k.startswith("conv:") and v["calls"]), None)
        if any_stage:   # stage breakdown: the separate pass with every stage timed (it runs ~7 % slower than the timed region)
            calls = any_stage["calls"]
            conv_ms = sum(v["total_ms"] for k, v in prof_all.items() if k.startswith("conv:")) / calls
            conv_fl = sum(v["flops"] for k, v in prof_all.items() if k.startswith("conv:"))
            out["stages_ms"] = {k: round(v["total_ms"] / max(v["calls"], 1), 4) for k, v in prof_all.items()
                                if not k.startswith(("conv:", "pool:", "l2norm:", "dwconv:"))}
            out["stages_ms"]["conv_stack_sum"] = round(conv_ms, 4)
            out["stages_ms"]["_source"] = "separate untimed pass with every stage bracketed by events"
            if args.dump_ops:   # per-layer times of the network (variant tuning)
                out["net_ops_ms"] = {k: round(v["total_ms"] / max(v["calls"], 1), 4) for k, v in prof_all.items()
                                     if k.startswith(("conv:", "pool:", "l2norm:", "dwconv:"))}
            out["conv_stack_tflops"] = round(conv_fl / (conv_ms * 1e-3) / 1e12, 2)
            mg = prof_all.get("match_gemm")
            if mg and mg["calls"] and mg["flops"] > 0:   # north_star: "MFMA utilisation on the distance GEMM" -- by HIP-event time of the launch, not by a counter quotient
                mms = mg["total_ms"] / mg["calls"]
                mtf = mg["flops"] / (mms * 1e-3) / 1e12
                mpeak = 2 * F16_MFMA_PEAK_TFLOPS if args.match_fp8 else FP32_MFMA_PEAK_TFLOPS
                out["roofline_matcher"] = {"kernel": "match_gemm_kernel" + ("<fp8 shortlist>" if args.match_fp8 else "<fp32, fused per-row reduction>") + ": the frame's two jobs (stereo, temporal) in one launch",
                                           "bound": "mfma", "avg_kernel_ms": round(mms, 5), "flops_per_launch": mg["flops"], "achieved": round(mtf, 2), "peak": mpeak, "unit": "TFLOP/s",
                                           "frac": round(mtf / mpeak, 4),
                                           "where": "inside the pipelined loop (stage pass: HIP events around the launch on the tail stream, which shares the chip with the next pairs' trunk); "
                                                    "un-contended: host_interface.synchronous.roofline_matcher"}
            # north_star: "rocprof reports achieved HBM GB/s on the conv stack".  Bytes per forward pass from the committed counter passes
            # (FETCH_SIZE x 2 + WRITE_SIZE per layer, tools/pmc_layers.py) over the stack's time measured HERE (sum of the layers' HIP-event
            # times in the pass above); the algorithmic bytes beside it.
            pl_path = os.path.join(ROOT, "profiles", "r06_pmc_layers.json")
            if "roofline" in out and headline and (NET_H, NET_W) == (360, 1176) and os.path.exists(pl_path):
                plj = json.load(open(pl_path))
                cs = plj.get("conv_stack", {})
                out["roofline"]["conv_stack_traffic_stale"] = plj.get("csrc_sha16") != out["roofline"]["csrc_sha16"]
                if cs.get("traffic_MB") and not out["roofline"]["conv_stack_traffic_stale"]:
                    # the counter pass ran two images per launch; the stage pass above averages launches of two and of four (trunk pairing):
                    # bytes per launch scale with the images, i.e. with the mean algorithmic flops per launch (141.44 GFLOP at two images without the heads)
                    pairs_per_launch = conv_fl / 141.44e9   # (the stages named conv:<i>: the fused heads launch is a stage of its own)
                    out["roofline"]["conv_stack_traffic"] = int(cs["traffic_MB"] * 1e6 * pairs_per_launch)
                    out["roofline"]["conv_stack_algorithmic_bytes"] = int(cs["algorithmic_MB"] * 1e6 * pairs_per_launch)
                    out["roofline"]["conv_stack_pairs_per_launch"] = round(pairs_per_launch, 3)
                    out["roofline"]["conv_stack_hbm_gbps"] = round(cs["traffic_MB"] * 1e6 * pairs_per_launch / (conv_ms * 1e-3) / 1e9, 1)
                    out["roofline"]["conv_stack_frac_of_hbm_peak"] = round(cs["traffic_MB"] * 1e6 * pairs_per_launch / (conv_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
                    out["roofline"]["conv_stack_traffic_source"] = "profiles/r06_pmc_layers.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE over a forward-only loop, per layer; counters include Infinity-Cache hits; same csrc_sha16) / conv_stack_sum of this run"
        if world == 1 and extras and "split" in legs:
            try:
                # Informational, never `value`: the same workload with the FP32 engine in its opt-in split mode (every fp32 operand as
                # three bf16 pieces, six partial products on the bf16 matrix pipe, fp32 accumulation: results agree with the
                # native engine to fp32 rounding level, tests/test_gpu_network.py::test_fp32_split_mode_*).
                fe.close()
                capi.set_tuning("fp32_split", 1)
                try:
                    fe = host.FrontEnd(tmp, prefix="superpoint_pretrained", selector="KNN", cross_check=True, batch=2,
                                       height=NET_H, width=NET_W, conf_thresh=0.015, dist_thresh=4, border_remove=4,
                                       stereo_threshold=2.0, min_disparity=0.25, refinement_degree=4, precision="FP32")
                finally:
                    capi.clear_tuning()
                if fe.engine_loaded:
                    run_frames(0, args.warmup)
                    fe.finish_solve()
                    e2, sp2, fs2 = leg_frames()
                    out["fp32_split_mode"] = {"value": round(args.steps / e2, 2), "unit": "stereo frames/s", "ms_per_step": round(1e3 * e2 / args.steps, 4), **sp2, **fs2,
                                              "note": "opt-in (spvo_set_fp32_split / bench.py --fp32-split), not the headline: fp32 operands as 3 bf16 pieces, "
                                                      "6 partial products per product, fp32 accumulate; fp32-equivalent results"}
            except Exception as exc:   # the headline line must survive a failure of this informational part
                out["fp32_split_mode"] = {"error": repr(exc)}
        if world == 1 and extras and "host" in legs:
            try:
                # The reference's own entry point, addStereoImagePair(cv::Mat&, ...) (node.cpp:175): images in HOST memory (as
                # cv_bridge hands them over), resized images and descriptors copied back into images_dq / descriptors_dq -- PCIe
                # both ways inside the timed region.  Never `value`.  "synchronous" = the unchanged node's call sequence, one pair at
                # a time (nothing can overlap across frames: the per-frame latency); "lookahead" = the next --depth pairs announced
                # through prefetchStereoImagePair as a node can do from its message queue (node.cpp:307-313: queue of 20).
                fe.close()
                fe = host.FrontEnd(tmp, prefix="superpoint_pretrained", selector="KNN", cross_check=True, batch=2,
                                   height=NET_H, width=NET_W, conf_thresh=0.015, dist_thresh=4, border_remove=4,
                                   stereo_threshold=2.0, min_disparity=0.25, refinement_degree=4, precision="FP32")
                # one cv::Mat pair per POSITION of the cycle (the front end recognises an announced pair by its data pointers: see cycle_buffers)
                mats = [(fe.make_image(frames[f][0]), fe.make_image(frames[f][1])) for f in order]
                hi = {}
                # images_dq / descriptors_dq: the class fills them inside addStereoImagePair by default (reference-observable state, nn.cpp:154,
                # 494-498); "synchronous" and "lookahead" OPT IN to setDeferredHostCopies(true) -- the two bulk copies made while the solver's
                # kernels run -- and say so; "synchronous_default_copies" is the class exactly as constructed.
                for name, depth, defer in (("synchronous", 0, True), ("synchronous_default_copies", 0, False), ("lookahead", args.depth, True)):
                    lat, ann = [], {}
                    fe.set_deferred_copies(defer)

                    def hstep(i, depth=depth, lat=lat, ann=ann):
                        a = [mats[(i + 1 + d) % len(mats)] if d < depth else None for d in range(4)]
                        m = mats[i % len(mats)]
                        t_in = time.perf_counter()
                        for f in range(i, i + depth + 1):
                            ann.setdefault(f, t_in)                         # the first call that hands frame f over
                        r = fe.step_host(m[0], m[1], P_l, P_r, a[0], a[1], deferred_solve=depth > 0 and deferred, next3_pair=a[2], next4_pair=a[3])
                        if r is not None:                                   # the pose of this frame, or -- deferred solve -- of the one before
                            f = i - 1 if depth > 0 and deferred else i
                            if f in ann:
                                lat.append(1e3 * (time.perf_counter() - ann.pop(f)))
                        return r
                    for i in range(args.warmup):
                        hstep(i)
                    fe.finish_solve()
                    lat.clear()
                    e3, sp3 = leg(hstep, lambda: fe.finish_solve())
                    ls = np.sort(np.asarray(lat)) if lat else np.zeros(1)
                    hi[name] = {"value": round(args.steps / e3, 2), "ms_per_step": round(1e3 * e3 / args.steps, 4), **sp3,
                                "deferred_host_copies": bool(defer),
                                "latency_ms": {"p50": round(float(ls[ls.size // 2]), 3), "p99": round(float(ls[min(ls.size - 1, int(0.99 * ls.size))]), 3), "frames": int(ls.size),
                                               "definition": "first call that hands the pair over -> its pose returned (Python clock around the calls): the reference's t_total for the synchronous sequence"}}
                    if depth == 0 and defer:
                        # the stage table of THIS leg (the headline's `stages_ms` describes the pipelined loop): host wall time of the node's
                        # three kinds of calls, then -- a second short pass with every stage bracketed by events -- what the device did in them
                        import ctypes as C
                        Plc, Prc = np.ascontiguousarray(P_l, np.float64), np.ascontiguousarray(P_r, np.float64)
                        hctx = fe.context()
                        for timed_stages in (False, True):
                            acc = np.zeros(3)
                            if timed_stages:
                                hctx.profile_only(None)
                                hctx.profile_enable(True)
                                hctx.profile_reset()
                            for i in range(100):
                                m = mats[i % len(mats)]
                                t0 = time.perf_counter()
                                fe.lib.spvo_host_add_stereo_pair_mat(fe.h, C.c_void_p(m[0]), C.c_void_p(m[1]), host._p(Plc), host._p(Prc))
                                t1 = time.perf_counter()
                                fe.match_descriptors(host.CURR_LEFT_CURR_RIGHT)
                                if fe.dq_size() >= 4:
                                    fe.match_descriptors(host.CURR_LEFT_PREV_LEFT)
                                    t2 = time.perf_counter()
                                    fe.solve_stereo_odometry()
                                    acc += [t1 - t0, t2 - t1, time.perf_counter() - t2]
                            if not timed_stages:
                                hi[name]["host_calls_ms"] = {"addStereoImagePair": round(1e3 * acc[0] / 100, 4), "matchDescriptors_x2": round(1e3 * acc[1] / 100, 4),
                                                             "solveStereoOdometry": round(1e3 * acc[2] / 100, 4)}
                            else:
                                barrier()
                                hp = hctx.profile()
                                hctx.profile_enable(False)
                                hi[name]["device_stages_ms"] = {k: round(v["total_ms"] / max(v["calls"], 1), 4) for k, v in hp.items()
                                                                if v["calls"] and not k.startswith(("conv:", "pool:", "l2norm:", "dwconv:"))}
                                hi[name]["device_stages_ms"]["conv_stack_sum"] = round(sum(v["total_ms"] / v["calls"] for k, v in hp.items() if k.startswith("conv:") and v["calls"]), 4)
                                hi[name]["device_stages_ms"]["_source"] = "second pass of 100 synchronous steps with every stage bracketed by HIP events (slower than the timed blocks)"
                                mg = hp.get("match_gemm")
                                if mg and mg["calls"] and mg["flops"] > 0:
                                    mms = mg["total_ms"] / mg["calls"]
                                    hi[name]["roofline_matcher"] = {"avg_kernel_ms": round(mms, 5), "achieved": round(mg["flops"] / (mms * 1e-3) / 1e12, 2), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                                                    "frac": round(mg["flops"] / (mms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4), "where": "alone on the chip (synchronous call sequence), HIP-event time"}
                out["host_interface"] = {"unit": "stereo frames/s", **hi,
                                         "note": "addStereoImagePair(cv::Mat&, ...): 2 x 0.47 MB host images in, 2 x 0.42 MB resized images + 2 x 1 MB "
                                                 "descriptors out per pair (PCIe inclusive); the headline `value` has the images resident in HBM.  "
                                                 "deferred_host_copies: setDeferredHostCopies(true), an opt-in of this script -- the class's default fills "
                                                 "images_dq / descriptors_dq inside addStereoImagePair as the reference does (synchronous_default_copies)"}
            except Exception as exc:   # the headline line must survive a failure of this informational part
                out["host_interface"] = {"error": repr(exc)}
        if world == 1 and extras and "trained" in legs:
            try:
                # Second workload, never `value`: the reference's TRAINED sp_squeeze graph (tests/golden/sp_squeeze.spvw = its ONNX file
                # re-packed), FP32, same stream and size.  With trained weights the geometry is real: the gate accepts, the LM refinement
                # iterates and is kept -- the solver's cost is measured, not gated away (no SPVO_QUIET: nothing to hide).
                import shutil
                fe.close()
                os.makedirs(os.path.join(tmp, "trained", "laptop"), exist_ok=True)
                shutil.copyfile(os.path.join(ROOT, "tests", "golden", "sp_squeeze.spvw"),
                                os.path.join(tmp, "trained", "laptop", weights.engine_name("sp_squeeze", 2, NET_H, NET_W, "FP32")))
                fe = host.FrontEnd(os.path.join(tmp, "trained"), prefix="sp_squeeze", selector="KNN", cross_check=True, batch=2,
                                   height=NET_H, width=NET_W, conf_thresh=0.015, dist_thresh=4, border_remove=4,
                                   stereo_threshold=2.0, min_disparity=0.25, refinement_degree=4, precision="FP32")
                if fe.engine_loaded:
                    # frames 0..7 over and over: seven real forward steps and one jump back to the start per cycle.  (The ping-pong
                    # order of the headline reverses the motion twice per cycle; the reference's acceleration gate, base.cpp:251-260,
                    # then rejects the pose and keeps its stale prediction until the motion reverses again: half of all frames.)
                    cyc = list(range(SEQ_LEN))
                    run_frames(0, args.warmup, cyc)
                    fe.finish_solve()
                    e4, sp4, fs4 = leg_frames(cyc)
                    out["trained_workload"] = {"graph": "sp_squeeze (the reference's trained ONNX graph, 844353 params), FP32, net %dx%d; frames 0..7 cyclically "
                                                        "(one jump back per cycle, which the gate rejects)" % (NET_H, NET_W),
                                               "value": round(args.steps / e4, 2), "unit": "stereo frames/s", "ms_per_step": round(1e3 * e4 / args.steps, 4), **sp4, **fs4}
            except Exception as exc:   # the headline line must survive a failure of this informational part
                out["trained_workload"] = {"error": repr(exc)}
        if world == 1 and extras and "classic" in legs:
            try:
                # BASELINE config 1's front end on the GPU, never `value`: ClassicFeatureFrontEnd(ORB, ORB, BF, KNN) as node.cpp:353-360
                # constructs it -- ORB (spvo_orb_detect) and Hamming matching (spvo_match_hamming) as HIP kernels, the same solver --
                # one pair at a time through the unchanged call sequence, host images in, at the native 376 x 1241.  The CPU
                # restatement of the same front end is timed in cpu_baseline.config1_orb_front_end.
                n_c = 5 + min(args.steps, 100)
                seqc = [frames[order[i % len(order)]] for i in range(n_c)]
                poses_c, stats_c, sec_c = host.classic_sequence(seqc, P_l, P_r, "KNN", True, 2.0, 4, warm=5)
                out["classic_front_end_gpu"] = {"value": round((n_c - 5) / sec_c, 2), "unit": "stereo frames/s", "ms_per_step": round(1e3 * sec_c / (n_c - 5), 4),
                                                "keypoints_per_image": int(np.median(stats_c[5:, 0])), "stereo_matches": int(np.median(stats_c[5:, 2])),
                                                "pnp_inliers": int(np.median(stats_c[5:, 3])),
                                                "note": "ORB 2000 features / 8 levels / scale 1.2 / FAST 20 (feature_detection_classic.cpp:13-24) + Hamming BF + KNN 0.8 on the GPU, "
                                                        "synchronous stereoCallback on host images at 376x1241; ORB as restated in oracle/cpu/orb_cpu.inc (bit-exact against THAT, tests/test_gpu_orb.py): "
                                                        "seeded test pairs and fixed rounding choices, so descriptors are not comparable with OpenCV's cv::ORB"}
            except Exception as exc:   # the headline line must survive a failure of this informational part
                out["classic_front_end_gpu"] = {"error": repr(exc)}
        if world == 1 and extras and "configs" in legs:
            # The other GPU configurations of BASELINE.json and the second network size of SURVEY.md section 8d, never `value`: each is
            # the SAME loop (two pairs handed over ahead, deferred solve) on an engine of its own, timed like the other legs (blocks of
            # >= 100 steps, the median block), followed by a short pass with every stage bracketed by events that names the dominant
            # convolution launch and the fraction of its roofline it reaches.
            from spvo import quant
            other_specs = [
                ("native_376x1240", "vgg", "FP32", (376, 1240), 1000, False,
                 "BASELINE configs[1] at the native network size (SURVEY.md section 8d: report both sizes)"),
                ("config3_fp16_192x640", "vgg", "FP16", (192, 640), 1000, False,
                 "BASELINE configs[2]: SuperPoint fp16, 640x192 downscaled input (engine_generation.py:20-24 FP16 engines)"),
                ("config5_int8_mbv1_2048kp_fp8", "sp_mbv1", "INT8", (360, 1176), 2048, True,
                 "BASELINE configs[4]: MobileNet-backbone SuperPoint int8 + 2048-keypoint cap, fp8 shortlist GEMM + exact fp32 re-rank"),
            ]
            out["other_configs"] = {}
            for oname, ograph, oprec, (oh, ow), okp, ofp8, owhat in other_specs:
                try:
                    fe.close()
                    oplan = weights.vgg_plan(seed=0) if ograph == "vgg" else weights.load(os.path.join(ROOT, "tests", "golden", ograph + ".spvw"))
                    o_params = int(sum(op.weight.size + op.bias.size for op in oplan.ops if op.weight is not None))
                    if oprec == "INT8":
                        ocal = [quant.calibration_inputs(oplan, frames[k], oh, ow) for k in (0, SEQ_LEN // 2, SEQ_LEN - 1)]
                        oplan.act_scales = quant.calibrate(oplan, ocal, oh, ow)
                    oplan.precision = oprec
                    oprefix = "superpoint_pretrained" if ograph == "vgg" else ograph
                    odir = os.path.join(tmp, oname)
                    os.makedirs(os.path.join(odir, "laptop"), exist_ok=True)
                    weights.save(oplan, os.path.join(odir, "laptop", weights.engine_name(oprefix, 2, oh, ow, oprec)))
                    host.set_options(device=local_rank, max_keypoints=okp, match_fp8=1 if ofp8 else 0)
                    two_tails = oprec in ("FP16", "INT8") and int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) >= 8 and "SPVO_TUNE_TAIL_STREAMS" not in os.environ
                    if two_tails:
                        capi.set_tuning("tail_streams", 2)   # read when the engine is loaded; the FP32 legs keep one tail stream
                    keep2 = oprec == "FP16" and "SPVO_TUNE_SOLVE_KEEP" not in os.environ
                    if "SPVO_TUNE_SOLVE_KEEP" not in os.environ:
                        capi.set_tuning("solve_keep", 2 if keep2 else 1)   # read when the front end creates its context, and by the block loop: reset behind the leg
                    try:
                        fe = host.FrontEnd(odir, prefix=oprefix, selector="KNN", cross_check=True, batch=2, height=oh, width=ow, conf_thresh=0.015,
                                           dist_thresh=4, border_remove=4, stereo_threshold=2.0, min_disparity=0.25, refinement_degree=4, precision=oprec)
                    finally:
                        host.set_options(device=local_rank, max_keypoints=args.max_keypoints, match_fp8=1 if args.match_fp8 else 0)
                        if two_tails:
                            capi.set_tuning("tail_streams", 1)
                    if not fe.engine_loaded:
                        raise RuntimeError("engine load failed: " + fe.last_error)
                    run_frames(0, args.warmup)
                    fe.finish_solve()
                    eo, spo, fso = leg_frames()
                    rec = {"what": owhat, "value": round(args.steps / eo, 2), "unit": "stereo frames/s", "ms_per_step": round(1e3 * eo / args.steps, 4), **spo, **fso,
                           "dtype": {"FP32": "f32", "FP16": "f16", "INT8": "i8"}[oprec], "tail_streams": 2 if two_tails else 1, "solves_kept_pending": 2 if keep2 else capi.get_tuning("solve_keep", 1),
                           "hw_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "4")),
                           "workload": (f"SuperPoint VGG {oprec.lower()} (seeded synthetic weights, {o_params} params)" if ograph == "vgg" else
                                        f"SuperPoint {ograph} {oprec.lower()} (the reference's TRAINED ONNX graph, {o_params} params; activation scales calibrated on this stream)")
                                       + f", 1241x376 stereo pairs, net {oh}x{ow}, {okp} kp cap" + (", fp8 shortlist + exact re-rank" if ofp8 else "")}
                    octx = fe.context()
                    octx.profile_only(None)
                    octx.profile_enable(True)
                    octx.profile_reset()
                    run_frames(0, 50)
                    fe.finish_solve()
                    barrier()
                    oprof = octx.profile()
                    octx.profile_enable(False)
                    convs = {k: v for k, v in oprof.items() if k.startswith("conv:") and v["calls"] and v["flops"] > 0}
                    if convs:
                        dk = max(convs, key=lambda k: convs[k]["total_ms"])
                        dms = convs[dk]["total_ms"] / convs[dk]["calls"]
                        kfam, kfac = octx.stage_kernel(dk)
                        opeak, ounit = {"FP32": (FP32_MFMA_PEAK_TFLOPS, "TFLOP/s"), "FP16": (F16_MFMA_PEAK_TFLOPS, "TFLOP/s"), "INT8": (I8_MFMA_PEAK_TOPS, "TOP/s")}[oprec]
                        oexec = convs[dk]["flops"] * kfac / (dms * 1e-3) / 1e12            # `flops` = algorithmic operations of ONE launch
                        stack_ms = sum(v["total_ms"] / v["calls"] for v in convs.values())
                        obytes = convs[dk].get("bytes", 0.0)                                  # algorithmic HBM bytes of one launch, where the library states them
                        ogbps = obytes / (dms * 1e-3) / 1e9 if obytes else None
                        # the roofline that bounds the launch: the larger of (executed operations / matrix peak) and (algorithmic bytes / 8 TB/s)
                        hbm_bound = bool(obytes) and obytes / (HBM_PEAK_GBPS * 1e9) > convs[dk]["flops"] * kfac / (opeak * 1e12)
                        rec["dominant_kernel"] = {"stage": dk, "kernel": kfam, "avg_kernel_ms": round(dms, 5), "executed_per_algorithmic": round(kfac, 4),
                                                  "bound": "hbm" if hbm_bound else "mfma",
                                                  "achieved": round(oexec, 2), "peak": opeak, "unit": ounit, "frac": round(oexec / opeak, 4),
                                                  "algorithmic_GBps": round(ogbps, 1) if ogbps else None, "frac_of_hbm_peak": round(ogbps / HBM_PEAK_GBPS, 4) if ogbps else None,
                                                  "conv_stack_sum_ms": round(stack_ms, 4),
                                                  "_source": "separate pass of 50 steps with every stage bracketed by HIP events (runs ~7 % slower than the timed blocks)"}
                        # HBM traffic of that launch from the committed per-layer counter pass of the same engine (two images per launch there; scaled to
                        # this leg's mean images per launch by the algorithmic operations), quoted only when collected on THESE kernel sources
                        pmc_name = {"config3_fp16_192x640": "r06_pmc_layers_fp16_192x640.json", "config5_int8_mbv1_2048kp_fp8": "r06_pmc_layers_int8.json",
                                    "native_376x1240": None}.get(oname)
                        ppath = os.path.join(ROOT, "profiles", pmc_name) if pmc_name else None
                        if ppath and os.path.exists(ppath):
                            sys.path.insert(0, os.path.join(ROOT, "tools"))
                            from csrc_hash import csrc_sha16
                            pj = json.load(open(ppath))
                            stale = pj.get("csrc_sha16") != csrc_sha16(ROOT)
                            layers_pj = pj.get("layers", [])
                            # the counter file lists the engine's launches in order; the dominant stage "conv:<i>" is matched by its name (INT8) or its
                            # position among the stages of this pass (FP16: the file names layers conv1a ...)
                            stage_names = [k for k in oprof if k.startswith(("conv:", "heads")) and oprof[k]["calls"]]
                            row = next((l for l in layers_pj if l.get("layer") == dk), None)
                            if row is None and dk in stage_names and len(layers_pj) >= len(stage_names):
                                row = layers_pj[stage_names.index(dk)]
                            rec["dominant_kernel"]["traffic_stale"] = stale
                            if row is not None and not stale and row.get("traffic_MB"):
                                two_img_ops = convs[dk]["flops"]
                                rec["dominant_kernel"].update({"traffic": int(row["traffic_MB"] * 1e6), "traffic_over_algorithmic": row.get("traffic_over_algorithmic"),
                                                               "traffic_kernel": row.get("kernel_name", "")[:60],
                                                               "traffic_source": "profiles/" + pmc_name + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, 2 x FETCH + WRITE; two images per launch; same csrc_sha16)"})
                            else:
                                rec["dominant_kernel"]["traffic"] = None
                    out["other_configs"][oname] = rec
                except Exception as exc:   # the headline line must survive a failure of this informational part
                    out["other_configs"][oname] = {"error": repr(exc)}
                finally:
                    if "SPVO_TUNE_SOLVE_KEEP" not in os.environ:
                        capi.set_tuning("solve_keep", 2 if keep2_main else 1)   # (the leg's setting does not outlive it)
        if args.full and not args.no_cpu_baseline and world == 1 and headline:
            try:
                # BASELINE.json's metric is "stereo frames/sec ...; ATE vs ref": the trajectory half, from an UNTIMED pass.  ATE_FRAMES synthetic frames
                # with exact ground truth through the reference's TRAINED sp_squeeze graph (the seeded VGG weights of the headline track nothing), FP32,
                # net size of the headline, the unchanged node's call sequence: once through the GPU front end, once end to end through oracle/cpu
                # (its own network, NMS, matcher and solver: inside cpu_baseline, the only place this script touches oracle/).
                import shutil
                fe.close()
                ate_frames, ate_poses = cached_ate_sequence(synth, tex)
                sq_path = os.path.join(ROOT, "tests", "golden", "sp_squeeze.spvw")
                os.makedirs(os.path.join(tmp, "ate", "laptop"), exist_ok=True)
                shutil.copyfile(sq_path, os.path.join(tmp, "ate", "laptop", weights.engine_name("sp_squeeze", 2, NET_H, NET_W, "FP32")))
                cb = cpu_baseline(frames, P_l, P_r, engine_path, order, ate_frames=ate_frames, ate_weights=sq_path)
                cpu_rows, ate_cpu = cb.pop("_per_frame"), cb.pop("_ate_cpu")
                out["cpu_baseline"] = cb
                try:
                    # like for like: the GPU front end (headline engine, synchronous call sequence, fresh state) over EXACTLY the frame indices the CPU
                    # sample ran (its warm-ups included), outcome by outcome
                    g = gpu_sequence(host, tmp, "superpoint_pretrained", [frames[order[k % len(order)]] for k in range(len(cpu_rows))], P_l, P_r)
                    c = cpu_rows
                    warm = 5
                    cb["solver_stats_same_frames"] = {
                        "frames": int(len(c) - warm), "frame_indices": f"frames {warm}..{len(c) - 1} of the ping-pong cycle after a reset, both sides (the CPU sample's frames; frames 0..{warm - 1} are run and not counted)",
                        "gpu": outcome_stats(g[warm:]), "cpu": outcome_stats(c[warm:]),
                        "accepted_flag_agreement": round(float((g[1:, 1] == c[1:, 1]).mean()), 4), "refined_flag_agreement": round(float((g[1:, 2] == c[1:, 2]).mean()), 4),
                        "pnp_ok_agreement": round(float((g[1:, 0] == c[1:, 0]).mean()), 4),
                        "mean_abs_inlier_difference": round(float(np.abs(g[1:, 4] - c[1:, 4]).mean()), 2),
                        "pose_t_difference_m": {"median": float(np.median(np.abs(g[1:, 11:14] - c[1:, 11:14]).max(axis=1))), "max": float(np.abs(g[1:, 11:14] - c[1:, 11:14]).max())},
                        "note": "GPU = libspvo through the host class, CPU = oracle/cpu, each on its OWN features (two fp32 networks that agree to ~1e-6: a few keypoints near the "
                                "threshold differ, so inlier counts differ by a few; a flag that differs is a frame whose acceleration sat at the gate's threshold)"}
                except Exception as exc:
                    cb["solver_stats_same_frames"] = {"error": repr(exc)}
                try:
                    ga = gpu_sequence(host, os.path.join(tmp, "ate"), "sp_squeeze", ate_frames, P_l, P_r)
                    gt_steps = []
                    for k in range(1, ATE_FRAMES):
                        gt_steps.append(synth.relative_pose(ate_poses[k - 1], ate_poses[k]))
                    traj_gt = integrate_steps(gt_steps)
                    traj_gpu = integrate_steps([(r[7:11], r[11:14]) for r in ga[1:]])
                    path_len = float(np.sum(np.linalg.norm(np.diff(traj_gt, axis=0), axis=1)))
                    rec = {"frames": ATE_FRAMES, "path_length_m": round(path_len, 2),
                           "workload": f"sp_squeeze (the reference's trained ONNX graph) FP32, net {NET_H}x{NET_W}, 1241x376 synthetic stereo sequence with exact ground truth "
                                       f"(spvo/synth.py, seed {ATE_SEED}), KNN 0.8, refinement degree 4, the unchanged node's call sequence; untimed",
                           "gpu_vs_gt_rmse_m": round(ate_rmse(traj_gpu, traj_gt)[0], 5), "gpu_vs_gt_max_m": round(ate_rmse(traj_gpu, traj_gt)[1], 5),
                           "gpu_solver": outcome_stats(ga[1:]),
                           "definition": "RMSE of camera centres after chaining the per-frame cam0_curr_T_cam0_prev (visual_odometry_node.cpp:118-127), no alignment (both start at identity); "
                                         "the reference publishes no ATE number (plots only, VO/figures), so there is no reference tolerance to quote"}
                    if isinstance(ate_cpu, list) and len(ate_cpu) == ATE_FRAMES:
                        ca = np.array(ate_cpu, np.float64)
                        traj_cpu = integrate_steps([(r[7:11], r[11:14]) for r in ca[1:]])
                        rec.update({"gpu_vs_cpu_rmse_m": float(f"{ate_rmse(traj_gpu, traj_cpu)[0]:.3e}"), "gpu_vs_cpu_max_m": float(f"{ate_rmse(traj_gpu, traj_cpu)[1]:.3e}"),
                                    "gpu_vs_cpu_gate_m": 1e-3,
                                    "cpu_vs_gt_rmse_m": round(ate_rmse(traj_cpu, traj_gt)[0], 5), "cpu_solver": outcome_stats(ca[1:]),
                                    "accepted_flag_agreement": round(float((ga[1:, 1] == ca[1:, 1]).mean()), 4),
                                    "cpu": "oracle/cpu end to end on its own features (kind: port)"})
                    else:
                        rec["cpu_error"] = str(ate_cpu)
                    out["ate"] = rec
                except Exception as exc:
                    out["ate"] = {"error": repr(exc)}
                fe = host.FrontEnd(tmp, prefix="superpoint_pretrained", selector="KNN", cross_check=True, batch=2, height=NET_H, width=NET_W, conf_thresh=0.015, dist_thresh=4,
                                   border_remove=4, stereo_threshold=2.0, min_disparity=0.25, refinement_degree=4, precision="FP32")   # (closed below)
            except Exception as exc:   # the headline line must survive a failure of this informational part
                out["cpu_baseline"] = {"error": repr(exc)}
        print(json.dumps(out), flush=True)
    fe.close()
    pg.close()
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
