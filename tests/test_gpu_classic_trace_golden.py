"""What ClassicFeatureFrontEnd leaves behind, frame by frame, pinned to a recording: for every detector / descriptor pair that runs, per image
and with the features resident on the device, the trace digests of host.classic_sequence (every field of every keypoint, every byte of every
descriptor row, the three match lists, the inlier sets), the counts, the poses and the number of pairs that stayed resident are those of
tests/golden/classic_front_end_trace.json EXACTLY.  The other host-class tests compare a per-image run with a resident run of the same build,
so a field both paths get wrong in the same way (cv::KeyPoint::angle, class_id: neither feeds the matcher or the solver) passes them; this
one holds the host class to what it produced when the fixture was recorded.

Six pairs per run: the ring of four slot pairs wraps once.  The fixture is written by running this module as a script on the GPU
(python tests/test_gpu_classic_trace_golden.py [path]) and in no other way; the test never writes it."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "classic_front_end_trace.json")
N_FRAMES = 6

pytestmark = pytest.mark.gpu

PAIRS = [("ORB", "ORB"), ("ShiTomasi", "ORB"), ("FAST", "ORB"), ("ShiTomasi", "BRISK"), ("FAST", "BRISK"), ("BRISK", "BRISK"), ("AKAZE", "BRISK"), ("AKAZE", "AKAZE"),
         ("SIFT", "SIFT")]
MIXED = "FAST+ORB resident, capacity = median rows"      # resident_capacity comes from the per-image run of the same pair: fitting and falling-back pairs mix


def _runs():
    """name -> (selector, keyword arguments of host.classic_sequence)"""
    runs = {}
    for det, desc in PAIRS:
        kw = dict(detector=det, descriptor=desc, akaze_descriptor=(desc == "AKAZE"))
        runs["%s+%s" % (det, desc)] = ("KNN", kw)
        runs["%s+%s resident" % (det, desc)] = ("KNN", dict(kw, resident=True))
    runs["BRISK+BRISK resident, brisk_resident"] = ("KNN", dict(detector="BRISK", descriptor="BRISK", resident=True, brisk_resident=True))
    runs[MIXED] = ("KNN", dict(detector="FAST", descriptor="ORB", resident=True))
    runs["ORB+ORB NN cross-check"] = ("NN", dict(detector="ORB", descriptor="ORB"))
    runs["ORB+ORB NN cross-check resident"] = ("NN", dict(detector="ORB", descriptor="ORB", resident=True))
    return runs


RUNS = _runs()


def load_sequence():
    from spvo import synth
    frames, _, P_l, P_r = synth.stereo_sequence(12, os.path.join(ROOT, "tests", "golden", "images", "0000000000.png"), seed=0)
    return frames[:N_FRAMES], P_l, P_r


def frames_sha256(frames):
    h = hashlib.sha256()
    for L, R in frames:
        h.update(np.ascontiguousarray(L, np.uint8).tobytes())
        h.update(np.ascontiguousarray(R, np.uint8).tobytes())
    return h.hexdigest()


def median_rows(stats):
    """the mixed run's slot capacity: the median of the twelve row counts (left and right of six pairs) of the per-image FAST + ORB run"""
    return int(np.median(np.asarray(stats)[:, :2]))


def replay(name, frames, P_l, P_r, capacity=0):
    """-> what the fixture holds for one run"""
    from spvo import host
    selector, kw = RUNS[name]
    poses, stats, _, digest = host.classic_sequence(frames, P_l, P_r, selector, True, 2.0, 4, input_size=(120, 392), trace=True, resident_capacity=capacity, **kw)
    return dict(digests=[["%016x" % int(v) for v in row] for row in digest], stats=[[int(v) for v in row] for row in stats],
                poses=[[float(v).hex() for v in row] for row in poses], resident_pairs=host.classic_resident_pairs())


@pytest.fixture(scope="module")
def sequence():
    return load_sequence()


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_names_every_run(fixture):
    assert sorted(fixture["runs"]) == sorted(RUNS)


@pytest.mark.parametrize("name", list(RUNS))
def test_trace_equals_the_recording(sequence, fixture, name):
    frames, P_l, P_r = sequence
    assert frames_sha256(frames) == fixture["frames_sha256"], \
        "the synthetic sequence changed: spvo.synth.stereo_sequence no longer gives the frames the fixture was recorded on, and the fixture must be re-recorded"
    want = fixture["runs"][name]
    got = replay(name, frames, P_l, P_r, capacity=median_rows(fixture["runs"]["FAST+ORB"]["stats"]) if name == MIXED else 0)
    assert got["stats"] == want["stats"]
    assert got["resident_pairs"] == want["resident_pairs"]
    cols = ["keypoints L", "descriptors L", "keypoints R", "descriptors R", "stereo matches", "temporal matches", "previous stereo matches + map", "inlier sets"]
    for k in range(N_FRAMES):
        for c in range(8):
            assert got["digests"][k][c] == want["digests"][k][c], "frame %d, %s" % (k, cols[c])
    assert got["poses"] == want["poses"]


def record(path):
    frames, P_l, P_r = load_sequence()
    out = {}
    for name in RUNS:                                    # (the per-image FAST + ORB run comes before the mixed one)
        run = replay(name, frames, P_l, P_r, capacity=median_rows(out["FAST+ORB"]["stats"]) if name == MIXED else 0)
        stats = np.asarray(run["stats"])
        # not vacuous: features on every image, and a solve that found something
        assert stats[:, :2].min() > 50, (name, stats.tolist())
        assert stats[:, 3].max() > 10, (name, stats.tolist())
        _, kw = RUNS[name]
        if name == MIXED:
            assert 0 < run["resident_pairs"] < N_FRAMES, (name, run["resident_pairs"], stats.tolist())
        elif not kw.get("resident") or kw["detector"] == "AKAZE" or (kw["detector"] == "BRISK" and not kw.get("brisk_resident")):
            assert run["resident_pairs"] == 0, (name, run["resident_pairs"])
        else:
            assert run["resident_pairs"] == N_FRAMES, (name, run["resident_pairs"])
        out[name] = run
        print(name, "keypoints", stats[:, :2].min(), "..", stats[:, :2].max(), "inliers", stats[:, 3].tolist(), "resident pairs", run["resident_pairs"], flush=True)
    with open(path, "w") as f:                           # one run per line
        f.write('{"frames_sha256": "%s",\n "runs": {\n' % frames_sha256(frames))
        f.write(",\n".join('  %s: %s' % (json.dumps(name), json.dumps(out[name])) for name in out))
        f.write("\n }}\n")
    print("wrote", path)


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "superpoint-stereo-visual-odometry_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    record(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
