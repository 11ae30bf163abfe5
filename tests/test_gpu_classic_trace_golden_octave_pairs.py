"""tests/test_gpu_classic_trace_golden.py for the three pairs that stay resident behind ClassicFeatureFrontEnd::setOctavePairsResident --
BRISK + ORB, AKAZE + ORB (both with setOrbExtractorOctaves) and AKAZE + BRISK: per image and with the features resident on the device,
the trace digests of host.classic_sequence, the counts, the poses and the number of pairs that stayed resident are those of
tests/golden/classic_front_end_trace_octave_pairs.json EXACTLY.  The sequence, the digests' meaning and the recording rule are that
module's: the fixture is written by running this module as a script on the GPU
(python tests/test_gpu_classic_trace_golden_octave_pairs.py [path]) and in no other way; the test never writes it."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "superpoint-stereo-visual-odometry_amd")):      # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests.test_gpu_classic_trace_golden import N_FRAMES, frames_sha256, load_sequence  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "classic_front_end_trace_octave_pairs.json")

pytestmark = pytest.mark.gpu

PAIRS = [("BRISK", "ORB"), ("AKAZE", "ORB"), ("AKAZE", "BRISK")]


def _runs():
    """name -> keyword arguments of host.classic_sequence"""
    runs = {}
    for det, desc in PAIRS:
        kw = dict(detector=det, descriptor=desc, orb_octaves=(desc == "ORB"))
        runs["%s+%s" % (det, desc)] = kw
        runs["%s+%s resident, octave_pairs_resident" % (det, desc)] = dict(kw, resident=True, octave_pairs_resident=True)
    return runs


RUNS = _runs()


def replay(name, frames, P_l, P_r):
    """-> what the fixture holds for one run"""
    from spvo import host
    poses, stats, _, digest = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, input_size=(120, 392), trace=True, **RUNS[name])
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
    got = replay(name, frames, P_l, P_r)
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
    for name in RUNS:
        run = replay(name, frames, P_l, P_r)
        stats = np.asarray(run["stats"])
        # not vacuous: features on every image, and a solve that found something
        assert stats[:, :2].min() > 50, (name, stats.tolist())
        assert stats[:, 3].max() > 10, (name, stats.tolist())
        assert run["resident_pairs"] == (N_FRAMES if RUNS[name].get("resident") else 0), (name, run["resident_pairs"])
        out[name] = run
        print(name, "keypoints", stats[:, :2].min(), "..", stats[:, :2].max(), "inliers", stats[:, 3].tolist(), "resident pairs", run["resident_pairs"], flush=True)
    for det, desc in PAIRS:                               # the resident run leaves what the per-image run leaves
        a, b = out["%s+%s" % (det, desc)], out["%s+%s resident, octave_pairs_resident" % (det, desc)]
        assert all(a[f] == b[f] for f in ("digests", "stats", "poses")), (det, desc)
    with open(path, "w") as f:                           # one run per line
        f.write('{"frames_sha256": "%s",\n "runs": {\n' % frames_sha256(frames))
        f.write(",\n".join('  %s: %s' % (json.dumps(name), json.dumps(out[name])) for name in out))
        f.write("\n }}\n")
    print("wrote", path)


if __name__ == "__main__":
    record(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
