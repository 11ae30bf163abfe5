"""Inputs shared by tests/test_akaze_mldb_ref_cpu.py and tests/test_gpu_akaze_mldb.py: the hand-made keypoint records of the AKAZE
orientation / MLDB descriptor parity cases, so the CPU test asserts on the very records the GPU test compares.  The images are
tests/akaze_cases.py's.  All deterministic."""
import numpy as np

from tests import akaze_cases as ac, akaze_mldb_ref as mr, akaze_ref as ak

HAND_IMAGES = ["two_odd", "blobs"]
HAND_COUNTS = [1, 63, 64, 65, 0]                       # one wave's worth of keypoints, one less, one more; a single one; none


def hand_records(shape, tables=None):
    """Records the detector would never produce, on EVERY level of a `shape` image (levels with no room inside their extrema border
    included): centres 2 - 3 pixels of the level's grid from each border and in each corner, so that orientation and descriptor samples
    leave the plane, and one at the middle with coordinates ending in .5 (every sample with an integer offset is then a tie of cvRound); per centre one of four sizes in turn -- so small that s = 0,
    the level's own (3 esigma), ending in .5 after the division so that cvRound meets a tie (s = 2.5 -> 2), and so large that most
    samples are skipped (s = 60).  More than 65 records for every shape."""
    rows, cols = shape
    T = tables or ak.make_tables(rows, cols)
    out = []
    for level, (o, esigma) in enumerate(zip(T["octave"], T["esigma"])):
        ratio = float(2 ** int(o))
        h, w = int(rows / ratio), int(cols / ratio)
        xs, ys = (2.0, w // 2 + 0.5, w - 3.0), (3.0, h // 2 + 0.5, h - 2.0)     # on the level's grid: x / ratio is exactly this
        sizes = (0.4 * ratio, float(np.float32(np.float32(esigma * np.float32(1.5)) * np.float32(2.0))), 5.0 * ratio, 120.0 * ratio)
        k = level                                                                # (so that every size meets every kind of centre)
        for y in ys:
            for x in xs:
                out.append((x * ratio, y * ratio, sizes[k % 4], -1.0, 0.0, int(o), level))
                k += 1
    return np.array(out, ak.KP_DTYPE)


def flat_records(shape):
    """Records on every level of a constant image whose 20 s x 20 s grid stays inside the plane (s = 0, 1, 2 on 48 rows): every cell of
    a grid then sums the same values in the same order, no comparison is strict and the row is zero.  (Next to a border it is not: cells
    that lose samples divide by another count, or keep the value 0 of an empty cell, and the mean of Lt differs.)"""
    rows, cols = shape
    T = ak.make_tables(rows, cols)
    out = []
    for level, o in enumerate(T["octave"]):
        ratio = float(2 ** int(o))
        h, w = int(rows / ratio), int(cols / ratio)
        for x, y in ((w // 2 + 0.5, h // 2 + 0.5), (w // 2 - 3.0, h // 2 - 1.0)):
            for size in (0.4, 2.0, 4.0):
                out.append((x * ratio, y * ratio, size * ratio, -1.0, 0.0, int(o), level))
    return np.array(out, ak.KP_DTYPE)


_REF = {}


def reference(name, sample_images=None):
    """-> (levels, derivs, detector keypoints, angle, desc) of a case by the restatements on their own tables"""
    if name not in _REF:
        levels, _, kp = ac.reference(name, sample_images)
        derivs = mr.derivatives(levels)
        _REF[name] = (levels, derivs, kp) + mr.describe(levels, kp, derivs)
    return _REF[name]
