"""Keypoint lists of the spvo_sift_describe tests and the restatement's rows for them (tests/sift_describe_ref.py), computed once per process."""
import functools

import numpy as np

from tests import classic_ref, sift_cases as sc, sift_describe_ref as sd, sift_ref as sr

LISTS = ("fast", "handmade")              # on sift_cases.image("kitti"); "brisk_style" lies on the noise image
IMAGE = {"fast": "kitti", "handmade": "kitti", "brisk_style": "noise"}


def records(x, y, size, angle, octave, response=0.0):
    n = len(x)
    kp = np.zeros(n, sr.KP_DTYPE)
    kp["x"], kp["y"], kp["size"], kp["angle"], kp["response"], kp["octave"] = x, y, size, angle, response, octave
    return kp


@functools.lru_cache(None)
def keypoints(name):
    if name == "fast":
        # what ClassicFeatureFrontEnd(FAST, SIFT) hands over: KeyPoint(x, y, 7.f, -1, score), octave 0
        f = classic_ref.fast(sc.image("kitti"))
        return records(f["xy"][:, 0], f["xy"][:, 1], np.full(len(f["xy"]), 7.0), np.full(len(f["xy"]), -1.0), np.zeros(len(f["xy"]), np.int32), f["response"])
    if name == "handmade":
        # 300 records on the same image: sizes 1 .. 200, octaves -1 .. 5 with layers 0 .. 5, angles -1 / 0 / 360 / 359.99999 / arbitrary,
        # positions up to 2 pixels outside the image
        rows, cols = sc.image("kitti").shape
        rs = np.random.RandomState(20)
        n = 300
        x = rs.uniform(-2.0, cols + 1.0, n)
        y = rs.uniform(-2.0, rows + 1.0, n)
        size = np.exp(rs.uniform(np.log(1.0), np.log(200.0), n))
        size[:4] = (1.0, 200.0, 7.0, 31.0)
        o = rs.randint(-1, 6, n)
        layer = rs.randint(0, 6, n)
        o[:7] = (-1, 0, 1, 2, 3, 4, 5)
        layer[:6] = (0, 1, 2, 3, 4, 5)
        xi = rs.randint(0, 256, n)                                   # the third byte is carried and ignored
        octave = ((o & 255) | (layer << 8) | (xi << 16)).astype(np.int32)
        angle = rs.uniform(0.0, 360.0, n)
        fixed = np.array([-1.0, 0.0, 360.0, 359.99999], np.float64)
        angle[:80] = fixed[np.arange(80) % 4]
        return records(x, y, size, angle, octave, rs.uniform(0, 1, n))
    if name == "brisk_style":
        # what a BRISK keypoint looks like: octave = layer 1 .. 5 (no second byte), size = 12 x its scale, angle -1, fractional positions
        rows, cols = sc.image("noise").shape
        rs = np.random.RandomState(21)
        n = 120
        o = 1 + np.arange(n) % 5
        scale = np.where(o % 2 == 0, 2.0 ** (o // 2), 1.5 * 2.0 ** (o // 2))
        return records(rs.uniform(4.0, cols - 4.0, n), rs.uniform(4.0, rows - 4.0, n), 12.0 * scale * rs.uniform(0.8, 1.2, n), np.full(n, -1.0), o.astype(np.int32),
                       rs.uniform(30, 90, n))
    raise KeyError(name)


def image(name):
    return np.ascontiguousarray(sc.image(IMAGE[name]))


@functools.lru_cache(None)
def gauss(name):
    return sd.pyramid(image(name), *sd.extent(keypoints(name)))


@functools.lru_cache(None)
def reference(name, dtype="float32"):
    d = sd.describe(image(name), keypoints(name), np.float64 if dtype == "float64" else np.float32, gauss=gauss(name))
    d.setflags(write=False)
    return d


def row_difference(a, b):
    """per-row largest absolute difference of two [n, 128] arrays of one list, rows in order"""
    assert a.shape == b.shape
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(axis=1) if len(a) else np.zeros(0)
