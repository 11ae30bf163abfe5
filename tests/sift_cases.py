"""Inputs of the SIFT tests and the restatement's output for them, computed once per process (tests/sift_ref.py is the slow part)."""
import functools
import os

import numpy as np

import oracle  # noqa: F401
from oracle import frontend as ofe
from tests import sift_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("kitti", "strided", "noise")     # the non-flat inputs


@functools.lru_cache(None)
def _golden_images():
    from PIL import Image
    d = os.path.join(GOLDEN, "images")
    return [np.asarray(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d)) if f.endswith(".png")]


@functools.lru_cache(None)
def image(name):
    """kitti: golden image 2 preprocessed to 120 x 392 (base 240 x 784, 7 octaves, the smallest levels are smaller than the blur radius);
    strided: a 101 x 147 view with both sides odd and rows that are not contiguous; noise: 64 x 96 uniform noise; flat: 64 x 64 of one value"""
    if name == "kitti":
        return ofe.preprocess(_golden_images()[2], np.eye(3, 4), 120, 392)[0]
    if name == "strided":
        return _golden_images()[1][3:104, 5:152]
    if name == "noise":
        return np.random.RandomState(1).randint(0, 256, (64, 96)).astype(np.uint8)
    if name == "flat":
        return np.full((64, 64), 117, np.uint8)
    raise KeyError(name)


@functools.lru_cache(None)
def stage(name):
    return sr.detect_candidates(np.ascontiguousarray(image(name)))


@functools.lru_cache(None)
def reference(name, dtype="float32"):
    return sr.describe(stage(name), np.float64 if dtype == "float64" else np.float32)


def compare(a, b):
    """two outputs of one image, keyed by (octave, layer, row, column, orientation bin of 10 degrees): -> dict(share = keys on one side only /
    the larger list, common = [(index in a, index in b)] in a's order, desc = per-row largest absolute descriptor difference over the
    common keys, angle = their angle differences in degrees (on the circle))"""
    ka, kb = sr.keys(a["kp"]), sr.keys(b["kp"])
    ib = {k: i for i, k in enumerate(kb)}
    common = [(i, ib[k]) for i, k in enumerate(ka) if k in ib]
    one = len(set(ka) ^ set(kb))
    ia = np.array([i for i, _ in common], np.int64)
    jb = np.array([j for _, j in common], np.int64)
    desc = np.abs(a["desc"][ia] - b["desc"][jb]).max(axis=1) if len(common) else np.zeros(0)
    ang = np.abs(a["kp"]["angle"][ia].astype(np.float64) - b["kp"]["angle"][jb].astype(np.float64))
    return dict(share=one / max(len(ka), len(kb), 1), common=common, desc=desc, angle=np.minimum(ang, 360 - ang))
