"""Inputs of the ORB-extractor-across-octaves tests (tests/test_orb_octaves_ref_cpu.py asserts what they are meant to cover,
tests/test_gpu_orb_octaves.py holds the kernels to the restatement on them): the 160 x 400 crop of the first sample image with two keypoint
sets, and the restatement's answer for each, computed once per process."""
import functools

import numpy as np

from tests import brisk_detect_ref as bd, orb_octaves_ref as oo

SETS = ["brisk", "handmade"]


def crop(sample_images):
    return np.ascontiguousarray(sample_images[0][40:200, 300:700])


@functools.lru_cache(maxsize=None)
def _brisk(key):
    kp = bd.detect(_IMAGES[key], 30)
    return np.stack([kp["x"], kp["y"]], 1).astype(np.float32), kp["octave"].astype(np.int32)


def handmade(shape):
    """the four corners of the border rule's rectangle and the centre at every octave; half-integer coordinates whose rounding decides
    whether they are kept -- half to even keeps 368.5 (368) and 128.5 (128) and drops 30.5 (30); half up would do the opposite -- and
    31.5 / 32.5, which both become 32; all of these at octaves 0, 3 and 7"""
    rows, cols = shape
    pts = [(31, 31), (cols - 32, 31), (31, rows - 32), (cols - 32, rows - 32), (cols // 2, rows // 2)]
    xy = [p for o in range(8) for p in pts]
    octave = [o for o in range(8) for _ in pts]
    halves = [(30.5, 60), (31.5, 60), (32.5, 60), (cols - 31.5, 60), (cols - 30.5, 60), (60, 30.5), (60, 31.5), (60, rows - 31.5), (60, rows - 30.5), (100.5, 70.5)]
    for o in (0, 3, 7):
        xy += halves
        octave += [o] * len(halves)
    return np.array(xy, np.float32), np.array(octave, np.int32)


_IMAGES = {}


def keypoints(name, sample_images):
    """(image, xy [n, 2] float32, octave [n] int32) of a set"""
    img = crop(sample_images)
    _IMAGES.setdefault("crop", img)
    if name == "brisk":
        return (img,) + _brisk("crop")
    return (img,) + handmade(img.shape)


@functools.lru_cache(maxsize=None)
def _reference(name):
    img = _IMAGES["crop"]
    xy, octave = _brisk("crop") if name == "brisk" else handmade(img.shape)
    return oo.describe(img, xy, octave)


def reference(name, sample_images):
    """the restatement on a set, in the set's own order (shared: do not modify)"""
    keypoints(name, sample_images)
    return _reference(name)
