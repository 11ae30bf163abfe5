"""Inputs shared by tests/test_akaze_ref_cpu.py and tests/test_gpu_akaze.py: the image of every AKAZE detector parity case, so the CPU
test asserts on the very inputs the GPU test compares.  All deterministic, built from brisk_detect_cases' helpers; each is the smallest
shape that still reaches its path."""
import functools

import numpy as np

from tests import akaze_ref as ak
from tests.brisk_detect_cases import blob_image, smoothed_noise

CASES = ["one_octave", "two_exact", "two_odd", "blobs", "ties", "border", "flat"]          # + "full_size" (golden image 0) through image_case

# (kind, cx, cy, r, amp): a blob's standard deviation is r / 2 -- sigma 2 .. 20
BLOBS = ([("blob", 45 + 62 * i, 45, r, 150.0) for i, r in enumerate((4, 5, 6, 7, 8, 10))]
         + [("blob", 60 + 95 * i, 125, r, 150.0) for i, r in enumerate((12, 16, 20, 24))]
         + [("blob", 90, 205, 32, 170.0), ("blob", 250, 200, 40, 170.0), ("square", 340, 205, 6, 120.0), ("square", 372, 170, 3, 120.0)])


def contrasted_noise(shape, seed, gain=3):
    img = smoothed_noise(shape, seed).astype(np.int32)
    return np.clip((img - 128) * gain + 128, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "one_octave":                    # 97 x 131: 131 / 2 < 80 -- a single octave
        return contrasted_noise((97, 131), 31)
    if name == "two_exact":                     # 96 x 160: octave 1 (48 x 80) by the exact 2 x 2 mean
        return contrasted_noise((96, 160), 32)
    if name == "two_odd":                       # 83 x 165: octave 1 (41 x 82) by the general area path, both axes inexact
        return contrasted_noise((83, 165), 33)
    if name == "blobs":                         # 270 x 400: three octaves, keypoints on many levels, suppression across levels
        return blob_image((270, 400), BLOBS)
    if name == "ties":                          # mirror-symmetric in both directions, 80 x 112: equal neighbouring Ldet
        q = contrasted_noise((40, 56), 34, 2)
        q[8:14, 18:24] = 230
        q[24:28, 28:38] = 15
        top = np.concatenate([q, q[:, ::-1]], 1)
        return np.ascontiguousarray(np.concatenate([top, top[::-1]], 0))
    if name == "border":                        # 140 x 180: structure only in a 40-pixel frame along the four borders
        img = contrasted_noise((140, 180), 35).astype(np.int32)
        img[40:100, 40:140] = 128
        return img.astype(np.uint8)
    if name == "flat":                          # gradient maximum 0
        return np.full((48, 64), 90, np.uint8)
    raise KeyError(name)


def image_case(name, sample_images):
    if name == "full_size":
        return np.ascontiguousarray(sample_images[0])
    return case(name)


_REF = {}


def reference(name, sample_images=None, tables=None):
    """-> (levels, k, keypoints) of a case by the restatement; `tables`: a dict from the library (cached under its identity: pass None
    for the restatement's own)"""
    key = (name, tables is not None)
    if key not in _REF:
        img = image_case(name, sample_images)
        levels, k = ak.scale_space(img, tables)
        _REF[key] = (levels, k, ak.detect(img, levels=levels))
    return _REF[key]
