"""Inputs shared by tests/test_brisk_detect_ref_cpu.py and tests/test_gpu_brisk_detect.py: image and threshold of every BRISK detector
parity case, so the CPU test asserts on the very inputs the GPU test compares.  All deterministic."""
import functools

import numpy as np

from tests import brisk_detect_ref as bd

CASES = ["inexact", "exact", "blobs", "ties", "border"]          # + "full_size" (golden image 0) through image_case


def smoothed_noise(shape, seed):
    """uniform noise under a 3x3 box filter (reflected border)"""
    raw = np.random.RandomState(seed).randint(0, 256, shape).astype(np.int32)
    p = np.pad(raw, 1, mode="reflect")
    h, w = shape
    acc = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return ((acc + 4) // 9).astype(np.uint8)


def draw_blob(img, cx, cy, r, amp):
    """adds a Gaussian blob of standard deviation r / 2 (float image)"""
    h, w = img.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * (r / 2.0) ** 2))


def draw_square(img, cx, cy, r, amp):
    """adds an axis-parallel square of half-width r with edges softened over r / 4 pixels: four corners of that scale"""
    h, w = img.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.maximum(np.abs(xx - cx), np.abs(yy - cy)) - r
    img += amp / (1.0 + np.exp(np.clip(d / max(r / 4.0, 0.35), -50, 50)))


def blob_image(shape, blobs, base=60.0):
    img = np.full(shape, base, np.float64)
    for kind, cx, cy, r, amp in blobs:
        (draw_blob if kind == "blob" else draw_square)(img, cx, cy, r, amp)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


BLOBS = ([("blob", 35 + 60 * i, 35, r, 150.0) for i, r in enumerate((2, 3, 4, 5, 6, 7))]
         + [("blob", 50 + 95 * i, 110, r, 150.0) for i, r in enumerate((8, 10, 12, 16))]
         + [("blob", 70, 205, 20, 170.0), ("blob", 200, 205, 24, 170.0), ("square", 320, 200, 3.5, 120.0), ("square", 370, 150, 2, 120.0)])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (image, threshold)"""
    if name == "inexact":                       # 97 x 131: odd, divisible by neither 2, 3 nor 4 -- layers 1, 2, 4 and 5 take the inexact-ratio path (layer 3 halves layer 1, whose sizes are always even)
        return smoothed_noise((97, 131), 21), 12
    if name == "exact":                         # 96 x 144: exact ratios throughout
        return smoothed_noise((96, 144), 22), 12
    if name == "blobs":                         # Gaussian blobs and squares of radii 2 .. 24
        return blob_image((270, 400), BLOBS), 8
    if name == "ties":                          # mirror-symmetric structures: equal neighbouring scores
        q = smoothed_noise((40, 56), 23)
        q[10:14, 20:24] = 230
        q[25:27, 30:38] = 15
        top = np.concatenate([q, q[:, ::-1]], 1)
        return np.ascontiguousarray(np.concatenate([top, top[::-1]], 0)), 12
    if name == "border":                        # corners within a few pixels of every border
        img = smoothed_noise((90, 126), 24).astype(np.int32)
        img = np.clip((img - 128) * 3 + 128, 0, 255)
        img[22:68, 22:104] = 128                 # structure only in a 22-pixel frame along the four borders
        return img.astype(np.uint8), 20
    raise KeyError(name)


def image_case(name, sample_images):
    if name == "full_size":
        return np.ascontiguousarray(sample_images[0]), 30
    return case(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (layers, keypoints, stats) of a synthetic case, computed once"""
    img, thr = case(name)
    layers = bd.build_layers(img)
    stats = {}
    return layers, bd.detect(img, thr, stats, layers), stats


_FULL = {}


def image_reference(name, sample_images):
    """`reference` for every case, the golden image included (computed once)"""
    if name != "full_size":
        return reference(name)
    if not _FULL:
        img, thr = image_case(name, sample_images)
        layers = bd.build_layers(img)
        stats = {}
        _FULL["r"] = (layers, bd.detect(img, thr, stats, layers), stats)
    return _FULL["r"]
