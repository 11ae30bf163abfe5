"""Inputs shared by tests/test_brisk_ref_cpu.py and tests/test_gpu_brisk.py: image, keypoints and sizes of every BRISK parity case, so the
CPU test can assert on the very inputs the GPU test compares (no boundary row among them, see tests/brisk_ref.py)."""
import functools
import os

import numpy as np

import oracle  # noqa: F401
from oracle import frontend as ofe
from tests import brisk_ref as br, classic_ref as cr

SIZES = (5.0, 7.0, 12.3, 31.0, 60.0)
CASES = ["noise_grid", "noise_fractional", "golden_120x392", "strided_view", "empty", "flat"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "images")


def smoothed_noise(shape, seed):
    """uniform noise under a 3x3 box filter (reflected border): every sample box sees a gradient, neighbouring values rarely tie"""
    raw = np.random.RandomState(seed).randint(0, 256, shape).astype(np.int32)
    p = np.pad(raw, 1, mode="reflect")
    h, w = shape
    acc = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return ((acc + 4) // 9).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (image, xy [n, 2] float32, size [n] float32)"""
    if name == "noise_grid":
        # 64 x 96, integer grid: at scale 0 (sizes 5 and 7) b = size_list[0] = 13, so x = 12 | 13 and x = 82 | 83 (cols - b - 1 | cols - b) and
        # y = 12 | 13, 50 | 51 straddle the border rule; 12.3 is a middle scale (10, b = 18), 31 and 60 drop everything at this image size
        img = smoothed_noise((64, 96), 11)
        xs = [12, 13, 17, 18, 30, 47, 64, 77, 78, 82, 83]
        ys = [12, 13, 17, 18, 25, 32, 40, 45, 46, 50, 51]
        xy = np.array([(x, y) for y in ys for x in xs], np.float32)
        size = np.array([SIZES[i % len(SIZES)] for i in range(len(xy))], np.float32)
        return img, xy, size
    if name == "noise_fractional":
        img = smoothed_noise((64, 96), 12)
        rng = np.random.RandomState(13)
        xy = np.stack([rng.uniform(8, 88, 150), rng.uniform(8, 56, 150)], 1).astype(np.float32)
        size = np.array([SIZES[i % 3] for i in range(len(xy))], np.float32)
        return img, xy, size
    if name == "empty":
        return smoothed_noise((64, 96), 14), np.zeros((0, 2), np.float32), np.zeros(0, np.float32)
    if name == "flat":
        img = np.full((64, 96), 77, np.uint8)
        xy = np.array([(x, y) for y in (20, 31.5, 43) for x in (20, 40.25, 60, 75)], np.float32)
        return img, xy, np.full(len(xy), 7.0, np.float32)
    raise KeyError(name)


def image_case(name, sample_images):
    """the cases on the golden images (sample_images: the conftest fixture)"""
    if name == "golden_120x392":
        img = ofe.preprocess(sample_images[2], np.eye(3, 4), 120, 392)[0]
        xy = cr.gftt(np.ascontiguousarray(img))["xy"]
        return img, xy, np.full(len(xy), 5.0, np.float32)
    if name == "strided_view":
        img = sample_images[1][3:153, 5:405]                                           # rows are not contiguous
        xy = cr.fast(np.ascontiguousarray(img))["xy"]
        return img, xy, np.full(len(xy), 7.0, np.float32)
    if name == "full_size":
        img = sample_images[0]
        xy = cr.fast(np.ascontiguousarray(img))["xy"]
        return img, xy, np.full(len(xy), 7.0, np.float32)
    return case(name)


def boundary_rows(ref):
    return int(ref["boundary"].sum())
