"""BRISK + SIFT and AKAZE + SIFT pair-resident (spvo_brisk_sift_pair, spvo_akaze_sift_pair, spvo_sift_link_debug,
ClassicFeatureFrontEnd::setSiftOctavePairsResident) as far as it can be asked without a device: the symbols, the bindings, the refusal of
a NULL context and the keyword's default; and the inputs of tests/test_gpu_sift_octave_pairs_resident.py pinned with the numpy
restatements (tests/brisk_detect_ref.py, tests/akaze_ref.py, tests/sift_describe_ref.py), so that the GPU test's byte comparisons are known
to cover every octave the BRISK detector reaches, a pyramid level no keypoint names, patches that their level's border clips and patches
it does not, and a last level of one row."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import capi, host
from tests import akaze_ref as ar, sift_describe_ref as sd, sift_ref as sr
from tests.test_octave_pairs_resident_cpu import stereo_pairs

NEW = ["spvo_brisk_sift_pair", "spvo_akaze_sift_pair", "spvo_sift_link_debug"]


def test_both_libraries_export_the_new_symbols():
    lib = capi.load()
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert hasattr(host.load(), "spvo_host_classic_set_sift_octave_pairs_resident")
    for m in ("brisk_sift_pair", "akaze_sift_pair", "sift_link_debug"):
        assert callable(getattr(capi.Context, m)), m
    assert [f[0] for f in capi.AkazeSiftFeatures._fields_] == ["n", "kp", "desc", "cap"]
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spvo.h")) as f:
        text = f.read()
    for name in NEW:
        assert "int %s(spvo_ctx *ctx, " % name in text, name
    assert "} spvo_akaze_sift_features;" in text


def test_a_null_context_is_refused():
    lib = capi.load()
    img = (C.c_uint8 * (64 * 96))()
    fs = [capi.SiftFeatures(0, None, None, 0) for _ in range(2)]
    fa = [capi.AkazeSiftFeatures(0, None, None, 0) for _ in range(2)]
    assert lib.spvo_brisk_sift_pair(None, img, img, 64, 96, 96, 30, 3, 0, 1, 8192, C.byref(fs[0]), C.byref(fs[1])) == -1
    assert lib.spvo_akaze_sift_pair(None, img, img, 64, 96, 96, 0.001, 0, 1, 8192, C.byref(fa[0]), C.byref(fa[1])) == -1
    kp = np.zeros(1, capi.SIFT_KP_DTYPE)
    kp["x"], kp["y"], kp["size"] = 40, 32, 7
    kept = (C.c_int32 * 1)()
    desc = (C.c_float * 128)()
    m = C.c_int(0)
    assert lib.spvo_sift_link_debug(None, 64, 96, kp.ctypes.data, None, 1, 0, kept, desc, C.byref(m)) == -1


def test_the_keyword_is_off_by_default():
    assert inspect.signature(host.classic_sequence).parameters["sift_octave_pairs_resident"].default is False


# ---------------------------------------------------------------- the GPU test's inputs
def sift_records(kp):
    """a detector's records as the SIFT extractor receives them: {x, y, size, angle, response, octave}, class_id left behind"""
    out = np.zeros(len(kp), sr.KP_DTYPE)
    for f in sr.KP_DTYPE.names:
        out[f] = kp[f]
    return out


def clipping(kp, shape):
    """-> (records whose patch its level's border clips, records whose patch lies inside), by the restatement's own point, scale and radius
    (sift_describe_ref.descriptor: the rows and columns 1 .. H - 2, 1 .. W - 2 hold the samples); and the octaves in use"""
    clipped = inside = 0
    octaves = set()
    for k in sift_records(kp):
        o, layer, px, py, scl = sd.point(k)
        assert layer == 0 and o >= 0
        H, W = sd.level_shapes(shape[0], shape[1], 0, o + 1)[o]
        hist_width = sd.F(3) * scl
        radius = int(np.rint(hist_width * sd.F(1.4142135623730951) * sd.F(5) * sd.F(0.5)))
        radius = min(radius, int(math.sqrt(float(W) * W + float(H) * H)))
        cut = max(-radius, 1 - py) > -radius or min(radius, H - 2 - py) < radius or max(-radius, 1 - px) > -radius or min(radius, W - 2 - px) < radius
        clipped += cut
        inside += not cut
        octaves.add(o)
    return clipped, inside, sorted(octaves)


def test_brisk_keypoints_of_the_crop_pair(sample_images):
    """1214 / 1190 records whose octave takes every value 0 .. 5: spvo_brisk_sift_pair's max_octave, and every level of its pyramid is read"""
    from tests import brisk_detect_ref as bd
    L, R = stereo_pairs(sample_images)["crop"]
    assert L.shape == (160, 400)
    pinned = [(1214, (1123, 91)), (1190, (1092, 98))]
    for img, (n, clip) in zip((L, R), pinned):
        kp = bd.detect(img, 30)
        c = clipping(kp, img.shape)
        print("BRISK", len(kp), "records, octaves", np.bincount(kp["octave"], minlength=6).tolist(), "clipped / inside", c[:2])
        assert len(kp) == n
        assert c[2] == [0, 1, 2, 3, 4, 5]
        assert c[:2] == clip and c[0] > 0 and c[1] > 0
        assert set(np.unique(kp["angle"]).tolist()) == {-1.0}


@pytest.mark.parametrize("name, side, detected", [("crop", 0, 247), ("crop", 1, 247), ("strided", 0, 137), ("strided", 1, 152)])
def test_akaze_keypoints_of_the_small_pairs(sample_images, name, side, detected):
    """the counts the pair tests see, on octaves 0 and 1 while the shape's last octave is 2: spvo_akaze_sift_pair builds a level no keypoint
    names.  No AKAZE patch is clipped, on these images or any: the detector keeps a keypoint of level i at least
    border = round(10 sqrt(2) sigma_size) + 1 pixels inside its octave's image; its size is 3 esigma, so the extractor's
    scl = 1.5 esigma / 2^octave <= sigma_size + 0.5 and the patch radius round(3 scl sqrt(2) 5 / 2) <= 10.7 sigma_size + 5.4, which
    14.1 sigma_size + 1 exceeds by more than the roundings for every sigma_size >= 2, the smallest there is (round(1.5 x 1.6)).  The clipped walk of the describe kernel is the BRISK pairs' (1123 of 1214 records above) and the hook's; what the
    AKAZE pairs add to it is reading 28-byte records, which every row here exercises."""
    img = np.ascontiguousarray(stereo_pairs(sample_images)[name][side])
    kp = ar.detect(img)
    c = clipping(kp, img.shape)
    print("AKAZE", name, side, img.shape, len(kp), "records, octaves", np.bincount(kp["octave"], minlength=3).tolist(), "clipped / inside", c[:2])
    assert len(kp) == detected
    assert c[2] == [0, 1]
    assert int(ar.make_tables(*img.shape)["octave"][-1]) == 2
    assert c[:2] == (0, detected)


def test_the_smallest_shape_with_octave_5():
    """a 32-row image has a level of one row on octave 5, a 31-row image has none: what spvo_brisk_sift_pair refuses"""
    assert sd.level_shapes(32, 400, 0, 6)[-1] == (1, 12)
    assert sd.level_shapes(31, 400, 0, 6)[-1][0] == 0
    assert (32 >> 5) == 1 and (31 >> 5) == 0
