"""BRISK + ORB, AKAZE + ORB and AKAZE + BRISK pair-resident (spvo_brisk_orb_pair, spvo_akaze_orb_pair, spvo_akaze_brisk_pair,
spvo_orb_octaves_link_debug, ClassicFeatureFrontEnd::setOctavePairsResident) as far as it can be asked without a device: the symbols,
the bindings, the refusal of a NULL context and the keyword's default; and the inputs of tests/test_gpu_octave_pairs_resident.py pinned
with the numpy restatements (tests/brisk_detect_ref.py, tests/akaze_ref.py, tests/orb_octaves_ref.py, tests/brisk_ref.py), so that the
GPU test's byte comparisons are known to cover every octave a detector reaches, the reflect zone, and both outcomes of the border rule."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import capi, host
from tests import akaze_ref as ar, brisk_ref as br, orb_octaves_cases as oc, orb_octaves_ref as oo

NEW = ["spvo_brisk_orb_pair", "spvo_akaze_orb_pair", "spvo_akaze_brisk_pair", "spvo_orb_octaves_link_debug"]


def test_both_libraries_export_the_new_symbols():
    lib = capi.load()
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert hasattr(host.load(), "spvo_host_classic_set_octave_pairs_resident")
    for m in ("brisk_orb_pair", "akaze_orb_pair", "akaze_brisk_pair", "orb_octaves_link_debug"):
        assert callable(getattr(capi.Context, m)), m
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spvo.h")) as f:
        text = f.read()
    for name in NEW:
        assert "int %s(spvo_ctx *ctx, " % name in text, name


def test_a_null_context_is_refused():
    lib = capi.load()
    img = (C.c_uint8 * (64 * 96))()
    fb = [capi.BriskFeatures(0, None, None, 0) for _ in range(2)]
    fa = [capi.AkazeFeatures(0, None, None, 0) for _ in range(2)]
    assert lib.spvo_brisk_orb_pair(None, img, img, 64, 96, 96, 30, 3, 0, 1, 8192, C.byref(fb[0]), C.byref(fb[1])) == -1
    assert lib.spvo_akaze_orb_pair(None, img, img, 64, 96, 96, 0.001, 0, 1, 8192, C.byref(fa[0]), C.byref(fa[1])) == -1
    assert lib.spvo_akaze_brisk_pair(None, img, img, 64, 96, 96, 0.001, 0, 1, 8192, C.byref(fa[0]), C.byref(fa[1])) == -1
    xy = (C.c_float * 2)(40, 32)
    octave = (C.c_int32 * 1)(0)
    kept = (C.c_int32 * 1)()
    desc = (C.c_uint8 * 32)()
    m = C.c_int(0)
    assert lib.spvo_orb_octaves_link_debug(None, 64, 96, xy, octave, None, 1, 0, kept, None, desc, C.byref(m)) == -1


def test_the_keyword_is_off_by_default():
    assert inspect.signature(host.classic_sequence).parameters["octave_pairs_resident"].default is False


# ---------------------------------------------------------------- the GPU test's inputs
def stereo_pairs(sample_images):
    """name -> (left, right) of the small pairs tests/test_gpu_octave_pairs_resident.py runs: the 160 x 400 crop with its mirror image,
    and the strided 200 x 400 views into sample images 1 and 2"""
    crop = oc.crop(sample_images)
    return {"crop": (crop, np.ascontiguousarray(crop[::-1, ::-1])), "strided": (sample_images[1][3:203, 5:405], sample_images[2][3:203, 5:405])}


def orb_rule(xy, octave, shape):
    k = oo.border_keep(xy, shape)
    return len(k), np.bincount(octave[k], minlength=8).tolist()


def test_brisk_keypoints_of_the_crop_pair(sample_images):
    from tests import brisk_detect_ref as bd
    L, R = stereo_pairs(sample_images)["crop"]
    img, xy, octave = oc.keypoints("brisk", sample_images)
    assert np.array_equal(img, L) and len(xy) == 1214
    assert orb_rule(xy, octave, L.shape) == (716, [377, 95, 125, 52, 49, 18, 0, 0])
    assert int(oc.reference("brisk", sample_images)["zone"].any(1).sum()) == 28            # within 19 pixels of their level's border
    kp = bd.detect(R, 30)
    rxy, roct = np.stack([kp["x"], kp["y"]], 1).astype(np.float32), kp["octave"].astype(np.int32)
    print("right image:", len(kp), orb_rule(rxy, roct, R.shape))
    assert len(kp) == 1190
    assert orb_rule(rxy, roct, R.shape) == (705, [385, 96, 116, 52, 41, 15, 0, 0])
    assert oo.level_shapes(*L.shape)[5] == (64, 161)                                    # level 5, the one spvo_brisk_orb_pair asks about
    assert oo.level_shapes(70, 400)[5][0] == 28 < oo.MIN_LEVEL                           # ... and what it refuses of a 70 x 400 image


@pytest.mark.parametrize("name, side, detected, orb_kept, per_octave",
                         [("crop", 0, 247, 235, [232, 3]), ("crop", 1, 247, 235, [232, 3]), ("strided", 0, 137, 134, [124, 10]), ("strided", 1, 152, 146, [137, 9])])
def test_akaze_keypoints_of_the_small_pairs(sample_images, name, side, detected, orb_kept, per_octave):
    """the counts the pair tests see, the octaves (two of the shape's three hold keypoints), that the octave never descends along the
    list, and that BRISK's border rule drops NO AKAZE keypoint on these inputs: the drop branch of the compaction spvo_akaze_brisk_pair
    goes through is the one tests/test_gpu_brisk_pair_resident.py already holds to the restatement"""
    img = np.ascontiguousarray(stereo_pairs(sample_images)[name][side])
    kp = ar.detect(img)
    xy, octave = np.stack([kp["x"], kp["y"]], 1).astype(np.float32), kp["octave"].astype(np.int32)
    n, hist = orb_rule(xy, octave, img.shape)
    print(name, side, img.shape, "detected", len(kp), "pass ORB's rule", n, hist, "pass BRISK's rule", len(br.border_keep(xy, kp["size"], img.shape)[0]))
    assert len(kp) == detected
    assert (n, hist) == (orb_kept, per_octave + [0] * 6)
    assert len(br.border_keep(xy, kp["size"], img.shape)[0]) == detected
    assert not (np.diff(octave) < 0).any()
    assert int(ar.make_tables(*img.shape)["octave"][-1]) == 2                             # spvo_akaze_orb_pair's max_octave for this shape: a level no keypoint names
