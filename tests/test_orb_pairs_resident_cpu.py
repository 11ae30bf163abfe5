"""ORB + BRISK and ORB + SIFT pair-resident (spvo_orb_brisk_pair, spvo_orb_sift_pair, ClassicFeatureFrontEnd::setOrbBriskExtractor /
setOrbPairsResident) as far as it can be asked without a device: the symbols, the bindings, the refusal of a NULL context, the keywords'
defaults and the refusal of ORB + BRISK without its switch; and the inputs of tests/test_gpu_orb_pairs_resident.py pinned with the CPU
oracle's ORB (oracle/cpu through oracle/cpu_backend.py) and BRISK's border rule (tests/brisk_ref.py), so that the GPU test's byte
comparisons are known to cover several octaves and both outcomes of the border rule at the sizes 31 * 1.2^octave.

The 160 x 400 crop of tests/test_octave_pairs_resident_cpu.py does NOT meet the conditions: BRISK's border rule at these sizes keeps
404 and 398 of its 1093 ORB keypoints, fewer than half (a keypoint of octave 3 needs more room than 160 rows leave).  The `crop` pair of
these tests is therefore another crop of the same sample image, rows 60 .. 300 of columns 300 .. 700 (240 x 400), with its mirror image
as the right view; the `strided` pair is the earlier file's."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import cpu_backend
from spvo import capi, host
from tests import brisk_ref as br
from tests.test_octave_pairs_resident_cpu import stereo_pairs as octave_stereo_pairs

NEW = ["spvo_orb_brisk_pair", "spvo_orb_sift_pair"]


def test_both_libraries_export_the_new_symbols():
    lib = capi.load()
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    hl = host.load()
    assert hasattr(hl, "spvo_host_classic_set_orb_brisk") and hasattr(hl, "spvo_host_classic_set_orb_pairs_resident")
    for m in ("orb_brisk_pair", "orb_sift_pair"):
        assert callable(getattr(capi.Context, m)), m
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spvo.h")) as f:
        text = f.read()
    for name in NEW:
        assert "int %s(spvo_ctx *ctx, " % name in text, name


def test_a_null_context_is_refused():
    lib = capi.load()
    img = (C.c_uint8 * (96 * 128))()
    fb = [capi.BriskFeatures(0, None, None, 0) for _ in range(2)]
    fs = [capi.SiftFeatures(0, None, None, 0) for _ in range(2)]
    assert lib.spvo_orb_brisk_pair(None, img, img, 96, 128, 128, 2000, 0, 1, 8192, C.byref(fb[0]), C.byref(fb[1])) == -1
    assert lib.spvo_orb_sift_pair(None, img, img, 96, 128, 128, 2000, 0, 1, 8192, C.byref(fs[0]), C.byref(fs[1])) == -1


def test_the_keywords_are_off_by_default():
    p = inspect.signature(host.classic_sequence).parameters
    assert p["orb_brisk"].default is False and p["orb_pairs_resident"].default is False
    assert inspect.signature(host.classic_pair_probe).parameters["orb_brisk"].default is False


def test_orb_brisk_is_refused_without_its_switch():
    """no device is asked: the pair is refused before a context exists, and the text lists the pairs that run -- ORB + BRISK not among them"""
    img = np.zeros((96, 128), np.uint8)
    P = np.eye(3, 4)
    rc, counts, err = host.classic_pair_probe("ORB", "BRISK", img, img, P, P)
    assert rc == 0 and not counts[:4].any()
    assert "OpenCV features2d call" in err and "ORB + ORB" in err and "ORB + BRISK" not in err and "ShiTomasi + BRISK" in err


# ---------------------------------------------------------------- the GPU test's inputs
def stereo_pairs(sample_images):
    """name -> (left, right) of the small pairs tests/test_gpu_orb_pairs_resident.py runs: the 240 x 400 crop with its mirror image, and the
    strided 200 x 400 views into sample images 1 and 2"""
    crop = np.ascontiguousarray(sample_images[0][60:300, 300:700])
    return {"crop": (crop, np.ascontiguousarray(crop[::-1, ::-1])), "strided": octave_stereo_pairs(sample_images)["strided"]}


def level_scale():
    """cv::ORB::create(2000, 1.2f, 8, ..): the repeated float product the host's to_keypoint and the device's record kernel share"""
    s = np.ones(8, np.float32)
    for l in range(1, 8):
        s[l] = s[l - 1] * np.float32(1.2)
    return s


def orb_sizes(octave):
    return (np.float32(31) * level_scale()[np.asarray(octave) & 7]).astype(np.float32)


@pytest.fixture(scope="module")
def cpu():
    c = cpu_backend.CpuBackend(net_height=64, net_width=96)
    yield c
    c.close()


@pytest.mark.parametrize("name, side, per_octave, kept, kept_per_octave",
                         [("crop", 0, [434, 362, 302, 251, 209, 116, 63, 13], 1074, [372, 288, 215, 129, 70, 0, 0, 0]),
                          ("crop", 1, [434, 362, 302, 251, 209, 116, 63, 13], 1079, [372, 291, 214, 132, 70, 0, 0, 0]),
                          ("strided", 0, [223, 167, 118, 89, 53, 24, 7, 0], 397, [174, 116, 71, 35, 1, 0, 0, 0]),
                          ("strided", 1, [248, 182, 137, 90, 57, 32, 4, 0], 413, [177, 124, 83, 29, 0, 0, 0, 0])])
def test_orb_keypoints_of_the_small_pairs(sample_images, cpu, name, side, per_octave, kept, kept_per_octave):
    img = np.ascontiguousarray(stereo_pairs(sample_images)[name][side])
    assert img.shape == dict(crop=(240, 400), strided=(200, 400))[name]
    o = cpu.orb(img)
    n = len(o["xy"])
    keep = br.border_keep(o["xy"], orb_sizes(o["octave"]), img.shape)[0]
    hist, khist = np.bincount(o["octave"], minlength=8).tolist(), np.bincount(o["octave"][keep], minlength=8).tolist()
    print(name, side, img.shape, "detected", n, hist, "pass BRISK's rule", len(keep), khist)
    assert hist == per_octave and n == sum(per_octave)
    assert (len(keep), khist) == (kept, kept_per_octave)
    # what the inputs must meet
    assert n > 100
    assert sum(1 for c in hist if c) >= 3
    assert 0 < n - len(keep) and 2 * len(keep) >= n
    assert not (np.diff(o["octave"]) < 0).any()                        # level by level, as the device's list


def test_the_earlier_crop_does_not_meet_them(sample_images, cpu):
    """(why these tests cut another crop: fewer than half of the 160 x 400 crop's keypoints pass BRISK's rule)"""
    img = octave_stereo_pairs(sample_images)["crop"][0]
    o = cpu.orb(img)
    keep = br.border_keep(o["xy"], orb_sizes(o["octave"]), img.shape)[0]
    assert (len(o["xy"]), len(keep)) == (1093, 404)


def test_level_geometry_of_the_degenerate_shapes():
    """a level can hold a keypoint when it is more than 2 * 31 + 2 pixels in both dimensions (sizes: the float quotient rounded): none of a
    64 x 96 image, level 0 alone of a 67 x 67 one; the crop has all eight levels, the strided pair seven"""
    def levels(rows, cols):
        side = lambda n, l: int(np.floor(np.float32(n) / level_scale()[l] + np.float32(0.5)))
        return [l for l in range(8) if side(rows, l) > 64 and side(cols, l) > 64]
    assert levels(64, 96) == [] and levels(67, 67) == [0] and levels(96, 128) == [0, 1, 2] and levels(240, 400) == list(range(8)) and levels(200, 400) == list(range(7))
