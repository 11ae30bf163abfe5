"""SIFT + BRISK (spvo_sift_brisk_pair, ClassicFeatureFrontEnd::setSiftBriskExtractor / setSiftBriskResident) as far as it can be asked
without a device: the symbols, the bindings, the refusal of a NULL context, the keywords' defaults and the refusal of SIFT + BRISK without
its switch; and the inputs of tests/test_gpu_sift_brisk.py pinned with the restatements -- tests/sift_ref.py's detector up to the ordered,
duplicate-free list (the descriptor stage is not needed) and tests/brisk_ref.py's border rule -- so that the GPU test's byte comparisons
are known to cover octave -1 (the doubled image) and several more, scale index 0 and indices above it, survivors and casualties of the
border rule, and several keypoints of one candidate (one per orientation peak)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import capi, host
from tests import brisk_ref as br
from tests import sift_cases
from tests import sift_ref as sr
from tests.test_orb_pairs_resident_cpu import stereo_pairs as orb_stereo_pairs

NEW = ["spvo_sift_brisk_pair", "spvo_sift_records_debug"]


def test_both_libraries_export_the_new_symbols():
    lib = capi.load()
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    hl = host.load()
    assert hasattr(hl, "spvo_host_classic_set_sift_brisk") and hasattr(hl, "spvo_host_classic_set_sift_brisk_resident")
    for m in ("sift_brisk_pair", "sift_records_debug"):
        assert callable(getattr(capi.Context, m)), m
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spvo.h")) as f:
        text = f.read()
    for name in NEW:
        assert "int %s(spvo_ctx *ctx, " % name in text, name


def test_a_null_context_is_refused():
    lib = capi.load()
    img = (C.c_uint8 * (96 * 128))()
    fb = [capi.BriskFeatures(77, None, None, 0) for _ in range(2)]
    assert lib.spvo_sift_brisk_pair(None, img, img, 96, 128, 128, 0, 1, 8192, C.byref(fb[0]), C.byref(fb[1])) == -1
    assert fb[0].n == 77 and fb[1].n == 77
    n = C.c_int(77)
    assert lib.spvo_sift_records_debug(None, img, 96, 128, 128, 0, None, 0, C.byref(n)) == -1 and n.value == 77


def test_the_diagnostic_switch_is_a_tuning_name():
    assert capi.get_tuning("sift_brisk_recheck", 0) == 0
    capi.set_tuning("sift_brisk_recheck", 1)
    try:
        assert capi.get_tuning("sift_brisk_recheck", 0) == 1
    finally:
        capi.set_tuning("sift_brisk_recheck", 0)
    assert capi.get_tuning("sift_brisk_recheck", 0) == 0


def test_the_keywords_are_off_by_default():
    p = inspect.signature(host.classic_sequence).parameters
    assert p["sift_brisk"].default is False and p["sift_brisk_resident"].default is False
    assert inspect.signature(host.classic_pair_probe).parameters["sift_brisk"].default is False
    p = inspect.signature(capi.Context.sift_brisk_pair).parameters
    assert p["slot_capacity"].default == 8192 and p["cap"].default is None


def test_sift_brisk_is_listed_only_with_its_switch():
    """no device is asked: the pair is refused before a context exists, and the text lists the pairs that run -- SIFT + BRISK not among
    them.  With the switch on the constructor accepts the pair (nothing is logged before a device is needed), and another refused pair's
    text lists it."""
    img = np.zeros((96, 128), np.uint8)
    P = np.eye(3, 4)
    rc, counts, err = host.classic_pair_probe("SIFT", "BRISK", img, img, P, P)
    assert rc == 0 and not counts[:4].any()
    assert "OpenCV features2d call" in err and "SIFT + SIFT" in err and "SIFT + BRISK" not in err and "ShiTomasi + BRISK" in err
    rc, counts, err = host.classic_pair_probe("SIFT", "ORB", img, img, P, P)
    assert "SIFT + BRISK" not in err and "SIFT + SIFT" in err
    rc, counts, err = host.classic_pair_probe("SIFT", "ORB", img, img, P, P, sift_brisk=True)       # still refused (KeyPoint::octave is packed), the list is longer
    assert rc == 0 and not counts[:4].any() and "SIFT + BRISK" in err and "ORB + BRISK" not in err
    rc, counts, err = host.classic_pair_probe("SIFT", "ORB", img, img, P, P)                         # the switch was reset
    assert "SIFT + BRISK" not in err


# ---------------------------------------------------------------- the GPU test's inputs
def stereo_pairs(sample_images):
    """name -> (left, right) of the small pairs tests/test_gpu_sift_brisk.py runs: the ORB pairs tests' 240 x 400 crop with its mirror image,
    their strided 200 x 400 views, and the SIFT tests' 120 x 392 image with its mirror image"""
    out = dict(orb_stereo_pairs(sample_images))
    kitti = np.ascontiguousarray(sift_cases.image("kitti"))
    out["kitti"] = (kitti, np.ascontiguousarray(kitti[:, ::-1]))
    return out


def tiny_image():
    """the smallest square of RandomState(1) noise with a SIFT keypoint: 14 x 14 (none of 6 .. 13 has one) -- and none of its keypoints
    passes BRISK's border rule"""
    return np.random.RandomState(1).randint(0, 256, (14, 14)).astype(np.uint8)


def sift_keypoints(img):
    """tests/sift_ref.py's detector without its descriptor stage: the ordered, duplicate-free records, one per orientation peak"""
    st = sr.detect_candidates(np.ascontiguousarray(img))
    recs = []
    for (o, l, r, c, xi, xr, xc, contr) in st["cand"]:
        x, y, size, resp, octv = sr.candidate_record(o, l, r, c, xi, xr, xc, contr)
        for a in sr.orientations(st["gauss"][o][l], l, r, c, xi, np.float32):
            recs.append((x, y, size, a, resp, octv))
    kp = np.array(recs, sr.KP_DTYPE) if recs else np.zeros(0, sr.KP_DTYPE)
    return kp[sr.sort_unique(kp)]


def counts(img):
    """(SIFT keypoints, those that pass BRISK's rule, kept per octave index 0 = the doubled image, (lowest, highest scale index among the
    kept, kept at index 0), distinct (x, y, size) among the kept)"""
    kp = sift_keypoints(img)
    if not len(kp):
        return 0, 0, [], None, 0
    keep, s = br.border_keep(np.stack([kp["x"], kp["y"]], 1), kp["size"], img.shape)
    k = kp[keep]
    octave = sr.unpack_octave(k["octave"])[0]
    idx = (int(s[keep].min()), int(s[keep].max()), int((s[keep] == 0).sum())) if len(keep) else None
    return len(kp), len(keep), np.bincount(octave, minlength=1).tolist() if len(keep) else [], idx, len(set(zip(k["x"].tolist(), k["y"].tolist(), k["size"].tolist())))


def test_the_sift_tests_inputs():
    n, kept, per_octave, idx, _ = counts(sift_cases.image("kitti"))
    assert (n, kept, per_octave, idx) == (287, 256, [162, 63, 23, 7, 1], (0, 28, 229))
    assert counts(sift_cases.image("strided"))[:2] == (8, 5) and not sift_cases.image("strided").flags["C_CONTIGUOUS"]
    assert counts(sift_cases.image("noise"))[:2] == (21, 13)
    assert counts(sift_cases.image("flat"))[:2] == (0, 0)


@pytest.mark.parametrize("name, side, expect",
                         [("crop", 0, (727, 672, [434, 174, 49, 12, 3], (0, 36, 610), 567)),
                          ("crop", 1, (728, 670, [432, 162, 61, 12, 3], (0, 36, 595), 556)),       # the mirror image
                          ("strided", 0, (285, 245, [155, 67, 14, 9], (0, 22, 222), 185)),
                          ("strided", 1, (279, 261, [158, 77, 18, 8], (0, 21, 236), 209))])
def test_sift_keypoints_of_the_small_pairs(sample_images, name, side, expect):
    img = stereo_pairs(sample_images)[name][side]
    assert img.shape == dict(crop=(240, 400), strided=(200, 400))[name]
    got = counts(img)
    print(name, side, img.shape, got)
    assert got == expect
    n, kept, per_octave, idx, distinct = got
    # what the inputs must meet
    assert n >= 200 and 2 * kept > n and kept < n                      # survivors and casualties of the border rule
    assert per_octave[0] > 0 and sum(1 for c in per_octave if c) >= 3  # octave -1 (the doubled image) and several more
    assert idx[0] == 0 and idx[1] > 0 and idx[2] > 0                   # scale index 0 and above
    assert distinct < kept                                             # several keypoints of one candidate: one per orientation peak


def test_the_tiny_inputs():
    """14 x 14 noise: keypoints, none of which passes the border rule; smaller squares of the same noise have none; 6 x 6 is the smallest
    image the detector takes"""
    assert counts(tiny_image())[:2] == (2, 0)
    for n in range(6, 14):
        assert counts(np.random.RandomState(1).randint(0, 256, (n, n)).astype(np.uint8))[0] == 0, n
    assert sr.MIN_SIDE == 6
    with pytest.raises(ValueError):
        sr.detect(np.zeros((5, 5), np.uint8))


def test_the_sizes_stay_clear_of_a_scale_index_boundary(sample_images):
    """why no natural input takes the second pass: the scale index changes where 64 log2(size / 7.2) / log2(30) + 0.5 crosses an integer;
    the inputs' sizes stay further from that than 5e-4 of the index, and one float ulp of a size moves it by about 2e-6"""
    worst = 1.0
    for img in [sift_cases.image("kitti")] + list(stereo_pairs(sample_images)["crop"]):
        size = sift_keypoints(img)["size"].astype(np.float64)
        w = 64.0 * np.log2(size / (12.0 * 0.6)) / np.log2(30.0) + 0.5
        w = w[(w >= 1.0) & (w < 64.0)]                                  # (below 1 the index is 0 whatever the fraction)
        worst = min(worst, float(np.abs(w - np.rint(w)).min()))
    print("closest to a boundary, in units of the index:", worst)
    assert worst > 5e-4
    ulp = 64.0 / np.log(30.0) * float(np.finfo(np.float32).eps)         # d index / d ln(size) x one relative ulp
    assert ulp < 3e-6
