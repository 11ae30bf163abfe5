"""tests/akaze_mldb_ref.py without a GPU: the Gaussian table against its formula, the polynomial arctangent's worst error (measured here:
the size of rule O4's deviation from OpenCV, and the bar of the ramp test), what linear ramps and a constant image give, the window and
sample counts, the unused bits, the hand-made records' coverage, the restatement's float32-versus-float64 figures on every parity case,
and the all-CPU pipeline on the synthetic frames -- what tests/test_gpu_akaze_mldb.py relies on, checked here first."""
import math
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import frontend as ofe, matching, odometry as od
from spvo import capi, synth
from tests import akaze_cases as ac, akaze_mldb_cases as mc, akaze_mldb_ref as mr, akaze_ref as ak


def test_library_exports_the_describe_entry_point():
    lib = capi.load()
    assert hasattr(lib, "spvo_akaze_describe") and "spvo_akaze_describe" in capi.SYMBOLS
    assert callable(capi.Context.akaze_describe) and capi.AKAZE_DESC_BYTES == mr.DESC_BYTES == 61
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "spvo.h")) as f:
        assert "#define SPVO_AKAZE_DESC_BYTES 61" in f.read()


# The table as written is the definition (SURF's gauss25, as OpenCV carries it).  Its entries are NOT all the formula's value to eight
# decimals: 25 of the 49 miss it by more than half a unit of the eighth decimal, the largest (the centre) by 1.91e-8, a relative 7.5e-7.  Pinned.
GAUSS25_LARGEST_DEVIATION = 1.92e-8


def test_gauss25_is_symmetric_and_close_to_its_formula():
    g = mr.GAUSS25
    assert g.shape == (7, 7) and np.array_equal(g, g.T) and len(mr._G) == 28
    assert g[0].tolist() == [0.02546481, 0.02350698, 0.01849125, 0.01239505, 0.00708017, 0.00344629, 0.00142946]
    exact = np.array([[math.exp(-(i * i + j * j) / 12.5) / (12.5 * math.pi) for j in range(7)] for i in range(7)])
    dev = np.abs(g - exact)
    print("gauss25: largest deviation from exp(-(i^2 + j^2) / 12.5) / (12.5 pi): %.3g at %s; entries beyond half a unit of the eighth decimal: %d of 49" % (
        dev.max(), np.unravel_index(dev.argmax(), dev.shape), int((dev > 0.5e-8).sum())))
    assert 0.5e-8 < dev.max() <= GAUSS25_LARGEST_DEVIATION


def _atan_worst():
    """the polynomial against math.atan2 over 3600 directions -- every multiple of 45 degrees as the EXACT direction (c = 0 or c = 1) --
    and five magnitudes -> degrees"""
    th = np.arange(3600) * (2.0 * math.pi / 3600.0)
    ux, uy = np.cos(th), np.sin(th)
    for k in range(0, 3600, 450):
        ux[k], uy[k] = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)][k // 450]
    worst = 0.0
    for mag in (1e-6, 1e-3, 1.0, 37.5, 1e4):
        y, x = (mag * uy).astype(np.float32), (mag * ux).astype(np.float32)
        a = mr.fast_atan(y, x).astype(np.float64)
        t = np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64))) % 360.0
        d = np.abs(a - t)
        worst = max(worst, float(np.minimum(d, 360.0 - d).max()))
    return worst


def test_polynomial_arctangent_error_is_measured():
    worst = _atan_worst()
    print("fastAtan32f polynomial against atan2: worst error %.6f degrees" % worst)
    assert 0.0 < worst < 0.3                                      # (OpenCV documents 0.3 degrees for fastAtan2; the figure itself is the ramp test's bar)
    a1, a2 = mr.windows()
    assert len(a1) == mr.NWINDOWS == 42 and len(mr.SAMPLES) == mr.NSAMPLES == 109
    assert a1[0] == 0 and a1[-1] < np.float32(2 * math.pi) <= np.float32(a1[-1] + np.float32(0.15))
    assert (a2[:35] > a1[:35]).all() and (a2[35:] < a1[35:]).all()            # the last seven windows wrap


@pytest.mark.parametrize("direction", range(0, 360, 45))
def test_a_linear_ramp_is_oriented_along_its_gradient(direction):
    """a ramp rising along `direction` (image axes: x right, y down; cv::KeyPoint's angle) with a level-0 record at the centre: the angle
    is the direction within the polynomial's measured worst error"""
    bar = _atan_worst()
    gx, gy = round(math.cos(math.radians(direction))), round(math.sin(math.radians(direction)))
    yy, xx = np.mgrid[0:97, 0:97]
    img = (128 + gx * (xx - 48) + gy * (yy - 48)).astype(np.uint8)
    levels, _ = ak.scale_space(img)
    rec = np.array([(48.0, 48.0, 4.8, -1.0, 0.0, 0, 0)], ak.KP_DTYPE)
    angle, desc = mr.describe(levels, rec)
    err = abs(float(angle[0]) - direction)
    err = min(err, 360.0 - err)
    print("ramp", direction, "angle", float(angle[0]), "error", err, "bar", bar)
    assert err <= bar
    assert desc.any()


def test_a_constant_image_gives_angle_zero_and_zero_bytes():
    img = ac.case("flat")
    levels, _ = ak.scale_space(img)
    rec = mc.flat_records(img.shape)
    angle, desc = mr.describe(levels, rec)
    assert len(rec) > 3 and angle.dtype == np.float32 and not angle.any() and desc.shape == (len(rec), 61) and not desc.any()


@pytest.mark.parametrize("name", mc.HAND_IMAGES)
def test_hand_made_records_cover_what_they_are_meant_to(name):
    img = ac.case(name)
    levels, derivs, _, _, _ = mc.reference(name)
    rec = mc.hand_records(img.shape)
    dbg = {}
    angle, desc = mr.describe(levels, rec, derivs, debug=dbg)
    ns = dbg["nsamples"]
    full = np.repeat(np.array(mr.GRIDS) ** 2, [4, 9, 16])[None, :]
    ratio = 2.0 ** rec["octave"]
    s = np.rint(np.float32(0.5) * rec["size"] / ratio.astype(np.float32))
    print(name, "records", len(rec), "s", sorted(set(s.tolist())), "cells with no sample", int((ns == 0).sum()), "partly skipped", int(((ns > 0) & (ns < full)).sum()))
    assert len(rec) > 65 and set(rec["class_id"].tolist()) == set(range(len(levels)))
    assert (s == 0).any() and (s == 60).any() and (s == 2).any()
    assert (ns == 0).any() and ((ns > 0) & (ns < full)).any() and (ns == full).all(1).any()
    assert (ns.sum(1)[s == 60] < 0.5 * full.sum()).all()                                  # "most samples are skipped"
    assert (((rec["x"] / ratio) % 1 == 0.5) & ((rec["y"] / ratio) % 1 == 0.5)).any()
    borders = [L for L in levels if min(L["Lt"].shape) <= 2 * ak.level_border(L["sigma_size"])]
    assert name != "two_odd" or borders                                                  # levels with no room inside their extrema border
    assert not (desc[:, 60] & 0xC0).any() and np.isfinite(angle).all() and ((angle >= 0) & (angle <= 360)).all()


# float32 against float64 restatement (same keypoints, the float32 detector's): rows that differ, bits that differ, the largest angle
# difference in degrees rounded up to 1e-3.  Informational (NOTES.md, "AKAZE descriptor"): it says how many comparisons sit within
# float32 rounding of a tie, not how good the descriptor is.
@pytest.mark.parametrize("name", ac.CASES + ["full_size"])
def test_float32_versus_float64_figures_and_unused_bits(sample_images, name):
    img = ac.image_case(name, sample_images)
    levels, derivs, kp, angle, desc = mc.reference(name, sample_images)
    levels64, _ = ak.scale_space(img, ft=np.float64)
    angle64, desc64 = mr.describe(levels64, kp, ft=np.float64)
    diff = np.unpackbits(desc ^ desc64, axis=1).sum(1)
    da = np.abs(angle.astype(np.float64) - angle64)
    da = np.minimum(da, 360 - da)
    print(name, img.shape, "keypoints", len(kp), "rows that differ", int((diff > 0).sum()), "bits that differ", int(diff.sum()), "of", len(kp) * 486,
          "largest angle difference %.4f" % (da.max() if len(kp) else 0.0))
    assert desc.shape == (len(kp), 61) and not (desc[:, 60] & 0xC0).any() and not (desc64[:, 60] & 0xC0).any()
    assert np.isfinite(angle).all() and ((angle >= 0) & (angle <= 360)).all()
    if name != "flat":
        assert len(kp) > 0 and desc.any(1).all()


def test_all_cpu_pipeline_clears_the_bars_the_gpu_sequence_test_asserts(golden_dir):
    """restatements (detector, orientation + MLDB), oracle.matching.bf_match_hamming and oracle.odometry on the three synthetic frames at
    120 x 392, KNN: more than 100 keypoints, more than 20 inliers, translation within 0.1 of the synthetic motion -- the absolute bars
    tests/test_gpu_akaze_mldb.py asserts on top of equality with the oracle.  The figures are in NOTES.md ("AKAZE descriptor")."""
    frames, gt, P_l, P_r = synth.stereo_sequence(3, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)
    st = od.FrontEndState()
    prev_dl = None
    for k, (L, R) in enumerate(frames):
        feats, Ps = [], []
        for img, P in ((L, P_l), (R, P_r)):
            small, Pk = ofe.preprocess(img, np.asarray(P, np.float64).reshape(3, 4), 120, 392)[:2]
            levels, _ = ak.scale_space(np.ascontiguousarray(small))
            kp = ak.detect(small, levels=levels)
            feats.append((np.stack([kp["x"], kp["y"]], 1), mr.describe(levels, kp)[1]))
            Ps.append(Pk)
        (xyl, dl), (xyr, dr) = feats
        od.add_features(st, xyl, dl, xyr, dr, Ps[0], Ps[1])
        idx0, _ = matching.bf_match_hamming(dl, dr, "KNN", False, 0.8)
        st.maps[od.PREV_LEFT_PREV_RIGHT] = st.maps[od.CURR_LEFT_CURR_RIGHT]
        st.maps[od.CURR_LEFT_CURR_RIGHT] = idx0
        print(k, "keypoints", len(xyl), len(xyr), "stereo matches", int((idx0 >= 0).sum()))
        assert len(xyl) > 100 and len(xyr) > 100
        if k > 0:
            idx1, _ = matching.bf_match_hamming(dl, prev_dl, "KNN", False, 0.8)
            st.maps[od.CURR_LEFT_PREV_LEFT] = idx1
            q, t, dbg = od.solve_stereo_odometry(st, 2.0, 2.0, 4)
            _, tt = synth.relative_pose(gt[k - 1], gt[k])
            err = float(np.abs(np.asarray(t) - tt).max())
            print("   temporal matches", int((idx1 >= 0).sum()), "inliers", len(dbg["inliers"]), "translation error %.4f" % err)
            assert len(dbg["inliers"]) > 20 and err < 0.1
        prev_dl = dl
