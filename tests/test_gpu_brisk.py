"""GPU parity of the classic front end's BRISK descriptor extractor (csrc/brisk.hip.h; spvo_brisk_describe, spvo_brisk_tables) against the
numpy restatement tests/brisk_ref.py: the tables against the restatement's own float64 build, the extractor bit for bit against the
restatement run on the LIBRARY's tables, the resident image and the error codes, and the two new configurations of
ClassicFeatureFrontEnd (ShiTomasi + BRISK, FAST + BRISK) through the host class.  Inputs: tests/brisk_cases.py; the CPU test
tests/test_brisk_ref_cpu.py asserts that none of their rows lies on a rotation boundary."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import matching, odometry as od
from spvo import capi, host, synth
from tests import brisk_cases as bc, brisk_ref as br, classic_ref as cr
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib_tables():
    return capi.brisk_tables()


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(5, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def _adjacent(a, b):
    """equal, or the neighbouring float32"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a == b) | (np.nextafter(b, np.float32(np.inf)) == a) | (np.nextafter(b, np.float32(-np.inf)) == a)


def test_tables_equal_the_restatements_own_float64_build(lib_tables):
    T = br.own_tables()
    for k in ("short_pairs", "long_pairs", "size_list"):                               # integer members: equal
        assert lib_tables[k].dtype == np.int32 and np.array_equal(lib_tables[k], T[k]), k
    for k in ("points", "scale_list"):                                                 # float members: equal or the adjacent float32
        assert lib_tables[k].shape == T[k].shape and _adjacent(lib_tables[k], T[k]).all(), k
        print(k, "elements that differ from the float64 build:", int((lib_tables[k] != T[k]).sum()))


def _compare(g, r, n_in):
    """spvo_brisk_describe's output against the restatement's: kept, values0, angle, theta, descriptor bytes"""
    assert np.array_equal(g["kept"], r["kept"])
    assert np.array_equal(g["values0"], r["values0"])
    assert g["desc"].shape == (len(r["kept"]), 64) and g["angle"].shape == (len(r["kept"]),)
    assert _adjacent(g["angle"], r["angle"]).all()
    boundary = r["boundary"]
    nb = int(boundary.sum())
    print("keypoints", n_in, "kept", len(r["kept"]), "boundary rows", nb, "angles that differ in the last place", int((g["angle"] != r["angle"]).sum()))
    assert nb <= 0.01 * len(r["kept"])
    ok = ~boundary
    assert np.array_equal(br.theta_from_reported(g["angle"])[ok], r["theta"][ok])
    assert np.array_equal(g["desc"][ok], r["desc"][ok])
    if len(r["kept"]):
        assert (g["angle"] >= 0).all() and (g["angle"] <= 360).all()


@pytest.mark.parametrize("name", bc.CASES)
def test_describe_equals_the_restatement_on_the_librarys_tables(sample_images, lib_tables, name):
    """64 x 96 smoothed noise with a keypoint grid across the four borders and sizes {5, 7, 12.3, 31, 60} (scale 0, scale 10, and two scales
    whose border drops everything here); fractional coordinates; the golden image at 120 x 392 with Shi-Tomasi keypoints; a strided view with
    FAST keypoints; no keypoint at all; a flat image -- where OpenCV's integer rules do NOT give dir == 0 and an all-zero descriptor (the
    truncated scaling2 depends on the ring's sigma: tests/test_brisk_ref_cpu.py has the figures), so the flat case is compared like the others."""
    img, xy, size = bc.image_case(name, sample_images)
    r = br.describe(img, xy, size, tables=lib_tables)
    ctx = make_ctx()
    g = ctx.brisk_describe(img, xy, size, values0=True)
    again = ctx.brisk_describe(img, xy, size)
    ctx.close()
    _compare(g, r, len(xy))
    assert np.array_equal(again["desc"], g["desc"]) and np.array_equal(again["angle"], g["angle"]) and "values0" not in again
    if name == "empty":
        assert len(g["kept"]) == 0 and g["desc"].shape == (0, 64)
    elif name == "noise_grid":
        assert set(np.unique(r["scale"]).tolist()) == {0, 10} and 0 < len(r["kept"]) < len(xy)
    elif name == "flat":
        assert len(r["kept"]) == len(xy)
    else:
        assert len(r["kept"]) > 50


def test_full_size_image_with_fast_keypoints_and_two_identical_calls(sample_images, lib_tables):
    img, xy, size = bc.image_case("full_size", sample_images)
    r = br.describe(img, xy, size, tables=lib_tables)
    assert len(r["kept"]) > 2000
    ctx = make_ctx()
    g = ctx.brisk_describe(img, xy, size, values0=True)
    h = ctx.brisk_describe(img, xy, size, values0=True)
    ctx.close()
    _compare(g, r, len(xy))
    for k in ("kept", "angle", "desc", "values0"):
        assert g[k].tobytes() == h[k].tobytes(), k


def test_the_resident_image_and_the_error_codes(sample_images):
    img = sample_images[0]
    h, w = img.shape
    ctx = make_ctx()
    with pytest.raises(capi.SpvoError) as e:                                           # nothing resident yet
        ctx.brisk_describe(None, np.array([[100, 100]], np.float32), 7.0, shape=img.shape)
    assert e.value.code == -4                                                       # SPVO_ERR_STATE
    xy = ctx.fast(img)["xy"]
    res = ctx.brisk_describe(None, xy, 7.0)                                            # the image of the detect call, still on the device
    up = ctx.brisk_describe(img, xy, 7.0)                                              # the same image uploaded again
    keep, _ = br.border_keep(xy, 7.0, img.shape)
    assert 0 < len(keep) < len(xy) and np.array_equal(res["kept"], keep)
    for k in ("kept", "angle", "desc"):
        assert np.array_equal(res[k], up[k]), k
    with pytest.raises(capi.SpvoError) as e:                                           # a shape that is not the resident one
        ctx.brisk_describe(None, xy[:10], 7.0, shape=(h - 1, w))
    assert e.value.code == -4
    one = np.array([[100, 100]], np.float32)
    for bad in (0.0, -3.0, np.inf, np.nan):
        with pytest.raises(capi.SpvoError) as e:
            ctx.brisk_describe(None, one, bad)
        assert e.value.code == -1, bad                                                 # SPVO_ERR_INVALID
    lib = ctx.lib
    m = capi.C.c_int(0)
    assert lib.spvo_brisk_describe(ctx.h, None, h, w, 0, None, None, -1, None, None, None, None, capi.C.byref(m)) == -1          # n < 0
    assert lib.spvo_brisk_describe(ctx.h, None, 65536, 65536, 0, None, None, 0, None, None, None, None, capi.C.byref(m)) == -1   # rows * cols * 255 >= 2^31
    assert lib.spvo_brisk_describe(ctx.h, None, 2903, 2901, 0, None, None, 0, None, None, None, None, capi.C.byref(m)) == -1     # 2147508765: the first shape of this width that does not fit
    assert lib.spvo_brisk_describe(ctx.h, None, 2902, 2901, 0, None, None, 0, None, None, None, None, capi.C.byref(m)) == -4     # 2146769010 fits: only not resident
    ok = ctx.brisk_describe(None, xy, 7.0)                                             # the context is still usable, the image still resident
    assert np.array_equal(ok["desc"], res["desc"])
    ctx.close()


def test_shitomasi_brisk_front_end_produces_aligned_features(sequence):
    """ClassicFeatureFrontEnd(ShiTomasi, BRISK, BF, ...) at the native resolution: keypoints and 64-byte descriptor rows one to one, as many
    as the restatement's border rule leaves."""
    frames, _, P_l, P_r = sequence
    L, R = frames[0]
    n, counts, err = host.classic_pair_probe("ShiTomasi", "BRISK", L, R, P_l, P_r)
    assert n == 2, err
    assert counts[0] == counts[1] > 0 and counts[2] == counts[3] > 0 and counts[4] == 64
    for img, got in ((L, counts[0]), (R, counts[2])):
        xy = cr.gftt(np.ascontiguousarray(img))["xy"]
        assert got == len(br.border_keep(xy, 5.0, img.shape)[0])


def _oracle_sequence(frames, P_l, P_r, detect, size):
    """oracle/odometry.py's state machine on the restatement's keypoints, the entry point's 64-byte descriptors and the Hamming oracle's maps
    (built as _oracle_sequence of tests/test_gpu_classic_detectors.py is)"""
    ctx = make_ctx()
    st = od.FrontEndState()
    out = []
    prev_dl = None
    for k, (L, R) in enumerate(frames):
        feats = []
        for img in (L, R):
            xy = detect(np.ascontiguousarray(img))["xy"]
            d = ctx.brisk_describe(img, xy, size)
            assert np.array_equal(d["kept"], br.border_keep(xy, size, img.shape)[0])
            feats.append((xy[d["kept"]], d["desc"]))
        (xyl, dl), (xyr, dr) = feats
        od.add_features(st, xyl, dl, xyr, dr, P_l, P_r)
        idx0, _ = matching.bf_match_hamming(dl, dr, "KNN", False, 0.8)
        st.maps[od.PREV_LEFT_PREV_RIGHT] = st.maps[od.CURR_LEFT_CURR_RIGHT]
        st.maps[od.CURR_LEFT_CURR_RIGHT] = idx0
        rec = dict(n_l=len(xyl), n_r=len(xyr), n_stereo=int((idx0 >= 0).sum()))
        if k > 0:
            idx1, _ = matching.bf_match_hamming(dl, prev_dl, "KNN", False, 0.8)
            st.maps[od.CURR_LEFT_PREV_LEFT] = idx1
            q, t, dbg = od.solve_stereo_odometry(st, 2.0, 2.0, 4)
            rec.update(q=q, t=t, n_inliers=len(dbg["inliers"]))
        prev_dl = dl
        out.append(rec)
    ctx.close()
    return out


@pytest.mark.parametrize("detector", ["ShiTomasi", "FAST"])
def test_classic_front_end_with_brisk_equals_the_oracle_state_machine(sequence, detector):
    """classic_sequence(frames[:4], detector=d, descriptor="BRISK") (KNN, native size, refinement degree 4) against oracle/odometry.py's
    FrontEndState: keypoint, stereo-match and PnP inlier counts identical, poses within 1e-6 (the bar of the ORB-descriptor test); with
    resident=True the same poses and stats, through the per-image fallback (the binary slots hold 32-byte rows)."""
    frames, gt, P_l, P_r = sequence
    frames = frames[:4]
    poses, stats, _ = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector=detector, descriptor="BRISK")
    ref = _oracle_sequence(frames, P_l, P_r, cr.gftt if detector == "ShiTomasi" else cr.fast, 5.0 if detector == "ShiTomasi" else 7.0)
    for k, r in enumerate(ref):
        print(detector, k, "stats", stats[k].tolist(), "oracle", {a: b for a, b in r.items() if a not in ("q", "t")})
    for k, r in enumerate(ref):
        assert stats[k, 0] == r["n_l"] > 100 and stats[k, 1] == r["n_r"] and stats[k, 2] == r["n_stereo"]
        if k == 0:
            continue
        assert stats[k, 3] == r["n_inliers"] and r["n_inliers"] > 20
        Rc, Rg = od.quat_to_rot(np.asarray(r["q"])), od.quat_to_rot(poses[k, :4])      # both: cam0_curr_T_cam0_prev
        assert np.abs(Rg - Rc).max() <= 1e-6 and np.abs(poses[k, 4:] - r["t"]).max() <= 1e-6
    poses_r, stats_r, _ = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector=detector, descriptor="BRISK", resident=True)
    assert np.array_equal(stats_r, stats) and np.array_equal(poses_r, poses)
    with pytest.raises(ValueError):
        host.classic_sequence(frames, P_l, P_r, detector=detector, descriptor="DAISY")
    with pytest.raises(RuntimeError):                                                  # BRISK on ORB keypoints is not a pair that runs: nothing is pushed
        host.classic_sequence(frames[:1], P_l, P_r, detector="ORB", descriptor="BRISK")
