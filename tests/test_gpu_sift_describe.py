"""spvo_sift_describe (csrc/sift.hip.h: sift_describe_given_kernel, csrc/spvo_sift.hip) against the numpy restatement
tests/sift_describe_ref.py, and the classic front end's five detector + SIFT pairs: the probes, and FAST + SIFT and BRISK + SIFT against
oracle/odometry.py's state machine.

The pyramid is bit-exact.  The descriptor uses exp / atan2 / sin / cos and sums in another order than the restatement; its tolerance comes
from the restatement's own float32-versus-float64 figures (tests/test_sift_describe_ref_cpu.py, YARDSTICKS: percentile 99 = 0 on all three
lists, maximum 1 / 0 / 0), with tests/test_gpu_sift.py's bars: at least 99 % of the rows within max(1, 2 x percentile 99) = 1, none beyond
4 x that."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import frontend as ofe, matching, odometry as od
from spvo import capi, host, synth
from tests import brisk_detect_ref as bd, classic_ref, sift_cases as sc, sift_describe_cases as dc, sift_describe_ref as sd
from tests.conftest import make_ctx
from tests.test_sift_describe_ref_cpu import YARDSTICKS

pytestmark = pytest.mark.gpu


def desc_bound(name):
    assert YARDSTICKS[name][1] <= 1                        # the condition under which an input may be used here
    return max(1.0, 2.0 * YARDSTICKS[name][1])


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def held_to_the_restatement(got, want, name, what):
    """every row, in order: the bars of the module's docstring"""
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, np.rint(got)) and (len(got) == 0 or (got.min() >= 0 and got.max() <= 255))
    d = dc.row_difference(got, want)
    bound = desc_bound(name)
    within = float((d <= bound).mean())
    print(what, "rows", len(d), "largest difference per row: percentile 50 / 99 / max", float(np.percentile(d, 50)), float(np.percentile(d, 99)), float(d.max()), "rows that differ",
          int((d > 0).sum()), "within", bound, ":", within)
    assert within >= 0.99 and d.max() <= 4 * bound


def raw_describe(c, img, shape, kp, desc):
    """the status of spvo_sift_describe writing into `desc`"""
    kp = np.ascontiguousarray(kp, capi.SIFT_KP_DTYPE)
    if img is not None:
        img = np.ascontiguousarray(img, np.uint8)
    return c.lib.spvo_sift_describe(c.h, None if img is None else img.ctypes.data, shape[0], shape[1], 0 if img is None else img.strides[0], kp.ctypes.data if len(kp) else None,
                                    len(kp), desc.ctypes.data)


def test_pyramid_without_doubling_on_the_strided_input(ctx):
    """octaves 0 .. 3 of the 101 x 147 view (both sides odd, rows not contiguous): the base is the image at its own size"""
    img = sc.image("strided")
    assert not img.flags["C_CONTIGUOUS"]
    kp = dc.records([20.0, 60.0, 90.0, 33.0], [20.0, 50.0, 70.0, 41.0], [7.0, 12.0, 30.0, 50.0], [-1.0, 10.0, 200.0, 359.0], [sd.pack(o, o + 1) for o in range(4)])
    got = ctx.sift_describe(img, kp)
    want = sd.pyramid(np.ascontiguousarray(img), 0, 4)
    for o in range(4):
        for i in range(6):
            lv = ctx.sift_level(o, i)
            assert lv.shape == want[o][i].shape and np.array_equal(bits(lv), bits(want[o][i])), (o, i, float(np.abs(lv - want[o][i]).max()))
    assert [ctx.sift_level(o, 0).shape for o in range(4)] == [(101, 147), (50, 73), (25, 36), (12, 18)]
    with pytest.raises(capi.SpvoError) as e:
        ctx.sift_level(4, 0)
    assert e.value.code == -1
    with pytest.raises(capi.SpvoError) as e:                # no difference of Gaussians is built
        ctx.sift_level(0, 0, dog=True)
    assert e.value.code == -4
    held_to_the_restatement(got, sd.describe(np.ascontiguousarray(img), kp, gauss=want), "handmade", "strided, octaves 0..3")
    ctx.sift_detect(img, cap=0)                             # the detector's pyramid takes the place over, differences included
    assert ctx.sift_level(0, 0, dog=True).shape == (202, 294)


@pytest.mark.parametrize("name", ["strided", "noise"])
def test_pyramid_of_a_list_with_octave_minus_one(ctx, name):
    img = sc.image(name)
    kp = dc.records([12.0, 30.0, 41.5], [9.0, 33.0, 20.25], [4.0, 9.0, 21.0], [-1.0, 90.0, 0.0], [sd.pack(-1, 2), sd.pack(0, 0), sd.pack(2, 5)])
    got = ctx.sift_describe(img, kp)
    want = sc.stage(name)["gauss"]
    for o in range(4):                                      # octaves -1 .. 2
        for i in range(6):
            lv = ctx.sift_level(o, i)
            assert lv.shape == want[o][i].shape and np.array_equal(bits(lv), bits(want[o][i])), (o, i)
    with pytest.raises(capi.SpvoError) as e:
        ctx.sift_level(4, 0)
    assert e.value.code == -1
    held_to_the_restatement(got, sd.describe(np.ascontiguousarray(img), kp, gauss=want), "handmade", name + ", octaves -1..2")


@pytest.mark.parametrize("name", ["fast", "handmade", "brisk_style"])
def test_descriptors(ctx, name):
    """Measured on the MI355X: no row of the three lists differs from the float32 restatement (fast 0 of 1224, handmade 0 of 300,
    brisk_style 0 of 120).  Before the kernels reproduced the rule's single wrap of the orientation bin (sift_share_bin: orientation 361,
    i.e. angle -1, with gradient angles below one degree) 326 rows of `fast` differed by 1 and 4 by 2."""
    kp = dc.keypoints(name)
    assert len(kp) == YARDSTICKS[name][0]
    got = ctx.sift_describe(dc.image(name), kp)
    held_to_the_restatement(got, dc.reference(name), name, name)
    assert got.any(axis=1).sum() >= 0.75 * len(kp)


def test_both_forms_of_the_sum_meet_the_bar(ctx):
    """tuning "sift_describe_form" = 1 selects the staged form NOTES.md measures against the columns: another order of the same sums"""
    kp, img = dc.keypoints("fast"), dc.image("fast")
    columns = ctx.sift_describe(img, kp)
    capi.set_tuning("sift_describe_form", 1)
    try:
        staged = ctx.sift_describe(img, kp)
        again = ctx.sift_describe(img, kp)
    finally:
        capi.set_tuning("sift_describe_form", 0)
    held_to_the_restatement(staged, dc.reference("fast"), "fast", "fast, staged form")
    assert staged.tobytes() == again.tobytes()
    d = dc.row_difference(staged, columns)
    print("staged against columns: rows that differ", int((d > 0).sum()), "largest", float(d.max()))
    assert ctx.sift_describe(img, kp).tobytes() == columns.tobytes()


def test_the_detectors_own_records(ctx):
    """spvo_sift_detect's records described again: within 1 of its rows (the restatement: 286 of 287 identical, largest difference 1)"""
    img = sc.image("kitti")
    g = ctx.sift_detect(img)
    rows = ctx.sift_describe(img, g["kp"])
    d = dc.row_difference(rows, g["desc"])
    print("own records:", int((d == 0).sum()), "of", len(d), "rows identical, largest difference", float(d.max()))
    assert len(d) > 100 and d.max() <= 1


def test_determinism_and_the_resident_image(ctx):
    img, kp = dc.image("fast"), dc.keypoints("fast")
    a = ctx.sift_describe(img, kp)
    b = ctx.sift_describe(img, kp)
    assert a.tobytes() == b.tobytes()
    f = ctx.fast(img)
    assert np.array_equal(f["xy"], np.stack([kp["x"], kp["y"]], 1))            # the restatement's corners are the library's
    c = ctx.sift_describe(None, kp, shape=img.shape)                             # the image spvo_fast_detect left on the device
    assert c.tobytes() == a.tobytes()
    part = ctx.sift_describe(None, kp[100:140], shape=img.shape)                 # a row depends on its own record only
    assert part.tobytes() == a[100:140].tobytes()
    other = sc.image("strided")                                                  # another shape and back: the scratch is regrown
    ko = dc.records([20.0], [20.0], [7.0], [-1.0], [0])
    o1 = ctx.sift_describe(other, ko)
    assert ctx.sift_describe(img, kp).tobytes() == a.tobytes()
    assert ctx.sift_describe(np.ascontiguousarray(other), ko).tobytes() == o1.tobytes()
    sentinel = np.full((1, 128), 7.5, np.float32)
    assert raw_describe(ctx, None, other.shape, kp[:0], sentinel) == 0 and (sentinel == 7.5).all()       # n == 0, on the resident image ...
    assert raw_describe(ctx, img, img.shape, kp[:0], sentinel) == 0 and (sentinel == 7.5).all()          # ... and with one
    assert ctx.sift_describe(None, kp[:5], shape=img.shape).tobytes() == a[:5].tobytes()
    fresh = make_ctx()
    try:
        assert raw_describe(fresh, None, img.shape, kp, np.zeros((len(kp), 128), np.float32)) == -4       # nothing resident
    finally:
        fresh.close()


def test_refusals_touch_nothing(ctx):
    """every SPVO_ERR_INVALID case with and without an image, the shape that is not resident; a valid call afterwards gives the earlier bytes
    and the resident pyramid is the earlier one"""
    img, kp = dc.image("brisk_style"), dc.keypoints("brisk_style")[:40].copy()
    rows, cols = img.shape                                                        # 64 x 96: octave 6 is the last with a level
    good = ctx.sift_describe(img, kp)
    level = ctx.sift_level(2, 3)
    desc = np.full((len(kp), 128), 7.5, np.float32)
    bad = []
    for field, value in (("x", np.nan), ("x", np.inf), ("y", -np.inf), ("y", np.nan), ("size", np.nan), ("size", np.inf), ("size", 0.0), ("size", -3.0), ("angle", np.nan),
                         ("angle", np.inf), ("octave", 254), ("octave", sd.pack(-2, 1)), ("octave", sd.pack(0, 6)), ("octave", sd.pack(1, 255)), ("octave", sd.pack(7, 0)),
                         ("octave", sd.pack(40, 0)), ("octave", sd.pack(127, 2))):
        r = kp.copy()
        r[field][17] = value
        bad.append(r)
    for r in bad:
        for image in (None, img):                                                 # checked before an image is uploaded, too
            assert raw_describe(ctx, image, img.shape, r, desc) == -1, r[17]
            assert (desc == 7.5).all()
    assert raw_describe(ctx, None, (5, 96), kp, desc) == -1 and raw_describe(ctx, np.zeros((5, 96), np.uint8), (5, 96), kp, desc) == -1     # an image spvo_sift_detect refuses
    assert raw_describe(ctx, None, (rows, cols + 1), kp, desc) == -4 and (desc == 7.5).all()                                                # no image of that shape is resident
    r = kp.copy()
    r["octave"][3] = sd.pack(6, 0)                                                # 64 >> 6 = 1: legal, a level of 1 x 1 without a sample
    assert raw_describe(ctx, None, img.shape, r, desc) == 0 and not desc[3].any() and desc[4].tobytes() == good[4].tobytes()
    ctx.sift_describe(None, kp, shape=img.shape)
    assert ctx.sift_level(2, 3).tobytes() == level.tobytes()
    assert ctx.sift_describe(None, kp, shape=img.shape).tobytes() == good.tobytes()


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(3, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def test_a_submission_in_flight_refuses_the_call_and_touches_nothing(sequence, squeeze_weights_path):
    frames, _, P_l, P_r = sequence
    img, kp = dc.image("brisk_style"), dc.keypoints("brisk_style")[:40]
    c = make_ctx(squeeze_weights_path)
    try:
        before = c.sift_describe(img, kp)
        level = c.sift_level(1, 2)
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)             # a SuperPoint submission in flight
        desc = np.full((len(kp), 128), 7.5, np.float32)
        for image in (None, img):
            assert raw_describe(c, image, img.shape, kp, desc) == -4
            assert (desc == 7.5).all()
        c.detect_collect(P_l, P_r)
        assert c.sift_level(1, 2).tobytes() == level.tobytes()
        assert c.sift_describe(None, kp, shape=img.shape).tobytes() == before.tobytes()
    finally:
        c.close()


def detector_counts(c, img):
    return {"ShiTomasi": len(c.gftt(img)["xy"]), "FAST": len(c.fast(img)["xy"]), "ORB": len(c.orb(img)["xy"]), "BRISK": c.brisk_detect(img)["n"], "AKAZE": c.akaze_detect(img)["n"]}


def test_front_end_pushes_aligned_features_for_the_five_pairs(ctx, sequence):
    """ClassicFeatureFrontEnd(d, SIFT, BF, ...) at the native resolution on the 160 x 400 crop: two deque entries, keypoints and rows of 128
    floats one to one and as many as the detector itself reports (the extractor erases nothing); no error logged."""
    frames, _, P_l, P_r = sequence
    L, R = (np.ascontiguousarray(im[40:200, 300:700]) for im in frames[0])
    want = [detector_counts(ctx, im) for im in (L, R)]
    for d in ("ShiTomasi", "FAST", "ORB", "BRISK", "AKAZE"):
        n, counts, err = host.classic_pair_probe(d, "SIFT", L, R, P_l, P_r)
        print(d, "+ SIFT:", n, counts.tolist(), err)
        assert n == 2 and err == "", err
        assert counts[0] == counts[1] == want[0][d] > 0 and counts[2] == counts[3] == want[1][d] > 0 and counts[4] == 128


def restatement_keypoints(detector, small):
    if detector == "FAST":                                  # KeyPoint(x, y, 7.f, -1, score), octave 0
        f = classic_ref.fast(small)
        n = len(f["xy"])
        return dc.records(f["xy"][:, 0], f["xy"][:, 1], np.full(n, 7.0), np.full(n, -1.0), np.zeros(n, np.int32), f["response"])
    k = bd.detect(small, 30)                                # the detector's records as they are: size 12 x scale, angle -1, octave = layer
    return dc.records(k["x"], k["y"], k["size"], k["angle"], k["octave"], k["response"])


@pytest.mark.parametrize("detector", ["FAST", "BRISK"])
def test_classic_front_end_with_sift_rows_equals_the_oracle_state_machine(sequence, detector):
    """classic_sequence(frames[:3], detector, descriptor="SIFT", input_size=(120, 392)) (KNN) against oracle/odometry.py's FrontEndState fed the
    RESTATEMENT's keypoints (tests/classic_ref.py / tests/brisk_detect_ref.py on the oracle's preprocessed image), the library's rows for
    them (held to tests/sift_describe_ref.py's by the descriptor's own bar, on the first pair) and oracle.matching's L2 maps: keypoint,
    stereo-match and inlier counts identical, poses within 1e-6.  Absolute bars: the all-CPU pipeline (restatements, oracle.matching,
    oracle.odometry) on these frames gives FAST + SIFT 1222 / 1234 / 1204 left keypoints, 372 and 394 inliers, translation 0.0069 and 0.0137
    from the synthetic motion; BRISK + SIFT 1040 / 1062 / 1049 keypoints, 154 and 161 inliers, 0.0096 and 0.0128 (NOTES.md, "SIFT extractor on
    given keypoints") -- so test_gpu_sift.py's bars are asserted: more than 100 keypoints, more than 20 inliers, within 0.1.  With
    resident=True the pair takes the per-image path: the same digests, no pair counted as resident."""
    frames, gt, P_l, P_r = sequence
    poses, stats, _, digests = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector=detector, descriptor="SIFT", input_size=(120, 392), trace=True)
    ctx = make_ctx()
    st = od.FrontEndState()
    prev_dl = None
    for k, (L, R) in enumerate(frames):
        feats, Ps = [], []
        for img, P in ((L, P_l), (R, P_r)):
            small, Pk = ofe.preprocess(img, np.asarray(P, np.float64).reshape(3, 4), 120, 392)[:2]
            small = np.ascontiguousarray(small)
            kp = restatement_keypoints(detector, small)
            d = ctx.sift_describe(small, kp)
            if k == 0:
                held_to_the_restatement(d, sd.describe(small, kp), "fast" if detector == "FAST" else "brisk_style", detector + " frame 0")
            feats.append((np.stack([kp["x"], kp["y"]], 1), d))
            Ps.append(Pk)
        (xyl, dl), (xyr, dr) = feats
        od.add_features(st, xyl, dl, xyr, dr, Ps[0], Ps[1])
        idx0, _ = matching.bf_match(dl, dr, "KNN", False, 0.8)
        st.maps[od.PREV_LEFT_PREV_RIGHT] = st.maps[od.CURR_LEFT_CURR_RIGHT]
        st.maps[od.CURR_LEFT_CURR_RIGHT] = idx0
        print(k, "stats", stats[k].tolist(), "oracle", len(xyl), len(xyr), int((idx0 >= 0).sum()))
        assert stats[k, 0] == len(xyl) > 100 and stats[k, 1] == len(xyr) and stats[k, 2] == int((idx0 >= 0).sum())
        if k > 0:
            idx1, _ = matching.bf_match(dl, prev_dl, "KNN", False, 0.8)
            st.maps[od.CURR_LEFT_PREV_LEFT] = idx1
            q, t, dbg = od.solve_stereo_odometry(st, 2.0, 2.0, 4)
            Rc, Rg = od.quat_to_rot(np.asarray(q)), od.quat_to_rot(poses[k, :4])
            _, tt = synth.relative_pose(gt[k - 1], gt[k])
            print("   inliers", stats[k, 3], len(dbg["inliers"]), "pose difference R %.3g t %.3g; t vs synthetic motion %.3g" % (
                np.abs(Rg - Rc).max(), np.abs(poses[k, 4:] - t).max(), np.abs(poses[k, 4:] - tt).max()))
            assert stats[k, 3] == len(dbg["inliers"]) > 20
            assert np.abs(Rg - Rc).max() <= 1e-6 and np.abs(poses[k, 4:] - t).max() <= 1e-6
            assert np.abs(poses[k, 4:] - tt).max() < 0.1
        prev_dl = dl
    ctx.close()
    poses_r, stats_r, _, digests_r = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector=detector, descriptor="SIFT", input_size=(120, 392), resident=True, trace=True)
    assert np.array_equal(digests_r, digests) and np.array_equal(stats_r, stats) and np.array_equal(poses_r, poses)
    assert host.classic_resident_pairs() == 0
