"""GPU parity of the classic front end's AKAZE orientation and MLDB descriptor (csrc/akaze_mldb.hip.h; spvo_akaze_describe) against the
numpy restatement tests/akaze_mldb_ref.py: every angle and every 61-byte row bit for bit (compared as raw bytes, no row excused) on the
detector's keypoints of every case and on hand-made records whose samples leave the plane; the call on a given image against the call on
the resident scale space; determinism; the statuses; and ClassicFeatureFrontEnd(AKAZE, AKAZE) through the host class.  The restatement
takes the library's tables (spvo_akaze_tables), as tests/test_gpu_akaze.py does, whose cached scale spaces this file shares.  Inputs:
tests/akaze_cases.py and tests/akaze_mldb_cases.py; tests/test_akaze_mldb_ref_cpu.py asserts what those records are meant to cover."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import frontend as ofe, matching, odometry as od
from spvo import capi, host, synth
from tests import akaze_cases as ac, akaze_mldb_cases as mc, akaze_mldb_ref as mr, akaze_ref as ak
from tests.conftest import make_ctx
from tests.test_gpu_akaze import _reference, _tables          # (levels, k, keypoints) on the library's tables, cached per key

pytestmark = pytest.mark.gpu

ALL_CASES = ac.CASES + ["full_size"]


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


_DERIVS = {}


def _levels(img, key):
    """(levels, derivatives, detector keypoints) of the restatement on the library's tables, once per key"""
    if key not in _DERIVS:
        levels, _, kp = _reference(img, key)
        _DERIVS[key] = (levels, mr.derivatives(levels), kp)
    return _DERIVS[key]


def _assert_equal(got, angle, desc, what):
    """angles and rows as raw bytes; on a difference, say where"""
    assert got["angle"].shape == angle.shape and got["desc"].shape == desc.shape == (len(angle), 61), what
    bad_a = np.nonzero(got["angle"].view(np.uint32) != angle.view(np.uint32))[0]
    bad_d = np.nonzero((got["desc"] != desc).any(1))[0]
    assert len(bad_a) == 0 and len(bad_d) == 0, "%s: %d of %d angles differ (first %s: %r / %r), %d rows differ (first %s, %d bits)" % (
        what, len(bad_a), len(angle), bad_a[:1].tolist(), got["angle"][bad_a[:1]].tolist(), angle[bad_a[:1]].tolist(), len(bad_d), bad_d[:1].tolist(),
        int(np.unpackbits(got["desc"][bad_d[:1]] ^ desc[bad_d[:1]]).sum()))
    assert got["angle"].tobytes() == angle.tobytes() and got["desc"].tobytes() == desc.tobytes()


@pytest.mark.parametrize("name", ALL_CASES)
def test_angles_and_rows_of_the_detectors_keypoints_equal_the_restatement(ctx, sample_images, name):
    """akaze_detect, then akaze_describe(None, kp): every angle and every row of every keypoint bit for bit"""
    img = ac.image_case(name, sample_images)
    levels, derivs, ref_kp = _levels(img, name)
    kp = ctx.akaze_detect(img)["kp"]
    assert kp.tobytes() == ref_kp.tobytes()
    got = ctx.akaze_describe(None, kp)
    angle, desc = mr.describe(levels, kp, derivs)
    print(name, img.shape, "keypoints", len(kp), "angles", np.round(angle[:4], 2).tolist(), "bits set per row %.1f" % (np.unpackbits(desc).sum() / max(len(kp), 1)))
    assert (len(kp) > 0) == (name != "flat")
    _assert_equal(got, angle, desc, name)
    assert not (got["desc"][:, 60] & 0xC0).any()


def test_given_image_equals_resident_also_after_another_shape(ctx):
    """akaze_describe(img, kp) on a fresh context, and on a context whose last detect was on another shape, equals the resident call byte
    for byte; the scale space it built stays resident (akaze_level answers, akaze_describe(None) answers the same)"""
    img = ac.case("two_odd")
    levels, derivs, kp = _levels(img, "two_odd")
    resident = (ctx.akaze_detect(img), ctx.akaze_describe(None, kp))[1]
    fresh = make_ctx()
    try:
        given = fresh.akaze_describe(img, kp)
        assert fresh.akaze_level(5, 3).tobytes() == levels[5]["Ldet"].tobytes() and fresh.akaze_level(2, 0).tobytes() == levels[2]["Lt"].tobytes()
        again = fresh.akaze_describe(None, kp, shape=img.shape)
        fresh.akaze_detect(ac.case("blobs"))                                              # another shape: the buffers grow, the layout changes
        with pytest.raises(capi.SpvoError) as e:                                          # ... and NULL for the old shape is refused
            fresh.akaze_describe(None, kp, shape=img.shape)
        assert e.value.code == -4
        after = fresh.akaze_describe(img, kp)
        empty = fresh.akaze_describe(ac.case("one_octave"), kp[:0])                        # n == 0 with an image: its scale space is built
        assert empty["desc"].shape == (0, 61) and fresh.akaze_level(0, 0).shape == ac.case("one_octave").shape
    finally:
        fresh.close()
    assert len(kp) > 20
    for other in (given, again, after):
        assert other["angle"].tobytes() == resident["angle"].tobytes() and other["desc"].tobytes() == resident["desc"].tobytes()
    _assert_equal(resident, *mr.describe(levels, kp, derivs), "two_odd")


@pytest.mark.parametrize("name", mc.HAND_IMAGES)
def test_hand_made_records_equal_the_restatement(ctx, name):
    """records on every level, next to every border and corner, with s = 0, a cvRound tie, and s = 60 (tests/akaze_mldb_cases.py), in
    counts 1, 63, 64, 65, 0 and all at once: bit for bit.  Asserted first, on the CPU: one record has a cell with no sample at all, one
    has cells with some but not all samples skipped"""
    img = ac.case(name)
    levels, derivs, _ = _levels(img, name)
    rec = mc.hand_records(img.shape, _tables(*img.shape))
    dbg = {}
    angle, desc = mr.describe(levels, rec, derivs, debug=dbg)
    full = np.repeat(np.array(mr.GRIDS) ** 2, [4, 9, 16])[None, :]
    ns = dbg["nsamples"]
    print(name, "records", len(rec), "levels", len(levels), "cells with no sample", int((ns == 0).sum()), "partly skipped", int(((ns > 0) & (ns < full)).sum()), "complete", int((ns == full).sum()))
    assert len(rec) > 65 and set(rec["class_id"].tolist()) == set(range(len(levels)))
    assert (ns == 0).any() and ((ns > 0) & (ns < full)).any() and (ns == full).all(1).any()
    ctx.akaze_detect(img)
    _assert_equal(ctx.akaze_describe(None, rec), angle, desc, name + " all")
    for n in mc.HAND_COUNTS:
        got = ctx.akaze_describe(None, rec[:n])
        _assert_equal(got, angle[:n], desc[:n], "%s first %d" % (name, n))
    tail = ctx.akaze_describe(None, rec[-65:])                                            # a row does not depend on its place in the list
    _assert_equal(tail, angle[-65:], desc[-65:], name + " last 65")


def test_flat_image_gives_angle_zero_and_zero_rows(ctx):
    img = ac.case("flat")
    rec = mc.flat_records(img.shape)
    ctx.akaze_detect(img)
    got = ctx.akaze_describe(None, rec)
    assert len(rec) > 3 and not got["angle"].any() and not got["desc"].any() and got["angle"].tobytes() == np.zeros(len(rec), np.float32).tobytes()


def test_same_bytes_twice_in_one_context_and_in_a_fresh_one(sample_images):
    img = ac.image_case("full_size", sample_images)
    a = make_ctx()
    kp = a.akaze_detect(img)["kp"]
    first = a.akaze_describe(None, kp)
    second = a.akaze_describe(None, kp)
    a.close()
    b = make_ctx()
    kp_b = b.akaze_detect(img)["kp"]
    fresh = b.akaze_describe(None, kp_b)
    b.close()
    assert len(kp) > 500 and kp.tobytes() == kp_b.tobytes()
    for other in (second, fresh):
        assert other["angle"].tobytes() == first["angle"].tobytes() and other["desc"].tobytes() == first["desc"].tobytes()


def _raw_describe(c, img, shape, kp, angle, desc):
    ptr, stride = (None, 0) if img is None else (img.ctypes.data, img.strides[0])
    return c.lib.spvo_akaze_describe(c.h, ptr, shape[0], shape[1], stride, kp.ctypes.data, len(kp), angle.ctypes.data, desc.ctypes.data)


def test_statuses_leave_the_outputs_untouched(ctx):
    img = ac.case("two_exact")
    levels, derivs, kp = _levels(img, "two_exact")
    kp = kp[:8].copy()
    fresh = make_ctx()
    try:
        with pytest.raises(capi.SpvoError) as e:                                          # nothing resident
            fresh.akaze_describe(None, kp, shape=img.shape)
        assert e.value.code == -4
    finally:
        fresh.close()
    ctx.akaze_detect(img)
    good = ctx.akaze_describe(None, kp)
    angle, desc = np.full(8, 7.5, np.float32), np.full((8, 61), 0xA5, np.uint8)
    levels_n = len(levels)
    bad = []
    for field, value in (("class_id", levels_n), ("class_id", -1), ("octave", 7), ("octave", -1), ("x", np.nan), ("x", np.inf), ("y", -np.inf), ("y", np.nan), ("size", np.nan),
                         ("size", np.inf), ("size", 0.0), ("size", -3.0)):
        r = kp.copy()
        r[field][5] = value
        bad.append(r)
    r = kp.copy()
    r["class_id"][7], r["octave"][7] = 4, 0                                                # level 4 lies on octave 1
    bad.append(r)
    for r in bad:
        for image in (None, img):                                                         # checked before an image is uploaded, too
            assert _raw_describe(ctx, image, img.shape, r, angle, desc) == -1
            assert (angle == 7.5).all() and (desc == 0xA5).all()
    assert _raw_describe(ctx, None, img.shape, kp[:0], angle, desc) == 0 and (angle == 7.5).all() and (desc == 0xA5).all()       # n == 0
    assert _raw_describe(ctx, None, (img.shape[0], img.shape[1] + 1), kp, angle, desc) == -4 and (desc == 0xA5).all()            # another shape than the resident one
    after = ctx.akaze_describe(None, kp)                                                  # the refused calls left the resident result alone
    assert after["desc"].tobytes() == good["desc"].tobytes() and after["angle"].tobytes() == good["angle"].tobytes()
    for replace in (ctx.brisk_detect, ctx.sift_detect):                                   # another detector takes the resident image over
        ctx.akaze_detect(img)
        replace(img)
        assert _raw_describe(ctx, None, img.shape, kp, angle, desc) == -4 and (angle == 7.5).all() and (desc == 0xA5).all()
    _assert_equal(ctx.akaze_describe(img, kp), *mr.describe(levels, kp, derivs), "two_exact after the statuses")


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(3, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def test_a_submission_in_flight_refuses_the_call_and_touches_nothing(sequence, squeeze_weights_path):
    """SPVO_ERR_STATE while a spvo_detect_submit is in flight, with and without an image; outputs stay as they were, and after the collect
    the resident scale space answers as before"""
    frames, _, P_l, P_r = sequence
    img, other = ac.case("two_exact"), ac.case("one_octave")
    levels, derivs, kp = _levels(img, "two_exact")
    c = make_ctx(squeeze_weights_path)
    try:
        c.akaze_detect(img)
        before = c.akaze_describe(None, kp)
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)             # a SuperPoint submission in flight
        angle, desc = np.full(len(kp), 7.5, np.float32), np.full((len(kp), 61), 0xA5, np.uint8)
        for image, shape in ((None, img.shape), (img, img.shape), (other, other.shape)):
            assert _raw_describe(c, image, shape, kp, angle, desc) == -4
            assert (angle == 7.5).all() and (desc == 0xA5).all()
        c.detect_collect(P_l, P_r)
        assert c.akaze_level(5, 3).tobytes() == levels[5]["Ldet"].tobytes()
        after = c.akaze_describe(None, kp)
        assert len(kp) > 0 and after["desc"].tobytes() == before["desc"].tobytes() and after["angle"].tobytes() == before["angle"].tobytes()
        _assert_equal(after, *mr.describe(levels, kp, derivs), "two_exact after the collect")
    finally:
        c.close()


def test_akaze_akaze_front_end_pushes_aligned_features(sequence):
    """ClassicFeatureFrontEnd(AKAZE, AKAZE, BF, ...) with setAkazeDescriptor at the native resolution on the crop the AKAZE + BRISK test
    uses: two deque entries, keypoints and 61-byte rows one to one and as many as the restatement's detector finds (nothing erased); no
    error logged.  Without the switch the pair is refused, and the switch does not outlive the probe."""
    frames, _, P_l, P_r = sequence
    L, R = (np.ascontiguousarray(im[40:200, 300:700]) for im in frames[0])
    n, counts, err = host.classic_pair_probe("AKAZE", "AKAZE", L, R, P_l, P_r, akaze_descriptor=True)
    assert n == 2 and err == "", err
    assert counts[0] == counts[1] > 0 and counts[2] == counts[3] > 0 and counts[4] == 61
    for img, got in ((L, counts[0]), (R, counts[2])):
        assert got == len(ak.detect(img, tables=_tables(*img.shape)))
    n, counts, err = host.classic_pair_probe("AKAZE", "AKAZE", L, R, P_l, P_r)
    assert n == 0 and err != ""
    for detector in ("FAST", "BRISK", "ORB"):                                             # the AKAZE descriptor on other keypoints stays refused
        n, counts, err = host.classic_pair_probe(detector, "AKAZE", L, R, P_l, P_r, akaze_descriptor=True)
        assert n == 0 and err != ""


def test_classic_front_end_with_akaze_akaze_equals_the_oracle_state_machine(sequence):
    """classic_sequence(frames, detector="AKAZE", descriptor="AKAZE", akaze_descriptor=True, input_size=(120, 392)) (KNN) against
    oracle/odometry.py's FrontEndState fed the RESTATEMENT's keypoints (tests/akaze_ref.py on the oracle's preprocessed image, the
    library's tables), the library's rows for them (held to tests/akaze_mldb_ref.py's bit for bit, here again) and the Hamming oracle's
    maps: keypoint, stereo-match and inlier counts identical, poses within 1e-6.  The BRISK test's absolute bars -- more than 100
    keypoints, more than 20 inliers, translation within 0.1 of the synthetic motion -- are asserted because the all-CPU pipeline
    (restatements, oracle.matching, oracle.odometry) clears them on these frames at 120 x 392 (NOTES.md, "AKAZE descriptor";
    tests/test_akaze_mldb_ref_cpu.py asserts it).  With resident=True: the same digests through the per-image path, no pair resident."""
    frames, gt, P_l, P_r = sequence
    kw = dict(detector="AKAZE", descriptor="AKAZE", akaze_descriptor=True, input_size=(120, 392), trace=True)
    poses, stats, _, digests = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, **kw)
    ctx = make_ctx()
    st = od.FrontEndState()
    prev_dl = None
    for k, (L, R) in enumerate(frames):
        feats, Ps = [], []
        for img, P in ((L, P_l), (R, P_r)):
            small, Pk = ofe.preprocess(img, np.asarray(P, np.float64).reshape(3, 4), 120, 392)[:2]
            small = np.ascontiguousarray(small)
            levels, _ = ak.scale_space(small, _tables(*small.shape))
            kp = ak.detect(small, levels=levels)
            d = ctx.akaze_describe(small, kp)
            _assert_equal(d, *mr.describe(levels, kp), "frame %d" % k)
            feats.append((np.stack([kp["x"], kp["y"]], 1), d["desc"]))
            Ps.append(Pk)
        (xyl, dl), (xyr, dr) = feats
        od.add_features(st, xyl, dl, xyr, dr, Ps[0], Ps[1])
        idx0, _ = matching.bf_match_hamming(dl, dr, "KNN", False, 0.8)
        st.maps[od.PREV_LEFT_PREV_RIGHT] = st.maps[od.CURR_LEFT_CURR_RIGHT]
        st.maps[od.CURR_LEFT_CURR_RIGHT] = idx0
        print(k, "stats", stats[k].tolist(), "oracle", len(xyl), len(xyr), int((idx0 >= 0).sum()))
        assert stats[k, 0] == len(xyl) > 100 and stats[k, 1] == len(xyr) and stats[k, 2] == int((idx0 >= 0).sum())
        if k > 0:
            idx1, _ = matching.bf_match_hamming(dl, prev_dl, "KNN", False, 0.8)
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
    poses_r, stats_r, _, digests_r = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, resident=True, **kw)
    assert np.array_equal(digests_r, digests) and np.array_equal(stats_r, stats) and np.array_equal(poses_r, poses)
    assert host.classic_resident_pairs() == 0
    with pytest.raises(RuntimeError):                                                   # the switch is opt-in and was reset: the pair is refused again
        host.classic_sequence(frames[:1], P_l, P_r, "KNN", True, 2.0, 4, detector="AKAZE", descriptor="AKAZE")
