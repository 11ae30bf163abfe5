"""GPU parity of the ORB extractor on keypoints that carry an octave (csrc/orb.hip.h: orb_describe_given_kernel;
spvo_orb_describe_octaves) against the numpy restatement tests/orb_octaves_ref.py: the detector's own records on every octave, the two
keypoint sets of tests/orb_octaves_cases.py that reach into the levels' reflect zone (tests/test_orb_octaves_ref_cpu.py asserts that they
do), AKAZE records on the resident image, the refusals, and BRISK + ORB / AKAZE + ORB through the host class behind
setOrbExtractorOctaves."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import frontend as ofe, matching, odometry as od
from spvo import host, synth
from tests import brisk_detect_ref as bd, orb_octaves_cases as oc, orb_octaves_ref as oo
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(3, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def _strided(img):
    """the image as a view whose row stride exceeds its width"""
    big = np.full((img.shape[0], img.shape[1] + 16), 255, np.uint8)
    big[:, :img.shape[1]] = img
    view = big[:, :img.shape[1]]
    assert view.strides[0] > view.shape[1]
    return view


def _equals(got, ref):
    """kept equal, rows byte-equal, the direction within 1e-5 rad (it passes through atan2)"""
    assert np.array_equal(got["kept"], ref["kept"])
    bad = int((got["desc"] != ref["desc"]).any(1).sum())
    err = float(np.abs(got["angle"] - ref["angle"]).max()) if len(ref["kept"]) else 0.0
    print("   kept", len(ref["kept"]), "rows that differ", bad, "largest direction difference", err)
    assert bad == 0
    assert err <= 1e-5


def test_every_octave_of_the_detector_s_own_records(ctx, sample_images):
    """spvo_orb_detect's records, shuffled: all kept, grouped by octave, the 32 bytes and the direction's bits the detector's; restricted to
    octave 0 (integer coordinates) the call gives spvo_orb_describe's kept, rows and directions"""
    img = sample_images[0]
    r = ctx.orb(img)
    n = len(r["xy"])
    perm = np.random.default_rng(3).permutation(n)
    g = ctx.orb_describe_octaves(img, r["xy"][perm], r["octave"][perm])
    assert n > 1000 and set(r["octave"].tolist()) == set(range(8))
    assert np.array_equal(g["kept"], np.argsort(r["octave"][perm], kind="stable"))
    src = perm[g["kept"]]
    print("keypoints", n, "rows that differ", int((g["desc"] != r["desc"][src]).any(1).sum()), "directions that differ",
          int((g["angle"].view(np.uint32) != r["angle"][src].view(np.uint32)).sum()))
    assert np.array_equal(g["desc"], r["desc"][src])
    assert np.array_equal(g["angle"].view(np.uint32), r["angle"][src].view(np.uint32))
    xy0 = r["xy"][r["octave"] == 0][::-1].copy()
    a, b = ctx.orb_describe(img, xy0), ctx.orb_describe_octaves(img, xy0, 0)
    assert len(a["kept"]) == len(xy0) > 100
    assert np.array_equal(a["kept"], b["kept"]) and a["desc"].tobytes() == b["desc"].tobytes() and a["angle"].tobytes() == b["angle"].tobytes()


@pytest.mark.parametrize("order", ["given", "shuffled"])
@pytest.mark.parametrize("name", oc.SETS)
def test_bit_for_bit_against_the_restatement(ctx, sample_images, name, order):
    """both keypoint sets on the 160 x 400 crop, uploaded as a strided view, in the set's order and shuffled"""
    img, xy, octave = oc.keypoints(name, sample_images)
    if order == "given":
        ref = oc.reference(name, sample_images)
    else:
        perm = np.random.default_rng(5).permutation(len(xy))
        xy, octave = xy[perm], octave[perm]
        ref = oo.describe(img, xy, octave)
    print(name, order, "keypoints", len(xy), "in the reflect zone", int(ref["zone"].any(1).sum()), "reading outside", int(ref["outside"].any(1).sum()))
    assert ref["zone"].any()
    _equals(ctx.orb_describe_octaves(_strided(img), xy, octave), ref)


def test_akaze_records_on_the_resident_image(sample_images):
    """the AKAZE detector's keypoints, described on the image it left on the device (img = NULL): the restatement's answer, and the image is
    still there for a second call"""
    img = oc.crop(sample_images)
    c = make_ctx()
    try:
        kp = c.akaze_detect(img)["kp"]
        xy, octave = np.stack([kp["x"], kp["y"]], 1), kp["octave"]
        ref = oo.describe(img, xy, octave)
        print("AKAZE keypoints", len(kp), "octaves", np.bincount(octave).tolist(), "kept", len(ref["kept"]))
        assert len(ref["kept"]) > 50 and len(set(octave.tolist())) > 1
        a = c.orb_describe_octaves(None, xy, octave, shape=img.shape)
        _equals(a, ref)
        b = c.orb_describe_octaves(None, xy, octave, shape=img.shape)
        assert np.array_equal(a["kept"], b["kept"]) and a["desc"].tobytes() == b["desc"].tobytes() and a["angle"].tobytes() == b["angle"].tobytes()
    finally:
        c.close()


def _raw(c, img, shape, xy, octave, n=None):
    """the call on outputs filled with a sentinel -> (status, n_kept, the outputs are untouched)"""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    octave = np.ascontiguousarray(octave, np.int32)
    rows = max(len(xy), 1)
    kept, angle, desc = np.full(rows, -7, np.int32), np.full(rows, 7.5, np.float32), np.full((rows, 32), 0xA5, np.uint8)
    m = C.c_int(-7)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = c.lib.spvo_orb_describe_octaves(c.h, None if img is None else vp(img), shape[0], shape[1], 0 if img is None else img.strides[0], vp(xy), vp(octave),
                                         len(xy) if n is None else n, vp(kept), vp(angle), vp(desc), C.byref(m))
    return rc, m.value, bool((kept == -7).all() and (angle == 7.5).all() and (desc == 0xA5).all())


def test_refusals_touch_nothing(sample_images, sequence, squeeze_weights_path):
    img, xy, octave = oc.keypoints("handmade", sample_images)
    ref = oc.reference("handmade", sample_images)
    frames, _, P_l, P_r = sequence
    c = make_ctx(squeeze_weights_path)
    try:
        _equals(c.orb_describe_octaves(img, xy, octave), ref)                          # the crop is resident from here on
        small = np.ascontiguousarray(sample_images[0][:64, :96])
        one = np.array([[100, 80]], np.float32)
        INVALID, STATE = -1, -4
        for what, args, status in (("octave 8", (img, img.shape, one, [8]), INVALID), ("octave -1", (None, img.shape, one, [-1]), INVALID),
                                   ("NaN", (img, img.shape, np.array([[100, np.nan]], np.float32), [0]), INVALID),
                                   ("infinity", (None, img.shape, np.array([[np.inf, 80]], np.float32), [0]), INVALID),
                                   ("n < 0", (img, img.shape, one, [0], -1), INVALID),
                                   ("a level of 31 x 46", (small, small.shape, np.array([[40, 32]], np.float32), [4]), INVALID),
                                   ("no image of that shape", (None, (img.shape[0] - 1, img.shape[1]), one, [0]), STATE)):
            rc, m, untouched = _raw(c, *args)
            print(what, "->", rc, c.lib.spvo_last_error(c.h).decode())
            assert rc == status and m == -7 and untouched, what
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)                             # a SuperPoint submission in flight
        for image in (None, img):
            rc, m, untouched = _raw(c, image, img.shape, xy, octave)
            assert rc == STATE and m == -7 and untouched
        c.detect_collect(P_l, P_r)
        _equals(c.orb_describe_octaves(None, xy, octave, shape=img.shape), ref)       # the resident image survived every refusal
        rc, m, untouched = _raw(c, None, img.shape, np.zeros((0, 2), np.float32), np.zeros(0, np.int32))
        assert rc == 0 and m == 0 and untouched
        rc, m, _ = _raw(c, None, img.shape, np.array([[5, 5]], np.float32), [2])        # nothing survives the border rule
        assert rc == 0 and m == 0
    finally:
        c.close()


@pytest.mark.parametrize("detector", ["BRISK", "AKAZE"])
def test_front_end_pushes_aligned_features_behind_the_switch(sequence, detector):
    """ClassicFeatureFrontEnd(detector, ORB) on the crop with setOrbExtractorOctaves: two deque entries, keypoints and 32-byte rows one to
    one, no error; for BRISK as many as the restatement's detector and the border rule leave.  Without the switch the pair is refused."""
    frames, _, P_l, P_r = sequence
    L, R = (np.ascontiguousarray(im[40:200, 300:700]) for im in frames[0])
    n, counts, err = host.classic_pair_probe(detector, "ORB", L, R, P_l, P_r, orb_octaves=True)
    print(detector, "entries", n, "counts", counts.tolist(), err)
    assert n == 2 and err == "", err
    assert counts[0] == counts[1] > 0 and counts[2] == counts[3] > 0 and counts[4] == 32
    if detector == "BRISK":
        for img, got in ((L, counts[0]), (R, counts[2])):
            kp = bd.detect(img, 30)
            assert got == len(oo.border_keep(np.stack([kp["x"], kp["y"]], 1), img.shape))
    n, counts, err = host.classic_pair_probe(detector, "ORB", L, R, P_l, P_r)
    assert n == 0 and not counts.any() and "only these pairs run" in err and detector + " + ORB" not in err


def _fnv(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _digest_matches(idx, dist):
    """spvo_host_classic_sequence_trace's digest of a match list: (query, train, distance) of every matched row, then their number"""
    q = np.nonzero(idx >= 0)[0]
    rec = np.zeros(len(q), np.dtype([("q", "<i4"), ("t", "<i4"), ("d", "<f4")]))
    rec["q"], rec["t"], rec["d"] = q, idx[q], dist[q]
    return _fnv(_fnv(1469598103934665603, rec.tobytes()), np.uint64(len(q)).tobytes())


def _digest_ints(a, b):
    h = 1469598103934665603
    for v in (a, b):
        v = np.ascontiguousarray(v, "<i4")
        h = _fnv(h, np.uint64(len(v)).tobytes())
        h = _fnv(h, v.tobytes())
    return h


def test_classic_front_end_with_brisk_orb_equals_the_oracle_state_machine(sequence):
    """classic_sequence(frames[:2], detector="BRISK", descriptor="ORB", input_size=(120, 392), orb_octaves=True) (KNN) against
    oracle/odometry.py's FrontEndState fed the restatements' keypoints (tests/brisk_detect_ref.py on the oracle's preprocessed image) and
    rows (tests/orb_octaves_ref.py) and the Hamming oracle's maps, built as tests/test_gpu_brisk_detect.py builds its comparison: keypoint,
    stereo-match and inlier counts identical, the match lists and the inlier sets identical (the trace's digests of them, recomputed here
    from the oracle's), the pose within 1e-6 (that test's bound).  With resident=True: the same digests through the per-image path, and no
    pair counted as resident."""
    frames, gt, P_l, P_r = sequence
    frames = frames[:2]
    poses, stats, _, digests = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="BRISK", descriptor="ORB", input_size=(120, 392), orb_octaves=True, trace=True)
    st = od.FrontEndState()
    prev_dl = None
    for k, (L, R) in enumerate(frames):
        feats, Ps = [], []
        for img, P in ((L, P_l), (R, P_r)):
            small, Pk = ofe.preprocess(img, np.asarray(P, np.float64).reshape(3, 4), 120, 392)[:2]
            small = np.ascontiguousarray(small)
            kp = bd.detect(small, 30)
            xy = np.stack([kp["x"], kp["y"]], 1)
            d = oo.describe(small, xy, kp["octave"])
            feats.append((xy[d["kept"]], d["desc"]))
            Ps.append(Pk)
        (xyl, dl), (xyr, dr) = feats
        od.add_features(st, xyl, dl, xyr, dr, Ps[0], Ps[1])
        idx0, dist0 = matching.bf_match_hamming(dl, dr, "KNN", False, 0.8)
        st.maps[od.PREV_LEFT_PREV_RIGHT] = st.maps[od.CURR_LEFT_CURR_RIGHT]
        st.maps[od.CURR_LEFT_CURR_RIGHT] = idx0
        print(k, "stats", stats[k].tolist(), "oracle", len(xyl), len(xyr), int((idx0 >= 0).sum()), "stereo digest", int(digests[k, 4]), _digest_matches(idx0, dist0))
        assert stats[k, 0] == len(xyl) > 100 and stats[k, 1] == len(xyr) and stats[k, 2] == int((idx0 >= 0).sum())
        assert int(digests[k, 4]) == _digest_matches(idx0, dist0)
        if k > 0:
            idx1, dist1 = matching.bf_match_hamming(dl, prev_dl, "KNN", False, 0.8)
            st.maps[od.CURR_LEFT_PREV_LEFT] = idx1
            q, t, dbg = od.solve_stereo_odometry(st, 2.0, 2.0, 4)
            Rc, Rg = od.quat_to_rot(np.asarray(q)), od.quat_to_rot(poses[k, :4])
            print("   inliers", stats[k, 3], len(dbg["inliers"]), "pose difference R %.3g t %.3g" % (np.abs(Rg - Rc).max(), np.abs(poses[k, 4:] - t).max()),
                  "temporal digest", int(digests[k, 5]), _digest_matches(idx1, dist1), "inlier digest", int(digests[k, 7]), _digest_ints(st.inliers_pnp, st.inliers_postmatching))
            assert int(digests[k, 5]) == _digest_matches(idx1, dist1)
            assert stats[k, 3] == len(dbg["inliers"]) > 0
            assert int(digests[k, 7]) == _digest_ints(st.inliers_pnp, st.inliers_postmatching)
            assert np.abs(Rg - Rc).max() <= 1e-6 and np.abs(poses[k, 4:] - t).max() <= 1e-6
        prev_dl = dl
    poses_r, stats_r, _, digests_r = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="BRISK", descriptor="ORB", input_size=(120, 392), orb_octaves=True,
                                                           resident=True, trace=True)
    assert np.array_equal(digests_r, digests) and np.array_equal(stats_r, stats) and np.array_equal(poses_r, poses)
    assert host.classic_resident_pairs() == 0
    with pytest.raises(RuntimeError):                                                   # without the keyword: still not a pair that runs
        host.classic_sequence(frames[:1], P_l, P_r, "KNN", True, 2.0, 4, detector="BRISK")
