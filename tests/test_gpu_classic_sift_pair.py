"""ShiTomasi / FAST + SIFT with the features resident on the device (spvo_classic_sift_pair, ClassicFeatureFrontEnd::setSiftDescribeResident):
everything equals the per-image entry points on the same context EXACTLY -- records and rows byte for byte against spvo_gftt_detect /
spvo_fast_detect followed by spvo_sift_describe(img = NULL), match indices and distances against spvo_match_l2 on the host copies, and
through the host class every digest, count and pose.  No tolerance anywhere.

The 120 x 392 image is tests/sift_describe_cases.py's image("fast") (= sift_cases.image("kitti"), the image of its FAST list); its right
partner is a copy rolled by nine columns, so the two sides differ in content and in count.  The 24 x 40 crop at (60, 200) gives 15 FAST
and 5 Shi-Tomasi keypoints in tests/classic_ref.py: fewer records than waves, and every patch of a size-7 keypoint (75 x 75 samples)
hangs over all four borders."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import capi, host, synth
from tests import sift_describe_cases as dc
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu

KINDS = ("ShiTomasi", "FAST")
SIZE = {"ShiTomasi": 5.0, "FAST": 7.0}
MODES = [("KNN", False), ("NN", True)]          # KNN at 0.8, NN with cross-check


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(3, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def large_pair():
    L = dc.image("fast")
    assert L.shape == (120, 392)
    return L, np.ascontiguousarray(np.roll(L, -9, axis=1))


def crop_pair():
    c = np.ascontiguousarray(dc.image("fast")[60:84, 200:240])
    return c, np.ascontiguousarray(c[:, ::-1])


def per_image(c, img, kind, fast_threshold=10):
    """the detector's call followed by spvo_sift_describe(img = NULL) on the records ClassicFeatureFrontEnd builds"""
    f = c.gftt(img) if kind == "ShiTomasi" else c.fast(img, threshold=fast_threshold)
    n = len(f["xy"])
    kp = np.zeros(n, capi.SIFT_KP_DTYPE)
    kp["x"], kp["y"], kp["size"], kp["angle"], kp["response"], kp["octave"] = f["xy"][:, 0], f["xy"][:, 1], SIZE[kind], -1.0, f["response"], 0
    return dict(kp=kp, desc=c.sift_describe(None, kp, shape=img.shape), n=n)


def same(got, ref):
    return (got["n"] == ref["n"] and np.array_equal(got["kp"].view(np.uint8), ref["kp"].view(np.uint8)) and
            np.array_equal(got["desc"].view(np.uint8).reshape(-1), ref["desc"].view(np.uint8).reshape(-1)))


def assert_matches(c, sa, sb, fa, fb):
    for sel, cross in MODES:
        gi, gd = c.match_l2_slots(sa, sb, sel, cross, 0.8)
        hi, hd = c.match_l2(fa["desc"], fb["desc"], sel, cross, 0.8, dim=128)
        assert np.array_equal(gi, hi) and gd.tobytes() == hd.tobytes(), (sa, sb, sel, cross)


def unfilled(c, slot):
    with pytest.raises(capi.SpvoError) as e:
        c.sift_slot_rows(slot)
    return e.value.code == -4


# ---------------------------------------------------------------- byte equality
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["large", "crop"])
def test_pair_equals_detector_then_describe(ctx, kind, which):
    L, R = large_pair() if which == "large" else crop_pair()
    thr = 10
    if kind == "FAST" and which == "crop":
        while thr > 1 and min(len(ctx.fast(L, threshold=thr)["xy"]), len(ctx.fast(R, threshold=thr)["xy"])) == 0:
            thr -= 1
    rl, rr = per_image(ctx, L, kind, thr), per_image(ctx, R, kind, thr)
    print(kind, which, "rows", rl["n"], rr["n"], "FAST threshold", thr)
    assert rl["n"] > 0 and rr["n"] > 0
    if which == "crop":
        assert rl["n"] < 64                                         # a handful: far fewer than the waves launched
    else:
        assert rl["n"] > 64 and not same(rl, rr)                     # the two sides are different lists
    gl, gr = ctx.classic_sift_pair(L, R, 0, 1, kind=kind, fast_threshold=thr)
    assert same(gl, rl) and same(gr, rr)
    assert ctx.sift_slot_rows(0) == rl["n"] and ctx.sift_slot_rows(1) == rr["n"]
    assert (gl["kp"]["size"] == SIZE[kind]).all() and (gl["kp"]["angle"] == -1).all() and (gl["kp"]["octave"] == 0).all()
    # host buffers smaller than n: the first `cap` rows, the count is still the full one
    cap = rl["n"] // 2
    pl, pr = ctx.classic_sift_pair(L, R, 4, 9, kind=kind, fast_threshold=thr, cap=cap)
    assert pl["n"] == rl["n"] and pl["kp"].tobytes() == rl["kp"][:cap].tobytes() and pl["desc"].tobytes() == rl["desc"][:cap].tobytes()
    assert pr["n"] == rr["n"] and pr["desc"].tobytes() == rr["desc"][:cap].tobytes()
    assert ctx.sift_slot_rows(4) == rl["n"] and ctx.sift_slot_rows(9) == rr["n"]


@pytest.mark.parametrize("kind", KINDS)
def test_zero_keypoints(ctx, kind):
    flat = np.full((16, 16), 93, np.uint8)
    gl, gr = ctx.classic_sift_pair(flat, flat.copy(), 2, 3, kind=kind)
    assert gl["n"] == 0 and gr["n"] == 0 and len(gl["kp"]) == 0 and gl["desc"].shape == (0, 128)
    assert ctx.sift_slot_rows(2) == 0 and ctx.sift_slot_rows(3) == 0
    for sel, cross in MODES:
        idx, dist = ctx.match_l2_slots(2, 3, sel, cross, 0.8)
        assert len(idx) == 0 and len(dist) == 0
    L, R = crop_pair()
    fl, _ = ctx.classic_sift_pair(L, R, 0, 1, kind=kind)
    assert fl["n"] > 0
    assert_matches(ctx, 0, 2, fl, gl)                               # empty train slot: every row -1
    assert_matches(ctx, 2, 0, gl, fl)                               # empty query slot


@pytest.mark.parametrize("kind", KINDS)
def test_capacity(kind):
    L, R = large_pair()
    c = make_ctx()
    try:
        rl, rr = per_image(c, L, kind), per_image(c, R, kind)
        with pytest.raises(capi.SpvoError) as e:
            c.classic_sift_pair(L, R, 0, 1, kind=kind, slot_capacity=rl["n"] - 1)
        assert e.value.code == -5 and e.value.counts == (rl["n"], rr["n"])
        assert unfilled(c, 0) and unfilled(c, 1)
        with pytest.raises(capi.SpvoError) as e:
            c.match_l2_slots(0, 1)
        assert e.value.code == -4
        gl, gr = c.classic_sift_pair(L, R, 0, 1, kind=kind)           # the default capacity
        assert same(gl, rl) and same(gr, rr)
        with pytest.raises(capi.SpvoError) as e:                      # the limit is the call's own, not the largest seen
            c.classic_sift_pair(L, R, 0, 1, kind=kind, slot_capacity=rl["n"] - 1)
        assert e.value.code == -5 and unfilled(c, 0) and unfilled(c, 1)
    finally:
        c.close()


# ---------------------------------------------------------------- matching
@pytest.mark.parametrize("kind", KINDS)
def test_match_l2_slots(ctx, kind):
    L, R = large_pair()
    fl, fr = ctx.classic_sift_pair(L, R, 0, 1, kind=kind)
    assert_matches(ctx, 0, 1, fl, fr)
    assert_matches(ctx, 1, 0, fr, fl)
    idx, _ = ctx.match_l2_slots(0, 1, "KNN", False, 0.8)
    assert (idx >= 0).sum() > 10


@pytest.mark.parametrize("mode", MODES)
def test_prematch_is_transparent(mode):
    """three pairs with spvo_set_prematch on: the stereo match and the temporal match against the previous call's left slot equal
    spvo_match_l2 on the host copies; then a left slot that spvo_sift_detect_pair filled is the temporal partner"""
    sel, cross = mode
    L, R = large_pair()
    pairs = [(L, R), (R, L), (np.ascontiguousarray(L[::-1]), np.ascontiguousarray(R[::-1]))]
    res = {}
    for on in (False, True):
        c = make_ctx()
        try:
            c.set_prematch(on, sel, cross, 0.8)
            out, prev = [], None
            for k, (a, b) in enumerate(pairs):
                fl, fr = c.classic_sift_pair(a, b, 2 * k, 2 * k + 1, kind="FAST", slot_capacity=2048)
                out.append(c.match_l2_slots(2 * k, 2 * k + 1, sel, cross, 0.8))
                hi, hd = c.match_l2(fl["desc"], fr["desc"], sel, cross, 0.8, dim=128)
                assert np.array_equal(out[-1][0], hi) and out[-1][1].tobytes() == hd.tobytes()
                if k:
                    out.append(c.match_l2_slots(2 * k, 2 * k - 2, sel, cross, 0.8))
                    hi, hd = c.match_l2(fl["desc"], prev["desc"], sel, cross, 0.8, dim=128)
                    assert np.array_equal(out[-1][0], hi) and out[-1][1].tobytes() == hd.tobytes()
                prev = fl
            assert (out[0][0] >= 0).sum() > 10
            sl, _ = c.sift_detect_pair(L, R, 6, 7, slot_capacity=2048)          # SIFT + SIFT rows in the same ring
            gl, gr = c.classic_sift_pair(R, L, 8, 9, kind="ShiTomasi", slot_capacity=2048)
            assert sl["n"] > 0 and gl["n"] > 0
            out.append(c.match_l2_slots(8, 6, sel, cross, 0.8))
            hi, hd = c.match_l2(gl["desc"], sl["desc"], sel, cross, 0.8, dim=128)
            assert np.array_equal(out[-1][0], hi) and out[-1][1].tobytes() == hd.tobytes()
            out.append(c.match_l2_slots(8, 9, sel, cross, 0.8))
            hi, hd = c.match_l2(gl["desc"], gr["desc"], sel, cross, 0.8, dim=128)
            assert np.array_equal(out[-1][0], hi) and out[-1][1].tobytes() == hd.tobytes()
            res[on] = out
        finally:
            c.close()
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------- determinism, state, refusals
@pytest.mark.parametrize("kind", KINDS)
def test_determinism_and_state(ctx, kind):
    L, R = large_pair()
    a = ctx.classic_sift_pair(L, R, 0, 1, kind=kind)
    b = ctx.classic_sift_pair(L, R, 2, 3, kind=kind)
    assert same(a[0], b[0]) and same(a[1], b[1])
    with pytest.raises(capi.SpvoError) as e:                          # no SIFT pyramid is resident
        ctx.sift_level(0, 0)
    assert e.value.code == -4
    again = ctx.sift_describe(None, a[1]["kp"], shape=R.shape)         # the resident u8 image is the RIGHT one
    assert again.tobytes() == a[1]["desc"].tobytes()
    assert ctx.sift_level(0, 0).shape == R.shape                      # ... and spvo_sift_describe's pyramid takes the place over


def raw_pair(c, kind, L, R, slot_l, slot_r, slot_capacity=None):
    """the status of spvo_classic_sift_pair and what it left in the two feature structs' n (77 going in)"""
    o = capi.ClassicOpts()
    c.lib.spvo_default_classic_opts(C.byref(o), kind)
    if slot_capacity is not None:
        o.slot_capacity = slot_capacity
    kp = np.full(4, 7.5, np.float32).repeat(6).view(capi.SIFT_KP_DTYPE)
    desc = np.full((4, 128), 7.5, np.float32)
    fl, fr = capi.SiftFeatures(77, kp.ctypes.data, desc.ctypes.data, 4), capi.SiftFeatures(77, kp.ctypes.data, desc.ctypes.data, 4)
    rc = c.lib.spvo_classic_sift_pair(c.h, C.byref(o), L.ctypes.data, R.ctypes.data, L.shape[0], L.shape[1], L.strides[0], slot_l, slot_r, C.byref(fl), C.byref(fr))
    return rc, fl.n, fr.n, bool((desc == 7.5).all() and (kp.view(np.float32) == 7.5).all())


def test_refusals_touch_nothing(squeeze_weights_path, sequence):
    frames, _, P_l, P_r = sequence
    L, R = large_pair()
    c = make_ctx(squeeze_weights_path)
    try:
        fl, fr = c.classic_sift_pair(L, R, 0, 1, kind="FAST")
        for kind in (5, 6):                                           # the binary-slot call refuses the float kinds and names the other call
            with pytest.raises(capi.SpvoError) as e:
                c.classic_detect(L, R, 0, 1, kind=kind)
            assert e.value.code == -1 and "spvo_classic_sift_pair" in str(e.value)
        refused = [raw_pair(c, kind, L, R, 0, 1) for kind in range(5)]
        refused += [raw_pair(c, 6, L, R, 0, 0), raw_pair(c, 6, L, R, 0, 10), raw_pair(c, 6, L, R, -1, 1), raw_pair(c, 5, L, R, 0, 1, slot_capacity=0),
                    raw_pair(c, 6, L, R, 0, 1, slot_capacity=32769)]
        small = np.zeros((5, 40), np.uint8)
        refused += [raw_pair(c, 5, small, small, 0, 1), raw_pair(c, 6, small, small, 0, 1)]      # what the detector / spvo_sift_describe refuse of the shape
        for r in refused:
            assert r == (-1, 77, 77, True), r
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)             # a SuperPoint submission in flight
        assert raw_pair(c, 6, L, R, 0, 1) == (-4, 77, 77, True)
        c.detect_collect(P_l, P_r)
        assert c.sift_slot_rows(0) == fl["n"] and c.sift_slot_rows(1) == fr["n"]      # outputs and slots are as they were
        assert_matches(c, 0, 1, fl, fr)
        gl, gr = c.classic_sift_pair(L, R, 0, 1, kind="FAST")
        assert same(gl, fl) and same(gr, fr)
    finally:
        c.close()


# ---------------------------------------------------------------- the host class
def _run(frames, P_l, P_r, detector, **kw):
    return host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector=detector, descriptor="SIFT", input_size=(120, 392), trace=True, **kw)


@pytest.mark.parametrize("detector", KINDS)
def test_host_class_is_identical_with_resident_features(sequence, detector):
    """keypoints_dq, descriptors_dq, the match lists, the inlier sets (digests of their full contents), counts and poses of three frames:
    the per-image run, the run with setDeviceResident alone (which takes the per-image path) and the run with the opt-in as well"""
    frames, _, P_l, P_r = sequence
    frames = frames[:3]
    p0, s0, _, d0 = _run(frames, P_l, P_r, detector)
    assert host.classic_resident_pairs() == 0
    p1, s1, _, d1 = _run(frames, P_l, P_r, detector, resident=True)
    assert host.classic_resident_pairs() == 0
    p2, s2, _, d2 = _run(frames, P_l, P_r, detector, resident=True, sift_describe_resident=True)
    assert host.classic_resident_pairs() == 3
    print(detector, "keypoints", s0[:, 0].tolist(), s0[:, 1].tolist(), "inliers", s0[:, 3].tolist())
    assert s0[:, 0].min() > 50
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
    assert np.array_equal(d0, d2) and np.array_equal(s0, s2) and np.array_equal(p0, p2)
    p3, s3, _, d3 = _run(frames, P_l, P_r, detector, sift_describe_resident=True)       # the opt-in alone does nothing
    assert host.classic_resident_pairs() == 0 and np.array_equal(d0, d3)


def test_host_class_with_slots_that_hold_the_median_pair(sequence):
    """FAST + SIFT with slots of the median pair's rows: the larger pairs take the per-image path and are matched from the host matrices,
    the others stay resident, and the run is still identical"""
    frames, _, P_l, P_r = sequence
    frames = frames[:3]
    p0, s0, _, d0 = _run(frames, P_l, P_r, "FAST")
    most = np.maximum(s0[:, 0], s0[:, 1])
    print("rows per pair", most.tolist())
    assert len(set(most.tolist())) > 1
    cap = int(np.sort(most)[1])
    p1, s1, _, d1 = _run(frames, P_l, P_r, "FAST", resident=True, sift_describe_resident=True, resident_capacity=cap)
    print("resident pairs", host.classic_resident_pairs(), "of 3 at capacity", cap)
    assert 0 < host.classic_resident_pairs() < 3
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
