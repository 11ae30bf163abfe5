"""The classic front end with its features resident on the device (spvo_classic_detect, spvo_match_hamming_slots,
ClassicFeatureFrontEnd::setDeviceResident): everything equals the per-image entry points and spvo_match_hamming EXACTLY -- counts,
keypoint records, descriptor bytes, match indices and distances, and through the host class every deque entry, match list, inlier
set and pose.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import cpu_backend, matching
from spvo import capi, host, synth
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu

KINDS = ["ORB", "ShiTomasi", "FAST"]
MODES = [("NN", False), ("NN", True), ("KNN", False)]          # NN, NN with cross-check, KNN at 0.8


def per_image(ctx, img, kind):
    """what the existing entry points return for one image, as the keypoint records spvo_classic_detect promises"""
    if kind == "ORB":
        return ctx.orb(img)
    g = ctx.gftt(img) if kind == "ShiTomasi" else ctx.fast(img)
    d = ctx.orb_describe(None, g["xy"])
    k = d["kept"]
    return dict(xy=g["xy"][k], angle=d["angle"], response=g["response"][k], octave=np.zeros(len(k), np.int32), desc=d["desc"])


def assert_same_features(got, ref):
    assert len(got["xy"]) == len(ref["xy"])
    for f in ("xy", "angle", "response", "octave", "desc"):
        assert got[f].dtype == ref[f].dtype and np.array_equal(got[f], ref[f]), f


def assert_matches(ctx, sa, sb, fa, fb):
    """the three modes on slots sa -> sb against spvo_match_hamming on the host copies and against oracle/matching.py"""
    for sel, cross in MODES:
        gi, gd = ctx.match_hamming_slots(sa, sb, sel, cross, 0.8)
        hi, hd = ctx.match_hamming(fa["desc"], fb["desc"], sel, cross, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd), (sel, cross)
        oi, od_ = matching.bf_match_hamming(fa["desc"], fb["desc"], sel, cross, 0.8)
        assert np.array_equal(gi, oi), (sel, cross)
        assert np.array_equal(gd[gi >= 0], od_[oi >= 0]), (sel, cross)


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(12, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


@pytest.fixture()
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.mark.parametrize("kind", KINDS)
def test_detect_equals_the_per_image_entry_points(ctx, sample_images, sequence, kind):
    """the three golden images (as left / right of two pairs) and a synthetic stereo pair"""
    pairs = [(sample_images[0], sample_images[1]), (sample_images[2], sample_images[0]), sequence[0][0]]
    for k, (L, R) in enumerate(pairs):
        gl, gr = ctx.classic_detect(L, R, 2 * k, 2 * k + 1, kind)
        assert_same_features(gl, per_image(ctx, L, kind))
        assert_same_features(gr, per_image(ctx, R, kind))
        assert ctx.classic_slot_rows(2 * k) == len(gl["xy"]) > 100 and ctx.classic_slot_rows(2 * k + 1) == len(gr["xy"]) > 100


def test_orb_detect_equals_the_compiled_oracle(ctx, sample_images):
    cpu = cpu_backend.CpuBackend(net_height=64, net_width=96)
    try:
        gl, gr = ctx.classic_detect(sample_images[0], sample_images[1], 0, 1, "ORB")
        for g, img in ((gl, sample_images[0]), (gr, sample_images[1])):
            r = cpu.orb(img)
            assert len(g["xy"]) == len(r["xy"]) > 500
            assert np.array_equal(g["octave"], r["octave"]) and np.array_equal(g["response"], r["response"])
            assert np.array_equal(g["xy"], r["xy"]) and np.array_equal(g["desc"], r["desc"])
            d = np.abs(g["angle"] - r["angle"])
            assert np.minimum(d, 2 * np.pi - d).max() <= 1e-5          # (the angle's bound is tests/test_gpu_orb.py's)
    finally:
        cpu.close()


@pytest.mark.parametrize("kind", KINDS)
def test_edge_images_and_matching_on_them(ctx, sample_images, kind):
    """a constant image (0 keypoints, a filled empty slot), a 64 x 96 crop, a strided view; the matcher with an empty slot on either
    side and with row counts that are no multiple of a tile size"""
    flat = np.full((120, 160), 77, np.uint8)
    el, er = ctx.classic_detect(flat, flat, 0, 1, kind)
    assert len(el["xy"]) == 0 and len(er["xy"]) == 0 and ctx.classic_slot_rows(0) == 0 and ctx.classic_slot_rows(1) == 0
    crop_l, crop_r = sample_images[0][100:164, 300:396], sample_images[1][100:164, 300:396]       # 64 x 96, strided
    cl, cr = ctx.classic_detect(crop_l, crop_r, 2, 3, kind)
    assert_same_features(cl, per_image(ctx, crop_l, kind))
    assert_same_features(cr, per_image(ctx, crop_r, kind))
    view_l, view_r = sample_images[1][3:370, 5:1200], sample_images[2][3:370, 5:1200]             # rows are not contiguous
    vl, vr = ctx.classic_detect(view_l, view_r, 4, 5, kind)
    assert_same_features(vl, per_image(ctx, view_l, kind))
    assert_same_features(vr, per_image(ctx, view_r, kind))
    assert len(vl["xy"]) > 256 and len(vr["xy"]) > 256      # more than one 256-row tile of the matcher: its tile loop, the prefetch and the last partial tile all run
    assert_matches(ctx, 4, 5, vl, vr)
    assert_matches(ctx, 4, 0, vl, el)            # empty train set: every row -1
    assert_matches(ctx, 0, 4, el, vl)            # empty query set
    assert_matches(ctx, 0, 1, el, er)
    assert_matches(ctx, 2, 3, cl, cr)            # the crop's few rows (ORB border 31 of 64 x 96: possibly none)
    assert_matches(ctx, 5, 2, vr, cl)


def test_knn_with_a_one_row_train_set(ctx, sample_images):
    """a train slot of exactly one row: KNN has no second neighbour and keeps nothing, NN finds that row"""
    img = sample_images[0]
    one = np.full_like(img, 60)
    one[150:200, 400:460] = 200                                     # one bright rectangle: its corners
    gl, gr = ctx.classic_detect(img, one, 0, 1, "ShiTomasi", max_corners=1)
    assert len(gr["xy"]) == 1 and len(gl["xy"]) <= 1
    fl, fr = ctx.classic_detect(img, img, 2, 3, "ORB")
    # binary slots of different calls may be matched with each other
    assert_matches(ctx, 2, 1, fl, gr)
    idx, dist = ctx.match_hamming_slots(2, 1, "KNN", False, 0.8)
    assert np.all(idx == -1)
    idx, dist = ctx.match_hamming_slots(2, 1, "NN", False, 0.8)
    assert np.all(idx == 0)


def test_matching_large_slots(ctx, sample_images):
    """FAST on the KITTI sample: at least 4000 rows per slot"""
    fl, fr = ctx.classic_detect(sample_images[0], sample_images[1], 0, 1, "FAST")
    assert len(fl["xy"]) >= 4000 and len(fr["xy"]) >= 4000
    assert_same_features(fl, per_image(ctx, sample_images[0], "FAST"))
    assert_matches(ctx, 0, 1, fl, fr)
    assert_matches(ctx, 1, 0, fr, fl)
    # 1777 rows: no multiple of the matcher's 8 rows per wave, 16 per workgroup, 64 per tile step or 256 per tile
    ol, orr = ctx.classic_detect(sample_images[0], sample_images[1], 2, 3, "ORB", nfeatures=1777)
    assert len(ol["xy"]) == 1777 and len(orr["xy"]) > 256      # (image 0 fills every level's quota at 2000 features, so also at 1777)
    assert_same_features(ol, ctx.orb(sample_images[0], nfeatures=1777))
    assert_matches(ctx, 2, 3, ol, orr)
    assert_matches(ctx, 2, 0, ol, fl)


@pytest.mark.parametrize("mode", MODES)
def test_prematch_is_transparent(sample_images, sequence, mode):
    """results with spvo_set_prematch on and off are equal (stereo and temporal), and a slot rewritten between detect and match is
    not served from the stored result.  A binary slot can only be rewritten by spvo_classic_detect, which drops both stored results
    itself; so what this covers is that invalidation plus the result's equality with spvo_match_hamming -- the generation comparison
    in spvo_match_hamming_slots is MatchCache's second line of defence and is not what rejects the entry here."""
    sel, cross = mode
    frames = sequence[0]
    res = {}
    for on in (False, True):
        c = make_ctx()
        try:
            c.set_prematch(on, sel, cross, 0.8)
            out = []
            for k in range(3):
                fl, fr = c.classic_detect(frames[k][0], frames[k][1], 2 * k, 2 * k + 1, "ORB")
                out.append(c.match_hamming_slots(2 * k, 2 * k + 1, sel, cross, 0.8))
                if k:
                    out.append(c.match_hamming_slots(2 * k, 2 * k - 2, sel, cross, 0.8))
                    hi, hd = c.match_hamming(fl["desc"], prev["desc"], sel, cross, 0.8)
                    assert np.array_equal(out[-1][0], hi) and np.array_equal(out[-1][1], hd)
                prev = fl
            # rewrite the right slot of the last pair with another image's features: the stored stereo match is stale
            nl, nr = c.classic_detect(sample_images[2], sample_images[1], 8, 5, "ORB")
            gi, gd = c.match_hamming_slots(4, 5, sel, cross, 0.8)
            hi, hd = c.match_hamming(fl["desc"], nr["desc"], sel, cross, 0.8)
            assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
            assert not (np.array_equal(gi, out[-2][0]) and np.array_equal(gd, out[-2][1]))
            res[on] = out
        finally:
            c.close()
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_binary_and_sift_prematches_stay_independent(sample_images):
    """Binary slots 0 / 1 and SIFT slots 0 / 1 of one context hold a pair each, with their prematches stored: rewriting the SIFT slots or
    switching the fp8 shortlist (which drops the stored L2 matches only) leaves the stored Hamming match what it was, and every result
    equals a context's that stores nothing.  64 x 96 crops, slots of 256 rows; FAST + BRISK because the ORB extractor's 31-pixel border
    leaves next to nothing of such a crop (the CPU references find 77 / 75 rows and more in these crops)."""
    def crop(i, r, c):
        return np.ascontiguousarray(sample_images[i][r:r + 64, c:c + 96])

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    first, second = (crop(0, 150, 420), crop(1, 150, 420)), (crop(2, 150, 420), crop(0, 150, 500))
    on, off = make_ctx(), make_ctx()
    try:
        on.set_prematch(True, "KNN", False, 0.8)
        for c in (on, off):
            bl, _ = c.classic_detect(*first, 0, 1, "FAST+BRISK", slot_capacity=256)
            sl, _ = c.sift_detect_pair(*first, 0, 1, slot_capacity=256)
            assert len(bl["xy"]) > 20 and sl["n"] > 20
        ham = on.match_hamming_slots(0, 1, "KNN", False, 0.8)
        assert (ham[0] >= 0).any()
        assert same(ham, off.match_hamming_slots(0, 1, "KNN", False, 0.8))
        assert same(on.match_l2_slots(0, 1, "KNN", False, 0.8), off.match_l2_slots(0, 1, "KNN", False, 0.8))
        for c in (on, off):                                            # the SIFT slots of the same numbers hold another pair now
            c.sift_detect_pair(*second, 0, 1, slot_capacity=256)
        assert same(on.match_hamming_slots(0, 1, "KNN", False, 0.8), ham)
        on.set_match_fp8(True)
        on.set_match_fp8(False)
        assert same(on.match_hamming_slots(0, 1, "KNN", False, 0.8), ham)
        l2 = off.match_l2_slots(0, 1, "KNN", False, 0.8)
        assert (l2[0] >= 0).any() and same(on.match_l2_slots(0, 1, "KNN", False, 0.8), l2)
    finally:
        on.close()
        off.close()


def test_status_codes(sample_images, squeeze_weights_path, sequence):
    frames, _, P_l, P_r = sequence
    c = make_ctx(squeeze_weights_path)
    try:
        n_orb = len(c.orb(sample_images[0])["xy"])
        assert n_orb > 1000
        c.classic_detect(sample_images[0], sample_images[1], 0, 1, "ORB")
        with pytest.raises(capi.SpvoError) as e:                       # more rows than a slot holds: reported, nothing truncated
            c.classic_detect(sample_images[0], sample_images[1], 0, 1, "ORB", slot_capacity=n_orb - 1)
        assert e.value.code == -5 and e.value.counts[0] == n_orb
        for s in (0, 1):
            with pytest.raises(capi.SpvoError) as e:                   # ... and both slots are unfilled afterwards
                c.classic_slot_rows(s)
            assert e.value.code == -4
        with pytest.raises(capi.SpvoError) as e:
            c.match_hamming_slots(0, 1)
        assert e.value.code == -4
        with pytest.raises(capi.SpvoError) as e:                       # a slot nothing was ever written to
            c.match_hamming_slots(6, 7)
        assert e.value.code == -4
        for bad in ((0, 0), (-1, 1), (0, 10)):
            with pytest.raises(capi.SpvoError) as e:
                c.classic_detect(sample_images[0], sample_images[1], bad[0], bad[1], "ORB")
            assert e.value.code == -1
        with pytest.raises(capi.SpvoError) as e:                       # what spvo_gftt_detect refuses
            c.classic_detect(sample_images[0], sample_images[1], 0, 1, "ShiTomasi", block_size=3)
        assert e.value.code == -1
        gl, gr = c.classic_detect(sample_images[0], sample_images[1], 0, 1, "ORB")
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)             # a SuperPoint submission in flight
        with pytest.raises(capi.SpvoError) as e:
            c.classic_detect(sample_images[0], sample_images[1], 2, 3, "ORB")
        assert e.value.code == -4
        c.detect_collect(P_l, P_r)
        assert c.classic_slot_rows(0) == len(gl["xy"])                 # the refused call touched nothing
        c.classic_detect(sample_images[0], sample_images[1], 2, 3, "ORB")
    finally:
        c.close()


def _run(frames, P_l, P_r, detector, **kw):
    return host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector=detector, trace=True, **kw)


@pytest.mark.parametrize("detector", KINDS)
def test_host_class_is_identical_with_resident_features(sequence, detector):
    """ClassicFeatureFrontEnd over 12 synthetic frames with setDeviceResident on and off: keypoints_dq, descriptors_dq, the three match
    lists, the inlier sets (digests of their full contents) and every pose are identical"""
    frames, _, P_l, P_r = sequence
    p0, s0, _, d0 = _run(frames, P_l, P_r, detector)
    p1, s1, _, d1 = _run(frames, P_l, P_r, detector, resident=True)
    assert len(frames) >= 12 and s0[:, 0].min() > 100 and s0[1:, 3].max() > 10
    assert np.array_equal(d0, d1)
    assert np.array_equal(s0, s1)
    assert np.array_equal(p0, p1)


def test_host_class_falls_back_when_a_pair_does_not_fit(sequence):
    """FAST with slots too small for some pairs and large enough for others: those pairs take the per-image path and are matched from
    the host matrices, and the run is still identical"""
    frames, _, P_l, P_r = sequence
    p0, s0, _, d0 = _run(frames, P_l, P_r, "FAST")
    rows = np.sort(np.maximum(s0[:, 0], s0[:, 1]))
    cap = int(rows[len(rows) // 2])                                    # the median pair just fits, the larger half does not
    assert rows[0] <= cap < rows[-1]
    p1, s1, _, d1 = _run(frames, P_l, P_r, "FAST", resident=True, resident_capacity=cap)
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
    p2, s2, _, d2 = _run(frames, P_l, P_r, "FAST", resident=True, resident_capacity=16)   # no pair fits
    assert np.array_equal(d0, d2) and np.array_equal(p0, p2)
