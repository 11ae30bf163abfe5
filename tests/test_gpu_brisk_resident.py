"""ShiTomasi + BRISK and FAST + BRISK with their features resident on the device (the two BRISK kinds of spvo_classic_detect, the
64-byte instantiation of the slot matcher, ClassicFeatureFrontEnd::setDeviceResident): everything equals the per-image entry points
(spvo_gftt_detect / spvo_fast_detect + spvo_brisk_describe) and spvo_match_hamming EXACTLY -- counts, keypoint records, descriptor
bytes, match indices and distances, and through the host class every deque entry, match list, inlier set and pose.  No tolerance."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import matching
from spvo import capi, host, synth
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu

KINDS = ["ShiTomasi+BRISK", "FAST+BRISK"]
MODES = [("NN", False), ("NN", True), ("KNN", False)]          # NN, NN with cross-check, KNN at 0.8
SIZE = {"ShiTomasi+BRISK": 5.0, "FAST+BRISK": 7.0}             # the keypoint size detectKeypoints assigns


def detector(ctx, img, kind):
    return ctx.gftt(img) if kind.startswith("ShiTomasi") else ctx.fast(img)


def per_image(ctx, img, kind):
    """what the per-image entry points return for one image, as the keypoint records spvo_classic_detect promises; also the detector's count"""
    g = detector(ctx, img, kind)
    d = ctx.brisk_describe(None, g["xy"], SIZE[kind])
    k = d["kept"]
    return dict(xy=g["xy"][k], angle=d["angle"], response=g["response"][k], octave=np.zeros(len(k), np.int32), desc=d["desc"]), len(g["xy"])


def assert_same_features(got, ref):
    assert len(got["xy"]) == len(ref["xy"])
    assert got["desc"].shape[1] == 64
    for f in ("xy", "angle", "response", "octave", "desc"):
        assert got[f].dtype == ref[f].dtype and got[f].tobytes() == ref[f].tobytes(), f


def match_all(ctx, sa, sb, da, db):
    """the three modes on slots sa -> sb: equal to spvo_match_hamming on the same arrays and to oracle/matching.py; -> {mode: (idx, dist)}"""
    out = {}
    for sel, cross in MODES:
        gi, gd = ctx.match_hamming_slots(sa, sb, sel, cross, 0.8)
        hi, hd = ctx.match_hamming(da, db, sel, cross, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd), (sel, cross)
        oi, od_ = matching.bf_match_hamming(da, db, sel, cross, 0.8)
        assert np.array_equal(gi, oi), (sel, cross)
        assert np.array_equal(gd[gi >= 0], od_[oi >= 0]), (sel, cross)
        out[(sel, cross)] = (gi, gd)
    return out


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(12, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


@pytest.fixture()
def ctx():
    c = make_ctx()
    yield c
    c.close()


# ---------------------------------------------------------------- 1. byte equality with the per-image entry points
@pytest.mark.parametrize("kind", KINDS)
def test_detect_equals_the_per_image_entry_points(ctx, sample_images, kind):
    """a 64 x 96 strided crop (a handful of rows; the BRISK border removes most), a strided view whose rows are not contiguous, one full
    golden pair, a constant image (zero rows, a filled empty slot)"""
    crop_l, crop_r = sample_images[0][100:164, 300:396], sample_images[1][100:164, 300:396]
    cl, cr = ctx.classic_detect(crop_l, crop_r, 0, 1, kind)
    for got, img in ((cl, crop_l), (cr, crop_r)):
        ref, n_det = per_image(ctx, img, kind)
        assert_same_features(got, ref)
        print(kind, "crop: detector", n_det, "kept", len(got["xy"]))
        assert 0 < len(got["xy"]) < n_det          # the border rule dropped at least one keypoint and kept at least one
    view_l, view_r = sample_images[1][3:370, 5:1200], sample_images[2][3:370, 5:1200]
    vl, vr = ctx.classic_detect(view_l, view_r, 2, 3, kind)
    assert_same_features(vl, per_image(ctx, view_l, kind)[0])
    assert_same_features(vr, per_image(ctx, view_r, kind)[0])
    fl, fr = ctx.classic_detect(sample_images[0], sample_images[1], 4, 5, kind)
    assert_same_features(fl, per_image(ctx, sample_images[0], kind)[0])
    assert_same_features(fr, per_image(ctx, sample_images[1], kind)[0])
    assert ctx.classic_slot_rows(4) == len(fl["xy"]) > 100 and ctx.classic_slot_rows(5) == len(fr["xy"]) > 100
    assert np.all((fl["angle"] >= 0) & (fl["angle"] <= 360)) and fl["angle"].max() > 7      # degrees, not radians
    flat = np.full((120, 160), 77, np.uint8)
    el, er = ctx.classic_detect(flat, flat, 6, 7, kind)
    assert len(el["xy"]) == 0 and len(er["xy"]) == 0 and ctx.classic_slot_rows(6) == 0 and ctx.classic_slot_rows(7) == 0
    assert el["desc"].shape == (0, 64)
    assert ctx.classic_slot_rows(4) == len(fl["xy"])             # the other slots keep what they hold


# ---------------------------------------------------------------- 2. the matcher on planted rows
def sparse_rows(rng, n):
    """rows of 64 bytes with about one bit in eight set: two unrelated rows are about 112 bits apart"""
    return np.packbits(rng.random((n, 512)) < 0.125, axis=1)


def flipped(rng, row, k):
    out = row.copy()
    for bit in rng.choice(512, k, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def planted(nq, nt, seed):
    """query rows, and train rows that are query rows with a few bits flipped (even train indices) between unrelated rows, with
         train[1] == train[0] (both one bit from query 0): a tie, the lowest index wins; KNN has d0 == d1 and rejects query 0
         query 3 = query 1 with three more bits flipped and no train row of its own: queries 1 and 3 both choose train 2, which chooses 1
         the last query all ones: ~448 bits from every train row, nearer to none of them than the sparse queries: no train row votes for it"""
    rng = np.random.default_rng(seed)
    q, t = sparse_rows(rng, nq), sparse_rows(rng, nt)
    n_rel = min(nq - 1, nt // 2)
    for i in range(n_rel):
        t[2 * i] = flipped(rng, q[i], 1 + i % 5)
    t[1] = t[0]
    q[3] = flipped(rng, q[1], 3)
    t[6] = sparse_rows(rng, 1)[0]
    q[nq - 1] = 0xFF
    return q, t


@pytest.mark.parametrize("shape", [(7, 300), (70, 513), (300, 255)])
def test_matcher_on_planted_rows(ctx, shape):
    """the issue's shapes: 7, 70, 513 and 255 are no multiple of the 8 query rows of a workgroup or of the 256 rows of a tile (300 is a
    multiple of 4 only); 513 train rows are two full tiles and one row, 255 one row short of a tile"""
    nq, nt = shape
    q, t = planted(nq, nt, seed=nq * 1000 + nt)
    ctx.classic_slot_fill(0, q)
    ctx.classic_slot_fill(1, t)
    assert ctx.classic_slot_rows(0) == nq and ctx.classic_slot_rows(1) == nt
    res = match_all(ctx, 0, 1, q, t)
    nn, _ = res[("NN", False)]
    cross, _ = res[("NN", True)]
    knn, kd = res[("KNN", False)]
    assert np.all(nn >= 0)                                       # (plain NN cannot reject while there is a train row)
    assert (cross >= 0).any() and (cross < 0).any()              # every other mode both keeps and rejects
    assert (knn >= 0).any() and (knn < 0).any()
    assert nn[0] == 0 and res[("NN", False)][1][0] == 1.0        # the tie train[0] == train[1]: the lowest index
    assert knn[0] == -1 and kd[0] == 1.0                         # ... and d0 == d1 fails the ratio test
    assert knn[2] == 4 and kd[2] == 3.0                          # a related row: kept, at its number of flipped bits
    assert nn[1] == 2 and nn[3] == 2                             # two query rows choose train row 2 ...
    assert cross[1] == 2 and cross[3] != 2                       # ... which chooses query 1
    assert cross[nq - 1] == -1 and nn[nq - 1] >= 0               # nobody votes for the all-ones row
    match_all(ctx, 1, 0, t, q)                                   # and the other way round


def test_matcher_small_shapes_and_distance_512(ctx):
    rng = np.random.default_rng(5)
    five = sparse_rows(rng, 5)
    five[2] = 0xFF
    none = np.zeros((0, 64), np.uint8)
    zero = np.zeros((1, 64), np.uint8)
    ones = np.full((1, 64), 0xFF, np.uint8)
    # 1 x 1: all ones against all zeros -- distance 512, the top bit of the matcher's 32-bit key
    ctx.classic_slot_fill(0, ones)
    ctx.classic_slot_fill(1, zero)
    res = match_all(ctx, 0, 1, ones, zero)
    assert res[("NN", False)][0][0] == 0 and res[("NN", False)][1][0] == 512.0
    assert res[("NN", True)][0][0] == 0 and res[("NN", True)][1][0] == 512.0
    assert res[("KNN", False)][0][0] == -1 and res[("KNN", False)][1][0] == 512.0
    # 5 x 1: KNN has no second neighbour and keeps nothing, NN finds the row everywhere; row 2 is 512 bits away
    ctx.classic_slot_fill(0, five)
    res = match_all(ctx, 0, 1, five, zero)
    assert np.all(res[("NN", False)][0] == 0) and np.all(res[("KNN", False)][0] == -1)
    assert res[("NN", False)][1][2] == 512.0 and res[("KNN", False)][1][2] == 512.0
    assert np.count_nonzero(res[("NN", True)][0] == 0) == 1      # the one train row chooses one query row
    # 5 x 0 and 0 x 5
    ctx.classic_slot_fill(1, none)
    assert ctx.classic_slot_rows(1) == 0
    res = match_all(ctx, 0, 1, five, none)
    assert all(np.all(i == -1) and len(i) == 5 for i, _ in res.values())
    res = match_all(ctx, 1, 0, none, five)
    assert all(len(i) == 0 for i, _ in res.values())


def test_slots_of_two_widths_are_not_matched(ctx):
    rng = np.random.default_rng(6)
    wide, narrow = sparse_rows(rng, 9), sparse_rows(rng, 9)[:, :32].copy()
    ctx.classic_slot_fill(0, wide)
    ctx.classic_slot_fill(1, narrow)
    for a, b in ((0, 1), (1, 0)):
        with pytest.raises(capi.SpvoError) as e:
            ctx.match_hamming_slots(a, b, "NN", False, 0.8)
        assert e.value.code == -1 and "32" in str(e.value) and "64" in str(e.value)
    with pytest.raises(capi.SpvoError) as e:
        ctx.classic_slot_fill(2, np.zeros((3, 48), np.uint8))
    assert e.value.code == -1
    # the context is usable afterwards, at either width
    ctx.classic_slot_fill(2, wide[::-1].copy())
    match_all(ctx, 0, 2, wide, wide[::-1].copy())
    ctx.classic_slot_fill(3, narrow[::-1].copy())
    match_all(ctx, 1, 3, narrow, narrow[::-1].copy())


# ---------------------------------------------------------------- 3. the matcher on image features
def test_matching_image_features(ctx, sample_images):
    """a 200 x 400 part of a golden pair: more than one 256-row tile a side, few enough rows for the O(n^2) oracle to take a second (the
    full pair is test_detect_equals_the_per_image_entry_points's)"""
    fl, fr = ctx.classic_detect(sample_images[0][100:300, 300:700], sample_images[1][100:300, 300:700], 0, 1, "FAST+BRISK")
    assert len(fl["xy"]) > 256 and len(fr["xy"]) > 256
    match_all(ctx, 0, 1, fl["desc"], fr["desc"])
    match_all(ctx, 1, 0, fr["desc"], fl["desc"])
    flat = np.full((120, 160), 77, np.uint8)
    el, er = ctx.classic_detect(flat, flat, 2, 3, "FAST+BRISK")
    res = match_all(ctx, 0, 2, fl["desc"], el["desc"])           # empty train set: every row -1
    assert all(np.all(i == -1) for i, _ in res.values())
    match_all(ctx, 2, 0, el["desc"], fl["desc"])                 # empty query set
    match_all(ctx, 2, 3, el["desc"], er["desc"])


# ---------------------------------------------------------------- 4. prematch
@pytest.mark.parametrize("mode", MODES)
def test_prematch_is_transparent(sample_images, sequence, mode):
    """results with spvo_set_prematch on and off are equal (stereo and temporal), and a slot rewritten between detect and match is not
    served from the stored result (test_gpu_classic_resident.py's test, on the BRISK kinds: ShiTomasi for two modes, FAST for one)"""
    sel, cross = mode
    kind = "FAST+BRISK" if mode == MODES[1] else "ShiTomasi+BRISK"
    frames = sequence[0]
    res = {}
    for on in (False, True):
        c = make_ctx()
        try:
            c.set_prematch(on, sel, cross, 0.8)
            out = []
            for k in range(3):
                fl, fr = c.classic_detect(frames[k][0], frames[k][1], 2 * k, 2 * k + 1, kind)
                out.append(c.match_hamming_slots(2 * k, 2 * k + 1, sel, cross, 0.8))
                hi, hd = c.match_hamming(fl["desc"], fr["desc"], sel, cross, 0.8)
                assert np.array_equal(out[-1][0], hi) and np.array_equal(out[-1][1], hd)
                if k:
                    out.append(c.match_hamming_slots(2 * k, 2 * k - 2, sel, cross, 0.8))
                    hi, hd = c.match_hamming(fl["desc"], prev["desc"], sel, cross, 0.8)
                    assert np.array_equal(out[-1][0], hi) and np.array_equal(out[-1][1], hd)
                prev = fl
            # rewrite the right slot of the last pair with another image's features: the stored stereo match is stale
            nl, nr = c.classic_detect(sample_images[2], sample_images[1], 8, 5, kind)
            gi, gd = c.match_hamming_slots(4, 5, sel, cross, 0.8)
            hi, hd = c.match_hamming(fl["desc"], nr["desc"], sel, cross, 0.8)
            assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
            assert not (np.array_equal(gi, out[-2][0]) and np.array_equal(gd, out[-2][1]))
            # ... and so is it after the test hook rewrote a slot
            zl, _ = c.classic_detect(frames[0][0], frames[0][1], 0, 1, kind)
            c.classic_slot_fill(1, nr["desc"])
            gi, gd = c.match_hamming_slots(0, 1, sel, cross, 0.8)
            hi, hd = c.match_hamming(zl["desc"], nr["desc"], sel, cross, 0.8)
            assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
            res[on] = out
        finally:
            c.close()
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_prematch_across_a_change_of_row_width(sequence):
    """an ORB-kind call, then a BRISK-kind call with prematch on: the temporal partner has 32-byte rows and is skipped, not an error; the
    stereo match is the stored one and correct"""
    frames = sequence[0]
    c = make_ctx()
    try:
        c.set_prematch(True, "KNN", False, 0.8)
        ol, orr = c.classic_detect(frames[0][0], frames[0][1], 0, 1, "FAST")
        bl, br = c.classic_detect(frames[1][0], frames[1][1], 2, 3, "FAST+BRISK")
        gi, gd = c.match_hamming_slots(2, 3, "KNN", False, 0.8)
        hi, hd = c.match_hamming(bl["desc"], br["desc"], "KNN", False, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd) and (gi >= 0).sum() > 10
        with pytest.raises(capi.SpvoError) as e:                 # asked for explicitly, the temporal match names the widths
            c.match_hamming_slots(2, 0, "KNN", False, 0.8)
        assert e.value.code == -1
        gi, gd = c.match_hamming_slots(0, 1, "KNN", False, 0.8)  # the ORB rows are still there
        hi, hd = c.match_hamming(ol["desc"], orr["desc"], "KNN", False, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
        c.classic_detect(frames[2][0], frames[2][1], 4, 5, "FAST+BRISK")      # and the next BRISK call has a temporal partner again
        ti, td = c.match_hamming_slots(4, 2, "KNN", False, 0.8)
        assert len(ti) == c.classic_slot_rows(4) and (ti >= 0).sum() > 10
    finally:
        c.close()


# ---------------------------------------------------------------- 5. status codes
def test_status_codes(sample_images, squeeze_weights_path, sequence):
    frames, _, P_l, P_r = sequence
    c = make_ctx(squeeze_weights_path)
    try:
        ol, orr = c.classic_detect(sample_images[0], sample_images[1], 6, 7, "ORB")          # kinds 0 .. 2 before any BRISK call
        gl0, _ = c.classic_detect(sample_images[0], sample_images[1], 8, 9, "ShiTomasi")
        fl, fr = c.classic_detect(sample_images[0], sample_images[1], 0, 1, "FAST+BRISK")
        n_l, n_r = len(fl["xy"]), len(fr["xy"])
        assert n_l > 1000
        # the ORB rows survived the BRISK kind's first call (every slot was allocated for 64-byte rows from the start)
        assert c.classic_slot_rows(6) == len(ol["xy"]) and c.classic_slot_rows(7) == len(orr["xy"])
        gi, gd = c.match_hamming_slots(6, 7, "NN", True, 0.8)
        hi, hd = c.match_hamming(ol["desc"], orr["desc"], "NN", True, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
        with pytest.raises(capi.SpvoError) as e:                       # more rows than a slot holds: reported, nothing truncated
            c.classic_detect(sample_images[0], sample_images[1], 0, 1, "FAST+BRISK", slot_capacity=max(n_l, n_r) - 1)
        assert e.value.code == -5 and e.value.counts == (n_l, n_r)
        for s in (0, 1):
            with pytest.raises(capi.SpvoError) as e:                   # ... and both slots are unfilled afterwards
                c.classic_slot_rows(s)
            assert e.value.code == -4
        with pytest.raises(capi.SpvoError) as e:
            c.match_hamming_slots(0, 1)
        assert e.value.code == -4
        big = np.zeros((2902, 2902), np.uint8)                         # 2902 * 2902 * 255 >= 2^31: the int32 integral image
        for kind in KINDS:
            with pytest.raises(capi.SpvoError) as e:
                c.classic_detect(big, big, 0, 1, kind)
            assert e.value.code == -1
            for bad in ((0, 0), (-1, 1), (0, 10)):
                with pytest.raises(capi.SpvoError) as e:
                    c.classic_detect(sample_images[0], sample_images[1], bad[0], bad[1], kind)
                assert e.value.code == -1
        with pytest.raises(capi.SpvoError) as e:                       # what spvo_gftt_detect refuses
            c.classic_detect(sample_images[0], sample_images[1], 0, 1, "ShiTomasi+BRISK", block_size=3)
        assert e.value.code == -1
        with pytest.raises(capi.SpvoError) as e:                       # what spvo_fast_detect refuses
            c.classic_detect(sample_images[0], sample_images[1], 0, 1, "FAST+BRISK", fast_threshold=256)
        assert e.value.code == -1
        bl, br = c.classic_detect(sample_images[0], sample_images[1], 0, 1, "ShiTomasi+BRISK")
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)             # a SuperPoint submission in flight
        with pytest.raises(capi.SpvoError) as e:
            c.classic_detect(sample_images[0], sample_images[1], 2, 3, "FAST+BRISK")
        assert e.value.code == -4
        with pytest.raises(capi.SpvoError) as e:
            c.classic_slot_fill(0, bl["desc"])
        assert e.value.code == -4
        c.detect_collect(P_l, P_r)
        assert c.classic_slot_rows(0) == len(bl["xy"]) and c.classic_slot_rows(6) == len(ol["xy"])      # the refused calls touched nothing
        # kinds 0 .. 2 after the BRISK calls return what they returned before
        ol2, orr2 = c.classic_detect(sample_images[0], sample_images[1], 2, 3, "ORB")
        gl2, _ = c.classic_detect(sample_images[0], sample_images[1], 4, 5, "ShiTomasi")
        for a, b in ((ol, ol2), (orr, orr2), (gl0, gl2)):
            assert a["desc"].shape[1] == 32
            for f in ("xy", "angle", "response", "octave", "desc"):
                assert a[f].tobytes() == b[f].tobytes(), f
    finally:
        c.close()


# ---------------------------------------------------------------- 6. the host class
def _run(frames, P_l, P_r, detector, **kw):
    return host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector=detector, descriptor="BRISK", trace=True, **kw)


@pytest.fixture(scope="module")
def per_image_runs(sequence):
    """the run with setDeviceResident off, once per detector, shared and left unchanged"""
    frames, _, P_l, P_r = sequence
    out = {}
    for det in ("ShiTomasi", "FAST"):
        out[det] = _run(frames, P_l, P_r, det)
        assert host.classic_resident_pairs() == 0
    return out


@pytest.mark.parametrize("det", ["ShiTomasi", "FAST"])
def test_host_class_is_identical_with_resident_features(sequence, per_image_runs, det):
    """ClassicFeatureFrontEnd over 12 synthetic frames with setDeviceResident on and off: keypoints_dq, descriptors_dq, the three match
    lists, the inlier sets (digests of their full contents) and every pose are identical, and every pair stayed resident"""
    frames, _, P_l, P_r = sequence
    p0, s0, _, d0 = per_image_runs[det]
    p1, s1, _, d1 = _run(frames, P_l, P_r, det, resident=True)
    assert host.classic_resident_pairs() == 12 == len(frames)
    assert s0[:, 0].min() > 100 and s0[1:, 3].max() > 10
    assert np.array_equal(d0, d1)
    assert np.array_equal(s0, s1)
    assert np.array_equal(p0, p1)


def test_host_class_falls_back_when_a_pair_does_not_fit(sequence, per_image_runs):
    """FAST + BRISK with slots that hold the median pair's rows: the larger pairs take the per-image path and are matched from the host
    matrices, the others stay resident, and the run is still identical"""
    frames, _, P_l, P_r = sequence
    p0, s0, _, d0 = per_image_runs["FAST"]
    rows = np.sort(np.maximum(s0[:, 0], s0[:, 1]))
    cap = int(rows[len(rows) // 2])
    assert rows[0] <= cap < rows[-1]
    p1, s1, _, d1 = _run(frames, P_l, P_r, "FAST", resident=True, resident_capacity=cap)
    assert 0 < host.classic_resident_pairs() < 12
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
