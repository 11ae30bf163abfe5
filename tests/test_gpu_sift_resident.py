"""SIFT with its features resident on the device (spvo_sift_detect_pair, spvo_match_l2_slots, spvo_sift_order_debug,
ClassicFeatureFrontEnd::setDeviceResident with SIFT): everything equals the per-image entry points on the same context EXACTLY --
keypoint records and descriptors byte for byte, match indices and distances, and through the host class every deque entry, match
list, inlier set and pose.  The ordering stage alone is compared with tests/sift_ref.py: sort_unique on records with planted ties and
duplicates (the natural inputs contain no duplicate at all: raw = kept rows are 21 / 8 / 287 for noise / strided / kitti).  No tolerance
anywhere."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import frontend as ofe, matching
from spvo import capi, host, synth
from tests import sift_cases as sc, sift_ref as sr
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu

MODES = [("NN", False), ("NN", True), ("KNN", False)]          # NN, NN with cross-check, KNN at 0.8
FIELDS = ("x", "y", "size", "angle", "response", "octave")


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(4, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def small(img, P=None):
    return ofe.preprocess(img, np.eye(3, 4) if P is None else np.asarray(P, np.float64).reshape(3, 4), 120, 392)[0]


def pair(name):
    """(left, right) of one shape and one row stride; left is tests/sift_cases.py's image of that name"""
    g = sc._golden_images()
    if name == "kitti":
        return sc.image("kitti"), small(g[0])
    if name == "strided":
        return sc.image("strided"), g[2][3:104, 5:152]
    if name == "noise":
        return sc.image("noise"), np.random.RandomState(2).randint(0, 256, (64, 96)).astype(np.uint8)
    if name == "flat":
        return sc.image("flat"), np.full((64, 64), 31, np.uint8)
    if name == "tiny":
        rs = np.random.RandomState(3)
        return rs.randint(0, 256, (6, 6)).astype(np.uint8), rs.randint(0, 256, (6, 6)).astype(np.uint8)
    raise KeyError(name)


def same(got, ref):
    return got["n"] == ref["n"] and got["kp"].tobytes() == ref["kp"].tobytes() and got["desc"].tobytes() == ref["desc"].tobytes()


def assert_matches(ctx, sa, sb, fa, fb):
    """the three modes on SIFT slots sa -> sb against spvo_match_l2 on the host copies and against oracle/matching.py: bf_match"""
    for sel, cross in MODES:
        gi, gd = ctx.match_l2_slots(sa, sb, sel, cross, 0.8)
        hi, hd = ctx.match_l2(fa["desc"], fb["desc"], sel, cross, 0.8, dim=128)
        assert np.array_equal(gi, hi) and gd.tobytes() == hd.tobytes(), (sel, cross)
        oi, od_ = matching.bf_match(fa["desc"].reshape(-1, 128), fb["desc"].reshape(-1, 128), sel, cross, 0.8)
        assert np.array_equal(gi, oi), (sel, cross)
        assert np.array_equal(gd[gi >= 0], od_[oi >= 0]), (sel, cross)


# ---------------------------------------------------------------- the ordering stage alone
def planted_records(n, seed):
    """n records: half from small pools of values (ties in every prefix of the key), half random, and planted on top: exact duplicates,
    rows equal in (x, y, size, angle) that differ in response or in octave, rows equal in x, y that differ only in angle, -0.0 against 0.0
    in x and in angle, and (n >= 3000) a run of 1200 identical rows, more than one scan chunk of 1024"""
    rs = np.random.RandomState(seed)
    rec = np.zeros(n, sr.KP_DTYPE)
    pool = rs.rand(n) < 0.5
    rec["x"] = np.where(pool, rs.randint(0, 40, n) * 0.5, rs.rand(n) * 20).astype(np.float32)
    rec["y"] = np.where(pool, rs.randint(0, 4, n) * 1.25, rs.rand(n) * 20).astype(np.float32)
    rec["size"] = np.where(pool, rs.randint(1, 3, n) * 1.6, rs.rand(n) * 8 + 1).astype(np.float32)
    rec["angle"] = np.where(pool, rs.randint(0, 3, n) * 90.0, rs.rand(n) * 360).astype(np.float32)
    rec["response"] = np.where(pool, rs.randint(1, 3, n) * 0.03125, rs.rand(n)).astype(np.float32)
    rec["octave"] = rs.randint(0, 3, n) + (rs.randint(1, 4, n) << 8)
    if n >= 2:
        rec[1] = rec[0]                                               # an exact duplicate
    if n >= 16:
        rec[3] = rec[2]; rec["response"][3] = rec["response"][2] * 2  # equal in (x, y, size, angle): the smaller response stays
        rec[5] = rec[4]; rec["octave"][4] = rec["octave"][5] + 1      # ... the smaller octave stays (the LATER row here)
        rec[7] = rec[6]; rec["angle"][7] = rec["angle"][6] + 10       # equal in x, y, size: both stay
        rec[9] = rec[8]; rec["x"][8] = 0.0; rec["x"][9] = -0.0        # -0.0 = 0.0: a duplicate
        rec[11] = rec[10]; rec["angle"][10] = -0.0; rec["angle"][11] = 0.0
        rec[13] = rec[12]; rec["x"][12] = -0.0; rec["x"][13] = 0.0; rec["response"][12] = rec["response"][13] * 2   # the +0.0 row sorts first
        rec[n - 1] = rec[14]                                          # duplicates far apart in raw order
    if n >= 3000:
        rec[1500:2700] = rec[15]
        rec[2800] = rec[15]; rec["octave"][2800] = rec["octave"][15] - 1   # ... and the row that sorts in front of the whole run
    return rec


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1025, 3000])
def test_ordering_stage_equals_sort_unique(ctx, n):
    rec = planted_records(n, seed=n)
    ref = sr.sort_unique(rec)
    got = ctx.sift_order(rec)
    print(n, "records", len(ref), "stay")
    assert len(got) == len(ref) and got.dtype == np.int32
    if n >= 16:
        assert len(ref) < n - 6
    if n >= 3000:
        assert len(ref) < n - 1200
    assert len(set(got.tolist())) == len(got) and (len(got) == 0 or (got.min() >= 0 and got.max() < n))
    # rows equal in all six fields may stand for each other: the RECORDS the indices point to are compared (== on floats: -0.0 = 0.0)
    for f in FIELDS:
        assert np.array_equal(rec[got][f], rec[ref][f]), f


# ---------------------------------------------------------------- detection
@pytest.mark.parametrize("name", ["kitti", "strided", "noise", "flat", "tiny"])
def test_detect_pair_equals_detect(ctx, name):
    L, R = pair(name)
    if name == "strided":
        assert L.strides[0] > L.shape[1] and L.strides == R.strides
    rl, rr = ctx.sift_detect(L), ctx.sift_detect(R)
    gl, gr = ctx.sift_detect_pair(L, R, 0, 1)
    print(name, "rows", gl["n"], gr["n"])
    assert same(gl, rl) and same(gr, rr)
    assert ctx.sift_slot_rows(0) == rl["n"] and ctx.sift_slot_rows(1) == rr["n"]
    if name == "flat":
        assert gl["n"] == 0 and gr["n"] == 0                       # filled, empty slots
    if name in sc.NAMES:
        assert gl["n"] > 5
    # host buffers smaller than n: the first `cap` rows; other slots: the same bytes
    cap = max(rl["n"] // 2, 0)
    pl, pr = ctx.sift_detect_pair(L, R, 4, 9, cap=cap)
    assert pl["n"] == rl["n"] and len(pl["kp"]) == min(cap, rl["n"]) and pl["kp"].tobytes() == rl["kp"][:cap].tobytes() and pl["desc"].tobytes() == rl["desc"][:cap].tobytes()
    assert pr["n"] == rr["n"] and pr["kp"].tobytes() == rr["kp"][:cap].tobytes() and pr["desc"].tobytes() == rr["desc"][:cap].tobytes()
    assert ctx.sift_slot_rows(4) == rl["n"] and ctx.sift_slot_rows(9) == rr["n"]
    al, ar = ctx.sift_detect_pair(R, L, 7, 2)                       # the sides exchanged
    assert same(al, rr) and same(ar, rl)
    assert same(ctx.sift_detect(L), rl)                             # ... and the per-image path is what it was


# ---------------------------------------------------------------- matching
def one_row_image():
    """a rotated elliptical blob on a flat 40 x 48 image: one extremum with one orientation peak (one row in the restatement, too)"""
    y, x = np.mgrid[0:40, 0:48].astype(np.float64)
    xr = (x - 23.6) * np.cos(0.5) + (y - 19.3) * np.sin(0.5)
    yr = -(x - 23.6) * np.sin(0.5) + (y - 19.3) * np.cos(0.5)
    return np.clip(np.rint(60 + 120 * np.exp(-0.5 * ((xr / 3.4) ** 2 + (yr / 2.2) ** 2))), 0, 255).astype(np.uint8)


def test_match_l2_slots(ctx):
    L, R = pair("kitti")
    fl, fr = ctx.sift_detect_pair(L, R, 0, 1)
    assert fl["n"] > 256 and fr["n"] > 256                          # more than one 64-row query tile and one 128-row train tile of the matcher
    assert_matches(ctx, 0, 1, fl, fr)
    assert_matches(ctx, 1, 0, fr, fl)
    el, er = ctx.sift_detect_pair(*pair("flat"), 2, 3)
    assert el["n"] == 0 and er["n"] == 0
    assert_matches(ctx, 0, 2, fl, el)                               # empty train slot: every row -1
    assert_matches(ctx, 2, 0, el, fl)                               # empty query slot
    assert_matches(ctx, 2, 3, el, er)
    noise = np.random.RandomState(5).randint(0, 256, (40, 48)).astype(np.uint8)
    nl, one = ctx.sift_detect_pair(noise, one_row_image(), 4, 5)
    assert one["n"] == 1 and nl["n"] > 1
    assert_matches(ctx, 0, 5, fl, one)                              # slots of different calls; a train slot of exactly one row
    idx, _ = ctx.match_l2_slots(0, 5, "KNN", False, 0.8)
    assert np.all(idx == -1)                                        # KNN has no second neighbour and keeps nothing
    idx, _ = ctx.match_l2_slots(0, 5, "NN", False, 0.8)
    assert np.all(idx == 0)
    assert_matches(ctx, 5, 0, one, fl)
    assert_matches(ctx, 4, 1, nl, fr)


def test_full_size_pair_and_its_prematch(sample_images):
    """the full-size golden pair (375 x 1242): more than 1024 rows per slot (more than one rank tile and scan chunk of the ordering, more than 1024 train columns in
    the matcher); with spvo_set_prematch the KNN match is the one enqueued with the detector, for full slots of 8192 rows"""
    c = make_ctx()
    try:
        c.set_prematch(True, "KNN", False, 0.8)
        L, R = sample_images[0], sample_images[1]
        assert L.shape == R.shape == (375, 1242)                  # the golden images at their full size
        fl, fr = c.sift_detect_pair(L, R, 0, 1)
        print("full size rows", fl["n"], fr["n"])
        assert fl["n"] > 1024 and fr["n"] > 1024
        assert same(fl, c.sift_detect(L)) and same(fr, c.sift_detect(R))
        assert_matches(c, 0, 1, fl, fr)
        assert_matches(c, 1, 0, fr, fl)
    finally:
        c.close()


@pytest.mark.parametrize("mode", MODES)
def test_prematch_is_transparent(sequence, mode):
    """three frames with spvo_set_prematch off and on: the stereo and the temporal matches are equal, and equal spvo_match_l2; a slot
    rewritten between detect and match is not served from the stored result"""
    sel, cross = mode
    frames, _, P_l, _ = sequence
    imgs = [(small(l, P_l), small(r, P_l)) for l, r in frames[:3]]
    other = small(sc._golden_images()[1])
    res = {}
    for on in (False, True):
        c = make_ctx()
        try:
            c.set_prematch(on, sel, cross, 0.8)
            out = []
            for k in range(3):
                fl, fr = c.sift_detect_pair(imgs[k][0], imgs[k][1], 2 * k, 2 * k + 1, slot_capacity=2048)
                out.append(c.match_l2_slots(2 * k, 2 * k + 1, sel, cross, 0.8))
                hi, hd = c.match_l2(fl["desc"], fr["desc"], sel, cross, 0.8, dim=128)
                assert np.array_equal(out[-1][0], hi) and out[-1][1].tobytes() == hd.tobytes()
                if k:
                    out.append(c.match_l2_slots(2 * k, 2 * k - 2, sel, cross, 0.8))
                    hi, hd = c.match_l2(fl["desc"], prev["desc"], sel, cross, 0.8, dim=128)
                    assert np.array_equal(out[-1][0], hi) and out[-1][1].tobytes() == hd.tobytes()
                prev = fl
            assert (out[0][0] >= 0).sum() > 20
            # rewrite the right slot of the last pair with another image's features: the stored stereo match is stale
            nl, nr = c.sift_detect_pair(other, other, 8, 5, slot_capacity=2048)
            gi, gd = c.match_l2_slots(4, 5, sel, cross, 0.8)
            hi, hd = c.match_l2(fl["desc"], nr["desc"], sel, cross, 0.8, dim=128)
            assert np.array_equal(gi, hi) and gd.tobytes() == hd.tobytes()
            assert not (np.array_equal(gi, out[-2][0]) and np.array_equal(gd, out[-2][1]))
            res[on] = out
        finally:
            c.close()
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def test_status_codes(squeeze_weights_path, sequence):
    frames, _, P_l, P_r = sequence
    L, R = pair("kitti")
    c = make_ctx(squeeze_weights_path)
    try:
        n, n_r = c.sift_detect(L)["n"], c.sift_detect(R)["n"]
        assert n > 100
        with pytest.raises(capi.SpvoError) as e:                       # more rows than a slot holds: reported, nothing truncated
            c.sift_detect_pair(L, R, 0, 1, slot_capacity=min(n, n_r) - 1)   # (the context's first call: the slots keep the largest capacity seen)
        assert e.value.code == -5 and e.value.counts == (n, n_r)
        for s in (0, 1):
            with pytest.raises(capi.SpvoError) as e:                   # ... and both slots are unfilled afterwards
                c.sift_slot_rows(s)
            assert e.value.code == -4
        with pytest.raises(capi.SpvoError) as e:
            c.match_l2_slots(0, 1)
        assert e.value.code == -4
        with pytest.raises(capi.SpvoError) as e:                       # a slot nothing was ever written to
            c.match_l2_slots(6, 7)
        assert e.value.code == -4
        for bad in ((0, 0), (-1, 1), (0, 10)):
            with pytest.raises(capi.SpvoError) as e:
                c.sift_detect_pair(L, R, bad[0], bad[1])
            assert e.value.code == -1
        for cap in (0, 32769):
            with pytest.raises(capi.SpvoError) as e:
                c.sift_detect_pair(L, R, 0, 1, slot_capacity=cap, cap=16)
            assert e.value.code == -1
        with pytest.raises(capi.SpvoError) as e:                       # what spvo_sift_detect refuses
            c.sift_detect_pair(np.zeros((5, 8), np.uint8), np.zeros((5, 8), np.uint8), 0, 1)
        assert e.value.code == -1
        gl, gr = c.sift_detect_pair(L, R, 0, 1)
        assert gl["n"] == n
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)             # a SuperPoint submission in flight
        with pytest.raises(capi.SpvoError) as e:
            c.sift_detect_pair(L, R, 0, 1)
        assert e.value.code == -4
        c.detect_collect(P_l, P_r)
        assert c.sift_slot_rows(0) == n and c.sift_slot_rows(1) == n_r      # the refused call touched nothing
        i0, d0 = c.match_l2_slots(0, 1)
        i1, d1 = c.match_l2(gl["desc"], gr["desc"], dim=128)
        assert np.array_equal(i0, i1) and d0.tobytes() == d1.tobytes()
        c.sift_detect_pair(L, R, 2, 3)
    finally:
        c.close()


# ---------------------------------------------------------------- the host class
def _run(frames, P_l, P_r, **kw):
    return host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="SIFT", input_size=(120, 392), trace=True, **kw)


def test_host_class_is_identical_with_resident_features(sequence):
    """ClassicFeatureFrontEnd with SIFT over four frames, setDeviceResident off and on: keypoints_dq, descriptors_dq, the three match lists,
    the inlier sets (digests of their full contents) and every pose are identical; with slots that hold the median pair the larger pairs
    take the per-image path and are matched from the host matrices, and the run is still identical"""
    frames, _, P_l, P_r = sequence
    frames = frames[:4]
    p0, s0, _, d0 = _run(frames, P_l, P_r)
    p1, s1, _, d1 = _run(frames, P_l, P_r, resident=True)
    assert s0[:, 0].min() > 100 and s0[1:, 3].max() > 10
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
    rows = np.sort(np.maximum(s0[:, 0], s0[:, 1]))
    cap = int(rows[len(rows) // 2])                                    # the median pair just fits, a larger one does not
    assert rows[0] <= cap < rows[-1]
    p2, s2, _, d2 = _run(frames, P_l, P_r, resident=True, resident_capacity=cap)
    assert np.array_equal(d0, d2) and np.array_equal(s0, s2) and np.array_equal(p0, p2)
