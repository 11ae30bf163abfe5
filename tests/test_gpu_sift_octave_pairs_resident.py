"""BRISK + SIFT and AKAZE + SIFT with a stereo pair's features resident on the device (spvo_brisk_sift_pair, spvo_akaze_sift_pair into the
SIFT slots, ClassicFeatureFrontEnd::setSiftOctavePairsResident): everything equals the per-image route on the same device EXACTLY --
spvo_brisk_detect / spvo_akaze_detect followed by spvo_sift_describe(img = NULL) on the detector's records, and spvo_match_l2 on the host
copies -- counts, the 24- / 28-byte keypoint records and the 128-float rows as raw bytes, match indices and distances, and through the
host class every deque entry, match list, inlier set and pose.  The link alone (spvo_sift_link_debug: compaction by keep flags, the
reduced pyramid, the describe launch with the count read on the device) is held to spvo_sift_describe on lists no image gives.  That
per-image route is held to the numpy restatements by tests/test_gpu_brisk_detect.py, tests/test_gpu_akaze.py and
tests/test_gpu_sift_describe.py; what the inputs cover is pinned by tests/test_sift_octave_pairs_resident_cpu.py.  No tolerance, no row
excused."""
import ctypes as C

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import capi, host
from tests import sift_describe_cases as dc
from tests.conftest import make_ctx
from tests.test_gpu_classic_trace_golden import load_sequence
from tests.test_octave_pairs_resident_cpu import stereo_pairs
from tests.test_sift_octave_pairs_resident_cpu import sift_records

pytestmark = pytest.mark.gpu

MODES = [("NN", False), ("NN", True), ("KNN", False)]          # NN, NN with cross-check, KNN at 0.8
KINDS = ["brisk_sift", "akaze_sift"]
PAIRS = ["crop", "strided", "full_size"]
DTYPE = dict(brisk_sift=capi.BRISK_KP_DTYPE, akaze_sift=capi.AKAZE_KP_DTYPE)


def pair(name, sample_images):
    if name == "full_size":
        return np.ascontiguousarray(sample_images[0]), np.ascontiguousarray(sample_images[1])
    return stereo_pairs(sample_images)[name]


def same_shape_pairs(sample_images):
    """two pairs of one shape: the crop, and the strided views cut to its 160 rows"""
    return [pair("crop", sample_images), tuple(np.ascontiguousarray(im[:160]) for im in pair("strided", sample_images))]


def call(ctx, kind, L, R, sl, sr, **kw):
    return getattr(ctx, kind + "_pair")(L, R, sl, sr, **kw)


def per_image(ctx, kind, img):
    """the per-image route of one image: the detector's records, unchanged, and spvo_sift_describe(img = NULL) on them (AKAZE: without class_id)"""
    det = ctx.brisk_detect(img) if kind == "brisk_sift" else ctx.akaze_detect(img)
    kp = det["kp"]
    assert len(kp) == det["n"]
    return dict(kp=kp.copy(), desc=ctx.sift_describe(None, sift_records(kp), shape=img.shape), n=len(kp))


def assert_same(got, ref, kind):
    dtype = DTYPE[kind]
    assert got["n"] == ref["n"] == len(got["kp"]) == len(got["desc"])
    assert got["kp"].dtype == dtype and dtype.itemsize == (24 if kind == "brisk_sift" else 28) and got["desc"].shape == (ref["n"], 128) and got["desc"].dtype == np.float32
    if got["kp"].tobytes() != ref["kp"].tobytes():
        for f in dtype.names:
            bad = np.nonzero(got["kp"][f].view(np.uint32) != ref["kp"][f].view(np.uint32))[0]
            if len(bad):
                print("  field", f, ":", len(bad), "rows differ, first", int(bad[0]), got["kp"][bad[0]], ref["kp"][bad[0]])
    assert got["kp"].tobytes() == ref["kp"].tobytes()
    assert got["desc"].tobytes() == ref["desc"].tobytes(), "%d rows differ" % int((got["desc"] != ref["desc"]).any(1).sum())


def assert_match(c, sa, sb, da, db, sel, cross):
    """slots sa -> sb equal spvo_match_l2 on the host copies, index for index and distance for distance"""
    gi, gd = c.match_l2_slots(sa, sb, sel, cross, 0.8)
    hi, hd = c.match_l2(da, db, sel, cross, 0.8, dim=128)
    assert np.array_equal(gi, hi) and gd.tobytes() == hd.tobytes() and len(gi) == len(da), (sa, sb, sel, cross)
    return gi, gd


def match_all(c, sa, sb, da, db):
    return {m: assert_match(c, sa, sb, da, db, *m) for m in MODES}


def unfilled(c, slot):
    with pytest.raises(capi.SpvoError) as e:
        c.sift_slot_rows(slot)
    return e.value.code == -4


@pytest.fixture()
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference(sample_images):
    """the per-image route of every pair and kind, computed once in a context of its own and left unchanged: (kind, name) -> (left, right)"""
    c = make_ctx()
    out = {}
    for kind in KINDS:
        for name in PAIRS:
            L, R = pair(name, sample_images)
            out[kind, name] = (per_image(c, kind, L), per_image(c, kind, R))
    c.close()
    return out


# ---------------------------------------------------------------- 1. the link alone against spvo_sift_describe
def hook_lists():
    img = dc.image("brisk_style")
    assert img.shape == (64, 96)
    kp = dc.keypoints("brisk_style").astype(capi.SIFT_KP_DTYPE)
    shuffled = kp[np.random.default_rng(11).permutation(len(kp))]
    third = np.ones(len(kp), np.uint8)
    third[::3] = 0
    outside = np.zeros(6, capi.SIFT_KP_DTYPE)                       # far enough that no sample of a patch has four neighbours in its level
    outside["x"] = [-500, 700, 48, 48, -1e6, 3e9]
    outside["y"] = [32, 32, -400, 500, 1e6, 3e9]
    outside["size"], outside["angle"], outside["octave"] = [7, 7, 12, 24, 7, 7], -1, [0, 0, 1, 2, 0, 5]
    return img, {"brisk_style": (kp, None), "shuffled": (shuffled, None), "every third dropped": (kp, third), "outside": (outside, None),
                 "empty": (np.zeros(0, capi.SIFT_KP_DTYPE), None)}


@pytest.mark.parametrize("name", ["brisk_style", "shuffled", "every third dropped", "outside", "empty"])
def test_link_hook_equals_sift_describe(ctx, name):
    img, lists = hook_lists()
    kp, keep = lists[name]
    ctx.fast(img)                                                      # any detector call leaves the image resident
    live = np.arange(len(kp)) if keep is None else np.nonzero(keep)[0]
    ref = ctx.sift_describe(None, kp[live], shape=img.shape)
    got = ctx.sift_link_debug(kp, keep, 5, shape=img.shape)
    print(name, len(kp), "records,", len(live), "with their flag set, octaves", np.bincount(kp["octave"][live] & 255, minlength=6).tolist())
    assert got["kept"].dtype == np.int32 and np.array_equal(got["kept"], live)
    assert got["desc"].shape == (len(live), 128) and got["desc"].tobytes() == ref.tobytes()
    if name in ("brisk_style", "shuffled"):
        assert len(live) == 120 and set(kp["octave"].tolist()) == {1, 2, 3, 4, 5}
    if name == "shuffled":
        assert (np.diff(kp["octave"]) < 0).any()
    if name == "every third dropped":
        assert len(live) == 80 and keep[got["kept"]].all()
    if name == "outside":
        assert len(live) == 6 and not ref.any()
    again = ctx.sift_link_debug(kp, keep, 5, shape=img.shape)
    assert all(again[f].tobytes() == got[f].tobytes() for f in got)
    after = ctx.sift_describe(None, kp[live], shape=img.shape)         # the image is still resident
    assert after.tobytes() == ref.tobytes()
    if len(kp):
        ctx.sift_link_debug(kp, keep, 5, shape=img.shape)
        with pytest.raises(capi.SpvoError) as e:                       # ... and the hook's pyramid is not one spvo_sift_debug_level serves
            ctx.sift_level(0, 0)
        assert e.value.code == -4


def test_link_hook_on_a_level_of_one_row(ctx, sample_images):
    """32 x 400: octave 5 is 1 x 12, the smallest shape spvo_brisk_sift_pair accepts"""
    img = np.ascontiguousarray(sample_images[0][100:132, 300:700])
    assert img.shape == (32, 400)
    ctx.fast(img)
    kp = np.zeros(3, capi.SIFT_KP_DTYPE)
    kp["x"], kp["y"], kp["size"], kp["angle"], kp["octave"] = [200, 100, 390], [16, 10, 30], [48, 12, 7], -1, [5, 2, 0]
    ref = ctx.sift_describe(None, kp, shape=img.shape)
    got = ctx.sift_link_debug(kp, None, 5, shape=img.shape)
    assert np.array_equal(got["kept"], [0, 1, 2]) and got["desc"].tobytes() == ref.tobytes()
    assert not ref[0].any() and ref[1].any() and ref[2].any()          # (a level of one row has no pixel with four neighbours)


def raw_hook(c, shape, kp, max_octave):
    """the status of spvo_sift_link_debug and whether its sentinel-filled outputs are as they were"""
    kp = np.ascontiguousarray(kp, capi.SIFT_KP_DTYPE)
    kept = np.full(max(len(kp), 1), -77, np.int32)
    desc = np.full((max(len(kp), 1), 128), 7.5, np.float32)
    m = C.c_int(-77)
    rc = c.lib.spvo_sift_link_debug(c.h, shape[0], shape[1], kp.ctypes.data, None, len(kp), max_octave, kept.ctypes.data, desc.ctypes.data, C.byref(m))
    return rc, bool((kept == -77).all() and (desc == 7.5).all() and m.value == -77)


def test_link_hook_statuses(squeeze_weights_path):
    frames, P_l, P_r = load_sequence()
    img, lists = hook_lists()
    kp, _ = lists["brisk_style"]
    one = kp[:1].copy()

    def with_(**fields):
        k = one.copy()
        for f, v in fields.items():
            k[f] = v
        return k

    c = make_ctx(squeeze_weights_path)
    try:
        assert raw_hook(c, img.shape, kp, 5) == (-4, True)             # nothing is resident yet
        c.fast(img)
        before = c.sift_link_debug(kp, None, 5, shape=img.shape)
        refused = [raw_hook(c, img.shape, one, -1), raw_hook(c, img.shape, one, 16),
                   raw_hook(c, img.shape, one, 7),                                        # 64 >> 7: an empty level
                   raw_hook(c, img.shape, with_(octave=6), 5), raw_hook(c, img.shape, with_(octave=255), 5),   # octaves 6 and -1
                   raw_hook(c, img.shape, with_(octave=2), 1),
                   raw_hook(c, img.shape, with_(octave=1 | (1 << 8)), 5),                 # layer 1
                   raw_hook(c, img.shape, with_(x=np.nan), 5), raw_hook(c, img.shape, with_(y=np.inf), 5), raw_hook(c, img.shape, with_(size=0), 5),
                   raw_hook(c, img.shape, with_(size=-3), 5), raw_hook(c, img.shape, with_(angle=np.nan), 5),
                   raw_hook(c, img.shape, np.concatenate([kp, with_(octave=6)]), 5)]      # the last record of a long list
        for r in refused:
            assert r == (-1, True), refused
        assert raw_hook(c, (64, 97), one, 5) == (-4, True)             # another shape than the resident one
        after = c.sift_link_debug(kp, None, 5, shape=img.shape)        # the next valid call gives the earlier bytes
        assert after["desc"].tobytes() == before["desc"].tobytes() and np.array_equal(after["kept"], before["kept"])
        assert one["octave"][0] == 1 and raw_hook(c, img.shape, one, 1)[0] == 0          # (the octave field with bits above the second byte is carried)
        assert raw_hook(c, img.shape, with_(octave=1 | (200 << 16)), 5)[0] == 0
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)              # a SuperPoint submission in flight
        assert raw_hook(c, img.shape, one, 5) == (-4, True)
        c.detect_collect(P_l, P_r)
    finally:
        c.close()


# ---------------------------------------------------------------- 2. byte equality with the per-image route
@pytest.mark.parametrize("name", PAIRS)
@pytest.mark.parametrize("kind", KINDS)
def test_pair_equals_the_per_image_route(ctx, sample_images, reference, kind, name):
    L, R = pair(name, sample_images)
    rl, rr = reference[kind, name]
    gl, gr = call(ctx, kind, L, R, 2, 3)
    print(kind, name, L.shape, "per image", rl["n"], rr["n"], "pair", gl["n"], gr["n"], "octaves", np.bincount(gl["kp"]["octave"], minlength=6).tolist())
    assert_same(gl, rl, kind)
    assert_same(gr, rr, kind)
    assert ctx.sift_slot_rows(2) == rl["n"] and ctx.sift_slot_rows(3) == rr["n"]
    assert rl["n"] > 100 and rr["n"] > 100 and gl["kp"].tobytes() != gr["kp"].tobytes()
    if name == "crop":                                                 # the counts tests/test_sift_octave_pairs_resident_cpu.py pins
        assert (rl["n"], rr["n"]) == dict(brisk_sift=(1214, 1190), akaze_sift=(247, 247))[kind]
        if kind == "brisk_sift":
            assert set(gl["kp"]["octave"].tolist()) == set(range(6)) and (gl["kp"]["angle"] == -1).all()
    if name == "strided":
        assert not L.flags["C_CONTIGUOUS"]
        if kind == "akaze_sift":
            assert (rl["n"], rr["n"]) == (137, 152) and set(gl["kp"]["octave"].tolist()) == {0, 1} and gl["kp"]["class_id"].max() > 3
    sl, sr = call(ctx, kind, L, R, 2, 3)                               # two calls in a row give identical bytes
    assert_same(sl, gl, kind)
    assert_same(sr, gr, kind)
    if name == "full_size":
        return                                                         # (once)
    tl, tr = call(ctx, kind, R, L, 4, 5)                               # the other order: left and right trade places
    assert_same(tl, rr, kind)
    assert_same(tr, rl, kind)
    cap = rl["n"] // 2                                                 # host buffers smaller than n: the first rows, the full count
    pl, pr = call(ctx, kind, L, R, 6, 9, cap=cap)
    assert pl["n"] == rl["n"] and pl["kp"].tobytes() == rl["kp"][:cap].tobytes() and pl["desc"].tobytes() == rl["desc"][:cap].tobytes()
    assert pr["n"] == rr["n"] and pr["desc"].tobytes() == rr["desc"][:cap].tobytes()
    assert ctx.sift_slot_rows(6) == rl["n"] and ctx.sift_slot_rows(9) == rr["n"]


@pytest.mark.parametrize("kind", KINDS)
def test_an_image_without_a_keypoint(ctx, sample_images, kind):
    flat = np.full((64, 96), 93, np.uint8)
    gl, gr = call(ctx, kind, flat, flat.copy(), 2, 3)
    assert gl["n"] == 0 and gr["n"] == 0 and len(gl["kp"]) == 0 and gl["desc"].shape == (0, 128)
    assert ctx.sift_slot_rows(2) == 0 and ctx.sift_slot_rows(3) == 0
    for sel, cross in MODES:
        idx, dist = ctx.match_l2_slots(2, 3, sel, cross, 0.8)
        assert len(idx) == 0 and len(dist) == 0


# ---------------------------------------------------------------- 3. matching
@pytest.mark.parametrize("kind", KINDS)
def test_matching_in_the_slots(ctx, sample_images, kind):
    L, R = pair("crop", sample_images)
    fl, fr = call(ctx, kind, L, R, 6, 7)
    res = match_all(ctx, 6, 7, fl["desc"], fr["desc"])
    match_all(ctx, 7, 6, fr["desc"], fl["desc"])
    assert (res[("NN", False)][0] >= 0).all() and (res[("NN", True)][0] >= 0).any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_prematch_is_transparent(sample_images, kind, mode):
    """two consecutive calls in ring order with spvo_set_prematch on and off: identical results, the stereo match equals the synchronous
    match on the host copies and the temporal match the one against the call before's left rows"""
    sel, cross = mode
    res = {}
    for on in (False, True):
        c = make_ctx()
        try:
            c.set_prematch(on, sel, cross, 0.8)
            out = []
            for k, (L, R) in enumerate(same_shape_pairs(sample_images)):
                fl, fr = call(c, kind, L, R, 2 * k, 2 * k + 1)
                out.append(assert_match(c, 2 * k, 2 * k + 1, fl["desc"], fr["desc"], sel, cross))
                if k:
                    out.append(assert_match(c, 2 * k, 2 * k - 2, fl["desc"], prev["desc"], sel, cross))
                prev = fl
            res[on] = out
        finally:
            c.close()
    assert len(res[True]) == 3
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def test_prematch_temporal_partner_across_entry_points(sample_images):
    """any filled SIFT slot is a temporal partner, whichever call filled it: spvo_classic_sift_pair's (FAST + SIFT) and
    spvo_sift_detect_pair's of the new calls, and the new calls' of those two and of each other"""
    (L0, R0), (L1, R1) = same_shape_pairs(sample_images)
    c = make_ctx()
    try:
        c.set_prematch(True, "KNN", False, 0.8)

        def ok(sa, sb, fa, fb):
            assert_match(c, sa, sb, fa["desc"], fb["desc"], "KNN", False)

        ff, ff_r = c.classic_sift_pair(L0, R0, 0, 1, kind="FAST")
        assert ff["n"] > 10
        bl, br_ = c.brisk_sift_pair(L1, R1, 2, 3)                      # partner: slot 0, FAST + SIFT's
        ok(2, 3, bl, br_)
        ok(2, 0, bl, ff)
        al, ar_ = c.akaze_sift_pair(L0, R0, 4, 5)                      # partner: slot 2, BRISK + SIFT's
        ok(4, 5, al, ar_)
        ok(4, 2, al, bl)
        gl, gr = c.classic_sift_pair(L1, R1, 6, 7, kind="ShiTomasi")   # partner: slot 4, AKAZE + SIFT's
        ok(6, 7, gl, gr)
        ok(6, 4, gl, al)
        sl, sr = c.sift_detect_pair(L0, R0, 8, 9)
        assert sl["n"] > 10
        xl, xr = c.akaze_sift_pair(L1, R1, 0, 1)                       # partner: slot 8, SIFT + SIFT's
        ok(0, 1, xl, xr)
        ok(0, 8, xl, sl)
        yl, yr = c.brisk_sift_pair(L0, R0, 2, 3)                       # partner: slot 0, AKAZE + SIFT's
        ok(2, 3, yl, yr)
        ok(2, 0, yl, xl)
        zl, zr = c.sift_detect_pair(L1, R1, 4, 5)                      # partner: slot 2, BRISK + SIFT's
        ok(4, 5, zl, zr)
        ok(4, 2, zl, yl)
    finally:
        c.close()


# ---------------------------------------------------------------- 4. capacity, shape and state
@pytest.mark.parametrize("kind", KINDS)
def test_capacity(ctx, sample_images, reference, kind):
    L, R = pair("crop", sample_images)
    rl, rr = reference[kind, "crop"]
    n_l, n_r = rl["n"], rr["n"]
    ctx.set_prematch(True, "KNN", False, 0.8)
    fl, fr = ctx.classic_sift_pair(L, R, 4, 5, kind="FAST", slot_capacity=4096)        # a sibling's slots, filled earlier
    assert 0 < fl["n"] <= 4096 and 0 < fr["n"] <= 4096
    with pytest.raises(capi.SpvoError) as e:                           # one below the larger count: both counts reported, nothing truncated
        call(ctx, kind, L, R, 0, 1, slot_capacity=max(n_l, n_r) - 1)
    assert e.value.code == -5 and (e.value.n_l, e.value.n_r) == (n_l, n_r) == e.value.counts
    assert unfilled(ctx, 0) and unfilled(ctx, 1)                       # ... and both slots are unfilled afterwards
    with pytest.raises(capi.SpvoError) as e:
        ctx.match_l2_slots(0, 1)
    assert e.value.code == -4
    assert ctx.sift_slot_rows(4) == fl["n"] and ctx.sift_slot_rows(5) == fr["n"]          # no growth: the sibling's slots are as they were
    match_all(ctx, 4, 5, fl["desc"], fr["desc"])
    gl, gr = call(ctx, kind, L, R, 0, 1, slot_capacity=max(n_l, n_r))
    assert_same(gl, rl, kind)
    assert_same(gr, rr, kind)
    match_all(ctx, 0, 1, gl["desc"], gr["desc"])
    assert ctx.sift_slot_rows(4) == fl["n"]
    hl, hr = call(ctx, kind, L, R, 2, 3, slot_capacity=8192)            # a larger capacity than any before empties every SIFT slot
    assert_same(hl, rl, kind)
    assert unfilled(ctx, 4) and unfilled(ctx, 5) and unfilled(ctx, 0) and unfilled(ctx, 1)
    assert ctx.sift_slot_rows(2) == n_l and ctx.sift_slot_rows(3) == n_r
    match_all(ctx, 2, 3, hl["desc"], hr["desc"])


def raw_pair(c, kind, L, R, slot_l, slot_r, slot_capacity=8192, threshold=None, octaves=3, cap=4, null_buffers=False):
    """the status of a pair call and what it left in the two feature structs' n (77 going in) and buffers (7.5 going in)"""
    dtype = DTYPE[kind]
    kp = np.full(4 * dtype.itemsize // 4, 7.5, np.float32)
    desc = np.full((4, 128), 7.5, np.float32)
    F = capi.SiftFeatures if kind == "brisk_sift" else capi.AkazeSiftFeatures
    fl, fr = (F(77, None if null_buffers else kp.ctypes.data, None if null_buffers else desc.ctypes.data, cap) for _ in range(2))
    head = (c.h, L.ctypes.data, R.ctypes.data, L.shape[0], L.shape[1], L.strides[0])
    if kind == "brisk_sift":
        rc = c.lib.spvo_brisk_sift_pair(*head, 30 if threshold is None else threshold, octaves, slot_l, slot_r, slot_capacity, C.byref(fl), C.byref(fr))
    else:
        rc = c.lib.spvo_akaze_sift_pair(*head, 0.001 if threshold is None else threshold, slot_l, slot_r, slot_capacity, C.byref(fl), C.byref(fr))
    return rc, fl.n, fr.n, bool((desc == 7.5).all() and (kp == 7.5).all())


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_touch_nothing(sample_images, reference, squeeze_weights_path, kind):
    frames, P_l, P_r = load_sequence()
    L, R = pair("crop", sample_images)
    rl, rr = reference[kind, "crop"]
    c = make_ctx(squeeze_weights_path)
    try:
        gl, gr = call(c, kind, L, R, 0, 1)
        assert_same(gl, rl, kind)
        refused = [raw_pair(c, kind, L, R, 0, 0), raw_pair(c, kind, L, R, 0, 10), raw_pair(c, kind, L, R, -1, 1), raw_pair(c, kind, L, R, 0, 1, slot_capacity=0),
                   raw_pair(c, kind, L, R, 0, 1, slot_capacity=32769), raw_pair(c, kind, L, R, 0, 1, cap=-1), raw_pair(c, kind, L, R, 0, 1, null_buffers=True),
                   raw_pair(c, kind, L, R, 0, 1, threshold=0)]          # what the detector's sibling refuses of the parameters
        small = np.zeros((5, 40), np.uint8)
        refused.append(raw_pair(c, kind, small, small, 0, 1))          # ... and of the shape
        if kind == "brisk_sift":
            refused.append(raw_pair(c, kind, L, R, 0, 1, octaves=4))
            L31, R31 = np.ascontiguousarray(L[:31]), np.ascontiguousarray(R[:31])
            refused.append(raw_pair(c, kind, L31, R31, 0, 1))          # a 31 x 400 pair has no octave 5
            with pytest.raises(capi.SpvoError) as e:
                c.brisk_sift_pair(L31, R31, 0, 1)
            assert e.value.code == -1 and "octave 5" in str(e.value) and "31 x 400" in str(e.value)
        for r in refused:
            assert r == (-1, 77, 77, True), refused
        # nothing was touched: the slots and the resident image are as before
        assert c.sift_slot_rows(0) == rl["n"] and c.sift_slot_rows(1) == rr["n"]
        match_all(c, 0, 1, gl["desc"], gr["desc"])
        assert c.sift_describe(None, sift_records(rr["kp"]), shape=R.shape).tobytes() == rr["desc"].tobytes()
        gl, gr = call(c, kind, L, R, 0, 1)
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)              # a SuperPoint submission in flight
        assert raw_pair(c, kind, L, R, 0, 1) == (-4, 77, 77, True)
        c.detect_collect(P_l, P_r)
        assert c.sift_slot_rows(0) == rl["n"] and c.sift_slot_rows(1) == rr["n"]
        match_all(c, 0, 1, gl["desc"], gr["desc"])
        nl, nr = call(c, kind, L, R, 4, 5)
        assert_same(nl, rl, kind)
        assert_same(nr, rr, kind)
        if kind == "brisk_sift":                                       # the smallest shape with an octave 5 runs
            L32, R32 = np.ascontiguousarray(L[:32]), np.ascontiguousarray(R[:32])
            sl, sr = c.brisk_sift_pair(L32, R32, 6, 7)
            other = make_ctx()
            try:
                assert_same(sl, per_image(other, kind, L32), kind)
                assert_same(sr, per_image(other, kind, R32), kind)
            finally:
                other.close()
    finally:
        c.close()


# ---------------------------------------------------------------- 5. what is resident afterwards
@pytest.mark.parametrize("kind", KINDS)
def test_the_right_image_is_resident_afterwards(ctx, sample_images, reference, kind):
    L, R = pair("strided", sample_images)
    rl, rr = reference[kind, "strided"]
    other = make_ctx()                                                 # the yardsticks from a second context: this one keeps what the pair call leaves
    try:
        xy = np.stack([rr["kp"]["x"], rr["kp"]["y"]], 1)
        brisk = other.brisk_describe(R, xy, rr["kp"]["size"])
        if kind == "akaze_sift":
            other.akaze_detect(R)
            level = other.akaze_level(3, 0)
    finally:
        other.close()
    gl, gr = call(ctx, kind, L, R, 0, 1)
    assert_same(gr, rr, kind)
    with pytest.raises(capi.SpvoError) as e:                           # no SIFT pyramid is resident
        ctx.sift_level(0, 0)
    assert e.value.code == -4
    if kind == "brisk_sift":
        with pytest.raises(capi.SpvoError) as e:                       # ... nor a detector result spvo_brisk_detect_debug_layer serves
            ctx.brisk_detect_layer(1, 0)
        assert e.value.code == -4
    else:                                                              # the right image's scale space is
        assert ctx.akaze_level(3, 0).tobytes() == level.tobytes()
    assert ctx.sift_describe(None, sift_records(rr["kp"]), shape=R.shape).tobytes() == rr["desc"].tobytes()
    b = ctx.brisk_describe(None, xy, rr["kp"]["size"], shape=R.shape)
    assert b["desc"].tobytes() == brisk["desc"].tobytes() and np.array_equal(b["kept"], brisk["kept"])


# ---------------------------------------------------------------- 6. the host class
HOST = dict(brisk_sift=dict(detector="BRISK", descriptor="SIFT"), akaze_sift=dict(detector="AKAZE", descriptor="SIFT"))


def _run(frames, P_l, P_r, kind, **kw):
    return host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, input_size=(120, 392), trace=True, **HOST[kind], **kw)


@pytest.fixture(scope="module")
def per_image_runs():
    """the runs with setDeviceResident off, shared and left unchanged"""
    frames, P_l, P_r = load_sequence()
    out = {}
    for kind in KINDS:
        out[kind] = _run(frames, P_l, P_r, kind)
        assert host.classic_resident_pairs() == 0
    return (frames, P_l, P_r), out


@pytest.mark.parametrize("kind", KINDS)
def test_host_class_is_identical_with_resident_features(per_image_runs, kind):
    """ClassicFeatureFrontEnd over six synthetic frames at 120 x 392 (the ring of four slot pairs wraps once): keypoints_dq, descriptors_dq,
    the three match lists, the inlier sets (digests of their full contents) and every pose are identical with both switches on, and every
    pair stayed resident; with only one of the two the pair takes the per-image path as before"""
    (frames, P_l, P_r), runs = per_image_runs
    p0, s0, _, d0 = runs[kind]
    p1, s1, _, d1 = _run(frames, P_l, P_r, kind, resident=True, sift_octave_pairs_resident=True)
    assert host.classic_resident_pairs() == 6 == len(frames)
    print(kind, "keypoints", s0[:, 0].tolist(), s0[:, 1].tolist(), "inliers", s0[:, 3].tolist())
    assert s0[:, :2].min() > 20
    assert np.array_equal(d0, d1)
    assert np.array_equal(s0, s1)
    assert np.array_equal(p0, p1)
    p2, s2, _, d2 = _run(frames, P_l, P_r, kind, resident=True)
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d2) and np.array_equal(s0, s2) and np.array_equal(p0, p2)
    p3, s3, _, d3 = _run(frames, P_l, P_r, kind, sift_octave_pairs_resident=True)       # the new switch alone changes nothing
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d3) and np.array_equal(s0, s3) and np.array_equal(p0, p3)
    p4, s4, _, d4 = _run(frames, P_l, P_r, kind, resident=True, sift_describe_resident=True, octave_pairs_resident=True)   # ... and no earlier switch takes the route
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d4) and np.array_equal(s0, s4) and np.array_equal(p0, p4)


@pytest.mark.parametrize("kind", KINDS)
def test_host_class_mixes_resident_and_fallen_back_pairs(per_image_runs, kind):
    """slots of the median row count of the per-image run: some pairs fit, some take the per-image path and are matched from the host
    matrices, and the run is still identical"""
    (frames, P_l, P_r), runs = per_image_runs
    p0, s0, _, d0 = runs[kind]
    cap = int(np.median(s0[:, :2]))
    p1, s1, _, d1 = _run(frames, P_l, P_r, kind, resident=True, sift_octave_pairs_resident=True, resident_capacity=cap)
    print(kind, "rows", s0[:, :2].tolist(), "capacity", cap, "resident pairs", host.classic_resident_pairs())
    assert 0 < host.classic_resident_pairs() < 6
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
