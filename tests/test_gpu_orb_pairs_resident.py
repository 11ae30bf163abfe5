"""ORB + BRISK and ORB + SIFT with a stereo pair's features resident on the device (spvo_orb_brisk_pair into the binary slots,
spvo_orb_sift_pair into the SIFT slots, ClassicFeatureFrontEnd::setOrbBriskExtractor / setOrbPairsResident): everything equals the
per-image route on the same device EXACTLY -- spvo_orb_detect, its records converted on the host (x, y, 31 * 1.2^octave, degrees,
response, octave), then spvo_brisk_describe(img, x, y, size) or spvo_sift_describe(img, records), and the host-copy matchers -- counts,
the 24-byte keypoint records and the rows as raw bytes, match indices and distances, and through the host class every deque entry, match
list, inlier set and pose.  That per-image route is held to the numpy restatements by tests/test_gpu_orb.py, tests/test_gpu_brisk.py and
tests/test_gpu_sift_describe.py; what the inputs cover is pinned by tests/test_orb_pairs_resident_cpu.py.  No tolerance, no row excused.
(A level's corner-buffer overflow, SPVO_ERR_CAPACITY, is not reached: the buffers hold a corner per 2 x 2 block, which no image exceeds.)"""
import ctypes as C

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import capi, host
from tests.conftest import make_ctx
from tests.test_gpu_classic_trace_golden import load_sequence
from tests.test_orb_pairs_resident_cpu import level_scale, orb_sizes, stereo_pairs

pytestmark = pytest.mark.gpu

MODES = [("NN", False), ("NN", True), ("KNN", False)]          # NN, NN with cross-check, KNN at 0.8
KINDS = ["orb_brisk", "orb_sift"]
PAIRS = ["crop", "strided", "full_size"]
DTYPE = capi.SIFT_KP_DTYPE                                      # both calls hand out 24-byte records (spvo_brisk_keypoint is spvo_sift_keypoint)
ROWS = dict(orb_brisk=(np.uint8, 64), orb_sift=(np.float32, 128))


def pair(name, sample_images):
    if name == "full_size":
        return np.ascontiguousarray(sample_images[0]), np.ascontiguousarray(sample_images[1])
    return stereo_pairs(sample_images)[name]


def same_shape_pairs(sample_images):
    """two pairs of one shape: the crop cut to 200 rows, and the strided views"""
    return [tuple(np.ascontiguousarray(im[:200]) for im in pair("crop", sample_images)), pair("strided", sample_images)]


def call(ctx, kind, L, R, sl, sr, **kw):
    return getattr(ctx, kind + "_pair")(L, R, sl, sr, **kw)


def orb_degrees(radians):
    """the host's conversion: ONE float multiply, then + 360 for a negative angle"""
    a = np.asarray(radians, np.float32) * np.float32(57.29577951308232)
    return np.where(a < 0, a + np.float32(360), a).astype(np.float32)


def records(o):
    """spvo_orb_detect's records as the host converts them: x, y, 31 * scale, orb_degrees(angle), response, octave"""
    rec = np.zeros(len(o["xy"]), DTYPE)
    rec["x"], rec["y"] = o["xy"][:, 0], o["xy"][:, 1]
    rec["size"], rec["angle"], rec["response"], rec["octave"] = orb_sizes(o["octave"]), orb_degrees(o["angle"]), o["response"], o["octave"]
    return rec


def per_image(ctx, kind, img):
    """the per-image route of one image, as the records and rows the pair call promises (detected: the detector's converted records)"""
    img = np.ascontiguousarray(img)
    det = records(ctx.orb(img))
    if kind == "orb_sift":
        return dict(kp=det.copy(), desc=ctx.sift_describe(img, det), n=len(det), detected=det, kept=np.arange(len(det)))
    d = ctx.brisk_describe(img, np.stack([det["x"], det["y"]], 1), det["size"])
    rec = det[d["kept"]].copy()
    rec["angle"] = d["angle"]
    return dict(kp=rec, desc=d["desc"], n=len(rec), detected=det, kept=d["kept"])


def assert_same(got, ref, kind):
    assert got["n"] == ref["n"] == len(got["kp"]) == len(got["desc"])
    assert got["kp"].dtype == DTYPE and DTYPE.itemsize == 24 and got["desc"].shape == (ref["n"], ROWS[kind][1]) and got["desc"].dtype == ROWS[kind][0]
    if got["kp"].tobytes() != ref["kp"].tobytes():
        for f in DTYPE.names:
            bad = np.nonzero(got["kp"][f].view(np.uint32) != ref["kp"][f].view(np.uint32))[0]
            if len(bad):
                print("  field", f, ":", len(bad), "rows differ, first", int(bad[0]), got["kp"][bad[0]], ref["kp"][bad[0]])
    assert got["kp"].tobytes() == ref["kp"].tobytes()
    assert got["desc"].tobytes() == ref["desc"].tobytes(), "%d rows differ" % int((got["desc"] != ref["desc"]).any(1).sum())


def matchers(kind):
    """(name, the matcher on two slots, the same matcher on host copies) of a kind's slots"""
    if kind == "orb_sift":
        return [("l2", lambda c, a, b, s, x: c.match_l2_slots(a, b, s, x, 0.8), lambda c, da, db, s, x: c.match_l2(da, db, s, x, 0.8, dim=128))]
    return [("hamming", lambda c, a, b, s, x: c.match_hamming_slots(a, b, s, x, 0.8), lambda c, da, db, s, x: c.match_hamming(da, db, s, x, 0.8)),
            ("l2_u8", lambda c, a, b, s, x: c.match_l2_u8_slots(a, b, s, x, 0.8), lambda c, da, db, s, x: c.match_l2_u8(da, db, s, x, 0.8))]


def assert_match(c, kind, sa, sb, da, db, sel, cross, only=None):
    """slots sa -> sb equal the host-copy matchers, index for index and distance for distance"""
    out = []
    for name, on_slots, on_host in matchers(kind):
        if only and name != only:
            continue
        gi, gd = on_slots(c, sa, sb, sel, cross)
        hi, hd = on_host(c, da, db, sel, cross)
        assert np.array_equal(gi, hi) and gd.tobytes() == hd.tobytes() and len(gi) == len(da), (name, sa, sb, sel, cross)
        out.append((gi, gd))
    return out


def match_all(c, kind, sa, sb, da, db):
    return {m: assert_match(c, kind, sa, sb, da, db, *m) for m in MODES}


def slot_rows(c, kind, slot):
    return c.sift_slot_rows(slot) if kind == "orb_sift" else c.classic_slot_rows(slot)


def unfilled(c, kind, slot):
    with pytest.raises(capi.SpvoError) as e:
        slot_rows(c, kind, slot)
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


# ---------------------------------------------------------------- 1. the record kernel
@pytest.mark.parametrize("kind", KINDS)
def test_records_are_the_hosts_conversion(ctx, sample_images, reference, kind):
    """the mirrors' records against spvo_orb_detect's converted on the host, field by field as bits: all of them (ORB + SIFT), the
    survivors of the extractor's border rule in order with the extractor's angle (ORB + BRISK)"""
    L, R = pair("crop", sample_images)
    for got, ref in zip(call(ctx, kind, L, R, 0, 1), reference[kind, "crop"]):
        det, kept = ref["detected"], ref["kept"]
        assert got["n"] == len(kept) and (kind == "orb_brisk" or len(kept) == len(det))
        assert 0 < len(kept) and (kind == "orb_sift" or len(kept) < len(det))
        for f in ("x", "y", "size", "response", "octave") + (("angle",) if kind == "orb_sift" else ()):
            assert got["kp"][f].tobytes() == det[f][kept].tobytes(), f
        sizes = (np.float32(31) * level_scale()).astype(np.float32)
        assert np.array_equal(got["kp"]["size"], sizes[got["kp"]["octave"]]) and len(set(got["kp"]["octave"].tolist())) >= 3
        assert (got["kp"]["angle"] >= 0).all() and (got["kp"]["angle"] <= 360).all() and (det["angle"] > 180).any()
        if kind == "orb_brisk":
            assert got["kp"]["angle"].tobytes() == ref["kp"]["angle"].tobytes() != det["angle"][kept].tobytes()


# ---------------------------------------------------------------- 2. byte equality with the per-image route
@pytest.mark.parametrize("name", PAIRS)
@pytest.mark.parametrize("kind", KINDS)
def test_pair_equals_the_per_image_route(ctx, sample_images, reference, kind, name):
    L, R = pair(name, sample_images)
    rl, rr = reference[kind, name]
    gl, gr = call(ctx, kind, L, R, 2, 3)
    print(kind, name, L.shape, "detected", len(rl["detected"]), len(rr["detected"]), "per image", rl["n"], rr["n"], "pair", gl["n"], gr["n"], "octaves",
          np.bincount(gl["kp"]["octave"], minlength=8).tolist())
    assert_same(gl, rl, kind)
    assert_same(gr, rr, kind)
    assert slot_rows(ctx, kind, 2) == rl["n"] and slot_rows(ctx, kind, 3) == rr["n"]
    assert rl["n"] > 100 and rr["n"] > 100 and gl["kp"].tobytes() != gr["kp"].tobytes()
    if name == "crop":                                                 # the counts tests/test_orb_pairs_resident_cpu.py pins
        assert (len(rl["detected"]), len(rr["detected"])) == (1750, 1750)
        assert (rl["n"], rr["n"]) == dict(orb_brisk=(1074, 1079), orb_sift=(1750, 1750))[kind]
    if name == "strided":
        assert not L.flags["C_CONTIGUOUS"]
        assert (rl["n"], rr["n"]) == dict(orb_brisk=(397, 413), orb_sift=(681, 750))[kind]
    if name == "full_size":
        assert len(rl["detected"]) == 2000                             # nfeatures binds: n = min(the levels' counts, nfeatures)
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
    assert slot_rows(ctx, kind, 6) == rl["n"] and slot_rows(ctx, kind, 9) == rr["n"]


# ---------------------------------------------------------------- 3. degenerate shapes
@pytest.mark.parametrize("shape", ["flat 96 x 128", "64 x 96"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_pair_without_a_keypoint(ctx, kind, shape):
    """an image without a corner, and a shape none of whose levels can hold a keypoint (textured, so that the shape is the reason)"""
    if shape == "64 x 96":
        L = np.random.default_rng(5).integers(0, 256, (64, 96)).astype(np.uint8)
        R = np.ascontiguousarray(L[::-1, ::-1])
    else:
        L, R = np.full((96, 128), 93, np.uint8), np.full((96, 128), 93, np.uint8)
    gl, gr = call(ctx, kind, L, R, 2, 3)
    assert gl["n"] == 0 and gr["n"] == 0 and len(gl["kp"]) == 0 and gl["desc"].shape == (0, ROWS[kind][1])
    assert slot_rows(ctx, kind, 2) == 0 and slot_rows(ctx, kind, 3) == 0
    for sel, cross in MODES:
        for name, on_slots, _ in matchers(kind):
            idx, dist = on_slots(ctx, 2, 3, sel, cross)
            assert len(idx) == 0 and len(dist) == 0, (name, sel, cross)


@pytest.mark.parametrize("kind", KINDS)
def test_the_smallest_shape_with_a_keypoint_area(ctx, sample_images, kind):
    """67 x 67: level 0 alone can hold a keypoint"""
    L, R = np.ascontiguousarray(sample_images[0][150:217, 500:567]), np.ascontiguousarray(sample_images[1][150:217, 500:567])
    assert L.shape == (67, 67)
    other = make_ctx()
    try:
        rl, rr = per_image(other, kind, L), per_image(other, kind, R)
    finally:
        other.close()
    gl, gr = call(ctx, kind, L, R, 0, 1)
    print(kind, "67 x 67: detected", len(rl["detected"]), len(rr["detected"]), "rows", rl["n"], rr["n"])
    assert_same(gl, rl, kind)
    assert_same(gr, rr, kind)
    assert (rl["detected"]["octave"] == 0).all()


# ---------------------------------------------------------------- 4. matching
@pytest.mark.parametrize("kind", KINDS)
def test_matching_in_the_slots(ctx, sample_images, kind):
    L, R = pair("strided", sample_images)
    fl, fr = call(ctx, kind, L, R, 6, 7)
    res = match_all(ctx, kind, 6, 7, fl["desc"], fr["desc"])
    match_all(ctx, kind, 7, 6, fr["desc"], fl["desc"])
    assert (res[("NN", False)][0][0] >= 0).all() and (res[("NN", True)][0][0] >= 0).any()


@pytest.mark.parametrize("kind, matcher", [("orb_brisk", "hamming"), ("orb_brisk", "l2_u8"), ("orb_sift", "l2")])
@pytest.mark.parametrize("mode", MODES)
def test_prematch_is_transparent(sample_images, kind, matcher, mode):
    """two consecutive calls in ring order with spvo_set_prematch on and off (binary slots: under either norm): identical results, the
    stereo match equals the synchronous match on the host copies and the temporal match the one against the call before's left rows"""
    sel, cross = mode
    res = {}
    for on in (False, True):
        c = make_ctx()
        try:
            c.set_prematch(on, sel, cross, 0.8)
            if matcher == "l2_u8":
                c.set_binary_prematch_norm("L2")
            out = []
            for k, (L, R) in enumerate(same_shape_pairs(sample_images)):
                fl, fr = call(c, kind, L, R, 2 * k, 2 * k + 1)
                out += assert_match(c, kind, 2 * k, 2 * k + 1, fl["desc"], fr["desc"], sel, cross, only=matcher)
                if k:
                    out += assert_match(c, kind, 2 * k, 2 * k - 2, fl["desc"], prev["desc"], sel, cross, only=matcher)
                prev = fl
            res[on] = out
        finally:
            c.close()
    assert len(res[True]) == 3
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def test_prematch_temporal_partner_across_entry_points(sample_images):
    """a filled slot of the ring (binary: of 64-byte rows) is a temporal partner, whichever call filled it: spvo_classic_detect's
    (ShiTomasi + BRISK) and spvo_brisk_sift_pair's of the new calls, and the new calls' of those; a 32-byte slot before ORB + BRISK is skipped"""
    (L0, R0), (L1, R1) = same_shape_pairs(sample_images)
    c = make_ctx()
    try:
        c.set_prematch(True, "KNN", False, 0.8)

        def ok(kind, sa, sb, fa, fb):
            assert_match(c, kind, sa, sb, fa["desc"], fb["desc"], "KNN", False)

        gb, gb_r = c.classic_detect(L0, R0, 0, 1, "ShiTomasi+BRISK")
        assert gb["desc"].shape[1] == 64 and len(gb["desc"]) > 10
        ol, or_ = c.orb_brisk_pair(L1, R1, 2, 3)                       # partner: slot 0, ShiTomasi + BRISK's
        ok("orb_brisk", 2, 3, ol, or_)
        ok("orb_brisk", 2, 0, ol, gb)
        fb, fb_r = c.classic_detect(L0, R0, 4, 5, "FAST+BRISK")        # partner: slot 2, ORB + BRISK's
        ok("orb_brisk", 4, 5, fb, fb_r)
        ok("orb_brisk", 4, 2, fb, ol)
        fo, fo_r = c.classic_detect(L1, R1, 6, 7, "FAST")              # 32-byte rows
        assert fo["desc"].shape[1] == 32
        xl, xr = c.orb_brisk_pair(L0, R0, 8, 9)                        # a 32-byte left slot before: skipped
        ok("orb_brisk", 8, 9, xl, xr)
        with pytest.raises(capi.SpvoError) as e:                       # asked for explicitly, the temporal match names the widths
            c.match_hamming_slots(8, 6, "KNN", False, 0.8)
        assert e.value.code == -1
        bl, br_ = c.brisk_sift_pair(L0, R0, 0, 1)                      # the SIFT ring
        sl, sr = c.orb_sift_pair(L1, R1, 2, 3)                         # partner: slot 0, BRISK + SIFT's
        ok("orb_sift", 2, 3, sl, sr)
        ok("orb_sift", 2, 0, sl, bl)
        yl, yr = c.brisk_sift_pair(L0, R0, 4, 5)                       # partner: slot 2, ORB + SIFT's
        ok("orb_sift", 4, 5, yl, yr)
        ok("orb_sift", 4, 2, yl, sl)
    finally:
        c.close()


# ---------------------------------------------------------------- 5. capacity, refusals and state
def sibling(ctx, kind, L, R, sl, sr):
    """a sibling entry point's features (at most 1000 Shi-Tomasi corners) in two slots of the kind's ring, at a capacity of 4096"""
    if kind == "orb_sift":
        return ctx.classic_sift_pair(L, R, sl, sr, kind="ShiTomasi", slot_capacity=4096)
    return ctx.classic_detect(L, R, sl, sr, "ShiTomasi+BRISK", slot_capacity=4096)


@pytest.mark.parametrize("kind", KINDS)
def test_capacity(ctx, sample_images, reference, kind):
    L, R = pair("crop", sample_images)
    rl, rr = reference[kind, "crop"]
    n_l, n_r = rl["n"], rr["n"]
    ctx.set_prematch(True, "KNN", False, 0.8)
    fl, fr = sibling(ctx, kind, L, R, 4, 5)                            # a sibling's slots, filled earlier
    assert 0 < len(fl["desc"]) <= 4096 and 0 < len(fr["desc"]) <= 4096
    with pytest.raises(capi.SpvoError) as e:                           # one below the larger count: both counts reported, nothing truncated
        call(ctx, kind, L, R, 0, 1, slot_capacity=max(n_l, n_r) - 1)
    assert e.value.code == -5 and (e.value.n_l, e.value.n_r) == (n_l, n_r) == e.value.counts
    assert unfilled(ctx, kind, 0) and unfilled(ctx, kind, 1)           # ... and both slots are unfilled afterwards
    with pytest.raises(capi.SpvoError) as e:
        matchers(kind)[0][1](ctx, 0, 1, "KNN", False)
    assert e.value.code == -4
    assert slot_rows(ctx, kind, 4) == len(fl["desc"]) and slot_rows(ctx, kind, 5) == len(fr["desc"])   # no growth: the sibling's slots are as they were
    match_all(ctx, kind, 4, 5, fl["desc"], fr["desc"])
    gl, gr = call(ctx, kind, L, R, 0, 1, slot_capacity=max(n_l, n_r))  # at the count it runs
    assert_same(gl, rl, kind)
    assert_same(gr, rr, kind)
    match_all(ctx, kind, 0, 1, gl["desc"], gr["desc"])
    assert slot_rows(ctx, kind, 4) == len(fl["desc"])


def raw_pair(c, kind, L, R, slot_l, slot_r, slot_capacity=8192, nfeatures=2000, cap=4, null_buffers=False):
    """the status of a pair call and what it left in the two feature structs' n (77 going in) and buffers (7.5 going in)"""
    kp = np.full(4 * 6, 7.5, np.float32)
    desc = np.full((4, 128), 7.5, np.float32)
    F = capi.SiftFeatures if kind == "orb_sift" else capi.BriskFeatures
    fl, fr = (F(77, None if null_buffers else kp.ctypes.data, None if null_buffers else desc.ctypes.data, cap) for _ in range(2))
    fn = c.lib.spvo_orb_sift_pair if kind == "orb_sift" else c.lib.spvo_orb_brisk_pair
    rc = fn(c.h, L.ctypes.data, R.ctypes.data, L.shape[0], L.shape[1], L.strides[0], nfeatures, slot_l, slot_r, slot_capacity, C.byref(fl), C.byref(fr))
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
                   raw_pair(c, kind, L, R, 0, 1, slot_capacity=32769), raw_pair(c, kind, L, R, 0, 1, nfeatures=0), raw_pair(c, kind, L, R, 0, 1, nfeatures=-3),
                   raw_pair(c, kind, L, R, 0, 1, cap=-1)]
        if kind == "orb_sift":
            refused.append(raw_pair(c, kind, L, R, 0, 1, null_buffers=True))       # (a binary call may leave kp / desc NULL)
            small = np.zeros((5, 40), np.uint8)
            refused.append(raw_pair(c, kind, small, small, 0, 1))      # what spvo_sift_describe refuses of the shape
        else:
            big = np.zeros((2903, 2903), np.uint8)                     # what brisk_check_image refuses: 2903^2 * 255 >= 2^31 (refused before a byte is read)
            refused.append(raw_pair(c, kind, big, big, 0, 1))
        for r in refused:
            assert r == (-1, 77, 77, True), refused
        # nothing was touched: the slots and the resident image are as before
        assert slot_rows(c, kind, 0) == rl["n"] and slot_rows(c, kind, 1) == rr["n"]
        match_all(c, kind, 0, 1, gl["desc"], gr["desc"])
        assert c.sift_describe(None, rr["detected"], shape=R.shape).tobytes() == reference["orb_sift", "crop"][1]["desc"].tobytes()
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)              # a SuperPoint submission in flight
        assert raw_pair(c, kind, L, R, 0, 1) == (-4, 77, 77, True)
        c.detect_collect(P_l, P_r)
        assert slot_rows(c, kind, 0) == rl["n"] and slot_rows(c, kind, 1) == rr["n"]
        match_all(c, kind, 0, 1, gl["desc"], gr["desc"])
        nl, nr = call(c, kind, L, R, 4, 5)
        assert_same(nl, rl, kind)
        assert_same(nr, rr, kind)
    finally:
        c.close()


# ---------------------------------------------------------------- 6. what is resident afterwards
@pytest.mark.parametrize("kind", KINDS)
def test_the_right_image_is_resident_afterwards(ctx, sample_images, reference, kind):
    L, R = pair("strided", sample_images)
    rb, rs = reference["orb_brisk", "strided"][1], reference["orb_sift", "strided"][1]   # a second context's results on the right image
    det = rs["detected"]
    gl, gr = call(ctx, kind, L, R, 0, 1)
    assert_same(gr, reference[kind, "strided"][1], kind)
    b = ctx.brisk_describe(None, np.stack([det["x"], det["y"]], 1), det["size"], shape=R.shape)
    assert b["desc"].tobytes() == rb["desc"].tobytes() and np.array_equal(b["kept"], rb["kept"]) and b["angle"].tobytes() == rb["kp"]["angle"].tobytes()
    assert ctx.sift_describe(None, det, shape=R.shape).tobytes() == rs["desc"].tobytes()


# ---------------------------------------------------------------- 7. the host class
HOST = dict(orb_brisk=dict(detector="ORB", descriptor="BRISK", orb_brisk=True), orb_sift=dict(detector="ORB", descriptor="SIFT"))
EARLIER = dict(brisk_resident=True, akaze_resident=True, sift_describe_resident=True, octave_pairs_resident=True, sift_octave_pairs_resident=True)


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
    pair stayed resident; with only one of the two, or with every earlier resident switch instead, the pair takes the per-image path"""
    (frames, P_l, P_r), runs = per_image_runs
    p0, s0, _, d0 = runs[kind]
    p1, s1, _, d1 = _run(frames, P_l, P_r, kind, resident=True, orb_pairs_resident=True)
    assert host.classic_resident_pairs() == 6 == len(frames)
    print(kind, "keypoints", s0[:, 0].tolist(), s0[:, 1].tolist(), "inliers", s0[:, 3].tolist())
    assert s0[:, :2].min() > 20
    assert np.array_equal(d0, d1)
    assert np.array_equal(s0, s1)
    assert np.array_equal(p0, p1)
    p2, s2, _, d2 = _run(frames, P_l, P_r, kind, resident=True)
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d2) and np.array_equal(s0, s2) and np.array_equal(p0, p2)
    p3, s3, _, d3 = _run(frames, P_l, P_r, kind, orb_pairs_resident=True)                # the new switch alone changes nothing
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d3) and np.array_equal(s0, s3) and np.array_equal(p0, p3)
    p4, s4, _, d4 = _run(frames, P_l, P_r, kind, resident=True, **EARLIER)               # ... and no earlier switch takes the route
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d4) and np.array_equal(s0, s4) and np.array_equal(p0, p4)


@pytest.mark.parametrize("kind", KINDS)
def test_host_class_mixes_resident_and_fallen_back_pairs(per_image_runs, kind):
    """slots of the median row count of the per-image run: some pairs fit, some take the per-image path and are matched from the host
    matrices, and the run is still identical"""
    (frames, P_l, P_r), runs = per_image_runs
    p0, s0, _, d0 = runs[kind]
    cap = int(np.median(s0[:, :2]))
    p1, s1, _, d1 = _run(frames, P_l, P_r, kind, resident=True, orb_pairs_resident=True, resident_capacity=cap)
    print(kind, "rows", s0[:, :2].tolist(), "capacity", cap, "resident pairs", host.classic_resident_pairs())
    assert 0 < host.classic_resident_pairs() < 6
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)


def test_orb_brisk_without_its_switch_is_refused(per_image_runs):
    (frames, P_l, P_r), _ = per_image_runs
    with pytest.raises(RuntimeError):
        host.classic_sequence(frames[:2], P_l, P_r, "KNN", True, 2.0, 4, input_size=(120, 392), detector="ORB", descriptor="BRISK")
    with pytest.raises(RuntimeError):                                  # ... whatever resident switch is on
        host.classic_sequence(frames[:2], P_l, P_r, "KNN", True, 2.0, 4, input_size=(120, 392), detector="ORB", descriptor="BRISK", resident=True, orb_pairs_resident=True)
