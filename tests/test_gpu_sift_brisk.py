"""SIFT + BRISK: the per-image route (spvo_sift_detect, then spvo_brisk_describe at the records' x, y, size;
ClassicFeatureFrontEnd::setSiftBriskExtractor) and the pair-resident one (spvo_sift_brisk_pair into the binary slots of 64-byte rows;
setSiftBriskResident).  The per-image route is held to the restatements -- spvo_sift_detect by tests/test_gpu_sift.py, and here
spvo_brisk_describe on SIFT keypoints to tests/brisk_ref.py as tests/test_gpu_brisk.py compares them -- and the pair call to the per-image
route on the same device EXACTLY: counts, the 24-byte records and the rows as raw bytes, match indices and distances, and through the
host class every deque entry, match list, inlier set and pose.  No tolerance, no row excused.  What the inputs cover is pinned on the CPU
by tests/test_sift_brisk_cpu.py; the GPU's orientation agrees with the restatement only to rounding level, so the counts are asserted
here as conditions.  (The SIFT lists' overflow and regrow is not reached: the lists hold at least 8192 candidates and a candidate per 4
pixels of the doubled image, which no input here exceeds.)"""
import ctypes as C

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import capi, host
from tests import brisk_ref as br
from tests import sift_cases
from tests.conftest import make_ctx
from tests.test_gpu_brisk import _compare as compare_with_restatement
from tests.test_gpu_classic_trace_golden import load_sequence
from tests.test_sift_brisk_cpu import stereo_pairs, tiny_image

pytestmark = pytest.mark.gpu

MODES = [("NN", False), ("NN", True), ("KNN", False)]          # NN, NN with cross-check, KNN at 0.8
PAIRS = ["crop", "strided", "kitti", "full_size"]
DTYPE = capi.SIFT_KP_DTYPE                                      # spvo_brisk_keypoint is spvo_sift_keypoint: 24 bytes


def pair(name, sample_images):
    if name == "full_size":
        return np.ascontiguousarray(sample_images[0]), np.ascontiguousarray(sample_images[1])
    return stereo_pairs(sample_images)[name]


def same_shape_pairs(sample_images):
    """two pairs of one shape: the crop cut to 200 rows, and the strided views"""
    return [tuple(np.ascontiguousarray(im[:200]) for im in pair("crop", sample_images)), pair("strided", sample_images)]


def per_image(ctx, img):
    """the per-image route of one image, as the records and rows the pair call promises (detected: spvo_sift_detect's records)"""
    img = np.ascontiguousarray(img)
    det = ctx.sift_detect(img)["kp"]
    d = ctx.brisk_describe(img, np.stack([det["x"], det["y"]], 1).reshape(-1, 2), det["size"])
    rec = det[d["kept"]].copy()
    rec["angle"] = d["angle"]
    return dict(kp=rec, desc=d["desc"], n=len(rec), detected=det, kept=d["kept"])


def assert_same(got, ref):
    assert got["n"] == ref["n"] == len(got["kp"]) == len(got["desc"])
    assert got["kp"].dtype == DTYPE and DTYPE.itemsize == 24 and got["desc"].shape == (ref["n"], 64) and got["desc"].dtype == np.uint8
    if got["kp"].tobytes() != ref["kp"].tobytes():
        for f in DTYPE.names:
            bad = np.nonzero(got["kp"][f].view(np.uint32) != ref["kp"][f].view(np.uint32))[0]
            if len(bad):
                print("  field", f, ":", len(bad), "rows differ, first", int(bad[0]), got["kp"][bad[0]], ref["kp"][bad[0]])
    assert got["kp"].tobytes() == ref["kp"].tobytes()
    assert got["desc"].tobytes() == ref["desc"].tobytes(), "%d rows differ" % int((got["desc"] != ref["desc"]).any(1).sum())


MATCHERS = [("hamming", lambda c, a, b, s, x: c.match_hamming_slots(a, b, s, x, 0.8), lambda c, da, db, s, x: c.match_hamming(da, db, s, x, 0.8)),
            ("l2_u8", lambda c, a, b, s, x: c.match_l2_u8_slots(a, b, s, x, 0.8), lambda c, da, db, s, x: c.match_l2_u8(da, db, s, x, 0.8))]


def assert_match(c, sa, sb, da, db, sel, cross, only=None):
    """slots sa -> sb equal the host-copy matchers, index for index and distance for distance"""
    out = []
    for name, on_slots, on_host in MATCHERS:
        if only and name != only:
            continue
        gi, gd = on_slots(c, sa, sb, sel, cross)
        hi, hd = on_host(c, da, db, sel, cross)
        assert np.array_equal(gi, hi) and gd.tobytes() == hd.tobytes() and len(gi) == len(da), (name, sa, sb, sel, cross)
        out.append((gi, gd))
    return out


def match_all(c, sa, sb, da, db):
    return {m: assert_match(c, sa, sb, da, db, *m) for m in MODES}


def unfilled(c, slot):
    with pytest.raises(capi.SpvoError) as e:
        c.classic_slot_rows(slot)
    return e.value.code == -4


@pytest.fixture()
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference(sample_images):
    """the per-image route of every pair, computed once in a context of its own and left unchanged: name -> (left, right)"""
    c = make_ctx()
    out = {name: tuple(per_image(c, im) for im in pair(name, sample_images)) for name in PAIRS}
    c.close()
    return out


# ---------------------------------------------------------------- 1. the per-image route against the restatement
@pytest.mark.parametrize("name", ["crop", "kitti"])
def test_brisk_on_sift_keypoints_equals_the_restatement(sample_images, reference, name):
    """spvo_sift_detect (the unchanged detector, held to tests/sift_ref.py by tests/test_gpu_sift.py), then spvo_brisk_describe on its x,
    y, size against brisk_ref.describe on those same keypoints and the library's tables: kept, the 60 intensities and the rows bit for
    bit, angles equal or adjacent"""
    img = np.ascontiguousarray(pair(name, sample_images)[0])
    det = reference[name][0]["detected"]
    xy = np.stack([det["x"], det["y"]], 1)
    c = make_ctx()
    g = c.brisk_describe(img, xy, det["size"], values0=True)
    c.close()
    r = br.describe(img, xy, det["size"], tables=capi.brisk_tables())
    compare_with_restatement(g, r, len(det))
    scale = br.scale_index(det["size"])[g["kept"]]
    octave = (det["octave"][g["kept"]] & 255).astype(np.int8)
    print(name, "SIFT keypoints", len(det), "kept", len(g["kept"]), "scale indices", int(scale.min()), "..", int(scale.max()), "octaves", sorted(set(octave.tolist())))
    assert len(det) >= 200 and 2 * len(g["kept"]) > len(det) > len(g["kept"])
    assert (scale == 0).any() and (scale > 0).any() and -1 in octave.tolist() and len(set(octave.tolist())) >= 3
    assert g["desc"].tobytes() == reference[name][0]["desc"].tobytes() and np.array_equal(g["kept"], reference[name][0]["kept"])


# ---------------------------------------------------------------- 2. the kernels in front of the extractor's chain
@pytest.mark.parametrize("name", ["crop", "strided", "kitti", "full_size", "noise", "flat"])
def test_records_are_the_detectors(ctx, sample_images, reference, name):
    """sift_records_kernel's list -- what the BRISK chain reads -- against spvo_sift_detect's output, field by field as bit patterns (the
    size, which picks the scale index, among them), from the orientation-only instantiation and from the describing one alike: the raw
    rows {candidate, angle} and the final order do not depend on the instantiation"""
    if name in ("noise", "flat"):
        img = np.ascontiguousarray(sift_cases.image(name))
        other = make_ctx()
        det = other.sift_detect(img)["kp"]
        other.close()
    else:
        img, det = pair(name, sample_images)[0], reference[name][0]["detected"]
    only, with_rows = ctx.sift_records_debug(img, describe=False), ctx.sift_records_debug(img, describe=True)
    print(name, img.shape, "records", len(only), len(with_rows), "spvo_sift_detect", len(det))
    assert len(only) == len(with_rows) == len(det) and (len(det) > 0) == (name != "flat")
    for f in DTYPE.names:
        assert only[f].view(np.uint32).tobytes() == det[f].view(np.uint32).tobytes(), f
    assert only.tobytes() == with_rows.tobytes() == det.tobytes()
    if name == "crop":                                                 # several keypoints of one candidate: one per orientation peak
        assert len(set(zip(det["x"].tolist(), det["y"].tolist(), det["size"].tolist()))) < len(det)
    # the image is the resident one afterwards
    d = ctx.brisk_describe(None, np.stack([det["x"], det["y"]], 1).reshape(-1, 2), det["size"], shape=img.shape)
    if name in reference:
        assert d["desc"].tobytes() == reference[name][0]["desc"].tobytes()


# ---------------------------------------------------------------- 3. byte equality of the pair call with the per-image route
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("name", PAIRS)
def test_pair_equals_the_per_image_route(ctx, sample_images, reference, name, forced):
    """forced: with the second pass on the host's records (tuning sift_brisk_recheck) -- the same bytes, the same slot contents"""
    L, R = pair(name, sample_images)
    rl, rr = reference[name]
    if forced:
        capi.set_tuning("sift_brisk_recheck", 1)
    try:
        gl, gr = ctx.sift_brisk_pair(L, R, 2, 3)
        print(name, L.shape, "forced" if forced else "", "detected", len(rl["detected"]), len(rr["detected"]), "per image", rl["n"], rr["n"], "pair", gl["n"], gr["n"])
        assert_same(gl, rl)
        assert_same(gr, rr)
        assert ctx.classic_slot_rows(2) == rl["n"] and ctx.classic_slot_rows(3) == rr["n"]
        assert rl["n"] > 100 and rr["n"] > 100 and gl["kp"].tobytes() != gr["kp"].tobytes()
        if name == "crop":                                             # the conditions tests/test_sift_brisk_cpu.py pins as counts
            for r in (rl, rr):
                scale = br.scale_index(r["kp"]["size"])
                assert len(r["detected"]) >= 200 and 2 * r["n"] > len(r["detected"]) > r["n"] and (scale == 0).any() and (scale > 0).any()
        if name == "strided":
            assert not L.flags["C_CONTIGUOUS"]
        match_all(ctx, 2, 3, gl["desc"], gr["desc"])                   # the slots hold those rows
        sl, sr = ctx.sift_brisk_pair(L, R, 2, 3)                       # two calls in a row give identical bytes
        assert_same(sl, gl)
        assert_same(sr, gr)
        if name == "full_size":
            return                                                     # (once)
        tl, tr = ctx.sift_brisk_pair(R, L, 4, 5)                       # the other order: left and right trade places
        assert_same(tl, rr)
        assert_same(tr, rl)
        cap = rl["n"] // 2                                             # host buffers smaller than n: the first rows, the full count
        pl, pr = ctx.sift_brisk_pair(L, R, 6, 9, cap=cap)
        assert pl["n"] == rl["n"] and pl["kp"].tobytes() == rl["kp"][:cap].tobytes() and pl["desc"].tobytes() == rl["desc"][:cap].tobytes()
        assert pr["n"] == rr["n"] and pr["desc"].tobytes() == rr["desc"][:cap].tobytes()
        assert ctx.classic_slot_rows(6) == rl["n"] and ctx.classic_slot_rows(9) == rr["n"]
        rc, n_l, n_r, untouched = raw_pair(ctx, np.ascontiguousarray(L), np.ascontiguousarray(R), 0, 1, cap=0, null_buffers=True)   # cap = 0, no buffers: the counts alone
        assert (rc, n_l, n_r, untouched) == (0, rl["n"], rr["n"], True)
        assert ctx.classic_slot_rows(0) == rl["n"] and ctx.classic_slot_rows(1) == rr["n"]
        match_all(ctx, 0, 1, rl["desc"], rr["desc"])
    finally:
        capi.set_tuning("sift_brisk_recheck", 0)


# ---------------------------------------------------------------- 4. empty and tiny inputs
def test_a_flat_pair_gives_two_empty_slots(ctx):
    L, R = np.full((64, 64), 117, np.uint8), np.full((64, 64), 93, np.uint8)
    gl, gr = ctx.sift_brisk_pair(L, R, 2, 3)
    assert gl["n"] == 0 and gr["n"] == 0 and len(gl["kp"]) == 0 and gl["desc"].shape == (0, 64)
    assert ctx.classic_slot_rows(2) == 0 and ctx.classic_slot_rows(3) == 0
    for sel, cross in MODES:
        for name, on_slots, _ in MATCHERS:
            idx, dist = on_slots(ctx, 2, 3, sel, cross)
            assert len(idx) == 0 and len(dist) == 0, (name, sel, cross)


@pytest.mark.parametrize("forced", [False, True])
def test_tiny_images(ctx, forced):
    """14 x 14 noise: SIFT keypoints of which none passes BRISK's border rule; 6 x 6: the smallest image that runs; 5 x 5 is refused"""
    tiny = tiny_image()
    other = make_ctx()
    try:
        ref = per_image(other, tiny)
        ref6 = per_image(other, tiny[:6, :6])
    finally:
        other.close()
    print("14 x 14: SIFT keypoints", len(ref["detected"]), "kept", ref["n"], "; 6 x 6:", len(ref6["detected"]), ref6["n"])
    assert len(ref["detected"]) > 0 and ref["n"] == 0 and ref6["n"] == 0
    capi.set_tuning("sift_brisk_recheck", int(forced))
    try:
        gl, gr = ctx.sift_brisk_pair(tiny, np.ascontiguousarray(tiny[::-1]), 0, 1)
        assert gl["n"] == 0 and gr["n"] == 0 and ctx.classic_slot_rows(0) == 0 and ctx.classic_slot_rows(1) == 0
        six = np.ascontiguousarray(tiny[:6, :6])
        gl, gr = ctx.sift_brisk_pair(six, six, 2, 3)
        assert gl["n"] == 0 and gr["n"] == 0 and ctx.classic_slot_rows(2) == 0
        five = np.ascontiguousarray(tiny[:5, :5])
        assert raw_pair(ctx, five, five, 4, 5) == (-1, 77, 77, True)
        assert raw_pair(ctx, np.ascontiguousarray(tiny[:5, :]), np.ascontiguousarray(tiny[:5, :]), 4, 5) == (-1, 77, 77, True)
        assert unfilled(ctx, 4) and ctx.classic_slot_rows(2) == 0
    finally:
        capi.set_tuning("sift_brisk_recheck", 0)


# ---------------------------------------------------------------- 5. matching and the slot protocol
def test_matching_in_the_slots(ctx, sample_images):
    L, R = pair("strided", sample_images)
    fl, fr = ctx.sift_brisk_pair(L, R, 6, 7)
    res = match_all(ctx, 6, 7, fl["desc"], fr["desc"])
    match_all(ctx, 7, 6, fr["desc"], fl["desc"])
    assert (res[("NN", False)][0][0] >= 0).all() and (res[("NN", True)][0][0] >= 0).any()


@pytest.mark.parametrize("matcher", ["hamming", "l2_u8"])
@pytest.mark.parametrize("mode", MODES)
def test_prematch_is_transparent(sample_images, matcher, mode):
    """two consecutive calls in ring order with spvo_set_prematch on and off, under either binary norm: identical results, the stereo match
    equals the synchronous match on the host copies and the temporal match the one against the call before's left rows"""
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
                fl, fr = c.sift_brisk_pair(L, R, 2 * k, 2 * k + 1)
                out += assert_match(c, 2 * k, 2 * k + 1, fl["desc"], fr["desc"], sel, cross, only=matcher)
                if k:
                    out += assert_match(c, 2 * k, 2 * k - 2, fl["desc"], prev["desc"], sel, cross, only=matcher)
                prev = fl
            res[on] = out
        finally:
            c.close()
    assert len(res[True]) == 3
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def test_prematch_temporal_partner_across_entry_points(sample_images):
    """a filled slot of 64-byte rows is a temporal partner, whichever call filled it: spvo_brisk_detect_pair's and spvo_orb_brisk_pair's of
    the new call, and the new call's of those; with the forced second pass the prematches are those of the final slot contents"""
    (L0, R0), (L1, R1) = same_shape_pairs(sample_images)
    c = make_ctx()
    try:
        c.set_prematch(True, "KNN", False, 0.8)

        def ok(sa, sb, fa, fb):
            assert_match(c, sa, sb, fa["desc"], fb["desc"], "KNN", False)

        bl, br_ = c.brisk_detect_pair(L0, R0, 0, 1)
        assert bl["desc"].shape[1] == 64 and len(bl["desc"]) > 10
        sl, sr = c.sift_brisk_pair(L1, R1, 2, 3)                       # partner: slot 0, BRISK + BRISK's
        ok(2, 3, sl, sr)
        ok(2, 0, sl, bl)
        ol, or_ = c.orb_brisk_pair(L0, R0, 4, 5)                       # partner: slot 2, SIFT + BRISK's
        ok(4, 5, ol, or_)
        ok(4, 2, ol, sl)
        capi.set_tuning("sift_brisk_recheck", 1)
        xl, xr = c.sift_brisk_pair(L1, R1, 6, 7)                       # partner: slot 4, ORB + BRISK's; both passes
        ok(6, 7, xl, xr)
        ok(6, 4, xl, ol)
        assert_same(xl, sl)
        capi.set_tuning("sift_brisk_recheck", 0)
        fo, fo_r = c.classic_detect(L0, R0, 8, 9, "FAST")              # 32-byte rows
        assert fo["desc"].shape[1] == 32
        yl, yr = c.sift_brisk_pair(L1, R1, 0, 1)                       # a 32-byte left slot before: skipped
        ok(0, 1, yl, yr)
        with pytest.raises(capi.SpvoError) as e:                       # asked for explicitly, the temporal match names the widths
            c.match_hamming_slots(0, 8, "KNN", False, 0.8)
        assert e.value.code == -1
    finally:
        capi.set_tuning("sift_brisk_recheck", 0)
        c.close()


def test_capacity(ctx, sample_images, reference):
    L, R = pair("crop", sample_images)
    rl, rr = reference["crop"]
    n_l, n_r = rl["n"], rr["n"]
    ctx.set_prematch(True, "KNN", False, 0.8)
    fl, fr = ctx.classic_detect(L, R, 4, 5, "ShiTomasi+BRISK", slot_capacity=4096)   # a sibling's slots, filled earlier
    assert 0 < len(fl["desc"]) <= 4096 and 0 < len(fr["desc"]) <= 4096
    with pytest.raises(capi.SpvoError) as e:                           # one below the larger count: both counts reported, nothing truncated
        ctx.sift_brisk_pair(L, R, 0, 1, slot_capacity=max(n_l, n_r) - 1)
    assert e.value.code == -5 and (e.value.n_l, e.value.n_r) == (n_l, n_r) == e.value.counts
    assert unfilled(ctx, 0) and unfilled(ctx, 1)                       # ... and both slots are unfilled afterwards
    with pytest.raises(capi.SpvoError) as e:
        ctx.match_hamming_slots(0, 1, "KNN", False, 0.8)
    assert e.value.code == -4
    assert ctx.classic_slot_rows(4) == len(fl["desc"]) and ctx.classic_slot_rows(5) == len(fr["desc"])   # no growth: the sibling's slots are as they were
    match_all(ctx, 4, 5, fl["desc"], fr["desc"])
    gl, gr = ctx.sift_brisk_pair(L, R, 0, 1, slot_capacity=max(n_l, n_r))   # at the count it runs
    assert_same(gl, rl)
    assert_same(gr, rr)
    match_all(ctx, 0, 1, gl["desc"], gr["desc"])
    assert ctx.classic_slot_rows(4) == len(fl["desc"])
    hl, hr = ctx.sift_brisk_pair(L, R, 2, 3, slot_capacity=8192)       # growth by a larger capacity than any before: every slot is emptied, the call runs
    assert_same(hl, rl)
    assert_same(hr, rr)
    assert unfilled(ctx, 0) and unfilled(ctx, 4)
    match_all(ctx, 2, 3, hl["desc"], hr["desc"])


def test_lists_of_a_small_first_call_serve_a_larger_image(sample_images, reference):
    """a fresh context whose first call is a small image, then the crop: the image, pyramid and BRISK buffers grow; the candidate lists
    hold 8192 rows from the first call on, which the crop does not exceed (the overflow and regrow is not reached)"""
    c = make_ctx()
    try:
        small = np.ascontiguousarray(sift_cases.image("noise"))
        gl, gr = c.sift_brisk_pair(small, np.ascontiguousarray(small[::-1]), 0, 1)
        assert gl["n"] > 0
        L, R = pair("crop", sample_images)
        hl, hr = c.sift_brisk_pair(L, R, 2, 3)
        assert_same(hl, reference["crop"][0])
        assert_same(hr, reference["crop"][1])
        assert c.classic_slot_rows(0) == gl["n"]
    finally:
        c.close()


# ---------------------------------------------------------------- 6. refusals and state
def raw_pair(c, L, R, slot_l, slot_r, slot_capacity=8192, cap=4, null_buffers=False):
    """the status of a pair call and what it left in the two feature structs' n (77 going in) and buffers (7.5 going in)"""
    kp = np.full(4 * 6, 7.5, np.float32)
    desc = np.full((4, 64), 7.5, np.float32)
    fl, fr = (capi.BriskFeatures(77, None if null_buffers else kp.ctypes.data, None if null_buffers else desc.ctypes.data, cap) for _ in range(2))
    rc = c.lib.spvo_sift_brisk_pair(c.h, L.ctypes.data, R.ctypes.data, L.shape[0], L.shape[1], L.strides[0], slot_l, slot_r, slot_capacity, C.byref(fl), C.byref(fr))
    return rc, fl.n, fr.n, bool((desc == 7.5).all() and (kp == 7.5).all())


def test_refusals_touch_nothing(sample_images, reference, squeeze_weights_path):
    frames, P_l, P_r = load_sequence()
    L, R = pair("crop", sample_images)
    rl, rr = reference["crop"]
    c = make_ctx(squeeze_weights_path)
    try:
        gl, gr = c.sift_brisk_pair(L, R, 0, 1)
        assert_same(gl, rl)
        big = np.zeros((2903, 2903), np.uint8)                         # what brisk_check_image refuses: 2903^2 * 255 >= 2^31 (refused before a byte is read)
        small = np.zeros((5, 40), np.uint8)                            # what spvo_sift_detect refuses
        refused = [raw_pair(c, L, R, 0, 0), raw_pair(c, L, R, 0, 10), raw_pair(c, L, R, -1, 1), raw_pair(c, L, R, 0, 1, slot_capacity=0),
                   raw_pair(c, L, R, 0, 1, slot_capacity=32769), raw_pair(c, L, R, 0, 1, slot_capacity=-5), raw_pair(c, L, R, 0, 1, cap=-1),
                   raw_pair(c, big, big, 0, 1), raw_pair(c, small, small, 0, 1)]
        for r in refused:
            assert r == (-1, 77, 77, True), refused
        f = capi.BriskFeatures(77, None, None, 0)
        lib, args = c.lib, (L.shape[0], L.shape[1], L.strides[0], 0, 1, 8192)
        assert lib.spvo_sift_brisk_pair(c.h, None, R.ctypes.data, *args, C.byref(f), C.byref(f)) == -1        # NULL arguments
        assert lib.spvo_sift_brisk_pair(c.h, L.ctypes.data, None, *args, C.byref(f), C.byref(f)) == -1
        assert lib.spvo_sift_brisk_pair(c.h, L.ctypes.data, R.ctypes.data, *args, None, C.byref(f)) == -1
        assert lib.spvo_sift_brisk_pair(c.h, L.ctypes.data, R.ctypes.data, *args, C.byref(f), None) == -1 and f.n == 77
        # nothing was touched: the slots and the resident image are as before
        assert c.classic_slot_rows(0) == rl["n"] and c.classic_slot_rows(1) == rr["n"]
        match_all(c, 0, 1, gl["desc"], gr["desc"])
        det = rr["detected"]
        xy = np.stack([det["x"], det["y"]], 1)
        assert c.brisk_describe(None, xy, det["size"], shape=R.shape)["desc"].tobytes() == rr["desc"].tobytes()
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)              # a SuperPoint submission in flight
        assert raw_pair(c, L, R, 0, 1) == (-4, 77, 77, True)
        c.detect_collect(P_l, P_r)
        assert c.classic_slot_rows(0) == rl["n"] and c.classic_slot_rows(1) == rr["n"]
        match_all(c, 0, 1, gl["desc"], gr["desc"])
        nl, nr = c.sift_brisk_pair(L, R, 4, 5)
        assert_same(nl, rl)
        assert_same(nr, rr)
    finally:
        c.close()


@pytest.mark.parametrize("forced", [False, True])
def test_the_right_image_is_resident_afterwards(ctx, sample_images, reference, forced):
    L, R = pair("strided", sample_images)
    rr = reference["strided"][1]
    det = rr["detected"]
    bl = ctx.brisk_detect(np.ascontiguousarray(L))                     # a BRISK detector result and its debug layers, resident before
    rows, cols = ctx.brisk_detect_layer(0, 0).shape
    assert (rows, cols) == L.shape and bl["n"] > 0
    capi.set_tuning("sift_brisk_recheck", int(forced))
    try:
        gl, gr = ctx.sift_brisk_pair(L, R, 0, 1)
    finally:
        capi.set_tuning("sift_brisk_recheck", 0)
    assert_same(gr, rr)
    with pytest.raises(capi.SpvoError) as e:                           # spvo_brisk_detect_debug_layer: no detector result belongs to the resident image
        ctx.brisk_detect_layer(0, 0)
    assert e.value.code == -4
    b = ctx.brisk_describe(None, np.stack([det["x"], det["y"]], 1), det["size"], shape=R.shape)
    assert b["desc"].tobytes() == rr["desc"].tobytes() and np.array_equal(b["kept"], rr["kept"]) and b["angle"].tobytes() == rr["kp"]["angle"].tobytes()
    other = make_ctx()
    try:
        want = other.sift_describe(np.ascontiguousarray(R), det)
    finally:
        other.close()
    assert ctx.sift_describe(None, det, shape=R.shape).tobytes() == want.tobytes()


# ---------------------------------------------------------------- 7. the host class
N_HOST = 3


def _run(frames, P_l, P_r, matcher="BF", **kw):
    return host.classic_sequence(frames, P_l, P_r, "KNN", matcher == "BF", 2.0, 4, input_size=(120, 392), trace=True, detector="SIFT", descriptor="BRISK", matcher=matcher, **kw)


@pytest.fixture(scope="module")
def per_image_runs():
    """the runs with setDeviceResident off, shared and left unchanged: matcher -> (poses, stats, seconds, digests)"""
    frames, P_l, P_r = load_sequence()
    frames = frames[:N_HOST]
    out = {}
    for matcher in ("BF", "FLANN"):
        out[matcher] = _run(frames, P_l, P_r, matcher, sift_brisk=True)
        assert host.classic_resident_pairs() == 0
    return (frames, P_l, P_r), out


def test_host_class_per_image_holds_aligned_brisk_rows_on_sift_keypoints(per_image_runs, sample_images):
    """with setSiftBriskExtractor the deques hold SIFT keypoints that passed BRISK's rule and as many 64-byte CV_8UC1 rows"""
    (frames, P_l, P_r), runs = per_image_runs
    _, stats, _, _ = runs["BF"]
    print("keypoints", stats[:, 0].tolist(), stats[:, 1].tolist(), "stereo matches", stats[:, 2].tolist(), "inliers", stats[:, 3].tolist())
    assert stats[:, :2].min() > 50 and stats[1:, 2].min() > 10 and stats[1:, 3].min() > 5
    L, R = pair("kitti", sample_images)
    n, counts, err = host.classic_pair_probe("SIFT", "BRISK", L, R, P_l, P_r, sift_brisk=True)
    c = make_ctx()
    try:
        rl, rr = per_image(c, L), per_image(c, R)
    finally:
        c.close()
    print("probe", n, counts.tolist(), err)
    assert err == "" and counts[:5].tolist() == [rl["n"], rl["n"], rr["n"], rr["n"], 64]
    assert 0 < rl["n"] < len(rl["detected"])                           # keypoints that fail the border rule are erased from the deque entry


def test_sift_brisk_without_its_switch_is_refused(per_image_runs, sample_images):
    (frames, P_l, P_r), _ = per_image_runs
    L, R = pair("kitti", sample_images)
    n, counts, err = host.classic_pair_probe("SIFT", "BRISK", L, R, P_l, P_r)
    assert n == 0 and not counts[:4].any() and "OpenCV features2d call" in err and "SIFT + BRISK" not in err and "SIFT + SIFT" in err
    with pytest.raises(RuntimeError):
        _run(frames[:2], P_l, P_r)
    with pytest.raises(RuntimeError):                                  # ... whatever resident switch is on
        _run(frames[:2], P_l, P_r, resident=True, sift_brisk_resident=True)


def test_sift_sift_is_unchanged_by_the_switch(per_image_runs):
    """the Detect::Sift case allocates SIFT's own 128-float rows whatever the pair: SIFT + SIFT gives the same bytes with and without
    setSiftBriskExtractor, per image and resident"""
    (frames, P_l, P_r), _ = per_image_runs
    run = lambda **kw: host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, input_size=(120, 392), trace=True, detector="SIFT", **kw)
    p0, s0, _, d0 = run()
    for kw in (dict(sift_brisk=True), dict(sift_brisk=True, sift_brisk_resident=True, resident=True), dict(resident=True)):
        p1, s1, _, d1 = run(**kw)
        assert host.classic_resident_pairs() == (N_HOST if kw.get("resident") else 0)
        assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1), kw
    assert s0[:, :2].min() > 50


@pytest.mark.parametrize("matcher", ["BF", "FLANN"])
def test_host_class_every_combination_of_the_switches(per_image_runs, matcher):
    """ClassicFeatureFrontEnd over three frames at 120 x 392: keypoints_dq, descriptors_dq, the three match lists, the inlier sets (digests
    of their full contents) and every pose are identical whatever setDeviceResident and setSiftBriskResident say; the pair stays resident
    only with both (and setSiftBriskExtractor, without which it is refused); no earlier resident switch takes the route"""
    (frames, P_l, P_r), runs = per_image_runs
    p0, s0, _, d0 = runs[matcher]
    for resident in (False, True):
        for sb_resident in (False, True):
            p1, s1, _, d1 = _run(frames, P_l, P_r, matcher, sift_brisk=True, resident=resident, sift_brisk_resident=sb_resident)
            assert host.classic_resident_pairs() == (N_HOST if resident and sb_resident else 0), (resident, sb_resident)
            assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1), (resident, sb_resident)
            with pytest.raises(RuntimeError):                          # the same combination without setSiftBriskExtractor
                _run(frames[:1], P_l, P_r, matcher, resident=resident, sift_brisk_resident=sb_resident)
    earlier = dict(brisk_resident=True, akaze_resident=True, sift_describe_resident=True, octave_pairs_resident=True, sift_octave_pairs_resident=True, orb_pairs_resident=True)
    p2, s2, _, d2 = _run(frames, P_l, P_r, matcher, sift_brisk=True, resident=True, **earlier)
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d2) and np.array_equal(s0, s2) and np.array_equal(p0, p2)


def test_host_class_ring_wraps_and_mixes_fallen_back_pairs():
    """six frames (the ring of four slot pairs wraps once), then slots of the median row count: some pairs fit, some take the per-image
    path and are matched from the host matrices, and the run is still identical"""
    frames, P_l, P_r = load_sequence()
    p0, s0, _, d0 = _run(frames, P_l, P_r, sift_brisk=True)
    p1, s1, _, d1 = _run(frames, P_l, P_r, sift_brisk=True, resident=True, sift_brisk_resident=True)
    assert host.classic_resident_pairs() == 6 == len(frames)
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
    cap = int(np.median(s0[:, :2]))
    p2, s2, _, d2 = _run(frames, P_l, P_r, sift_brisk=True, resident=True, sift_brisk_resident=True, resident_capacity=cap)
    print("rows", s0[:, :2].tolist(), "capacity", cap, "resident pairs", host.classic_resident_pairs())
    assert 0 < host.classic_resident_pairs() < 6
    assert np.array_equal(d0, d2) and np.array_equal(s0, s2) and np.array_equal(p0, p2)
