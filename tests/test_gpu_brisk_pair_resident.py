"""BRISK + BRISK with a stereo pair's features resident on the device (spvo_brisk_detect_pair into the binary slots, the 64-byte
instantiation of the slot matcher, ClassicFeatureFrontEnd::setBriskPairResident): everything equals the per-image entry points
(spvo_brisk_detect followed by spvo_brisk_describe(img = NULL) with the detector's x, y and size) and spvo_match_hamming on the same device
EXACTLY -- counts, the 24-byte keypoint records and the 64-byte rows as raw bytes, match indices and distances, and through the host class
every deque entry, match list, inlier set and pose.  That path is held to tests/brisk_detect_ref.py and tests/brisk_ref.py by
tests/test_gpu_brisk_detect.py and tests/test_gpu_brisk.py.  No tolerance, no row excused.  The counts named below are the restatements'."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import capi, host, synth
from tests import brisk_detect_cases as bc, brisk_ref as br
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu

MODES = [("NN", False), ("NN", True), ("KNN", False)]          # NN, NN with cross-check, KNN at 0.8
PAIRS = ["inexact", "exact", "blobs", "border", "ties", "golden", "strided"]
# detected / kept per image, from tests/brisk_detect_ref.py and tests/brisk_ref.py's border rule
COUNTS = {"inexact": ((1170, 506), (1173, 512)), "exact": ((1222, 538), (1207, 539)), "blobs": ((22, 12), (21, 11)), "border": ((708, 117), (708, 117))}


def pair(name, sample_images):
    """-> (left, right, threshold)"""
    if name == "golden":                        # full size, about 3100 keypoints each
        return sample_images[0], sample_images[1], 30
    if name == "strided":                       # rows are not contiguous
        return sample_images[1][3:203, 5:405], sample_images[2][3:203, 5:405], 30
    img, thr = bc.case(name)
    if name in ("inexact", "blobs"):
        return img, np.ascontiguousarray(img[:, ::-1]), thr
    if name == "exact":
        return img, bc.smoothed_noise((96, 144), 41), thr
    return img, img, thr


def per_image(ctx, img, thr):
    """what spvo_brisk_detect followed by spvo_brisk_describe(img = NULL) returns for one image, as the records and rows
    spvo_brisk_detect_pair promises; n_det: the detector's count"""
    det = ctx.brisk_detect(img, thr)
    kp = det["kp"]
    assert len(kp) == det["n"]
    d = ctx.brisk_describe(None, np.stack([kp["x"], kp["y"]], 1).reshape(-1, 2), kp["size"], shape=img.shape)
    rec = kp[d["kept"]].copy()
    rec["angle"] = d["angle"]
    return dict(kp=rec, desc=d["desc"], n=len(rec), n_det=det["n"])


def assert_same(got, ref):
    assert got["n"] == ref["n"] == len(got["kp"]) == len(got["desc"])
    assert got["kp"].dtype == capi.BRISK_KP_DTYPE and got["kp"].dtype.itemsize == 24 and got["desc"].shape == (ref["n"], 64)
    if got["kp"].tobytes() != ref["kp"].tobytes():
        for f in capi.BRISK_KP_DTYPE.names:
            bad = np.nonzero(got["kp"][f].view(np.uint32) != ref["kp"][f].view(np.uint32))[0]
            if len(bad):
                print("  field", f, ":", len(bad), "rows differ, first", int(bad[0]), got["kp"][bad[0]], ref["kp"][bad[0]])
    assert got["kp"].tobytes() == ref["kp"].tobytes()
    assert got["desc"].tobytes() == ref["desc"].tobytes(), "%d rows differ" % int((got["desc"] != ref["desc"]).any(1).sum())


def match_all(ctx, sa, sb, da, db):
    """the three modes on slots sa -> sb: equal to spvo_match_hamming on the host copies, index for index and distance for distance"""
    out = {}
    for sel, cross in MODES:
        gi, gd = ctx.match_hamming_slots(sa, sb, sel, cross, 0.8)
        hi, hd = ctx.match_hamming(da, db, sel, cross, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd), (sel, cross)
        out[(sel, cross)] = (gi, gd)
    return out


@pytest.fixture()
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference(sample_images):
    """the per-image sequence of every pair, computed once in a context of its own and left unchanged: name -> (left, right)"""
    c = make_ctx()
    out = {}
    for name in PAIRS:
        L, R, thr = pair(name, sample_images)
        out[name] = (per_image(c, L, thr), per_image(c, R, thr))
    c.close()
    return out


# ---------------------------------------------------------------- 1. byte equality with the per-image entry points
@pytest.mark.parametrize("name", PAIRS)
def test_pair_equals_the_per_image_entry_points(ctx, sample_images, reference, name):
    L, R, thr = pair(name, sample_images)
    gl, gr = ctx.brisk_detect_pair(L, R, 2, 3, thr)
    rl, rr = reference[name]
    print(name, L.shape, "threshold", thr, "detected", rl["n_det"], rr["n_det"], "kept", rl["n"], rr["n"], "pair", gl["n"], gr["n"])
    assert_same(gl, rl)
    assert_same(gr, rr)
    assert ctx.classic_slot_rows(2) == rl["n"] and ctx.classic_slot_rows(3) == rr["n"]
    assert rl["n"] > 0 and rr["n"] > 0
    assert np.all((gl["kp"]["angle"] >= 0) & (gl["kp"]["angle"] <= 360))          # the extractor's angle, not the detector's -1
    if name in COUNTS:
        assert ((rl["n_det"], rl["n"]), (rr["n_det"], rr["n"])) == COUNTS[name]
    if name == "inexact":
        assert rl["n_det"] > 1024 and rr["n_det"] > 1024                          # the compaction crosses a chunk
    if name == "exact":
        assert gl["kp"].tobytes() != gr["kp"].tobytes()                           # left and right differ: a swapped or shared buffer shows
    if name == "blobs":                                                            # every keypoint's own scale index, above 0 on every layer
        s = br.scale_index(gl["kp"]["size"])
        assert s.min() > 0 and len(set(s.tolist())) >= 4
        assert sorted(set(gl["kp"]["octave"].tolist())) == [0, 1, 3, 4, 5]
    if name == "border":
        assert rl["n"] * 4 < rl["n_det"]                                           # most are removed by the border rule
    if name == "golden":
        assert rl["n"] > 2000 and rr["n"] > 2000
    if name == "strided":
        assert not L.flags["C_CONTIGUOUS"]
        pl, pr = ctx.brisk_detect_pair(np.ascontiguousarray(L), np.ascontiguousarray(R), 4, 5, thr)
        assert_same(pl, rl)
        assert_same(pr, rr)


def test_host_buffer_smaller_than_the_slot(ctx, sample_images, reference):
    """cap < n: n is reported, exactly cap leading rows are written, the slot holds all of them"""
    L, R, thr = pair("exact", sample_images)
    rl, rr = reference["exact"]
    gl, gr = ctx.brisk_detect_pair(L, R, 0, 1, thr, cap=100)
    assert gl["n"] == rl["n"] and gr["n"] == rr["n"] and len(gl["kp"]) == len(gr["desc"]) == 100
    assert gl["kp"].tobytes() == rl["kp"][:100].tobytes() and gr["desc"].tobytes() == rr["desc"][:100].tobytes()
    assert ctx.classic_slot_rows(0) == rl["n"]
    match_all(ctx, 0, 1, rl["desc"], rr["desc"])


# ---------------------------------------------------------------- 2. empty results
def test_empty_results(ctx, sample_images, reference):
    """47 detected and 0 kept (the border is 13 pixels at scale index 0 and the image 24 x 32), and a flat image with nothing detected: the
    slots are filled with 0 rows, matching treats them as spvo_match_hamming_slots documents, a following pair is unaffected"""
    L, R, thr = pair("exact", sample_images)
    rl, rr = reference["exact"]
    fl, fr = ctx.brisk_detect_pair(L, R, 0, 1, thr)
    small = bc.smoothed_noise((24, 32), 31)
    ref = per_image(ctx, small, 12)
    assert (ref["n_det"], ref["n"]) == (47, 0)
    flat = np.full((24, 32), 77, np.uint8)
    assert per_image(ctx, flat, 12)["n_det"] == 0
    el, er = ctx.brisk_detect_pair(small, flat, 2, 3, 12)
    for e in (el, er):
        assert e["n"] == 0 and e["kp"].shape == (0,) and e["desc"].shape == (0, 64)
    assert ctx.classic_slot_rows(2) == 0 and ctx.classic_slot_rows(3) == 0
    assert ctx.classic_slot_rows(0) == rl["n"] and ctx.classic_slot_rows(1) == rr["n"]          # the other slots keep what they hold
    res = match_all(ctx, 0, 2, fl["desc"], el["desc"])                                          # empty train set: every row -1
    assert all(np.all(i == -1) and len(i) == rl["n"] for i, _ in res.values())
    res = match_all(ctx, 2, 0, el["desc"], fl["desc"])                                          # empty query set
    assert all(len(i) == 0 for i, _ in res.values())
    match_all(ctx, 2, 3, el["desc"], er["desc"])
    nl, nr = ctx.brisk_detect_pair(L, R, 4, 5, thr)                                              # a following non-empty pair
    assert_same(nl, rl)
    assert_same(nr, rr)
    match_all(ctx, 4, 5, nl["desc"], nr["desc"])


# ---------------------------------------------------------------- 3. matching
@pytest.mark.parametrize("name", ["inexact", "golden"])
def test_matching_in_the_slots(ctx, sample_images, name):
    """506 x 512 rows (two tiles of 256 a side, neither full) and about 3100 x 3100"""
    L, R, thr = pair(name, sample_images)
    fl, fr = ctx.brisk_detect_pair(L, R, 6, 7, thr)
    res = match_all(ctx, 6, 7, fl["desc"], fr["desc"])
    match_all(ctx, 7, 6, fr["desc"], fl["desc"])
    assert (res[("NN", False)][0] >= 0).all() and (res[("NN", True)][0] >= 0).any()
    if name == "golden":
        assert (res[("KNN", False)][0] >= 0).sum() > 100


# ---------------------------------------------------------------- 4. prematch
@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(3, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def crops(sequence, k):
    """a 200 x 400 part of frame k: several hundred rows a side"""
    return tuple(np.ascontiguousarray(im[100:300, 300:700]) for im in sequence[0][k])


@pytest.mark.parametrize("mode", MODES)
def test_prematch_is_transparent(sequence, mode):
    """three consecutive calls in ring order with spvo_set_prematch on and off: identical results, the stereo match equals the synchronous
    match on the host copies and the temporal match of call k the one against call k - 1's left rows; a slot rewritten between detect and
    match is not served from the stored result"""
    sel, cross = mode
    res = {}
    for on in (False, True):
        c = make_ctx()
        try:
            c.set_prematch(on, sel, cross, 0.8)
            out = []
            for k in range(3):
                L, R = crops(sequence, k)
                fl, fr = c.brisk_detect_pair(L, R, 2 * k, 2 * k + 1)
                assert fl["n"] > 256
                out.append(c.match_hamming_slots(2 * k, 2 * k + 1, sel, cross, 0.8))
                hi, hd = c.match_hamming(fl["desc"], fr["desc"], sel, cross, 0.8)
                assert np.array_equal(out[-1][0], hi) and np.array_equal(out[-1][1], hd)
                if k:
                    out.append(c.match_hamming_slots(2 * k, 2 * k - 2, sel, cross, 0.8))
                    hi, hd = c.match_hamming(fl["desc"], prev["desc"], sel, cross, 0.8)
                    assert np.array_equal(out[-1][0], hi) and np.array_equal(out[-1][1], hd)
                    assert (hi >= 0).sum() > 10
                prev = fl
            L0, R0 = crops(sequence, 0)
            _, nr = c.brisk_detect_pair(R0, L0, 8, 5)                   # rewrite the right slot of the last pair: the stored stereo match is stale
            gi, gd = c.match_hamming_slots(4, 5, sel, cross, 0.8)
            hi, hd = c.match_hamming(fl["desc"], nr["desc"], sel, cross, 0.8)
            assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
            assert not (np.array_equal(gi, out[-2][0]) and np.array_equal(gd, out[-2][1]))
            res[on] = out
        finally:
            c.close()
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_prematch_temporal_partner_across_entry_points(sequence):
    """after a spvo_classic_detect call of 32-byte rows the next pair call has no temporal partner and does not fail; after one of 64-byte
    rows (FAST + BRISK) it has one, and the stored temporal match is the synchronous one"""
    c = make_ctx()
    try:
        c.set_prematch(True, "KNN", False, 0.8)
        L0, R0 = crops(sequence, 0)
        L1, R1 = crops(sequence, 1)
        L2, R2 = crops(sequence, 2)
        ol, orr = c.classic_detect(L0, R0, 0, 1, "ORB")
        bl, br_ = c.brisk_detect_pair(L1, R1, 2, 3)
        gi, gd = c.match_hamming_slots(2, 3, "KNN", False, 0.8)
        hi, hd = c.match_hamming(bl["desc"], br_["desc"], "KNN", False, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd) and (gi >= 0).sum() > 10
        with pytest.raises(capi.SpvoError) as e:                       # asked for explicitly, the temporal match names the widths
            c.match_hamming_slots(2, 0, "KNN", False, 0.8)
        assert e.value.code == -1
        gi, gd = c.match_hamming_slots(0, 1, "KNN", False, 0.8)        # the ORB rows are still there
        hi, hd = c.match_hamming(ol["desc"], orr["desc"], "KNN", False, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
        fl, _ = c.classic_detect(L0, R0, 4, 5, "FAST+BRISK")
        assert fl["desc"].shape[1] == 64 and len(fl["desc"]) > 10
        nl, nr = c.brisk_detect_pair(L2, R2, 6, 7)                     # ... and this call has a temporal partner: slot 4
        ti, td = c.match_hamming_slots(6, 4, "KNN", False, 0.8)
        hi, hd = c.match_hamming(nl["desc"], fl["desc"], "KNN", False, 0.8)
        assert np.array_equal(ti, hi) and np.array_equal(td, hd) and len(ti) == nl["n"]
        ql, _ = c.classic_detect(L1, R1, 8, 9, "FAST+BRISK")           # and the other way round: a BRISK pair's left slot serves spvo_classic_detect
        ti, td = c.match_hamming_slots(8, 6, "KNN", False, 0.8)
        hi, hd = c.match_hamming(ql["desc"], nl["desc"], "KNN", False, 0.8)
        assert np.array_equal(ti, hi) and np.array_equal(td, hd)
    finally:
        c.close()


# ---------------------------------------------------------------- 5. capacity
def test_capacity(ctx, sample_images, reference):
    L, R, thr = pair("exact", sample_images)
    rl, rr = reference["exact"]
    n_l, n_r = rl["n"], rr["n"]
    crop_l, crop_r = sample_images[0][100:164, 300:396], sample_images[1][100:164, 300:396]
    cap = max(n_l, n_r)
    ol, orr = ctx.classic_detect(crop_l, crop_r, 6, 7, "FAST", slot_capacity=cap)
    fl, fr = ctx.classic_detect(crop_l, crop_r, 8, 9, "FAST+BRISK", slot_capacity=cap)
    ctx.set_prematch(True, "KNN", False, 0.8)
    with pytest.raises(capi.SpvoError) as e:                           # one row short of the larger image: reported, nothing truncated
        ctx.brisk_detect_pair(L, R, 0, 1, thr, slot_capacity=cap - 1)
    assert e.value.code == -5 and (e.value.n_l, e.value.n_r) == (n_l, n_r) == e.value.counts
    for s in (0, 1):
        with pytest.raises(capi.SpvoError) as e:                       # ... and both slots are unfilled afterwards
            ctx.classic_slot_rows(s)
        assert e.value.code == -4
    with pytest.raises(capi.SpvoError) as e:                           # (the call's prematch results are dropped with them)
        ctx.match_hamming_slots(0, 1)
    assert e.value.code == -4
    gl, gr = ctx.brisk_detect_pair(L, R, 0, 1, thr, slot_capacity=cap)
    assert_same(gl, rl)
    assert_same(gr, rr)
    match_all(ctx, 0, 1, gl["desc"], gr["desc"])
    # slots filled by spvo_classic_detect in other slot numbers, at the same capacity, keep their rows
    assert ctx.classic_slot_rows(6) == len(ol["xy"]) and ctx.classic_slot_rows(9) == len(fr["xy"])
    gi, gd = ctx.match_hamming_slots(6, 7, "NN", True, 0.8)
    hi, hd = ctx.match_hamming(ol["desc"], orr["desc"], "NN", True, 0.8)
    assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
    match_all(ctx, 8, 9, fl["desc"], fr["desc"])
    gl2, _ = ctx.brisk_detect_pair(L, R, 2, 3, thr, slot_capacity=cap + 1)      # a larger capacity than any before empties every slot
    assert_same(gl2, rl)
    for s in (0, 6, 8):
        with pytest.raises(capi.SpvoError) as e:
            ctx.classic_slot_rows(s)
        assert e.value.code == -4


# ---------------------------------------------------------------- 6. statuses
def test_status_codes(sample_images, reference, squeeze_weights_path, sequence):
    frames, _, P_l, P_r = sequence
    L, R, thr = pair("exact", sample_images)
    rl, rr = reference["exact"]
    c = make_ctx(squeeze_weights_path)
    try:
        lib, by = c.lib, capi.C.byref
        gl, gr = c.brisk_detect_pair(L, R, 0, 1, thr)
        assert_same(gl, rl)

        def call(ctx_h=c.h, l=L.ctypes.data, r=R.ctypes.data, rows=L.shape[0], cols=L.shape[1], stride=L.strides[0], threshold=thr, octaves=3, sl=2, sr=3, slot_capacity=8192, cap=0,
                 null_out=False):
            fl, fr = capi.BriskFeatures(0, None, None, cap), capi.BriskFeatures(0, None, None, cap)
            return lib.spvo_brisk_detect_pair(ctx_h, l, r, rows, cols, stride, threshold, octaves, sl, sr, slot_capacity, None if null_out else by(fl), by(fr))

        assert call() == 0 and c.classic_slot_rows(2) == rl["n"]        # (kp, desc may be NULL: the slots are filled all the same)
        bad = [dict(l=None), dict(r=None), dict(null_out=True), dict(cap=-1), dict(sl=0, sr=0), dict(sl=-1, sr=1), dict(sl=0, sr=10), dict(slot_capacity=0), dict(slot_capacity=-3),
               dict(slot_capacity=(1 << 22) + 1), dict(threshold=0), dict(threshold=256), dict(octaves=2), dict(octaves=4), dict(rows=7), dict(cols=7),
               dict(rows=2903, cols=2901, stride=2901), dict(rows=65536, cols=65536, stride=65536), dict(stride=L.shape[1] - 1)]
        for kw in bad:
            assert call(**kw) == -1, kw
        assert call(ctx_h=None) == -1
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)             # a SuperPoint submission in flight
        with pytest.raises(capi.SpvoError) as e:
            c.brisk_detect_pair(L, R, 4, 5, thr)
        assert e.value.code == -4
        c.detect_collect(P_l, P_r)
        # the refused calls touched nothing: the slots hold what they held, and a valid call returns the bytes of test 1
        assert c.classic_slot_rows(0) == rl["n"] and c.classic_slot_rows(1) == rr["n"] and c.classic_slot_rows(2) == rl["n"]
        with pytest.raises(capi.SpvoError) as e:
            c.classic_slot_rows(4)
        assert e.value.code == -4
        match_all(c, 0, 1, gl["desc"], gr["desc"])
        nl, nr = c.brisk_detect_pair(L, R, 4, 5, thr)
        assert_same(nl, rl)
        assert_same(nr, rr)
    finally:
        c.close()


# ---------------------------------------------------------------- 7. neighbours unharmed
def test_neighbours_are_unharmed(sample_images, reference):
    img, thr = bc.case("inexact")
    L, R, pthr = pair("exact", sample_images)                          # another shape than `img`
    crop_l, crop_r = sample_images[0][100:164, 300:396], sample_images[1][100:164, 300:396]
    kinds = ["ORB", "ShiTomasi", "FAST", "ShiTomasi+BRISK", "FAST+BRISK"]            # spvo_classic_kind 0 .. 4
    c = make_ctx()
    try:
        before = c.brisk_detect(img, thr)["kp"]
        assert np.array_equal(c.brisk_detect_layer(0, 0), img)
        classic_before = [c.classic_detect(crop_l, crop_r, 6, 7, k) for k in kinds]
        gl, gr = c.brisk_detect_pair(L, R, 0, 1, pthr)
        assert_same(gr, reference["exact"][1])
        for layer, what in ((0, 0), (3, 1), (0, 2)):                   # the detector's maps are the pair's right image's: not served
            with pytest.raises(capi.SpvoError) as e:
                c.brisk_detect_layer(layer, what)
            assert e.value.code == -4
        # spvo_brisk_describe(img = NULL) after the pair call works on the RIGHT image (include/spvo.h)
        rr = reference["exact"][1]
        d = c.brisk_describe(None, np.stack([rr["kp"]["x"], rr["kp"]["y"]], 1), rr["kp"]["size"], shape=R.shape)
        assert np.array_equal(d["kept"], np.arange(rr["n"])) and d["desc"].tobytes() == rr["desc"].tobytes() and d["angle"].tobytes() == rr["kp"]["angle"].tobytes()
        up = c.brisk_describe(R, np.stack([rr["kp"]["x"], rr["kp"]["y"]], 1), rr["kp"]["size"])
        assert up["desc"].tobytes() == d["desc"].tobytes()
        with pytest.raises(capi.SpvoError) as e:                       # ... and on no other shape
            c.brisk_describe(None, np.zeros((1, 2), np.float32), 12.0, shape=img.shape)
        assert e.value.code == -4
        c.brisk_detect_pair(L, R, 2, 3, pthr)
        after = c.brisk_detect(img, thr)["kp"]
        assert len(before) == 1170 and before.tobytes() == after.tobytes() == bc.reference("inexact")[1].tobytes()
        assert np.array_equal(c.brisk_detect_layer(0, 0), img)
        c.brisk_detect_pair(L, R, 2, 3, pthr)
        for k, (bl, br_) in zip(kinds, classic_before):
            al, ar = c.classic_detect(crop_l, crop_r, 8, 9, k)
            for a, b in ((al, bl), (ar, br_)):
                for f in ("xy", "angle", "response", "octave", "desc"):
                    assert a[f].tobytes() == b[f].tobytes(), (k, f)
        assert c.classic_slot_rows(2) == gl["n"]                       # the pair's slots outlive the classic calls in other slots
    finally:
        c.close()


# ---------------------------------------------------------------- 8. repeatability
def test_same_bytes_twice_after_another_shape_and_in_a_fresh_context(sample_images, reference):
    L, R, thr = pair("ties", sample_images)
    rl, rr = reference["ties"]
    a = make_ctx()
    first = a.brisk_detect_pair(L, R, 0, 1, thr)
    second = a.brisk_detect_pair(L, R, 0, 1, thr)
    a.brisk_detect_pair(sample_images[0], sample_images[1], 2, 3, 30)              # a larger shape: every buffer grows
    a.brisk_detect_pair(*pair("inexact", sample_images)[:2], 4, 5, 12)              # ... and a smaller one
    third = a.brisk_detect_pair(L, R, 6, 7, thr)
    a.close()
    b = make_ctx()
    fresh = b.brisk_detect_pair(L, R, 8, 9, thr)
    b.close()
    assert rl["n"] > 100
    for got in (first, second, third, fresh):
        assert_same(got[0], rl)
        assert_same(got[1], rr)


# ---------------------------------------------------------------- 9. the host class
def _run(frames, P_l, P_r, **kw):
    return host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="BRISK", descriptor="BRISK", input_size=(120, 392), trace=True, **kw)


@pytest.fixture(scope="module")
def per_image_run(sequence):
    """the run with setDeviceResident off, shared and left unchanged"""
    frames, _, P_l, P_r = sequence
    out = _run(frames, P_l, P_r)
    assert host.classic_resident_pairs() == 0
    return out


def test_host_class_is_identical_with_resident_features(sequence, per_image_run):
    """ClassicFeatureFrontEnd(BRISK, BRISK) over three synthetic frames at 120 x 392: keypoints_dq, descriptors_dq, the three match lists,
    the inlier sets (digests of their full contents) and every pose are identical with both switches on, and every pair stayed resident;
    with the new switch off (the keyword's default) the pair takes the per-image path as before"""
    frames, _, P_l, P_r = sequence
    p0, s0, _, d0 = per_image_run
    p1, s1, _, d1 = _run(frames, P_l, P_r, resident=True, brisk_resident=True)
    assert host.classic_resident_pairs() == 3 == len(frames)
    assert s0[:, 0].min() > 100 and s0[1:, 3].max() > 10
    assert np.array_equal(d0, d1)
    assert np.array_equal(s0, s1)
    assert np.array_equal(p0, p1)
    p2, s2, _, d2 = _run(frames, P_l, P_r, resident=True)
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d2) and np.array_equal(s0, s2) and np.array_equal(p0, p2)
    p3, s3, _, d3 = _run(frames, P_l, P_r, brisk_resident=True)                     # the new switch alone changes nothing
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d3) and np.array_equal(s0, s3) and np.array_equal(p0, p3)


def test_host_class_falls_back_when_a_pair_does_not_fit(sequence, per_image_run):
    """slots that hold the median pair's rows: the larger pairs take the per-image path and are matched from the host matrices, the others
    stay resident, and the run is still identical"""
    frames, _, P_l, P_r = sequence
    p0, s0, _, d0 = per_image_run
    rows = np.sort(np.maximum(s0[:, 0], s0[:, 1]))
    cap = int(rows[len(rows) // 2])
    assert rows[0] <= cap < rows[-1]
    p1, s1, _, d1 = _run(frames, P_l, P_r, resident=True, brisk_resident=True, resident_capacity=cap)
    assert 0 < host.classic_resident_pairs() < 3
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
