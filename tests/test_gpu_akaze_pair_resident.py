"""AKAZE + AKAZE with a stereo pair's features resident on the device (spvo_akaze_detect_pair into the binary slots as 61-byte rows, the
16-word instantiation of the slot matcher, ClassicFeatureFrontEnd::setAkazePairResident): everything equals the per-image entry points
(spvo_akaze_detect followed by spvo_akaze_describe(img = NULL)) and spvo_match_hamming(desc_bytes = 61) on the same device EXACTLY --
counts, the 28-byte keypoint records and the 61-byte rows as raw bytes, match indices and distances, and through the host class every
deque entry, match list, inlier set and pose.  That path is held to tests/akaze_ref.py and tests/akaze_mldb_ref.py by
tests/test_gpu_akaze.py and tests/test_gpu_akaze_mldb.py.  The device suppression alone (spvo_akaze_suppress_debug) is held to the flat
restatement of rule 11 in tests/akaze_suppress_cases.py, index for index, on lists that reach the branches no image reaches.  No
tolerance, no row excused."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import capi, host, synth
from tests import akaze_cases as ac, akaze_suppress_cases as sc
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu

MODES = [("NN", False), ("NN", True), ("KNN", False)]          # NN, NN with cross-check, KNN at 0.8
PAIRS = ac.CASES + ["frame", "full_size"]


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(3, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def pair(name, sample_images, sequence):
    """-> (left, right): two different images of one shape"""
    if name == "full_size":
        return np.ascontiguousarray(sample_images[0]), np.ascontiguousarray(sample_images[1])
    if name == "frame":                         # a synthetic frame of the host-class test, at its 120 x 392
        l, r = sequence[0][0]
        return np.ascontiguousarray(l[100:220, 300:692]), np.ascontiguousarray(r[100:220, 300:692])
    img = ac.case(name)
    return img, np.ascontiguousarray(img[::-1, ::-1])


def per_image(ctx, img):
    """what spvo_akaze_detect followed by spvo_akaze_describe(img = NULL) returns for one image, as the records and rows
    spvo_akaze_detect_pair promises"""
    det = ctx.akaze_detect(img)
    kp = det["kp"]
    assert len(kp) == det["n"]
    d = ctx.akaze_describe(None, kp)
    rec = kp.copy()
    rec["angle"] = d["angle"]
    return dict(kp=rec, desc=d["desc"], n=len(rec))


def assert_same(got, ref):
    assert got["n"] == ref["n"] == len(got["kp"]) == len(got["desc"])
    assert got["kp"].dtype == capi.AKAZE_KP_DTYPE and got["kp"].dtype.itemsize == 28 and got["desc"].shape == (ref["n"], 61)
    if got["kp"].tobytes() != ref["kp"].tobytes():
        for f in capi.AKAZE_KP_DTYPE.names:
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
def reference(sample_images, sequence):
    """the per-image sequence of every pair, computed once in a context of its own and left unchanged: name -> (left, right)"""
    c = make_ctx()
    out = {}
    for name in PAIRS:
        L, R = pair(name, sample_images, sequence)
        out[name] = (per_image(c, L), per_image(c, R))
    c.close()
    return out


# ---------------------------------------------------------------- 1. the suppression kernels against their definition
@pytest.mark.parametrize("name", list(sc.LISTS))
def test_suppression_hook_equals_the_restatement(ctx, name):
    rows, cols, _, cand, keep, st = sc.case(name)
    got = ctx.akaze_suppress_debug(rows, cols, cand)
    print(name, len(cand), "candidates", len(keep), "kept", st)
    assert got.dtype == np.int32 and got.tolist() == keep.tolist()


def test_suppression_hook_statuses(ctx, squeeze_weights_path, sequence):
    frames, _, P_l, P_r = sequence
    rows, cols, _, cand, keep, _ = sc.case("n65")
    bad = cand.copy()
    bad["level"][-1] = 8                                               # 96 x 160 has levels 0 .. 7
    with pytest.raises(capi.SpvoError) as e:
        ctx.akaze_suppress_debug(rows, cols, bad)
    assert e.value.code == -1
    bad = cand.copy()
    bad["level"][:2] = (1, 0)                                          # not level by level
    with pytest.raises(capi.SpvoError) as e:
        ctx.akaze_suppress_debug(rows, cols, bad)
    assert e.value.code == -1
    with pytest.raises(capi.SpvoError) as e:
        ctx.akaze_suppress_debug(15, 160, cand[:0])
    assert e.value.code == -1
    c = make_ctx(squeeze_weights_path)
    try:
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)              # a SuperPoint submission in flight
        with pytest.raises(capi.SpvoError) as e:
            c.akaze_suppress_debug(rows, cols, cand)
        assert e.value.code == -4
        c.detect_collect(P_l, P_r)
        assert c.akaze_suppress_debug(rows, cols, cand).tolist() == keep.tolist()
    finally:
        c.close()


# ---------------------------------------------------------------- 2. byte equality with the per-image entry points
@pytest.mark.parametrize("name", PAIRS)
def test_pair_equals_the_per_image_entry_points(ctx, sample_images, sequence, reference, name):
    L, R = pair(name, sample_images, sequence)
    rl, rr = reference[name]
    gl, gr = ctx.akaze_detect_pair(L, R, 2, 3)
    print(name, L.shape, "per image", rl["n"], rr["n"], "pair", gl["n"], gr["n"])
    assert_same(gl, rl)
    assert_same(gr, rr)
    assert ctx.classic_slot_rows(2) == rl["n"] and ctx.classic_slot_rows(3) == rr["n"]
    if name == "full_size":
        assert rl["n"] > 500 and rr["n"] > 500 and gl["kp"].tobytes() != gr["kp"].tobytes()
        return                                                         # (once)
    sl, sr = ctx.akaze_detect_pair(R, L, 4, 5)                         # the other order: left and right trade places
    assert_same(sl, rr)
    assert_same(sr, rl)
    if name == "flat":
        assert rl["n"] == rr["n"] == 0 and gl["desc"].shape == (0, 61)
        assert all(len(i) == 0 for i, _ in match_all(ctx, 2, 3, gl["desc"], gr["desc"]).values())
    else:
        assert rl["n"] > 0 and rr["n"] > 0
        assert np.all((gl["kp"]["angle"] >= 0) & (gl["kp"]["angle"] <= 360))
    if name == "blobs":
        assert len(set(gl["kp"]["class_id"].tolist())) >= 4            # keypoints on many levels


def test_host_buffer_smaller_than_the_slot_and_null_buffers(ctx, sample_images, sequence, reference):
    """cap < n: n is reported, exactly cap leading rows are written, the slot holds all of them; kp and desc may be NULL"""
    L, R = pair("frame", sample_images, sequence)
    rl, rr = reference["frame"]
    assert rl["n"] > 20 and rr["n"] > 20
    gl, gr = ctx.akaze_detect_pair(L, R, 0, 1, cap=10)
    assert gl["n"] == rl["n"] and gr["n"] == rr["n"] and len(gl["kp"]) == len(gr["desc"]) == 10
    assert gl["kp"].tobytes() == rl["kp"][:10].tobytes() and gr["desc"].tobytes() == rr["desc"][:10].tobytes()
    assert ctx.classic_slot_rows(0) == rl["n"]
    match_all(ctx, 0, 1, rl["desc"], rr["desc"])
    fl, fr = capi.AkazeFeatures(0, None, None, 0), capi.AkazeFeatures(0, None, None, 0)
    rc = ctx.lib.spvo_akaze_detect_pair(ctx.h, L.ctypes.data, R.ctypes.data, L.shape[0], L.shape[1], L.strides[0], 0.001, 2, 3, 8192, capi.C.byref(fl), capi.C.byref(fr))
    assert rc == 0 and (fl.n, fr.n) == (rl["n"], rr["n"]) and ctx.classic_slot_rows(3) == rr["n"]
    match_all(ctx, 2, 3, rl["desc"], rr["desc"])


# ---------------------------------------------------------------- 3. matching
@pytest.mark.parametrize("name", ["frame", "full_size"])
def test_matching_in_the_slots(ctx, sample_images, sequence, name):
    L, R = pair(name, sample_images, sequence)
    fl, fr = ctx.akaze_detect_pair(L, R, 6, 7)
    res = match_all(ctx, 6, 7, fl["desc"], fr["desc"])
    match_all(ctx, 7, 6, fr["desc"], fl["desc"])
    assert (res[("NN", False)][0] >= 0).all() and (res[("NN", True)][0] >= 0).any()
    assert (res[("KNN", False)][0] >= 0).sum() > 10


def test_width_mismatch_is_refused(ctx, sample_images, sequence):
    L, R = pair("frame", sample_images, sequence)
    fl, _ = ctx.akaze_detect_pair(L, R, 0, 1)
    rows64 = np.zeros((fl["n"], 64), np.uint8)
    rows64[:, :61] = fl["desc"]
    ctx.classic_slot_fill(4, rows64)                                   # the same bits as 64-byte rows: still another width
    for a, b in ((0, 4), (4, 0)):
        with pytest.raises(capi.SpvoError) as e:
            ctx.match_hamming_slots(a, b, "KNN", False, 0.8)
        assert e.value.code == -1 and "61" in str(e.value) and "64" in str(e.value)
    with pytest.raises(capi.SpvoError) as e:                           # the fill hook takes 32 and 64 only
        ctx.classic_slot_fill(5, fl["desc"])
    assert e.value.code == -1


# ---------------------------------------------------------------- 4. prematch
def crops(sequence, k):
    return tuple(np.ascontiguousarray(im[100:220, 300:692]) for im in sequence[0][k])


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
                fl, fr = c.akaze_detect_pair(L, R, 2 * k, 2 * k + 1)
                assert fl["n"] > 20
                out.append(c.match_hamming_slots(2 * k, 2 * k + 1, sel, cross, 0.8))
                hi, hd = c.match_hamming(fl["desc"], fr["desc"], sel, cross, 0.8)
                assert np.array_equal(out[-1][0], hi) and np.array_equal(out[-1][1], hd)
                if k:
                    out.append(c.match_hamming_slots(2 * k, 2 * k - 2, sel, cross, 0.8))
                    hi, hd = c.match_hamming(fl["desc"], prev["desc"], sel, cross, 0.8)
                    assert np.array_equal(out[-1][0], hi) and np.array_equal(out[-1][1], hd)
                    assert (hi >= 0).sum() > 5
                prev = fl
            L0, R0 = crops(sequence, 0)
            _, nr = c.akaze_detect_pair(R0, L0, 8, 5)                   # rewrite the right slot of the last pair: the stored stereo match is stale
            gi, gd = c.match_hamming_slots(4, 5, sel, cross, 0.8)
            hi, hd = c.match_hamming(fl["desc"], nr["desc"], sel, cross, 0.8)
            assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
            res[on] = out
        finally:
            c.close()
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_prematch_temporal_partner_across_entry_points(sequence):
    """after a FAST + BRISK pair (64-byte rows) the next AKAZE pair has no temporal partner and does not fail; after an AKAZE pair it has
    one, and the stored temporal match is the synchronous one; a BRISK kind after an AKAZE pair skips it the same way"""
    c = make_ctx()
    try:
        c.set_prematch(True, "KNN", False, 0.8)
        L0, R0 = crops(sequence, 0)
        L1, R1 = crops(sequence, 1)
        L2, R2 = crops(sequence, 2)
        bl, br_ = c.classic_detect(L0, R0, 0, 1, "FAST+BRISK")
        assert bl["desc"].shape[1] == 64 and len(bl["desc"]) > 10
        al, ar = c.akaze_detect_pair(L1, R1, 2, 3)
        gi, gd = c.match_hamming_slots(2, 3, "KNN", False, 0.8)
        hi, hd = c.match_hamming(al["desc"], ar["desc"], "KNN", False, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd) and (gi >= 0).sum() > 5
        with pytest.raises(capi.SpvoError) as e:                       # asked for explicitly, the temporal match names the widths
            c.match_hamming_slots(2, 0, "KNN", False, 0.8)
        assert e.value.code == -1
        gi, gd = c.match_hamming_slots(0, 1, "KNN", False, 0.8)        # the BRISK rows are still there
        hi, hd = c.match_hamming(bl["desc"], br_["desc"], "KNN", False, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
        nl, _ = c.akaze_detect_pair(L2, R2, 4, 5)                      # ... and this call has a temporal partner: slot 2
        ti, td = c.match_hamming_slots(4, 2, "KNN", False, 0.8)
        hi, hd = c.match_hamming(nl["desc"], al["desc"], "KNN", False, 0.8)
        assert np.array_equal(ti, hi) and np.array_equal(td, hd) and len(ti) == nl["n"]
        ql, qr = c.classic_detect(L1, R1, 6, 7, "FAST+BRISK")          # the reverse: an AKAZE left slot is no partner of a BRISK kind
        gi, gd = c.match_hamming_slots(6, 7, "KNN", False, 0.8)
        hi, hd = c.match_hamming(ql["desc"], qr["desc"], "KNN", False, 0.8)
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd)
    finally:
        c.close()


# ---------------------------------------------------------------- 5. capacity
def test_capacity(ctx, sample_images, sequence, reference):
    L, R = pair("frame", sample_images, sequence)
    rl, rr = reference["frame"]
    n_l, n_r = rl["n"], rr["n"]
    cap = max(n_l, n_r)
    ctx.set_prematch(True, "KNN", False, 0.8)
    with pytest.raises(capi.SpvoError) as e:                           # one row short of the larger image: reported, nothing truncated
        ctx.akaze_detect_pair(L, R, 0, 1, slot_capacity=cap - 1)
    assert e.value.code == -5 and (e.value.n_l, e.value.n_r) == (n_l, n_r) == e.value.counts
    for s in (0, 1):
        with pytest.raises(capi.SpvoError) as e:                       # ... and both slots are unfilled afterwards
            ctx.classic_slot_rows(s)
        assert e.value.code == -4
    with pytest.raises(capi.SpvoError) as e:                           # (the call's prematch results are dropped with them)
        ctx.match_hamming_slots(0, 1)
    assert e.value.code == -4
    gl, gr = ctx.akaze_detect_pair(L, R, 0, 1, slot_capacity=cap)
    assert_same(gl, rl)
    assert_same(gr, rr)
    match_all(ctx, 0, 1, gl["desc"], gr["desc"])


# ---------------------------------------------------------------- 6. statuses
def test_status_codes(sample_images, reference, squeeze_weights_path, sequence):
    frames, _, P_l, P_r = sequence
    L, R = pair("two_exact", sample_images, sequence)
    rl, rr = reference["two_exact"]
    c = make_ctx(squeeze_weights_path)
    try:
        lib, by = c.lib, capi.C.byref
        gl, gr = c.akaze_detect_pair(L, R, 0, 1)
        assert_same(gl, rl)

        def call(ctx_h=c.h, l=L.ctypes.data, r=R.ctypes.data, rows=L.shape[0], cols=L.shape[1], stride=L.strides[0], threshold=0.001, sl=2, sr=3, slot_capacity=8192, cap=0, null_out=False):
            fl, fr = capi.AkazeFeatures(0, None, None, cap), capi.AkazeFeatures(0, None, None, cap)
            return lib.spvo_akaze_detect_pair(ctx_h, l, r, rows, cols, stride, threshold, sl, sr, slot_capacity, None if null_out else by(fl), by(fr))

        assert call() == 0 and c.classic_slot_rows(2) == rl["n"]
        bad = [dict(l=None), dict(r=None), dict(null_out=True), dict(cap=-1), dict(sl=0, sr=0), dict(sl=-1, sr=1), dict(sl=0, sr=10), dict(slot_capacity=0), dict(slot_capacity=-3),
               dict(slot_capacity=(1 << 22) + 1), dict(threshold=0.0), dict(threshold=-0.001), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(rows=15), dict(cols=15),
               dict(rows=2903, cols=2901, stride=2901), dict(rows=65536, cols=65536, stride=65536), dict(stride=L.shape[1] - 1)]
        for kw in bad:
            assert call(**kw) == -1, kw
        assert call(ctx_h=None) == -1
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)             # a SuperPoint submission in flight
        fl, fr = capi.AkazeFeatures(77, None, None, 0), capi.AkazeFeatures(78, None, None, 0)
        assert lib.spvo_akaze_detect_pair(c.h, L.ctypes.data, R.ctypes.data, L.shape[0], L.shape[1], L.strides[0], 0.001, 0, 1, 8192, by(fl), by(fr)) == -4
        assert (fl.n, fr.n) == (77, 78)                               # the outputs are untouched ...
        c.detect_collect(P_l, P_r)
        assert c.classic_slot_rows(0) == rl["n"] and c.classic_slot_rows(1) == rr["n"] and c.classic_slot_rows(2) == rl["n"]      # ... and so are the slots
        with pytest.raises(capi.SpvoError) as e:
            c.classic_slot_rows(4)
        assert e.value.code == -4
        match_all(c, 0, 1, gl["desc"], gr["desc"])
        nl, nr = c.akaze_detect_pair(L, R, 4, 5)
        assert_same(nl, rl)
        assert_same(nr, rr)
    finally:
        c.close()


# ---------------------------------------------------------------- 7. what is resident afterwards
def test_the_right_image_is_resident_afterwards(ctx, sample_images, sequence, reference):
    L, R = pair("two_odd", sample_images, sequence)
    rl, rr = reference["two_odd"]
    ref = make_ctx()
    try:
        ref.akaze_detect(R)
        planes = [ref.akaze_level(lev, what) for lev, what in ((0, 0), (3, 1), (5, 2), (7, 3))]
        k = ref.akaze_last_contrast()
    finally:
        ref.close()
    gl, gr = ctx.akaze_detect_pair(L, R, 0, 1)
    d = ctx.akaze_describe(None, gr["kp"])
    assert d["desc"].tobytes() == rr["desc"].tobytes() and d["angle"].tobytes() == rr["kp"]["angle"].tobytes()
    for (lev, what), p in zip(((0, 0), (3, 1), (5, 2), (7, 3)), planes):
        assert ctx.akaze_level(lev, what).tobytes() == p.tobytes(), (lev, what)
    assert ctx.akaze_last_contrast().tobytes() == k.tobytes()
    b = ctx.brisk_describe(None, np.stack([gr["kp"]["x"], gr["kp"]["y"]], 1), gr["kp"]["size"], shape=R.shape)       # the image itself
    up = ctx.brisk_describe(R, np.stack([gr["kp"]["x"], gr["kp"]["y"]], 1), gr["kp"]["size"])
    assert b["desc"].tobytes() == up["desc"].tobytes() and np.array_equal(b["kept"], up["kept"])


# ---------------------------------------------------------------- 8. neighbours, repeatability
def test_neighbours_are_unharmed(sample_images, sequence, reference):
    L, R = pair("two_exact", sample_images, sequence)
    rl, rr = reference["two_exact"]
    crop_l, crop_r = sample_images[0][100:164, 300:396], sample_images[1][100:164, 300:396]
    c = make_ctx()
    try:
        orb = c.classic_detect(crop_l, crop_r, 6, 7, "ORB")
        sift = c.sift_detect_pair(crop_l, crop_r, 0, 1)
        brisk = c.brisk_detect_pair(crop_l, crop_r, 8, 9, 30)
        gl, gr = c.akaze_detect_pair(L, R, 0, 1)
        assert_same(gl, rl)
        assert_same(gr, rr)
        orb2 = c.classic_detect(crop_l, crop_r, 6, 7, "ORB")
        sift2 = c.sift_detect_pair(crop_l, crop_r, 2, 3)
        brisk2 = c.brisk_detect_pair(crop_l, crop_r, 8, 9, 30)
        for a, b in zip(orb + sift + brisk, orb2 + sift2 + brisk2):
            for f in a:
                assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f
        assert c.classic_slot_rows(0) == rl["n"]                       # the pair's slots outlive the other calls in other slots
        nl, nr = c.akaze_detect_pair(L, R, 2, 3)
        assert_same(nl, rl)
        assert_same(nr, rr)
    finally:
        c.close()


def test_same_bytes_twice_after_another_shape_and_in_a_fresh_context(sample_images, sequence, reference):
    L, R = pair("ties", sample_images, sequence)
    rl, rr = reference["ties"]
    a = make_ctx()
    first = a.akaze_detect_pair(L, R, 0, 1)
    second = a.akaze_detect_pair(L, R, 0, 1)
    a.akaze_detect_pair(*pair("blobs", sample_images, sequence), 2, 3)            # a larger shape: every buffer grows
    a.akaze_detect_pair(*pair("flat", sample_images, sequence), 4, 5)             # ... and a smaller one
    third = a.akaze_detect_pair(L, R, 6, 7)
    a.close()
    b = make_ctx()
    fresh = b.akaze_detect_pair(L, R, 8, 9)
    b.close()
    for got in (first, second, third, fresh):
        assert_same(got[0], rl)
        assert_same(got[1], rr)


# ---------------------------------------------------------------- 9. the host class
def _run(frames, P_l, P_r, **kw):
    return host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="AKAZE", descriptor="AKAZE", akaze_descriptor=True, input_size=(120, 392), trace=True, **kw)


@pytest.fixture(scope="module")
def per_image_run(sequence):
    """the run with setDeviceResident off, shared and left unchanged"""
    frames, _, P_l, P_r = sequence
    out = _run(frames, P_l, P_r)
    assert host.classic_resident_pairs() == 0
    return out


def test_host_class_is_identical_with_resident_features(sequence, per_image_run):
    """ClassicFeatureFrontEnd(AKAZE, AKAZE) over three synthetic frames at 120 x 392: keypoints_dq, descriptors_dq, the three match lists,
    the inlier sets (digests of their full contents) and every pose are identical with all switches on, and every pair stayed resident;
    with the new switch off (the keyword's default) the pair takes the per-image path as before"""
    frames, _, P_l, P_r = sequence
    p0, s0, _, d0 = per_image_run
    p1, s1, _, d1 = _run(frames, P_l, P_r, resident=True, akaze_resident=True)
    assert host.classic_resident_pairs() == 3 == len(frames)
    assert s0[:, 0].min() > 20
    assert np.array_equal(d0, d1)
    assert np.array_equal(s0, s1)
    assert np.array_equal(p0, p1)
    p2, s2, _, d2 = _run(frames, P_l, P_r, resident=True)
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d2) and np.array_equal(s0, s2) and np.array_equal(p0, p2)
    p3, s3, _, d3 = _run(frames, P_l, P_r, akaze_resident=True)                     # the new switch alone changes nothing
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d3) and np.array_equal(s0, s3) and np.array_equal(p0, p3)


def test_host_class_falls_back_when_a_pair_does_not_fit(sequence, per_image_run):
    """slots one row short of the largest image: that pair takes the per-image path and is matched from the host matrices, and the run is
    still identical"""
    frames, _, P_l, P_r = sequence
    p0, s0, _, d0 = per_image_run
    cap = int(np.maximum(s0[:, 0], s0[:, 1]).max()) - 1
    p1, s1, _, d1 = _run(frames, P_l, P_r, resident=True, akaze_resident=True, resident_capacity=cap)
    assert host.classic_resident_pairs() < 3
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
