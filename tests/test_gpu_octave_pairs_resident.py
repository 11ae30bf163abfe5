"""BRISK + ORB, AKAZE + ORB and AKAZE + BRISK with a stereo pair's features resident on the device (spvo_brisk_orb_pair,
spvo_akaze_orb_pair, spvo_akaze_brisk_pair into the binary slots, ClassicFeatureFrontEnd::setOctavePairsResident): everything equals the
per-image route on the same device EXACTLY -- spvo_brisk_detect / spvo_akaze_detect followed by spvo_orb_describe_octaves(img = NULL) or
spvo_brisk_describe(img = NULL), and spvo_match_hamming on the host copies -- counts, the 24- / 28-byte keypoint records and the rows as
raw bytes, match indices and distances, and through the host class every deque entry, match list, inlier set and pose.  The device link
of the ORB pairs alone (spvo_orb_octaves_link_debug) is held to spvo_orb_describe_octaves on lists no image gives: octaves that do not
ascend, octaves 6 and 7, keep flags between survivors.  That per-image route is held to the numpy restatements by
tests/test_gpu_orb_octaves.py, tests/test_gpu_brisk_detect.py, tests/test_gpu_akaze.py and tests/test_gpu_brisk.py; what the inputs cover
is pinned by tests/test_octave_pairs_resident_cpu.py.  No tolerance, no row excused."""
import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import capi, host
from tests import orb_octaves_cases as oc
from tests.conftest import make_ctx
from tests.test_gpu_classic_trace_golden import load_sequence
from tests.test_octave_pairs_resident_cpu import stereo_pairs

pytestmark = pytest.mark.gpu

MODES = [("NN", False), ("NN", True), ("KNN", False)]          # NN, NN with cross-check, KNN at 0.8
KINDS = ["brisk_orb", "akaze_orb", "akaze_brisk"]
PAIRS = ["crop", "strided", "full_size"]
ROW_BYTES = dict(brisk_orb=32, akaze_orb=32, akaze_brisk=64)


def pair(name, sample_images):
    if name == "full_size":
        return np.ascontiguousarray(sample_images[0]), np.ascontiguousarray(sample_images[1])
    return stereo_pairs(sample_images)[name]


def call(ctx, kind, L, R, sl, sr, **kw):
    return getattr(ctx, kind + "_pair")(L, R, sl, sr, **kw)


def per_image(ctx, kind, img):
    """the per-image route of one image, as the records and rows the pair call promises"""
    det = ctx.brisk_detect(img) if kind == "brisk_orb" else ctx.akaze_detect(img)
    kp = det["kp"]
    assert len(kp) == det["n"]
    xy = np.stack([kp["x"], kp["y"]], 1)
    d = ctx.brisk_describe(None, xy, kp["size"], shape=img.shape) if kind == "akaze_brisk" else ctx.orb_describe_octaves(None, xy, kp["octave"], shape=img.shape)
    rec = kp[d["kept"]].copy()
    rec["angle"] = d["angle"]
    return dict(kp=rec, desc=d["desc"], n=len(rec), detected=len(kp))


def assert_same(got, ref, kind):
    dtype = capi.BRISK_KP_DTYPE if kind == "brisk_orb" else capi.AKAZE_KP_DTYPE
    assert got["n"] == ref["n"] == len(got["kp"]) == len(got["desc"])
    assert got["kp"].dtype == dtype and dtype.itemsize == (24 if kind == "brisk_orb" else 28) and got["desc"].shape == (ref["n"], ROW_BYTES[kind])
    if got["kp"].tobytes() != ref["kp"].tobytes():
        for f in dtype.names:
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
    """the per-image route of every pair and kind, computed once in a context of its own and left unchanged: (kind, name) -> (left, right)"""
    c = make_ctx()
    out = {}
    for kind in KINDS:
        for name in PAIRS:
            L, R = pair(name, sample_images)
            out[kind, name] = (per_image(c, kind, L), per_image(c, kind, R))
    c.close()
    return out


# ---------------------------------------------------------------- 1. the link's kernels against the host path
def hook_lists(sample_images):
    img, hxy, hoct = oc.keypoints("handmade", sample_images)
    _, bxy, boct = oc.keypoints("brisk", sample_images)
    perm = np.random.default_rng(7).permutation(len(bxy))
    bxy, boct = bxy[perm], boct[perm]
    third = np.ones(len(bxy), np.uint8)
    third[::3] = 0
    return img, {"handmade": (hxy, hoct, None, 7), "brisk shuffled": (bxy, boct, None, 5), "brisk shuffled, every third dropped": (bxy, boct, third, 5),
                 "empty": (np.zeros((0, 2), np.float32), np.zeros(0, np.int32), None, 0)}


@pytest.mark.parametrize("name", ["handmade", "brisk shuffled", "brisk shuffled, every third dropped", "empty"])
def test_link_hook_equals_the_host_path(ctx, sample_images, name):
    img, lists = hook_lists(sample_images)
    xy, octave, keep, max_octave = lists[name]
    ctx.fast(img)                                                      # any detector call leaves the image resident
    live = np.arange(len(xy)) if keep is None else np.nonzero(keep)[0]
    ref = ctx.orb_describe_octaves(None, xy[live], octave[live], shape=img.shape)
    got = ctx.orb_octaves_link_debug(xy, octave, keep, max_octave, shape=img.shape)
    print(name, len(xy), "keypoints", len(live), "with their flag set", len(ref["kept"]), "kept, octaves", np.bincount(octave[live][ref["kept"]], minlength=8).tolist())
    assert got["kept"].dtype == np.int32 and np.array_equal(got["kept"], live[ref["kept"]])
    assert got["angle"].tobytes() == ref["angle"].tobytes()
    assert got["desc"].tobytes() == ref["desc"].tobytes()
    if name == "handmade":
        assert (np.diff(octave) < 0).any() and set(octave[got["kept"]].tolist()) == set(range(8))
    if name == "brisk shuffled":
        assert len(got["kept"]) == 716
    if name == "brisk shuffled, every third dropped":
        assert 0 < len(got["kept"]) < 716 and keep[got["kept"]].all()
    again = ctx.orb_octaves_link_debug(xy, octave, keep, max_octave, shape=img.shape)
    assert all(again[f].tobytes() == got[f].tobytes() for f in got)
    after = ctx.orb_describe_octaves(None, xy[live], octave[live], shape=img.shape)     # the image is still resident
    assert after["desc"].tobytes() == ref["desc"].tobytes()


def test_link_hook_statuses(sample_images, squeeze_weights_path):
    frames, P_l, P_r = load_sequence()
    img, lists = hook_lists(sample_images)
    xy, octave, _, _ = lists["handmade"]
    c = make_ctx(squeeze_weights_path)
    try:
        with pytest.raises(capi.SpvoError) as e:                       # nothing is resident yet
            c.orb_octaves_link_debug(xy, octave, None, 7, shape=img.shape)
        assert e.value.code == -4
        c.fast(img)
        for bad in (-1, 8):
            with pytest.raises(capi.SpvoError) as e:
                c.orb_octaves_link_debug(xy[:1], octave[:1], None, bad, shape=img.shape)
            assert e.value.code == -1
        with pytest.raises(capi.SpvoError) as e:                       # an octave above max_octave
            c.orb_octaves_link_debug(xy, octave, None, 6, shape=img.shape)
        assert e.value.code == -1
        with pytest.raises(capi.SpvoError) as e:
            c.orb_octaves_link_debug(np.array([[np.nan, 60]], np.float32), [0], None, 0, shape=img.shape)
        assert e.value.code == -1
        small = np.ascontiguousarray(img[:70])                         # level 5 of 70 x 400 is 28 x 161
        c.fast(small)
        with pytest.raises(capi.SpvoError) as e:
            c.orb_octaves_link_debug(np.array([[100, 35]], np.float32), [0], None, 5, shape=small.shape)
        assert e.value.code == -1 and "28 x 161" in str(e.value) and "level 5" in str(e.value)
        assert len(c.orb_octaves_link_debug(np.array([[100, 35]], np.float32), [0], None, 4, shape=small.shape)["kept"]) == 1
        with pytest.raises(capi.SpvoError) as e:                       # another shape than the resident one
            c.orb_octaves_link_debug(xy, octave, None, 7, shape=img.shape)
        assert e.value.code == -4
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)              # a SuperPoint submission in flight
        with pytest.raises(capi.SpvoError) as e:
            c.orb_octaves_link_debug(np.array([[100, 35]], np.float32), [0], None, 4, shape=small.shape)
        assert e.value.code == -4
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
    print(kind, name, L.shape, "detected", rl["detected"], rr["detected"], "per image", rl["n"], rr["n"], "pair", gl["n"], gr["n"])
    assert_same(gl, rl, kind)
    assert_same(gr, rr, kind)
    assert ctx.classic_slot_rows(2) == rl["n"] and ctx.classic_slot_rows(3) == rr["n"]
    assert rl["n"] > 100 and rr["n"] > 100 and gl["kp"].tobytes() != gr["kp"].tobytes()
    if name == "crop":                                                 # the counts tests/test_octave_pairs_resident_cpu.py pins
        assert (rl["detected"], rl["n"], rr["detected"], rr["n"]) == dict(brisk_orb=(1214, 716, 1190, 705), akaze_orb=(247, 235, 247, 235), akaze_brisk=(247, 247, 247, 247))[kind]
    if name == "strided":
        assert not L.flags["C_CONTIGUOUS"]
        if kind != "brisk_orb":
            assert (rl["detected"], rl["n"], rr["detected"], rr["n"]) == dict(akaze_orb=(137, 134, 152, 146), akaze_brisk=(137, 137, 152, 152))[kind]
    if kind != "akaze_brisk":
        assert np.array_equal(gl["kp"]["octave"], np.sort(gl["kp"]["octave"])) and np.all(np.abs(gl["kp"]["angle"]) <= np.float32(np.pi))
    else:
        assert np.all((gl["kp"]["angle"] >= 0) & (gl["kp"]["angle"] <= 360))
    if name == "full_size":
        return                                                         # (once)
    sl, sr = call(ctx, kind, L, R, 2, 3)                               # two calls give identical bytes
    assert_same(sl, gl, kind)
    assert_same(sr, gr, kind)
    tl, tr = call(ctx, kind, R, L, 4, 5)                               # the other order: left and right trade places
    assert_same(tl, rr, kind)
    assert_same(tr, rl, kind)


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
    imgs = [pair("crop", sample_images), pair("strided", sample_images)]
    imgs[1] = tuple(np.ascontiguousarray(im[:160]) for im in imgs[1])  # one shape for both calls
    res = {}
    for on in (False, True):
        c = make_ctx()
        try:
            c.set_prematch(on, sel, cross, 0.8)
            out = []
            for k, (L, R) in enumerate(imgs):
                fl, fr = call(c, kind, L, R, 2 * k, 2 * k + 1)
                out.append(c.match_hamming_slots(2 * k, 2 * k + 1, sel, cross, 0.8))
                hi, hd = c.match_hamming(fl["desc"], fr["desc"], sel, cross, 0.8)
                assert np.array_equal(out[-1][0], hi) and np.array_equal(out[-1][1], hd)
                if k:
                    out.append(c.match_hamming_slots(2 * k, 2 * k - 2, sel, cross, 0.8))
                    hi, hd = c.match_hamming(fl["desc"], prev["desc"], sel, cross, 0.8)
                    assert np.array_equal(out[-1][0], hi) and np.array_equal(out[-1][1], hd)
                prev = fl
            res[on] = out
        finally:
            c.close()
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_prematch_temporal_partner_across_entry_points(sample_images):
    """a 32-byte slot spvo_classic_detect(FAST+ORB) filled is a temporal partner of spvo_brisk_orb_pair and of spvo_akaze_orb_pair; a
    64-byte or a 61-byte left slot before them is skipped without error; spvo_akaze_brisk_pair partners with a spvo_brisk_detect_pair slot
    and skips a 32-byte one"""
    L0, R0 = pair("crop", sample_images)
    L1, R1 = (np.ascontiguousarray(im[:160]) for im in pair("strided", sample_images))
    c = make_ctx()
    try:
        c.set_prematch(True, "KNN", False, 0.8)

        def stereo_ok(sl, sr, fl, fr):
            gi, gd = c.match_hamming_slots(sl, sr, "KNN", False, 0.8)
            hi, hd = c.match_hamming(fl["desc"], fr["desc"], "KNN", False, 0.8)
            assert np.array_equal(gi, hi) and np.array_equal(gd, hd) and len(gi) == len(fl["desc"])

        fo, fo_r = c.classic_detect(L0, R0, 0, 1, "FAST")
        assert fo["desc"].shape[1] == 32 and len(fo["desc"]) > 10
        bl, br_ = c.brisk_orb_pair(L1, R1, 2, 3)                       # partner: slot 0
        stereo_ok(2, 3, bl, br_)
        stereo_ok(2, 0, bl, fo)
        al, ar_ = c.akaze_orb_pair(L0, R0, 4, 5)                       # partner: slot 2, an ORB pair's
        stereo_ok(4, 5, al, ar_)
        stereo_ok(4, 2, al, bl)
        kl, kr = c.akaze_brisk_pair(L1, R1, 6, 7)                      # 64-byte rows: slot 4 is skipped
        stereo_ok(6, 7, kl, kr)
        with pytest.raises(capi.SpvoError) as e:                       # asked for explicitly, the temporal match names the widths
            c.match_hamming_slots(6, 4, "KNN", False, 0.8)
        assert e.value.code == -1
        ol, or_ = c.brisk_orb_pair(L0, R0, 8, 9)                       # a 64-byte left slot before an ORB pair: skipped
        stereo_ok(8, 9, ol, or_)
        dl, dr = c.brisk_detect_pair(L1, R1, 0, 1)                     # 64-byte rows, BRISK's own pair
        xl, xr = c.akaze_brisk_pair(L0, R0, 2, 3)                      # partner: slot 0
        stereo_ok(2, 3, xl, xr)
        stereo_ok(2, 0, xl, dl)
        ml, mr = c.akaze_detect_pair(L1, R1, 4, 5)                     # 61-byte rows
        assert ml["desc"].shape[1] == 61
        nl, nr = c.akaze_orb_pair(L0, R0, 6, 7)                        # a 61-byte left slot before an ORB pair: skipped
        stereo_ok(6, 7, nl, nr)
    finally:
        c.close()


# ---------------------------------------------------------------- 4. capacity and state
@pytest.mark.parametrize("kind", KINDS)
def test_capacity(ctx, sample_images, reference, kind):
    L, R = pair("crop", sample_images)
    rl, rr = reference[kind, "crop"]
    n_l, n_r = rl["n"], rr["n"]
    cap = min(n_l, n_r) - 1
    ctx.set_prematch(True, "KNN", False, 0.8)
    with pytest.raises(capi.SpvoError) as e:                           # neither image fits: both counts reported, nothing truncated
        call(ctx, kind, L, R, 0, 1, slot_capacity=cap)
    assert e.value.code == -5 and (e.value.n_l, e.value.n_r) == (n_l, n_r) == e.value.counts
    for s in (0, 1):
        with pytest.raises(capi.SpvoError) as e:                       # ... and both slots are unfilled afterwards
            ctx.classic_slot_rows(s)
        assert e.value.code == -4
    with pytest.raises(capi.SpvoError) as e:
        ctx.match_hamming_slots(0, 1)
    assert e.value.code == -4
    gl, gr = call(ctx, kind, L, R, 0, 1, slot_capacity=max(n_l, n_r))
    assert_same(gl, rl, kind)
    assert_same(gr, rr, kind)
    match_all(ctx, 0, 1, gl["desc"], gr["desc"])


def test_small_shape_and_submission_in_flight(sample_images, reference, squeeze_weights_path):
    frames, P_l, P_r = load_sequence()
    L, R = pair("crop", sample_images)
    rl, rr = reference["brisk_orb", "crop"]
    c = make_ctx(squeeze_weights_path)
    try:
        gl, gr = c.brisk_orb_pair(L, R, 0, 1)
        assert_same(gl, rl, "brisk_orb")
        with pytest.raises(capi.SpvoError) as e:                       # level 5 of a 70 x 400 image is 28 rows
            c.brisk_orb_pair(np.ascontiguousarray(L[:70]), np.ascontiguousarray(R[:70]), 0, 1)
        assert e.value.code == -1 and "level 5" in str(e.value) and "28 x 161" in str(e.value)
        assert c.classic_slot_rows(0) == rl["n"] and c.classic_slot_rows(1) == rr["n"]      # the slots filled before stay filled
        match_all(c, 0, 1, gl["desc"], gr["desc"])
        with pytest.raises(capi.SpvoError) as e:
            c.brisk_orb_pair(L, R, 2, 3, octaves=4)
        assert e.value.code == -1
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)              # a SuperPoint submission in flight
        for kind in KINDS:
            with pytest.raises(capi.SpvoError) as e:
                call(c, kind, L, R, 0, 1)
            assert e.value.code == -4, kind
        c.detect_collect(P_l, P_r)
        assert c.classic_slot_rows(0) == rl["n"] and c.classic_slot_rows(1) == rr["n"]
        nl, nr = c.brisk_orb_pair(L, R, 4, 5)
        assert_same(nl, rl, "brisk_orb")
        assert_same(nr, rr, "brisk_orb")
    finally:
        c.close()


# ---------------------------------------------------------------- 5. what is resident afterwards
@pytest.mark.parametrize("kind", KINDS)
def test_the_right_image_is_resident_afterwards(ctx, sample_images, reference, kind):
    L, R = pair("strided", sample_images)
    rl, rr = reference[kind, "strided"]
    other = make_ctx()                                                 # the right image's keypoints from a second context: this one keeps what the pair call leaves
    try:
        det = (other.brisk_detect if kind == "brisk_orb" else other.akaze_detect)(R)["kp"]
    finally:
        other.close()
    gl, gr = call(ctx, kind, L, R, 0, 1)
    xy = np.stack([det["x"], det["y"]], 1)
    d = ctx.brisk_describe(None, xy, det["size"], shape=R.shape) if kind == "akaze_brisk" else ctx.orb_describe_octaves(None, xy, det["octave"], shape=R.shape)
    assert d["desc"].tobytes() == rr["desc"].tobytes() == gr["desc"].tobytes() and d["angle"].tobytes() == rr["kp"]["angle"].tobytes()
    if kind != "brisk_orb":                                            # ... and so is its scale space
        a = ctx.akaze_describe(None, det)
        up = ctx.akaze_describe(R, det)
        assert a["desc"].tobytes() == up["desc"].tobytes() and a["angle"].tobytes() == up["angle"].tobytes()


# ---------------------------------------------------------------- 6. the host class
HOST = dict(brisk_orb=dict(detector="BRISK", descriptor="ORB", orb_octaves=True), akaze_orb=dict(detector="AKAZE", descriptor="ORB", orb_octaves=True),
            akaze_brisk=dict(detector="AKAZE", descriptor="BRISK"))


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
    the three match lists, the inlier sets (digests of their full contents) and every pose are identical with the switches on, and every
    pair stayed resident; with the new switch off (the keyword's default) the pair takes the per-image path as before"""
    (frames, P_l, P_r), runs = per_image_runs
    p0, s0, _, d0 = runs[kind]
    p1, s1, _, d1 = _run(frames, P_l, P_r, kind, resident=True, octave_pairs_resident=True)
    assert host.classic_resident_pairs() == 6 == len(frames)
    assert s0[:, :2].min() > 20
    assert np.array_equal(d0, d1)
    assert np.array_equal(s0, s1)
    assert np.array_equal(p0, p1)
    p2, s2, _, d2 = _run(frames, P_l, P_r, kind, resident=True)
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d2) and np.array_equal(s0, s2) and np.array_equal(p0, p2)
    p3, s3, _, d3 = _run(frames, P_l, P_r, kind, octave_pairs_resident=True)            # the new switch alone changes nothing
    assert host.classic_resident_pairs() == 0
    assert np.array_equal(d0, d3) and np.array_equal(s0, s3) and np.array_equal(p0, p3)


@pytest.mark.parametrize("kind", KINDS)
def test_host_class_mixes_resident_and_fallen_back_pairs(per_image_runs, kind):
    """slots of the median row count of the per-image run: some pairs fit, some take the per-image path and are matched from the host
    matrices, and the run is still identical"""
    (frames, P_l, P_r), runs = per_image_runs
    p0, s0, _, d0 = runs[kind]
    cap = int(np.median(s0[:, :2]))
    p1, s1, _, d1 = _run(frames, P_l, P_r, kind, resident=True, octave_pairs_resident=True, resident_capacity=cap)
    print(kind, "rows", s0[:, :2].tolist(), "capacity", cap, "resident pairs", host.classic_resident_pairs())
    assert 0 < host.classic_resident_pairs() < 6
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
