"""GPU parity of the classic front end's AKAZE keypoint detector (csrc/akaze.hip.h; spvo_akaze_detect, spvo_akaze_debug_level,
spvo_akaze_last_contrast) against the numpy restatement tests/akaze_ref.py: the four planes of every level, the contrast factor of every
octave and the keypoints bit for bit (planes and records compared as raw bytes, nothing excused), determinism, the capacity and error
conventions, the detector followed by the BRISK extractor on the resident image, and ClassicFeatureFrontEnd(AKAZE, BRISK) through the host
class.  The restatement takes the library's tables (spvo_akaze_tables), so the comparison does not depend on the last place of two math
libraries' cos / exp / pow.  Inputs: tests/akaze_cases.py; tests/test_akaze_ref_cpu.py asserts what those cases are meant to cover."""
import functools
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import frontend as ofe, matching, odometry as od
from spvo import capi, host, synth
from tests import akaze_cases as ac, akaze_ref as ak, brisk_ref as br
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu

ALL_CASES = ac.CASES + ["full_size"]
PLANES = ("Lt", "Lsmooth", "Lflow", "Ldet")


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib_tables():
    return capi.brisk_tables()


@functools.lru_cache(maxsize=None)
def _tables(rows, cols):
    return capi.akaze_tables(rows, cols)


_REF = {}


def _reference(img, key):
    """(levels, k, keypoints) of the restatement on the library's tables, computed once per key"""
    if key not in _REF:
        levels, k = ak.scale_space(img, _tables(*img.shape))
        _REF[key] = (levels, k, ak.detect(img, levels=levels))
    return _REF[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ALL_CASES)
def test_planes_contrast_and_keypoints_equal_the_restatement(ctx, sample_images, name):
    """Lt, Lsmooth, Lflow and Ldet of every level and k of every octave bit for bit; the keypoints: same count, same order, every field bit
    for bit (raw bytes of the records)"""
    img = ac.image_case(name, sample_images)
    levels, k, ref = _reference(img, name)
    got = ctx.akaze_detect(img)
    gk = ctx.akaze_last_contrast()
    print(name, img.shape, "levels", len(levels), "k", gk.tolist(), "keypoints", got["n"], "restatement", len(ref), "per level", np.bincount(ref["class_id"], minlength=len(levels)).tolist())
    assert gk.tobytes() == np.asarray(k, np.float32).tobytes()
    for i, L in enumerate(levels):
        for what, plane in enumerate(PLANES):
            g = ctx.akaze_level(i, what)
            assert g.shape == L[plane].shape
            bad = _bits(g) != _bits(L[plane])
            assert not bad.any(), "%s of level %d: %d of %d values differ, first at %s, largest difference %g" % (
                plane, i, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), float(np.abs(g.astype(np.float64) - L[plane]).max()))
    with pytest.raises(capi.SpvoError) as e:
        ctx.akaze_level(len(levels), 0)
    assert e.value.code == -1
    kp = got["kp"]
    assert got["n"] == len(ref) == len(kp) and (len(ref) > 0) == (name != "flat")
    if kp.tobytes() != ref.tobytes():
        for f in ak.KP_DTYPE.names:
            bad = np.nonzero(kp[f].view(np.uint32) != ref[f].view(np.uint32))[0]
            if len(bad):
                print("  field", f, ":", len(bad), "rows differ, first", int(bad[0]), kp[bad[0]], ref[bad[0]])
    assert kp.dtype.itemsize == ak.KP_DTYPE.itemsize == 28 and kp.tobytes() == ref.tobytes()


def test_same_bytes_twice_in_one_context_in_a_fresh_one_and_after_another_shape(sample_images):
    """atomics order and stale buffers: a call repeated, repeated after a larger and a smaller image went through the same context (buffer
    growth, then a layout inside the grown buffers), and in a fresh context gives identical bytes; a strided view gives what its packed
    copy gives"""
    img = ac.case("two_odd")
    a = make_ctx()
    first = a.akaze_detect(img)["kp"]
    second = a.akaze_detect(img)["kp"]
    big = ac.image_case("full_size", sample_images)
    a.akaze_detect(big)
    a.akaze_detect(ac.case("ties"))
    third = a.akaze_detect(img)["kp"]
    ldet = a.akaze_level(5, 3)
    view = big[5:165, 7:307]                                                             # rows are not contiguous
    strided, packed = a.akaze_detect(view)["kp"], a.akaze_detect(np.ascontiguousarray(view))["kp"]
    a.close()
    b = make_ctx()
    fresh = b.akaze_detect(img)["kp"]
    b.close()
    levels, _, ref = _reference(img, "two_odd")
    assert len(first) > 20 and first.tobytes() == second.tobytes() == third.tobytes() == fresh.tobytes() == ref.tobytes()
    assert ldet.tobytes() == levels[5]["Ldet"].tobytes()
    assert len(strided) > 20 and strided.tobytes() == packed.tobytes()


def test_cap_smaller_than_n_and_the_error_statuses(ctx):
    img = ac.case("two_exact")
    ref = _reference(img, "two_exact")[2]
    lib = ctx.lib
    fresh = make_ctx()
    with pytest.raises(capi.SpvoError) as e:                                            # no call yet
        fresh.akaze_level(0, 0)
    assert e.value.code == -4
    fresh.close()
    cap = 17
    buf = np.zeros(cap + 3, capi.AKAZE_KP_DTYPE)
    n = capi.C.c_int(0)
    thr = capi.C.c_float(0.001)
    assert lib.spvo_akaze_detect(ctx.h, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], thr, buf.ctypes.data, cap, capi.C.byref(n)) == 0
    assert n.value == len(ref) > cap                                                    # n is reported ...
    assert buf[:cap].tobytes() == ref[:cap].tobytes() and not buf[cap:].tobytes().strip(b"\0")   # ... and exactly cap leading records are written
    assert lib.spvo_akaze_detect(ctx.h, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], thr, None, 0, capi.C.byref(n)) == 0 and n.value == len(ref)
    for bad_thr in (0.0, -0.001, float("inf"), float("nan")):
        with pytest.raises(capi.SpvoError) as e:
            ctx.akaze_detect(img, bad_thr)
        assert e.value.code == -1
    for shape in ((15, 40), (40, 15)):                                                  # below 16 x 16
        with pytest.raises(capi.SpvoError) as e:
            ctx.akaze_detect(np.zeros(shape, np.uint8))
        assert e.value.code == -1
    # rows * cols * 255 >= 2^31 is refused before anything is read (the extractor that follows could not build its int32 integral image)
    assert lib.spvo_akaze_detect(ctx.h, img.ctypes.data, 2903, 2901, 2901, thr, None, 0, capi.C.byref(n)) == -1
    assert lib.spvo_akaze_detect(ctx.h, None, 96, 160, 160, thr, None, 0, capi.C.byref(n)) == -1                              # no image
    tiny = np.random.RandomState(5).randint(0, 256, (16, 16)).astype(np.uint8)          # the minimum size runs: one octave, no room inside the border
    assert ctx.akaze_detect(tiny)["n"] == 0 and ctx.akaze_level(3, 3).tobytes() == _reference(tiny, "tiny")[0][3]["Ldet"].tobytes()
    higher = ctx.akaze_detect(img, 0.01)                                                # the threshold is an argument
    assert 0 < higher["n"] < len(ref) and higher["kp"].tobytes() == ak.detect(img, 0.01, levels=_reference(img, "two_exact")[0]).tobytes()
    assert ctx.akaze_detect(img)["kp"].tobytes() == ref.tobytes()                       # the context is still usable
    ctx.fast(img)                                                                       # another call takes the resident image over: even the same
    with pytest.raises(capi.SpvoError) as e:                                            # image ends the detector's claim on it
        ctx.akaze_level(0, 0)
    assert e.value.code == -4
    with pytest.raises(capi.SpvoError) as e:
        ctx.akaze_last_contrast()
    assert e.value.code == -4
    ctx.brisk_detect(img)
    ctx.akaze_detect(img)                                                               # ... and AKAZE ends the BRISK detector's
    with pytest.raises(capi.SpvoError) as e:
        ctx.brisk_detect_layer(0, 0)
    assert e.value.code == -4
    assert ctx.akaze_level(0, 0).shape == img.shape


def test_a_submission_in_flight_refuses_the_call_and_touches_nothing(sequence, squeeze_weights_path):
    """SPVO_ERR_STATE while a spvo_detect_submit is in flight, from spvo_akaze_detect and from the debug hooks; the refused calls leave the
    earlier result and the resident image as they were: after the collect the planes, the contrast factor and a
    spvo_brisk_describe(img = NULL) answer as before"""
    frames, _, P_l, P_r = sequence
    img, other = ac.case("two_exact"), ac.case("one_octave")
    levels, k, ref = _reference(img, "two_exact")
    xy = np.stack([ref["x"], ref["y"]], 1)
    c = make_ctx(squeeze_weights_path)
    try:
        assert c.akaze_detect(img)["kp"].tobytes() == ref.tobytes()
        before = c.brisk_describe(None, xy, ref["size"], shape=img.shape)
        c.detect_submit(frames[0][0], frames[0][1], 2, 3)             # a SuperPoint submission in flight
        n = capi.C.c_int(-7)
        buf = np.zeros(8, capi.AKAZE_KP_DTYPE)
        for image in (other, img):
            assert c.lib.spvo_akaze_detect(c.h, image.ctypes.data, image.shape[0], image.shape[1], image.strides[0], capi.C.c_float(0.001), buf.ctypes.data, 8, capi.C.byref(n)) == -4
            assert n.value == 0 and not buf.tobytes().strip(b"\0")
        with pytest.raises(capi.SpvoError) as e:
            c.akaze_level(0, 3)
        assert e.value.code == -4
        c.detect_collect(P_l, P_r)
        assert c.akaze_last_contrast().tobytes() == np.asarray(k, np.float32).tobytes()          # the refused calls touched nothing
        for i in (0, 3, 5):
            assert c.akaze_level(i, 3).tobytes() == levels[i]["Ldet"].tobytes() and c.akaze_level(i, 0).tobytes() == levels[i]["Lt"].tobytes()
        after = c.brisk_describe(None, xy, ref["size"], shape=img.shape)
        assert len(after["kept"]) > 0 and all(after[f].tobytes() == before[f].tobytes() for f in ("kept", "angle", "desc"))
        assert c.akaze_detect(img)["kp"].tobytes() == ref.tobytes()
    finally:
        c.close()


def _adjacent(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a == b) | (np.nextafter(b, np.float32(np.inf)) == a) | (np.nextafter(b, np.float32(-np.inf)) == a)


def _describe_equals(g, r):
    """spvo_brisk_describe's rows against tests/brisk_ref.py's, by the bar of tests/test_gpu_brisk.py: everything equal except that a row
    within one float step of a rotation boundary (at most 1 %) may take the neighbouring rotation"""
    assert np.array_equal(g["kept"], r["kept"]) and _adjacent(g["angle"], r["angle"]).all()
    ok = ~r["boundary"]
    assert r["boundary"].sum() <= 0.01 * max(len(r["kept"]), 1) + 1
    assert np.array_equal(g["desc"][ok], r["desc"][ok])


@pytest.mark.parametrize("name", ["blobs", "one_octave"])
def test_detect_then_describe_on_the_resident_image(ctx, lib_tables, name):
    """spvo_akaze_detect followed by spvo_brisk_describe(img = NULL) with the detector's x, y and size: the rows tests/brisk_ref.py computes
    from the restatement's keypoints, and the rows of the same image uploaded again, byte for byte"""
    img = ac.case(name)
    ref = _reference(img, name)[2]
    xy = np.stack([ref["x"], ref["y"]], 1)
    r = br.describe(img, xy, ref["size"], tables=lib_tables)
    got = ctx.akaze_detect(img)
    assert got["kp"].tobytes() == ref.tobytes()
    g = ctx.brisk_describe(None, np.stack([got["kp"]["x"], got["kp"]["y"]], 1), got["kp"]["size"], shape=img.shape)
    up = ctx.brisk_describe(img, xy, ref["size"])                                        # the same image uploaded again
    print(name, "keypoints", len(ref), "described", len(r["kept"]), "scale indices", sorted(set(r["scale"].tolist())), "boundary rows", int(r["boundary"].sum()))
    _describe_equals(g, r)
    assert len(r["kept"]) > 0 and g["desc"].tobytes() == up["desc"].tobytes() and g["angle"].tobytes() == up["angle"].tobytes()
    if name == "blobs":
        assert len(set(r["scale"].tolist())) >= 4


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(3, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def test_akaze_brisk_front_end_pushes_aligned_features(sequence):
    """ClassicFeatureFrontEnd(AKAZE, BRISK, BF, ...) at the native resolution on the crop the BRISK test uses: two deque entries, keypoints
    and 64-byte rows one to one, as many as the restatement's detector and the extractor's border rule leave; no error logged.  AKAZE
    keypoints with the AKAZE (MLDB) or the ORB descriptor stay pairs that do not run."""
    frames, _, P_l, P_r = sequence
    L, R = (np.ascontiguousarray(im[40:200, 300:700]) for im in frames[0])
    n, counts, err = host.classic_pair_probe("AKAZE", "BRISK", L, R, P_l, P_r)
    assert n == 2 and err == "", err
    assert counts[0] == counts[1] > 0 and counts[2] == counts[3] > 0 and counts[4] == 64
    for img, got in ((L, counts[0]), (R, counts[2])):
        kp = ak.detect(img, tables=_tables(*img.shape))
        assert got == len(br.border_keep(np.stack([kp["x"], kp["y"]], 1), kp["size"], img.shape)[0])
    for descriptor in ("AKAZE", "ORB"):
        n, counts, err = host.classic_pair_probe("AKAZE", descriptor, L, R, P_l, P_r)
        assert n == 0 and err != ""


def test_classic_front_end_with_akaze_brisk_equals_the_oracle_state_machine(sequence, lib_tables):
    """classic_sequence(frames, detector="AKAZE", descriptor="BRISK", input_size=(120, 392)) (KNN) against oracle/odometry.py's FrontEndState
    fed the RESTATEMENT's keypoints (tests/akaze_ref.py on the oracle's preprocessed image, the library's tables), the extractor's rows for
    them (held to tests/brisk_ref.py's by the extractor's own bar) and the Hamming oracle's maps: keypoint, stereo-match and inlier counts
    identical, poses within 1e-6.  The BRISK test's absolute bars -- more than 100 keypoints, more than 20 inliers, translation within 0.1
    of the synthetic motion -- are asserted because the all-CPU pipeline (restatement, tests/brisk_ref.py, oracle.matching, oracle.odometry)
    clears them on these frames at 120 x 392: 191 .. 201 keypoints, 80 and 92 inliers, 0.061 and 0.013 (NOTES.md, "AKAZE detector").
    With resident=True: the same digests through the per-image path, and no pair counted as resident."""
    frames, gt, P_l, P_r = sequence
    poses, stats, _, digests = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="AKAZE", descriptor="BRISK", input_size=(120, 392), trace=True)
    ctx = make_ctx()
    st = od.FrontEndState()
    prev_dl = None
    for k, (L, R) in enumerate(frames):
        feats, Ps = [], []
        for img, P in ((L, P_l), (R, P_r)):
            small, Pk = ofe.preprocess(img, np.asarray(P, np.float64).reshape(3, 4), 120, 392)[:2]
            small = np.ascontiguousarray(small)
            kp = ak.detect(small, tables=_tables(*small.shape))
            xy = np.stack([kp["x"], kp["y"]], 1)
            d = ctx.brisk_describe(small, xy, kp["size"])
            _describe_equals(d, br.describe(small, xy, kp["size"], tables=lib_tables))
            feats.append((xy[d["kept"]], d["desc"]))
            Ps.append(Pk)
        (xyl, dl), (xyr, dr) = feats
        od.add_features(st, xyl, dl, xyr, dr, Ps[0], Ps[1])
        idx0, _ = matching.bf_match_hamming(dl, dr, "KNN", False, 0.8)
        st.maps[od.PREV_LEFT_PREV_RIGHT] = st.maps[od.CURR_LEFT_CURR_RIGHT]
        st.maps[od.CURR_LEFT_CURR_RIGHT] = idx0
        print(k, "stats", stats[k].tolist(), "oracle", len(xyl), len(xyr), int((idx0 >= 0).sum()))
        assert stats[k, 0] == len(xyl) > 100 and stats[k, 1] == len(xyr) and stats[k, 2] == int((idx0 >= 0).sum())
        if k > 0:
            idx1, _ = matching.bf_match_hamming(dl, prev_dl, "KNN", False, 0.8)
            st.maps[od.CURR_LEFT_PREV_LEFT] = idx1
            q, t, dbg = od.solve_stereo_odometry(st, 2.0, 2.0, 4)
            Rc, Rg = od.quat_to_rot(np.asarray(q)), od.quat_to_rot(poses[k, :4])
            _, tt = synth.relative_pose(gt[k - 1], gt[k])
            print("   inliers", stats[k, 3], len(dbg["inliers"]), "pose difference R %.3g t %.3g; t vs synthetic motion %.3g" % (
                np.abs(Rg - Rc).max(), np.abs(poses[k, 4:] - t).max(), np.abs(poses[k, 4:] - tt).max()))
            assert stats[k, 3] == len(dbg["inliers"]) > 20
            assert np.abs(Rg - Rc).max() <= 1e-6 and np.abs(poses[k, 4:] - t).max() <= 1e-6
            assert np.abs(poses[k, 4:] - tt).max() < 0.1
        prev_dl = dl
    ctx.close()
    poses_r, stats_r, _, digests_r = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="AKAZE", descriptor="BRISK", input_size=(120, 392), resident=True,
                                                           trace=True)
    assert np.array_equal(digests_r, digests) and np.array_equal(stats_r, stats) and np.array_equal(poses_r, poses)
    assert host.classic_resident_pairs() == 0
    with pytest.raises(RuntimeError):                                                   # AKAZE keypoints with the default (ORB) descriptor: still not a pair that runs
        host.classic_sequence(frames[:1], P_l, P_r, "KNN", True, 2.0, 4, detector="AKAZE")
