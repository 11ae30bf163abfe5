"""GPU parity of the classic front end's BRISK keypoint detector (csrc/brisk_detect.hip.h; spvo_brisk_detect,
spvo_brisk_detect_debug_layer) against the numpy restatement tests/brisk_detect_ref.py: the six layer images and the score maps byte for
byte, the keypoints bit for bit in every field (compared as raw bytes, no row excused), determinism, the capacity and error conventions,
the detector followed by the extractor on the resident image, and ClassicFeatureFrontEnd(BRISK, BRISK) through the host class.  Inputs:
tests/brisk_detect_cases.py; tests/test_brisk_detect_ref_cpu.py asserts what those cases are meant to cover."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import frontend as ofe, matching, odometry as od
from spvo import capi, host, synth
from tests import brisk_detect_cases as bc, brisk_detect_ref as bd, brisk_ref as br
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu

ALL_CASES = bc.CASES + ["full_size"]


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib_tables():
    return capi.brisk_tables()


@pytest.mark.parametrize("name", ALL_CASES)
def test_layers_scores_and_keypoints_equal_the_restatement(ctx, sample_images, name):
    """every layer image, every 9-16 score map and the 5-8 map byte for byte; the keypoints: same count, same order, every field bit for
    bit (raw bytes of the records)"""
    img, thr = bc.image_case(name, sample_images)
    layers, ref, _ = bc.image_reference(name, sample_images)
    got = ctx.brisk_detect(img, thr)
    for i, L in enumerate(layers):
        im, sc = ctx.brisk_detect_layer(i, 0), ctx.brisk_detect_layer(i, 1)
        assert im.shape == L.im.shape and sc.shape == L.s.shape
        assert np.array_equal(im, L.im), "image of layer %d: %d pixels differ" % (i, int((im != L.im).sum()))
        assert np.array_equal(sc, L.s), "9-16 score of layer %d: %d pixels differ" % (i, int((sc != L.s).sum()))
    s5 = ctx.brisk_detect_layer(0, 2)
    assert np.array_equal(s5, layers[0].s5), "5-8 score: %d pixels differ" % int((s5 != layers[0].s5).sum())
    kp = got["kp"]
    print(name, img.shape, "threshold", thr, "keypoints", got["n"], "restatement", len(ref), "per layer", np.bincount(ref["octave"], minlength=6).tolist())
    assert got["n"] == len(ref) == len(kp) and len(ref) > 0
    if kp.tobytes() != ref.tobytes():
        for f in bd.KP_DTYPE.names:
            bad = np.nonzero(kp[f].view(np.uint32) != ref[f].view(np.uint32))[0]
            if len(bad):
                print("  field", f, ":", len(bad), "rows differ, first", int(bad[0]), kp[bad[0]], ref[bad[0]])
    assert kp.dtype.itemsize == bd.KP_DTYPE.itemsize == 24 and kp.tobytes() == ref.tobytes()


def test_same_bytes_twice_in_one_context_in_a_fresh_one_and_after_another_shape(sample_images):
    """atomics order and stale buffers: a call repeated, repeated after a larger and a smaller image went through the same context, and in a
    fresh context gives identical bytes; a strided view gives what its packed copy gives"""
    img, thr = bc.case("ties")
    a = make_ctx()
    first = a.brisk_detect(img, thr)["kp"]
    second = a.brisk_detect(img, thr)["kp"]
    big, big_thr = bc.image_case("full_size", sample_images)
    a.brisk_detect(big, big_thr)
    a.brisk_detect(bc.case("inexact")[0], 12)
    third = a.brisk_detect(img, thr)["kp"]
    view = big[5:165, 7:307]                                                             # rows are not contiguous
    strided, packed = a.brisk_detect(view, 20)["kp"], a.brisk_detect(np.ascontiguousarray(view), 20)["kp"]
    a.close()
    b = make_ctx()
    fresh = b.brisk_detect(img, thr)["kp"]
    b.close()
    assert len(first) > 100 and first.tobytes() == second.tobytes() == third.tobytes() == fresh.tobytes()
    assert first.tobytes() == bc.reference("ties")[1].tobytes()
    assert len(strided) > 50 and strided.tobytes() == packed.tobytes()


def test_cap_smaller_than_n_and_the_error_statuses(ctx):
    img, thr = bc.case("exact")
    ref = bc.reference("exact")[1]
    lib = ctx.lib
    cap = 37
    buf = np.zeros(cap + 3, capi.BRISK_KP_DTYPE)
    n = capi.C.c_int(0)
    assert lib.spvo_brisk_detect(ctx.h, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], thr, 3, buf.ctypes.data, cap, capi.C.byref(n)) == 0
    assert n.value == len(ref) > cap                                                    # n is reported ...
    assert buf[:cap].tobytes() == ref[:cap].tobytes() and not buf[cap:].tobytes().strip(b"\0")   # ... and exactly cap leading records are written
    assert lib.spvo_brisk_detect(ctx.h, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], thr, 3, None, 0, capi.C.byref(n)) == 0 and n.value == len(ref)
    for octaves in (0, 1, 2, 4):                                                        # only the reference's six layers are built
        with pytest.raises(capi.SpvoError) as e:
            ctx.brisk_detect(img, thr, octaves=octaves)
        assert e.value.code == -1
    for bad_thr in (0, -5, 256):
        with pytest.raises(capi.SpvoError) as e:
            ctx.brisk_detect(img, bad_thr)
        assert e.value.code == -1
    for shape in ((7, 40), (40, 7)):                                                    # below 8 x 8
        with pytest.raises(capi.SpvoError) as e:
            ctx.brisk_detect(np.zeros(shape, np.uint8), thr)
        assert e.value.code == -1
    # rows * cols * 255 >= 2^31 is refused before anything is read (the extractor that follows could not build its int32 integral image)
    assert lib.spvo_brisk_detect(ctx.h, img.ctypes.data, 2903, 2901, 2901, thr, 3, None, 0, capi.C.byref(n)) == -1
    assert lib.spvo_brisk_detect(ctx.h, img.ctypes.data, 65536, 65536, 65536, thr, 3, None, 0, capi.C.byref(n)) == -1
    assert lib.spvo_brisk_detect(ctx.h, None, 96, 144, 144, thr, 3, None, 0, capi.C.byref(n)) == -1                              # no image
    small = ctx.brisk_detect(np.random.RandomState(5).randint(0, 256, (8, 8)).astype(np.uint8), 1)                          # the minimum size runs: layers down to 1 x 1
    assert small["n"] == len(bd.detect(np.random.RandomState(5).randint(0, 256, (8, 8)).astype(np.uint8), 1))
    assert [ctx.brisk_detect_layer(i, 0).shape for i in range(6)] == bd.layer_shapes(8, 8)
    with pytest.raises(capi.SpvoError) as e:
        ctx.brisk_detect_layer(1, 2)                                                    # the 5-8 map exists for layer 0 only
    assert e.value.code == -1
    assert ctx.brisk_detect(img, thr)["kp"].tobytes() == ref.tobytes()                  # the context is still usable
    assert np.array_equal(ctx.brisk_detect_layer(0, 0), img)
    ctx.fast(img)                                                                       # another call takes the resident image over: even the same
    with pytest.raises(capi.SpvoError) as e:                                            # image ends the detector's claim on it
        ctx.brisk_detect_layer(0, 0)
    assert e.value.code == -4
    ctx.brisk_detect(img, thr)
    ctx.fast(np.zeros((300, 400), np.uint8))                                            # a larger image re-allocates the resident buffer ...
    ctx.fast(img)                                                                       # ... and the first shape comes back
    for layer, what in ((0, 0), (3, 1)):
        with pytest.raises(capi.SpvoError) as e:
            ctx.brisk_detect_layer(layer, what)
        assert e.value.code == -4
    assert ctx.brisk_detect(img, thr)["kp"].tobytes() == ref.tobytes() and np.array_equal(ctx.brisk_detect_layer(0, 0), img)


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


@pytest.mark.parametrize("name", ["blobs", "inexact"])
def test_detect_then_describe_on_the_resident_image(ctx, lib_tables, name):
    """spvo_brisk_detect followed by spvo_brisk_describe(img = NULL) with the detector's x, y and size: the rows tests/brisk_ref.py computes
    from the restatement's keypoints; the blobs case reaches scale indices above 0 (the Shi-Tomasi / FAST keypoints never do)"""
    img, thr = bc.case(name)
    ref = bc.reference(name)[1]
    xy = np.stack([ref["x"], ref["y"]], 1)
    r = br.describe(img, xy, ref["size"], tables=lib_tables)
    got = ctx.brisk_detect(img, thr)
    assert got["kp"].tobytes() == ref.tobytes()
    g = ctx.brisk_describe(None, np.stack([got["kp"]["x"], got["kp"]["y"]], 1), got["kp"]["size"], shape=img.shape)
    up = ctx.brisk_describe(img, xy, ref["size"])                                        # the same image uploaded again
    print(name, "keypoints", len(ref), "described", len(r["kept"]), "scale indices", sorted(set(r["scale"].tolist())), "boundary rows", int(r["boundary"].sum()))
    _describe_equals(g, r)
    assert len(r["kept"]) > 0 and g["desc"].tobytes() == up["desc"].tobytes() and g["angle"].tobytes() == up["angle"].tobytes()
    if name == "blobs":
        assert r["scale"].min() > 0 and len(set(r["scale"].tolist())) >= 4


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(3, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def test_brisk_brisk_front_end_pushes_aligned_features(sequence):
    """ClassicFeatureFrontEnd(BRISK, BRISK, BF, ...) at the native resolution: two deque entries, keypoints and 64-byte rows one to one, as
    many as the restatement's detector and the extractor's border rule leave; no error logged.  BRISK keypoints with the ORB descriptor stay
    a pair that does not run."""
    frames, _, P_l, P_r = sequence
    L, R = (np.ascontiguousarray(im[40:200, 300:700]) for im in frames[0])
    n, counts, err = host.classic_pair_probe("BRISK", "BRISK", L, R, P_l, P_r)
    assert n == 2 and err == "", err
    assert counts[0] == counts[1] > 0 and counts[2] == counts[3] > 0 and counts[4] == 64
    for img, got in ((L, counts[0]), (R, counts[2])):
        kp = bd.detect(img, 30)
        assert got == len(br.border_keep(np.stack([kp["x"], kp["y"]], 1), kp["size"], img.shape)[0])
    n, counts, err = host.classic_pair_probe("BRISK", "ORB", L, R, P_l, P_r)
    assert n == 0 and err != ""


def test_classic_front_end_with_brisk_brisk_equals_the_oracle_state_machine(sequence, lib_tables):
    """classic_sequence(frames, detector="BRISK", descriptor="BRISK", input_size=(120, 392)) (KNN) against oracle/odometry.py's FrontEndState
    fed the RESTATEMENT's keypoints (tests/brisk_detect_ref.py on the oracle's preprocessed image), the extractor's rows for them (held to
    tests/brisk_ref.py's by the extractor's own bar) and the Hamming oracle's maps: keypoint, stereo-match and inlier counts identical, poses
    within 1e-6, more than 20 inliers -- the SIFT test's bar.  The translation lies within 0.1 of the synthetic motion: the CPU pipeline on
    the restatement's features gives 0.025 and 0.073 on these frames (NOTES.md, "BRISK detector"), so the SIFT test's bound is asserted.
    With resident=True: the same digests through the per-image path, and no pair counted as resident."""
    frames, gt, P_l, P_r = sequence
    poses, stats, _, digests = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="BRISK", descriptor="BRISK", input_size=(120, 392), trace=True)
    ctx = make_ctx()
    st = od.FrontEndState()
    prev_dl = None
    for k, (L, R) in enumerate(frames):
        feats, Ps = [], []
        for img, P in ((L, P_l), (R, P_r)):
            small, Pk = ofe.preprocess(img, np.asarray(P, np.float64).reshape(3, 4), 120, 392)[:2]
            small = np.ascontiguousarray(small)
            kp = bd.detect(small, 30)
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
    poses_r, stats_r, _, digests_r = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="BRISK", descriptor="BRISK", input_size=(120, 392), resident=True,
                                                           trace=True)
    assert np.array_equal(digests_r, digests) and np.array_equal(stats_r, stats) and np.array_equal(poses_r, poses)
    assert host.classic_resident_pairs() == 0
    with pytest.raises(RuntimeError):                                                   # BRISK keypoints with the default (ORB) descriptor: still not a pair that runs
        host.classic_sequence(frames[:1], P_l, P_r, "KNN", True, 2.0, 4, detector="BRISK")
