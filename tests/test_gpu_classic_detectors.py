"""GPU parity of the classic front end's Shi-Tomasi and FAST detectors and of the ORB extractor for given keypoints
(csrc/classic_detect.hip.h; spvo_gftt_detect, spvo_fast_detect, spvo_orb_describe) -- the detectors against the numpy restatement
tests/classic_ref.py bit for bit, the extractor against the compiled ORB oracle (oracle/cpu/orb_cpu.inc), and the two new
configurations of ClassicFeatureFrontEnd (ShiTomasi + ORB, its default constructor; FAST + ORB) through the host class."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import cpu_backend, frontend as ofe, matching, odometry as od
from spvo import capi, host, synth
from tests import classic_ref as cr
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu

CASES = ["kitti", "kitti_view", "kitti_120x392", "noise", "noise_large", "flat"]


def _image(case, sample_images):
    if case == "kitti":
        return sample_images[0]
    if case == "kitti_view":
        return sample_images[1][3:370, 5:1200]                                        # a strided view: rows are not contiguous
    if case == "kitti_120x392":
        return ofe.preprocess(sample_images[2], np.eye(3, 4), 120, 392)[0]            # preprocessImageImpl at the default constructor's size
    if case == "noise":
        return np.random.RandomState(1).randint(0, 256, (200, 320)).astype(np.uint8)   # ties, dense candidates
    if case == "noise_large":
        return np.random.RandomState(2).randint(0, 256, (376, 1241)).astype(np.uint8)  # more than 1000 corners survive the distance rule
    return np.full((120, 160), 77, np.uint8)                                          # no corner at all


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(5, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


@pytest.fixture(scope="module")
def cpu():
    c = cpu_backend.CpuBackend(net_height=64, net_width=96)
    yield c
    c.close()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("case", CASES)
def test_gftt_equals_the_restatement_bit_for_bit(sample_images, case):
    """Coordinates, response bits, count and order.  Counts (restatement, asserted below): sample 0 at its native size keeps 541 of
    1276 candidates, the strided view of sample 1 584, sample 2 at 120 x 392 127 -- the cap of 1000 does not bind; 200 x 320 uniform
    noise keeps 624 of 3679 candidates; on 376 x 1241 uniform noise 4552 survive the distance rule and the cap binds (as it does on
    sample 0 at quality level 0.001: test_gftt_parameters_and_buffers_follow_the_call)."""
    img = _image(case, sample_images)
    r = cr.gftt(np.ascontiguousarray(img))
    n = len(r["xy"])
    print(case, "restatement: candidates", len(r["candidates"]), "kept", len(r["kept_all"]), "returned", n)
    if case == "flat":
        assert n == 0
    elif case == "noise_large":
        assert n == 1000 and len(r["kept_all"]) > 1000                                 # the cap binds
    else:
        assert 100 < n < 1000 and len(r["kept_all"]) == n                              # it does not
    ctx = make_ctx()
    g = ctx.gftt(img)
    rem, fin = ctx.gftt_rounds()
    print(case, "gpu: n", len(g["xy"]), "undecided after the round launches", rem.tolist(), "finish rounds", fin)
    ctx.close()
    assert len(g["xy"]) == n
    assert _same_bits(g["xy"], r["xy"]) and _same_bits(g["response"], r["response"])


def test_gftt_parameters_and_buffers_follow_the_call(sample_images):
    """One context, several shapes and parameter sets in turn (a later image with fewer pixels but longer rows, then the first shape
    again); other max_corners / quality / min_distance; what is not built answers SPVO_ERR_INVALID and leaves the context usable."""
    rng = np.random.RandomState(7)
    ctx = make_ctx()
    for shape in ((400, 400), (100, 1500), (700, 120), (400, 400)):
        img = rng.randint(0, 256, shape).astype(np.uint8)
        g, r = ctx.gftt(img), cr.gftt(img)
        assert len(r["xy"]) > 100 and _same_bits(g["xy"], r["xy"]) and _same_bits(g["response"], r["response"]), shape
    img = sample_images[0]
    for kw in (dict(max_corners=200), dict(quality=0.001), dict(min_distance=3.0), dict(min_distance=15.0), dict(min_distance=0.5, max_corners=5000)):
        g, r = ctx.gftt(img, **kw), cr.gftt(img, **kw)
        assert len(r["xy"]) > 50 and _same_bits(g["xy"], r["xy"]) and _same_bits(g["response"], r["response"]), kw
    assert len(cr.gftt(img, quality=0.001)["xy"]) == 1000                              # the cap binds on a KITTI sample at this quality level
    for kw in (dict(block_size=3), dict(min_distance=16.0)):
        with pytest.raises(capi.SpvoError) as e:
            ctx.gftt(img, **kw)
        assert e.value.code == -1                                                   # SPVO_ERR_INVALID
    g = ctx.gftt(img)
    assert _same_bits(g["xy"], cr.gftt(img)["xy"])
    ctx.close()


@pytest.mark.parametrize("case", CASES)
def test_fast_equals_the_restatement_bit_for_bit(sample_images, case):
    """Thresholds 10 and 20, suppression on and off, one context for all four.  On the noise images far more than 2048 corners come
    back: nothing downstream of the score is sized by a fixed keypoint count."""
    img = _image(case, sample_images)
    ctx = make_ctx()
    for t in (10, 20):
        for nms in (True, False):
            r = cr.fast(np.ascontiguousarray(img), t, nms)
            g = ctx.fast(img, t, nms)
            print(case, t, nms, "restatement", len(r["xy"]), "gpu", len(g["xy"]))
            if case == "flat":
                assert len(r["xy"]) == 0
            elif case.startswith("noise"):
                assert len(r["xy"]) > 2048
            else:
                assert len(r["xy"]) > 200
            assert len(g["xy"]) == len(r["xy"])
            assert _same_bits(g["xy"], r["xy"]) and _same_bits(g["response"], r["response"]), (t, nms)
    ctx.close()


@pytest.mark.parametrize("which", [0, 1])
def test_orb_describe_equals_the_compiled_oracle_on_its_own_keypoints(cpu, sample_images, which):
    """The octave-0 keypoints of the compiled ORB oracle, handed over in shuffled order: all kept, the 32 descriptor bytes equal,
    the direction within 1e-5 rad."""
    img = sample_images[which]
    r = cpu.orb(img)
    m = r["octave"] == 0
    assert 300 < m.sum() < 600
    perm = np.random.RandomState(5).permutation(int(m.sum()))
    xy, desc, angle = r["xy"][m][perm], r["desc"][m][perm], r["angle"][m][perm]
    ctx = make_ctx()
    g = ctx.orb_describe(img, xy)
    ctx.close()
    assert np.array_equal(g["kept"], np.arange(len(xy)))
    assert np.array_equal(g["desc"], desc)
    d = np.abs(g["angle"] - angle)
    assert np.minimum(d, 2 * np.pi - d).max() <= 1e-5


def test_orb_describe_border_rule_independence_and_the_resident_image(sample_images):
    img = sample_images[0]
    h, w = img.shape
    ctx = make_ctx()
    with pytest.raises(capi.SpvoError) as e:                                           # nothing resident yet
        ctx.orb_describe(None, np.array([[100, 100]], np.float32), shape=img.shape)
    assert e.value.code == -4                                                       # SPVO_ERR_STATE
    f = ctx.fast(img)
    xy = f["xy"]
    keep = cr.orb_border_keep(xy, img.shape)
    assert 0 < len(keep) < len(xy)                                                     # FAST's border is 3 pixels, the extractor's 31
    res = ctx.orb_describe(None, xy)                                                   # the image of the detect call, still on the device
    assert np.array_equal(res["kept"], keep) and np.all(np.diff(res["kept"]) > 0)
    kx, ky = xy[res["kept"], 0], xy[res["kept"], 1]
    assert kx.min() >= 31 and kx.max() < w - 31 and ky.min() >= 31 and ky.max() < h - 31
    up = ctx.orb_describe(img, xy)                                                     # the same image uploaded again
    assert np.array_equal(up["kept"], res["kept"]) and np.array_equal(up["desc"], res["desc"]) and np.array_equal(up["angle"], res["angle"])
    # a keypoint's descriptor does not depend on which others are in the list
    pick = np.random.RandomState(9).choice(len(xy), 300, replace=False)
    sub = ctx.orb_describe(None, xy[pick])
    pos = {int(i): k for k, i in enumerate(res["kept"])}
    rows = [pos[int(pick[j])] for j in sub["kept"]]
    assert len(rows) > 100 and np.array_equal(sub["desc"], res["desc"][rows]) and np.array_equal(sub["angle"], res["angle"][rows])
    # edge cases: all dropped, empty list, a shape that is not the resident one, non-integer coordinates
    edge = ctx.orb_describe(None, np.array([[30, 100], [100, 30], [w - 31, 100], [100, h - 31]], np.float32))
    assert len(edge["kept"]) == 0 and edge["desc"].shape == (0, 32)
    assert len(ctx.orb_describe(None, np.zeros((0, 2), np.float32))["kept"]) == 0
    inside = ctx.orb_describe(None, np.array([[31, 31], [w - 32, h - 32]], np.float32))
    assert np.array_equal(inside["kept"], [0, 1])
    with pytest.raises(capi.SpvoError) as e:
        ctx.orb_describe(None, xy[:10], shape=(h - 1, w))
    assert e.value.code == -4
    with pytest.raises(capi.SpvoError) as e:
        ctx.orb_describe(None, np.array([[100.5, 100]], np.float32))
    assert e.value.code == -1
    # after a Shi-Tomasi detect the resident image is that call's
    other = sample_images[1]
    g = ctx.gftt(other)
    a = ctx.orb_describe(None, g["xy"])
    b = ctx.orb_describe(other, g["xy"])
    assert len(a["kept"]) > 100 and np.array_equal(a["kept"], b["kept"]) and np.array_equal(a["desc"], b["desc"])
    ctx.close()


def test_the_default_constructed_classic_front_end_produces_aligned_features(sequence):
    """ClassicFeatureFrontEnd() = ShiTomasi + ORB, BF, NN, cross-check, 120 x 392: one stereo pair fills the deques, keypoints and
    descriptor rows one to one (the extractor's drops are erased from the keypoint vectors), as many as the restatement says."""
    frames, _, P_l, P_r = sequence
    L, R = frames[0]
    n, counts, err = host.classic_default_probe(L, R, P_l, P_r)
    assert n == 2, err
    assert counts[0] == counts[1] > 0 and counts[2] == counts[3] > 0
    for img, got in ((L, counts[0]), (R, counts[2])):
        small = ofe.preprocess(img, np.asarray(P_l, np.float64).reshape(3, 4), 120, 392)[0]
        xy = cr.gftt(small)["xy"]
        assert got == len(cr.orb_border_keep(xy, small.shape))


def _oracle_sequence(frames, P_l, P_r, detect):
    """oracle/odometry.py's state machine on the restatement's keypoints, the entry point's descriptors and the Hamming oracle's maps
    (KNN: no cross-check, base.cpp:27-28; the classic constructor passes stereo_threshold as min_disparity, hpp:203-206)"""
    ctx = make_ctx()
    st = od.FrontEndState()
    out = []
    prev_dl = None
    for k, (L, R) in enumerate(frames):
        feats = []
        for img in (L, R):
            xy = detect(np.ascontiguousarray(img))["xy"]
            d = ctx.orb_describe(img, xy)
            assert np.array_equal(d["kept"], cr.orb_border_keep(xy, img.shape))
            feats.append((xy[d["kept"]], d["desc"]))
        (xyl, dl), (xyr, dr) = feats
        od.add_features(st, xyl, dl, xyr, dr, P_l, P_r)
        idx0, _ = matching.bf_match_hamming(dl, dr, "KNN", False, 0.8)
        st.maps[od.PREV_LEFT_PREV_RIGHT] = st.maps[od.CURR_LEFT_CURR_RIGHT]
        st.maps[od.CURR_LEFT_CURR_RIGHT] = idx0
        rec = dict(n_l=len(xyl), n_r=len(xyr), n_stereo=int((idx0 >= 0).sum()))
        if k > 0:
            idx1, _ = matching.bf_match_hamming(dl, prev_dl, "KNN", False, 0.8)
            st.maps[od.CURR_LEFT_PREV_LEFT] = idx1
            q, t, dbg = od.solve_stereo_odometry(st, 2.0, 2.0, 4)
            rec.update(q=q, t=t, n_inliers=len(dbg["inliers"]), n_join=len(dbg["join"]["post"]))
        prev_dl = dl
        out.append(rec)
    ctx.close()
    return out


@pytest.mark.parametrize("detector", ["ShiTomasi", "FAST"])
def test_classic_front_end_with_the_new_detectors_equals_the_oracle_state_machine(sequence, detector):
    """classic_sequence(frames[:4], detector=...) (KNN, native size, refinement degree 4) against oracle/odometry.py's FrontEndState:
    keypoint, stereo-match and PnP inlier counts identical, poses within 1e-6, translation within 0.1 of the synthetic motion."""
    frames, gt, P_l, P_r = sequence
    frames = frames[:4]
    poses, stats, _ = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector=detector)
    ref = _oracle_sequence(frames, P_l, P_r, cr.gftt if detector == "ShiTomasi" else cr.fast)
    for k, r in enumerate(ref):
        print(detector, k, "stats", stats[k].tolist(), "oracle", {a: b for a, b in r.items() if a not in ("q", "t")})
        if k:
            Rc, Rg = od.quat_to_rot(np.asarray(r["q"])), od.quat_to_rot(poses[k, :4])
            print("   pose difference: R %.3g t %.3g; t vs synthetic motion %.3g" % (np.abs(Rg - Rc).max(), np.abs(poses[k, 4:] - r["t"]).max(),
                                                                                    np.abs(poses[k, 4:] - synth.relative_pose(gt[k - 1], gt[k])[1]).max()))
    for k, r in enumerate(ref):
        assert stats[k, 0] == r["n_l"] > 100 and stats[k, 1] == r["n_r"] and stats[k, 2] == r["n_stereo"]
        if k == 0:
            continue
        assert stats[k, 3] == r["n_inliers"] and r["n_inliers"] > 20
        Rc, Rg = od.quat_to_rot(np.asarray(r["q"])), od.quat_to_rot(poses[k, :4])      # both: cam0_curr_T_cam0_prev
        assert np.abs(Rg - Rc).max() <= 1e-6 and np.abs(poses[k, 4:] - r["t"]).max() <= 1e-6
        _, tt = synth.relative_pose(gt[k - 1], gt[k])
        assert np.abs(poses[k, 4:] - tt).max() < 0.1


def test_orb_through_the_extended_export_is_what_the_first_export_returns(sequence):
    import ctypes as C
    frames, _, P_l, P_r = sequence
    frames = frames[:3]
    poses, stats, _ = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4)     # defaults: detector "ORB", native resolution
    lib = host.load()
    lib.spvo_host_classic_sequence.restype = C.c_int
    lib.spvo_host_classic_sequence.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                               C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    n = len(frames)
    ls = [np.ascontiguousarray(f[0], np.uint8) for f in frames]
    rs = [np.ascontiguousarray(f[1], np.uint8) for f in frames]
    pl = (C.c_void_p * n)(*[a.ctypes.data for a in ls])
    pr = (C.c_void_p * n)(*[a.ctypes.data for a in rs])
    Pl = np.ascontiguousarray(P_l, np.float64).reshape(12)
    Pr = np.ascontiguousarray(P_r, np.float64).reshape(12)
    poses0 = np.zeros((n, 7), np.float64)
    stats0 = np.zeros((n, 4), np.int32)
    sec = C.c_double(0)
    assert lib.spvo_host_classic_sequence(n, pl, pr, ls[0].shape[0], ls[0].shape[1], Pl.ctypes.data, Pr.ctypes.data, 1, 1, 2.0, 4, 0, poses0.ctypes.data,
                                          stats0.ctypes.data, C.byref(sec)) == n
    assert np.array_equal(stats, stats0) and np.array_equal(poses, poses0) and (stats[:, 0] == 2000).all()
    with pytest.raises(ValueError):
        host.classic_sequence(frames, P_l, P_r, detector="HARRIS")
    with pytest.raises(RuntimeError):                                                  # still an OpenCV call: nothing is pushed
        host.classic_sequence(frames, P_l, P_r, detector="BRISK")
