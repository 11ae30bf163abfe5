"""spvo_sift_detect / spvo_sift_debug_level / spvo_match_l2 (csrc/sift.hip.h, csrc/spvo_sift.hip) against the numpy restatement
tests/sift_ref.py, and the classic front end with SIFT + SIFT against oracle/odometry.py's state machine.

Tolerances of the stages that are not bit-exact come from the restatement's own float32-versus-float64 figures, measured by
tests/test_sift_ref_cpu.py (YARDSTICKS there): on all three inputs (a) = 0 keys on one side only (<= 0.25 %: every listed input may be
used), (b) = 0 at percentile 99 and at the maximum, largest angle difference 3.05e-5 / 2.29e-5 / 3.05e-5 degrees (kitti / strided / noise)."""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import frontend as ofe, matching, odometry as od
from spvo import capi, host, synth
from tests import sift_cases as sc, sift_ref as sr
from tests.conftest import make_ctx
from tests.test_sift_ref_cpu import YARDSTICKS

pytestmark = pytest.mark.gpu

KEY_SHARE_CAP = 0.01                                        # keys on one side only / the larger list


def desc_bound(name):
    return max(1.0, 2.0 * YARDSTICKS[name][1])             # max(1, 2 x percentile 99 of figure (b)) = 1 on every input


def angle_bound(name):
    return 4.0 * YARDSTICKS[name][3]                        # 4 x the restatement's largest float32 / float64 angle difference


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpu(ctx):
    return {name: ctx.sift_detect(sc.image(name)) for name in sc.NAMES}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sc.NAMES)
def test_pyramid_and_dog_equal_the_restatement_bit_for_bit(ctx, name):
    img = sc.image(name)
    ctx.sift_detect(img, cap=0)
    st = sc.stage(name)
    assert len(st["gauss"]) == sr.octave_count(*img.shape)
    for o, (g, d) in enumerate(zip(st["gauss"], st["dog"])):
        for i, ref in enumerate(g):
            got = ctx.sift_level(o, i)
            assert got.shape == ref.shape and np.array_equal(bits(got), bits(ref)), ("gauss", o, i, float(np.abs(got - ref).max()))
        for i, ref in enumerate(d):
            got = ctx.sift_level(o, i, dog=True)
            assert got.shape == ref.shape and np.array_equal(bits(got), bits(ref)), ("dog", o, i, float(np.abs(got - ref).max()))
    with pytest.raises(capi.SpvoError) as e:
        ctx.sift_level(len(st["gauss"]), 0)
    assert e.value.code == -1


def refined(kp):
    """the candidates that survived refinement, as the set of (packed octave, x, y, size, response) bit patterns -- octave, layer, row and
    column are functions of these (sift_ref.keys)"""
    return {(int(k["octave"]),) + tuple(int(v) for v in bits(np.array([k["x"], k["y"], k["size"], k["response"]]))) for k in kp}


@pytest.mark.parametrize("name", sc.NAMES)
def test_refined_candidates_equal_the_restatement_exactly(gpu, name):
    """Extrema, refinement, contrast and edge tests have one float32 order (division and nothing else correctly rounded on both sides: no
    field needed a tolerance).  A candidate shows in the output through its orientation peaks; one whose histogram has no peak shows on
    neither side."""
    ref = sc.reference(name)
    a, b = refined(gpu[name]["kp"]), refined(ref["kp"])
    print(name, "refined candidates", len(a), len(b), "only gpu", len(a - b), "only ref", len(b - a))
    assert a == b and len(a) > 0
    assert set(sr.keys(gpu[name]["kp"], angle_bin=False)) == set(sr.keys(ref["kp"], angle_bin=False))


@pytest.mark.parametrize("name", sc.NAMES)
def test_keypoints_after_orientation(gpu, name):
    """(a) measured per input: kitti 0, strided 0, noise 0 (float32 against float64 restatement)."""
    ref, got = sc.reference(name), gpu[name]
    c = sc.compare(got, ref)
    print(name, "keypoints", len(got["kp"]), len(ref["kp"]), "share on one side", c["share"], "largest angle difference", float(c["angle"].max()), "bound", angle_bound(name))
    assert YARDSTICKS[name][0] <= 0.0025
    assert c["share"] <= KEY_SHARE_CAP
    assert c["angle"].max() <= angle_bound(name)
    assert [j for _, j in c["common"]] == sorted(j for _, j in c["common"])       # the common keys come in one order


@pytest.mark.parametrize("name", sc.NAMES)
def test_descriptors(gpu, name):
    """(b) measured per input: percentile 99 = 0 and maximum = 0 on kitti, strided and noise."""
    ref, got = sc.reference(name), gpu[name]
    d = got["desc"]
    assert d.dtype == np.float32 and d.shape == (len(got["kp"]), 128) and np.array_equal(d, np.rint(d)) and d.min() >= 0 and d.max() <= 255
    c = sc.compare(got, ref)
    bound = desc_bound(name)
    within = float((c["desc"] <= bound).mean())
    print(name, "rows", len(c["desc"]), "largest difference per row: percentile 50 / 99 / max", float(np.percentile(c["desc"], 50)), float(np.percentile(c["desc"], 99)),
          float(c["desc"].max()), "within", bound, ":", within)
    assert within >= 0.99 and c["desc"].max() <= 4 * bound


def test_buffers_and_calls(ctx, gpu):
    img = sc.image("kitti")
    full = gpu["kitti"]
    n = full["n"]
    assert n == len(full["kp"]) > 100
    part = ctx.sift_detect(img, cap=50)
    assert part["n"] == n and len(part["kp"]) == 50 and part["kp"].tobytes() == full["kp"][:50].tobytes() and part["desc"].tobytes() == full["desc"][:50].tobytes()
    again = ctx.sift_detect(img)
    assert again["kp"].tobytes() == full["kp"].tobytes() and again["desc"].tobytes() == full["desc"].tobytes()
    other = ctx.sift_detect(sc.image("strided"))              # another shape (a strided view) ...
    assert other["kp"].tobytes() == gpu["strided"]["kp"].tobytes() and other["desc"].tobytes() == gpu["strided"]["desc"].tobytes()
    back = ctx.sift_detect(img)                              # ... and the first shape again
    assert back["kp"].tobytes() == full["kp"].tobytes() and back["desc"].tobytes() == full["desc"].tobytes()
    packed = ctx.sift_detect(np.ascontiguousarray(sc.image("strided")))
    assert packed["kp"].tobytes() == other["kp"].tobytes() and packed["desc"].tobytes() == other["desc"].tobytes()
    flat = ctx.sift_detect(sc.image("flat"))
    assert flat["n"] == 0 and len(flat["kp"]) == 0
    with pytest.raises(capi.SpvoError) as e:
        ctx.sift_detect(np.zeros((5, 8), np.uint8))
    assert e.value.code == -1
    assert ctx.sift_detect(np.random.RandomState(3).randint(0, 256, (6, 6)).astype(np.uint8))["n"] >= 0     # the minimum size runs


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(4, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def test_match_l2(ctx, sequence):
    frames, _, P_l, _ = sequence
    L, R = (ofe.preprocess(im, np.asarray(P_l, np.float64).reshape(3, 4), 120, 392)[0] for im in frames[0])
    a, b = ctx.sift_detect(L)["desc"], ctx.sift_detect(R)["desc"]
    assert len(a) > 100 and len(b) > 100
    for sel, cross in (("NN", True), ("KNN", False)):
        idx, dist = ctx.match_l2(a, b, sel, cross, 0.8)
        ridx, rdist = matching.bf_match(a, b, sel, cross, 0.8)
        print(sel, "matches", int((idx >= 0).sum()), int((ridx >= 0).sum()))
        assert np.array_equal(idx, ridx) and np.array_equal(dist[idx >= 0], rdist[ridx >= 0]) and (idx >= 0).sum() > 20
    rs = np.random.RandomState(0)
    u = rs.standard_normal((300, 256)).astype(np.float32)
    v = rs.standard_normal((280, 256)).astype(np.float32)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for sel, cross in (("NN", True), ("KNN", False)):
        i0, d0 = ctx.match(u, v, sel, cross, 0.8)
        i1, d1 = ctx.match_l2(u, v, sel, cross, 0.8, dim=256)
        assert np.array_equal(i0, i1) and d0.tobytes() == d1.tobytes()
    for dim in (0, 257):
        with pytest.raises(capi.SpvoError) as e:
            ctx.match_l2(np.zeros((4, max(dim, 1)), np.float32), np.zeros((4, max(dim, 1)), np.float32), dim=dim)
        assert e.value.code == -1
    idx, _ = ctx.match_l2(a[:40], b[:1], "KNN", False, 0.8)
    assert (idx < 0).all()


def test_classic_front_end_with_sift_equals_the_oracle_state_machine(sequence):
    """classic_sequence(frames[:4], detector="SIFT", input_size=(120, 392)) (SIFT + SIFT, KNN) against oracle/odometry.py's FrontEndState fed
    the context's own sift_detect features and matching.bf_match: keypoint, stereo-match and inlier counts identical, poses within 1e-6,
    more than 20 inliers, translation within 0.1 of the synthetic motion."""
    frames, gt, P_l, P_r = sequence
    frames = frames[:4]
    poses, stats, _ = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="SIFT", input_size=(120, 392))
    ctx = make_ctx()
    st = od.FrontEndState()
    prev_dl = None
    for k, (L, R) in enumerate(frames):
        feats, Ps = [], []
        for img, P in ((L, P_l), (R, P_r)):
            small, Pk = ofe.preprocess(img, np.asarray(P, np.float64).reshape(3, 4), 120, 392)[:2]
            f = ctx.sift_detect(small)
            feats.append((np.stack([f["kp"]["x"], f["kp"]["y"]], 1), f["desc"]))
            Ps.append(Pk)
        (xyl, dl), (xyr, dr) = feats
        od.add_features(st, xyl, dl, xyr, dr, Ps[0], Ps[1])
        idx0, _ = matching.bf_match(dl, dr, "KNN", False, 0.8)
        st.maps[od.PREV_LEFT_PREV_RIGHT] = st.maps[od.CURR_LEFT_CURR_RIGHT]
        st.maps[od.CURR_LEFT_CURR_RIGHT] = idx0
        print(k, "stats", stats[k].tolist(), "oracle", len(xyl), len(xyr), int((idx0 >= 0).sum()))
        assert stats[k, 0] == len(xyl) > 100 and stats[k, 1] == len(xyr) and stats[k, 2] == int((idx0 >= 0).sum())
        if k > 0:
            idx1, _ = matching.bf_match(dl, prev_dl, "KNN", False, 0.8)
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
    with pytest.raises(RuntimeError):
        host.classic_sequence(frames[:1], P_l, P_r, "KNN", True, 2.0, 4, detector="BRISK")
