"""MatcherType::FLANN through the host class (host/feature_detection.cpp: initMatcher, matchDescriptors; ClassicFeatureFrontEnd::residentPair).
FLANN here is the exact L2 search the reference's randomized KD-trees approximate, so the maps are oracle.matching.bf_match's on the rows
cast to float32 with the cross-check OFF (cv::FlannBasedMatcher has none), equal index for index; matchDescriptors leaves both descriptor
matrices CV_32F as the reference's in-place conversion does."""
import os
import shutil

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import host, synth, weights
from tests import match_u8_cases as mc

pytestmark = pytest.mark.gpu

CV_8U, CV_32F = 0, 5
STEREO, TEMPORAL = host.CURR_LEFT_CURR_RIGHT, host.CURR_LEFT_PREV_LEFT


def feature_sets(width, seed=3):
    """prevL, prevR, currL, currR with stereo and temporal partners, some of them one step away"""
    rng = np.random.RandomState(seed + width)
    sets = [rng.randint(0, 256, (n, width)).astype(np.uint8) for n in (300, 280, 330, 310)]
    sets[3][:120] = sets[2][40:160]
    sets[3][:120:3, 1] ^= 2
    sets[0][50:200] = sets[2][100:250]
    sets[0][50:100, 2] ^= 1
    return sets


@pytest.mark.parametrize("selector,cross", [("KNN", False), ("NN", True)])
@pytest.mark.parametrize("width", [32, 61, 64])
def test_pushed_deques(selector, cross, width):
    """the stereo match on two fresh CV_8U matrices (spvo_match_l2_u8), then the temporal match that meets the converted current-left
    matrix and a fresh CV_8U previous-left one (spvo_match_l2 on the float rows): both maps are the oracle's without a cross-check, and
    every entry touched is CV_32F afterwards"""
    sets = feature_sets(width)
    maps, depths, err = host.classic_match(sets, [STEREO, TEMPORAL], "ORB", "FLANN", selector, cross)
    assert err == ""
    ref_s = mc.oracle_match(sets[2], sets[3], selector, False)[0]
    ref_t = mc.oracle_match(sets[2], sets[0], selector, False)[0]
    assert np.array_equal(maps[0], ref_s) and np.array_equal(maps[1], ref_t)
    assert (ref_s >= 0).sum() > 50 and (ref_t >= 0).sum() > 50
    if selector == "NN":                                               # a cross-check would have dropped rows: it was not applied
        assert (mc.oracle_match(sets[2], sets[3], "NN", True)[0] < 0).any() and (maps[0] >= 0).all()
    assert depths.tolist() == [CV_32F, CV_8U, CV_32F, CV_32F]           # prevR was not touched
    # the stereo match alone leaves the previous frame's matrices as they were
    maps, depths, err = host.classic_match(sets, [STEREO], "ORB", "FLANN", selector, cross)
    assert err == "" and np.array_equal(maps[0], ref_s) and depths.tolist() == [CV_8U, CV_8U, CV_32F, CV_32F]
    # both sides converted by earlier calls: the float route again, the same map
    maps, depths, err = host.classic_match(sets, [STEREO, TEMPORAL, TEMPORAL], "ORB", "FLANN", selector, cross)
    assert err == "" and np.array_equal(maps[2], ref_t)


def test_bf_on_the_same_deques_is_still_hamming():
    from oracle import matching
    sets = feature_sets(32)
    maps, depths, err = host.classic_match(sets, [STEREO], "ORB", "BF", "KNN", False)
    assert err == "" and np.array_equal(maps[0], matching.bf_match_hamming(sets[2], sets[3], "KNN", False)[0])
    assert depths.tolist() == [CV_8U] * 4


@pytest.mark.parametrize("selector", ["KNN", "NN"])
def test_sift_rows_take_the_l2_route_unchanged(selector):
    """SIFT + SIFT: FLANN gives the maps of BF with the cross-check off (integers 0 .. 255 in 128 float columns)"""
    rng = np.random.RandomState(11)
    sets = [rng.randint(0, 256, (n, 128)).astype(np.float32) for n in (200, 190, 220, 210)]
    sets[3][:90] = sets[2][30:120]
    sets[0][20:120] = sets[2][100:200]
    flann, depths, err = host.classic_match(sets, [STEREO, TEMPORAL], "SIFT", "FLANN", selector, True)
    assert err == "" and depths.tolist() == [CV_32F] * 4
    bf, _, err = host.classic_match(sets, [STEREO, TEMPORAL], "SIFT", "BF", selector, False)
    assert err == ""
    for a, b in zip(flann, bf):
        assert np.array_equal(a, b) and (a >= 0).sum() > 50


@pytest.fixture(scope="module")
def sequence(golden_dir):
    return synth.stereo_sequence(12, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)


def test_sequence_is_identical_with_resident_features(sequence):
    """ORB + ORB, FLANN, KNN over 12 synthetic frames, per-image (spvo_match_l2_u8 / spvo_match_l2 on the host matrices) against
    setDeviceResident (spvo_match_l2_u8_slots, served by the pair call's prematch under SPVO_NORM_L2): poses, stats and the digests of every
    deque entry, match list and inlier set are identical -- and not BF's"""
    frames, _, P_l, P_r = sequence
    p0, s0, _, d0 = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="ORB", trace=True, matcher="FLANN")
    assert host.classic_resident_pairs() == 0
    p1, s1, _, d1 = host.classic_sequence(frames, P_l, P_r, "KNN", True, 2.0, 4, detector="ORB", trace=True, matcher="FLANN", resident=True)
    assert host.classic_resident_pairs() > 0
    assert s0[:, 0].min() > 100 and s0[:, 2].min() > 10 and s0[1:, 3].max() > 10
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(p0, p1)
    _, sb, _, db = host.classic_sequence(frames[:2], P_l, P_r, "KNN", True, 2.0, 4, detector="ORB", trace=True)
    assert not np.array_equal(db[:, 4], d0[:2, 4])                     # another norm, other matches


@pytest.fixture(scope="module")
def models_dir(tmp_path_factory, squeeze_weights_path):
    d = tmp_path_factory.mktemp("models")
    os.makedirs(d / "laptop")
    shutil.copyfile(squeeze_weights_path, d / "laptop" / weights.engine_name("sp_squeeze", 2, 360, 1176, "FP32"))
    return str(d)


@pytest.mark.parametrize("selector", ["KNN", "NN"])
def test_superpoint_front_end(models_dir, sequence, selector):
    """the SuperPoint front end: FLANN (cross_check = true, not looked at) gives the maps of BF with the cross-check off"""
    frames, _, P_l, P_r = sequence
    out = {}
    for matcher, cross in (("FLANN", True), ("BF", False)):
        fe = host.FrontEnd(models_dir, prefix="sp_squeeze", selector=selector, cross_check=cross, matcher=matcher)
        try:
            assert fe.engine_loaded, fe.last_error
            maps = []
            for k in range(2):
                fe.step(frames[k][0], frames[k][1], P_l, P_r)
                assert "matchDescriptors" not in fe.last_error and "initMatcher" not in fe.last_error, fe.last_error
                maps.append(fe.map_of_indices(STEREO))
            maps.append(fe.map_of_indices(TEMPORAL))
            out[matcher] = maps
        finally:
            fe.close()
    for a, b in zip(out["FLANN"], out["BF"]):
        assert len(a) > 100 and np.array_equal(a, b) and (a >= 0).sum() > 20
