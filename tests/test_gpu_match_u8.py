"""The byte-L2 matcher on the GPU (MatcherType::FLANN on binary descriptors; match.hip.h K12u through spvo_match_l2_u8 and
spvo_match_l2_u8_slots) against oracle.matching.bf_match on the rows cast to float32: indices equal, distances equal AS BITS.  No tolerance
anywhere (tests/match_u8_cases.py says why none is needed)."""
import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import matching
from spvo import capi
from tests import match_u8_cases as mc
from tests.conftest import make_ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


def check(ctx, a, b, what=""):
    """the three modes through spvo_match_l2_u8 against the oracle; -> the results by mode"""
    d2 = matching.sq_distances(a.astype(np.float32), b.astype(np.float32)) if len(a) and len(b) else None
    out = {}
    for sel, cross in mc.MODES:
        got = ctx.match_l2_u8(a, b, sel, cross, 0.8)
        ref = matching.bf_match(a.astype(np.float32), b.astype(np.float32), sel, cross, 0.8, d2=d2)
        if not mc.same_bits(got, ref):
            bad = np.nonzero((got[0] != ref[0]) | (got[1].view(np.uint32) != ref[1].view(np.uint32)))[0]
            print(what, a.shape, b.shape, sel, cross, len(bad), "rows differ, first", int(bad[0]), "got", got[0][bad[0]], got[1][bad[0]], "oracle", ref[0][bad[0]], ref[1][bad[0]])
        assert mc.same_bits(got, ref), (what, a.shape, b.shape, sel, cross)
        out[(sel, cross)] = got
    return out


# ---------------------------------------------------------------- the kernel through spvo_match_l2_u8
@pytest.mark.parametrize("width", mc.WIDTHS)
def test_random_bytes(ctx, width):
    for na, nb in mc.SHAPES:
        a, b = mc.random_rows(width, na, nb)
        out = check(ctx, a, b, "random")
        if nb == 1:
            assert (out[("KNN", False)][0] == -1).all()                # knnMatch(k = 2) on one train row: nothing passes the ratio test
        if na >= 64:
            assert (out[("KNN", False)][0] >= 0).any() and (out[("KNN", False)][0] < 0).any()


@pytest.mark.parametrize("width", [32, 61, 64])
def test_tile_boundaries(ctx, width):
    """one row less, exactly and one row more than the kernel's query block and train tile, on either side; more than one tile"""
    for na, nb in mc.TILE_SHAPES:
        a, b = mc.random_rows(width, na, nb)
        check(ctx, a, b, "tiles")


def test_empty_sides(ctx):
    a, _ = mc.random_rows(32, 5, 5)
    for sel, cross in mc.MODES:
        idx, dist = ctx.match_l2_u8(a, a[:0], sel, cross, 0.8)
        assert idx.tolist() == [-1] * 5 and dist.tolist() == [0.0] * 5
        idx, dist = ctx.match_l2_u8(a[:0], a, sel, cross, 0.8)
        assert len(idx) == 0 and len(dist) == 0


def test_argument_rules(ctx):
    a = np.zeros((2, 65), np.uint8)
    with pytest.raises(capi.SpvoError) as e:
        ctx.match_l2_u8(a, a)
    assert e.value.code == -1 and "1 .. 64" in str(e.value)
    rows = np.zeros((2, 32), np.uint8)
    idx, dist = np.zeros(2, np.int32), np.zeros(2, np.float32)
    assert ctx.lib.spvo_match_l2_u8(ctx.h, rows.ctypes.data, 2, rows.ctypes.data, 2, 32, 7, 0, 0.8, idx.ctypes.data, dist.ctypes.data) == -1   # bad selector
    assert ctx.lib.spvo_match_l2_u8(ctx.h, None, 2, rows.ctypes.data, 2, 32, 1, 0, 0.8, idx.ctypes.data, dist.ctypes.data) == -1


@pytest.mark.parametrize("width", [32, 61, 64])
def test_it_is_not_a_hamming_search(ctx, width):
    a, b = mc.not_hamming(width)
    out = check(ctx, a, b, "not hamming")
    idx, dist = out[("NN", False)]
    assert idx.tolist() == [1, 1, 1] and np.all(dist == np.float32(np.sqrt(np.float32(8))))
    assert ctx.match_hamming(a, b, "NN", False)[0].tolist() == [0, 0, 0]


def test_full_range_survives_the_key(ctx):
    """d2 = 4 161 600 as the nearest and as the second nearest distance"""
    a, b = mc.full_range()
    out = check(ctx, a, b, "range")
    one = check(ctx, a[:1], b[:2], "range")
    assert one[("NN", False)][1][0] == np.float32(2040.0) and one[("NN", False)][0][0] == 0
    assert one[("KNN", False)][0][0] == -1                             # 2040 < 0.8 * 2040 is false: the second nearest came through intact
    assert out[("KNN", False)][0].tolist() == [2, 2] and out[("KNN", False)][1].tolist() == [56.0, 0.0]   # 56 < 0.8 * 2040: the second nearest is 2040 there


def test_sign_boundary_and_ties(ctx):
    a, b = mc.sign_and_ties()
    out = check(ctx, a, b, "ties")
    assert out[("NN", False)][0].tolist() == [11, 11, 11, 5, 5]
    assert out[("NN", False)][1].tolist() == [0, 0, 0, 0, 8.0]
    assert out[("NN", True)][0][0] == 11 and out[("NN", True)][0][3] == 5
    check(ctx, b, a, "ties, sides swapped")


def test_ratio_boundary(ctx):
    got = []
    for k0, k1 in mc.RATIO_BOUNDARY:
        a, b = mc.ratio_boundary(k0, k1)
        got.append(int(check(ctx, a, b, "ratio")[("KNN", False)][0][0]))
    assert got == [-1, 0, -1, 0]                                       # 4 < 0.8f * 5 is false in float32


@pytest.mark.parametrize("width", [32, 61])
def test_equals_the_float_route(ctx, width):
    """spvo_match_l2 on the float casts of the same rows: the same answer, indices and distance bits"""
    a, b = mc.random_rows(width, 300, 517)
    for sel, cross in mc.MODES:
        got = ctx.match_l2_u8(a, b, sel, cross, 0.8)
        flt = ctx.match_l2(a.astype(np.float32), b.astype(np.float32), sel, cross, 0.8)
        assert mc.same_bits(got, flt), (sel, cross)


# ---------------------------------------------------------------- slots
@pytest.mark.parametrize("width", [32, 64])
def test_caller_filled_slots(ctx, width):
    a, b = mc.random_rows(width, 257, 300)
    ctx.classic_slot_fill(0, a)
    ctx.classic_slot_fill(1, b)
    ctx.classic_slot_fill(2, a[:0])
    ref = check(ctx, a, b, "slots")
    for (sel, cross), r in ref.items():
        assert mc.same_bits(ctx.match_l2_u8_slots(0, 1, sel, cross, 0.8), r), (sel, cross)
        idx, dist = ctx.match_l2_u8_slots(0, 2, sel, cross, 0.8)       # an empty train slot
        assert (idx == -1).all() and (dist == 0).all() and len(idx) == len(a)
        idx, dist = ctx.match_l2_u8_slots(2, 1, sel, cross, 0.8)       # an empty query slot
        assert len(idx) == 0


def test_slot_status_codes(ctx):
    ctx.classic_slot_fill(0, np.zeros((4, 32), np.uint8))
    ctx.classic_slot_fill(1, np.zeros((4, 64), np.uint8))
    with pytest.raises(capi.SpvoError) as e:
        ctx.match_l2_u8_slots(0, 1)
    assert e.value.code == -1 and "32 bytes" in str(e.value) and "64 bytes" in str(e.value)
    c = make_ctx()
    try:
        c.classic_slot_fill(0, np.zeros((4, 32), np.uint8))
        with pytest.raises(capi.SpvoError) as e:                       # a slot nothing was ever written to
            c.match_l2_u8_slots(0, 5)
        assert e.value.code == -4
        assert c.lib.spvo_set_binary_prematch_norm(c.h, 2) == -1        # neither norm
    finally:
        c.close()


@pytest.fixture(scope="module")
def crops(sample_images):
    """two different images of one small shape cut from the golden images: (left, right)"""
    l = np.ascontiguousarray(sample_images[0][100:260, 300:692])
    r = np.ascontiguousarray(sample_images[1][100:260, 300:692])
    return l, r


def pair_call(c, route, crops, sl, sr):
    l, r = crops
    if route == "ORB":
        return c.classic_detect(l, r, sl, sr, "ORB", slot_capacity=2048)
    if route == "ShiTomasi+BRISK":
        return c.classic_detect(l, r, sl, sr, "ShiTomasi+BRISK", slot_capacity=2048)
    return c.akaze_detect_pair(l, r, sl, sr, slot_capacity=2048)


@pytest.mark.parametrize("route,width", [("ORB", 32), ("ShiTomasi+BRISK", 64), ("AKAZE", 61)])
def test_prematch_under_the_l2_norm(crops, route, width):
    """spvo_set_binary_prematch_norm(L2) with spvo_set_prematch on: the pair call's stored match is what spvo_match_l2_u8_slots hands out --
    equal to a context's that stores nothing and to the oracle on the rows the call handed out; back under the Hamming norm the Hamming
    query is the Hamming oracle's and the L2 query is computed again, not served from a stale entry."""
    for sel, cross in [("KNN", False), ("NN", True)]:
        on, off = make_ctx(), make_ctx()
        try:
            on.set_binary_prematch_norm("L2")
            on.set_prematch(True, sel, cross, 0.8)
            fl, fr = pair_call(on, route, crops, 0, 1)
            pair_call(off, route, crops, 0, 1)
            da, db = fl["desc"], fr["desc"]
            assert da.shape[1] == width and len(da) > 10 and len(db) > 10, (da.shape, db.shape)
            ref = mc.oracle_match(da, db, sel, cross)
            stored = on.match_l2_u8_slots(0, 1, sel, cross, 0.8)
            assert mc.same_bits(stored, ref) and (ref[0] >= 0).sum() > 3
            assert mc.same_bits(off.match_l2_u8_slots(0, 1, sel, cross, 0.8), ref)
            # a Hamming query is never served the stored L2 result ...
            href = matching.bf_match_hamming(da, db, sel, cross, 0.8)
            assert mc.same_bits(on.match_hamming_slots(0, 1, sel, cross, 0.8), href)
            assert not np.array_equal(href[1], ref[1])
            # ... and after the norm went back, both queries still say what they should (the stored entry was dropped)
            on.set_binary_prematch_norm("HAMMING")
            assert mc.same_bits(on.match_hamming_slots(0, 1, sel, cross, 0.8), href)
            assert mc.same_bits(on.match_l2_u8_slots(0, 1, sel, cross, 0.8), ref)
            # a pair call under the Hamming norm stores a Hamming match: the L2 query of the same slots is computed, not served that
            fl2, fr2 = pair_call(on, route, crops[::-1], 2, 3)
            ref2 = mc.oracle_match(fl2["desc"], fr2["desc"], sel, cross)
            assert mc.same_bits(on.match_l2_u8_slots(2, 3, sel, cross, 0.8), ref2)
            assert mc.same_bits(on.match_hamming_slots(2, 3, sel, cross, 0.8), matching.bf_match_hamming(fl2["desc"], fr2["desc"], sel, cross, 0.8))
        finally:
            on.close()
            off.close()
