"""The keypoint-list steps the detectors' and extractors' kernels share (csrc/list_steps.hip.h) at the edges of the one-workgroup
compaction's chunks of 1024 and of the rank kernels' tile, at every site a test can reach.

Sites with a hook that takes a caller's list -- spvo_sift_link_debug (sift_link_compact_kernel), spvo_brisk_describe (brisk_compact_kernel:
the border rule on top of the walk), spvo_akaze_suppress_debug (akaze_suppress_compact_kernel) -- get every length of LENGTHS crossed with
the keep patterns of patterns(): the kept indices are the pattern's, in ascending order, by the definition each neighbouring suite uses
(the hook's contract, tests/brisk_ref.py, tests/akaze_suppress_cases.py).  One resident image of 64 x 96 serves the two hooks that read one.
The suppression hook reads no image, only the level tables of a shape, and 64 x 96 cannot hold the lists: level-0 candidates must lie more
than 2.4 pixels apart not to suppress one another (a squared distance of 8 or more on the pixel grid: at most one candidate per 6.9 of its
6144 pixels), so 2049 of them do not fit -- the lists are laid out on level 0 of a 192 x 288 shape, where the radius is the same.

Sites without a list hook -- cls_compact_kernel, brisk_det_compact_kernel, cls_rank_kernel, orb_rank_kernel -- run once through their
entry points on 120 x 392 uniform noise, chosen so that every list is longer than 1024 entries (asserted from the CPU restatements), and
are compared with the restatements exactly as the neighbouring suites compare them."""
import os
import re

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import cpu_backend
from spvo import capi
from tests import akaze_ref as ak, akaze_suppress_cases as sc, brisk_detect_ref as bd, brisk_ref as br, classic_ref as cr, sift_describe_cases as dc
from tests.conftest import PKG, make_ctx

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049]
AKAZE_SHAPE = (192, 288)


def patterns(n):
    """name -> keep flags [n]; the two single indices on either side of the first chunk edge where the list has them"""
    i = np.arange(n)
    p = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "every third": i % 3 == 0, "only the last": i == n - 1}
    if n > 1023:
        p["only index 1023"] = i == 1023
    if n > 1024:
        p["only index 1024"] = i == 1024
    return p


@pytest.fixture(scope="module")
def image():
    img = dc.image("brisk_style")
    assert img.shape == (64, 96)
    return img


@pytest.fixture(scope="module")
def noise():
    return np.random.RandomState(3).randint(0, 256, (120, 392)).astype(np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def rank_tile():
    with open(os.path.join(PKG, "csrc", "spvo_types.hip.h")) as f:
        return int(re.search(r"constexpr int RANK_TILE = (\d+);", f.read()).group(1))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------- 1. the walk at the sites with a list hook
@pytest.mark.parametrize("n", LENGTHS)
def test_sift_link_keeps_the_flagged_indices_in_order(ctx, image, n):
    """spvo_sift_link_debug's contract: kept = the indices whose flag is set, ascending; rows as spvo_sift_describe on those records"""
    base = dc.keypoints("brisk_style").astype(capi.SIFT_KP_DTYPE)
    kp = base[np.arange(n) % len(base)]
    ctx.fast(image)                                                    # any detector call leaves the image resident
    for name, keep in patterns(n).items():
        live = np.nonzero(keep)[0]
        got = ctx.sift_link_debug(kp, keep, 5, shape=image.shape)
        print(n, name, "kept", len(got["kept"]), "of", len(live))
        assert got["kept"].dtype == np.int32 and np.array_equal(got["kept"], live), (n, name)
        ref = ctx.sift_describe(None, kp[got["kept"]], shape=image.shape)
        assert got["desc"].shape == (len(live), 128) and got["desc"].tobytes() == ref.tobytes(), (n, name)


@pytest.mark.parametrize("n", LENGTHS)
def test_brisk_border_rule_keeps_the_planted_indices_in_order(ctx, image, n):
    """coordinates inside the border of size 5's scale where the pattern keeps, outside one of the four borders in turn where it does not"""
    sizes = capi.brisk_tables()["size_list"]
    b = float(sizes[br.scale_index(5.0)])
    rows, cols = image.shape
    i = np.arange(n)
    inside = np.stack([b + i % (cols - 2 * b), b + (i // 7) % (rows - 2 * b)], 1)
    outside = np.array([[b - 0.5, 30.0], [cols - b, 30.0], [40.0, b - 0.5], [40.0, rows - b]])[i % 4].reshape(n, 2)
    for name, keep in patterns(n).items():
        xy = np.where(keep[:, None], inside, outside).astype(np.float32)
        expected, _ = br.border_keep(xy, 5.0, image.shape, sizes=sizes)
        assert np.array_equal(expected, np.nonzero(keep)[0]), (n, name)          # (the plant is what the restatement's rule keeps)
        got = ctx.brisk_describe(image, xy, 5.0)
        print(n, name, "kept", len(got["kept"]), "of", len(expected))
        assert got["kept"].dtype == np.int32 and np.array_equal(got["kept"], expected), (n, name)
        assert got["desc"].shape == (len(expected), 64) and got["angle"].shape == (len(expected),), (n, name)


@pytest.mark.parametrize("n", LENGTHS)
def test_akaze_suppression_keeps_the_ok_candidates_in_order(ctx, n):
    """level-0 candidates on a 3-pixel lattice (9 > 2.4^2: none is within another's radius), in raster order, `ok` in the pattern"""
    rows, cols = AKAZE_SHAPE
    tables = ak.make_tables(rows, cols)
    i = np.arange(n)
    cand = np.zeros(n, sc.CAND_DTYPE)
    cand["row"], cand["col"], cand["response"] = 3 * (i // (cols // 3)), 3 * (i % (cols // 3)), sc.RESPONSES[i % len(sc.RESPONSES)]
    assert n == 0 or cand["row"].max() < rows
    for name, keep in patterns(n).items():
        cand["ok"] = keep
        expected, st = sc.flat_suppress(tables, cand)
        assert st["drops"] == st["same_level"] == st["from_below"] == st["second_loop"] == 0 and st["not_ok"] == n - int(keep.sum()), (n, name, st)
        assert np.array_equal(expected, np.nonzero(keep)[0]), (n, name)          # (the whole list reaches the compaction: its length is n)
        got = ctx.akaze_suppress_debug(rows, cols, cand)
        print(n, name, "kept", len(got), "of", len(expected))
        assert got.dtype == np.int32 and got.tolist() == expected.tolist(), (n, name)


# ---------------------------------------------------------------- 2. the sites without a list hook, through their entry points
def test_classic_detect_compacts_more_than_one_chunk_of_fast_corners(ctx, noise):
    """cls_compact_kernel: FAST's list and what the ORB extractor's border rule keeps of it are both longer than a chunk"""
    pair = (noise, np.ascontiguousarray(noise[::-1, ::-1]))
    got = ctx.classic_detect(pair[0], pair[1], 0, 1, "FAST")
    for g, img in zip(got, pair):
        r = cr.fast(img)
        keep = cr.orb_border_keep(r["xy"], img.shape)
        print("FAST corners", len(r["xy"]), "kept by the border rule", len(keep))
        assert len(r["xy"]) > 1024 and len(keep) > 1024
        assert _same_bits(g["xy"], r["xy"][keep]) and _same_bits(g["response"], r["response"][keep])
        ctx.fast(img)
        d = ctx.orb_describe(None, r["xy"])                            # the per-image entry points, as tests/test_gpu_classic_resident.py
        assert np.array_equal(d["kept"], keep) and np.array_equal(g["desc"], d["desc"]) and _same_bits(g["angle"], d["angle"])


def test_brisk_detect_compacts_more_than_one_chunk_of_records(ctx, noise):
    """brisk_det_compact_kernel: more than 1024 records are KEPT, so the list it walks is longer still"""
    ref = bd.detect(noise, 30)
    got = ctx.brisk_detect(noise, 30)
    print("BRISK keypoints", got["n"], "restatement", len(ref))
    assert len(ref) > 1024
    assert got["n"] == len(ref) == len(got["kp"]) and got["kp"].tobytes() == ref.tobytes()


def test_fast_and_gftt_rank_more_keys_than_a_tile(ctx, noise, rank_tile):
    """cls_rank_kernel: FAST ranks its corners, Shi-Tomasi the candidates the distance rule keeps (at min_distance 0.5: all of them)"""
    r = cr.fast(noise)
    g = ctx.fast(noise)
    assert len(r["xy"]) > rank_tile
    assert _same_bits(g["xy"], r["xy"]) and _same_bits(g["response"], r["response"])
    kw = dict(max_corners=5000, min_distance=0.5)
    r = cr.gftt(noise, **kw)
    g = ctx.gftt(noise, **kw)
    print("FAST keys", len(cr.fast(noise)["xy"]), "Shi-Tomasi keys", len(r["kept_all"]))
    assert len(r["kept_all"]) == len(r["xy"]) > rank_tile
    assert _same_bits(g["xy"], r["xy"]) and _same_bits(g["response"], r["response"])


def test_orb_ranks_more_keys_than_a_tile(ctx, noise, rank_tile):
    """orb_rank_kernel: level 0's key list holds at least the strict 3 x 3 maxima of the FAST-20 score inside the 31-pixel border (ORB's own
    rule keeps those and the first of equal neighbours; a score map that is zero outside the border only adds maxima)"""
    strict = cr.fast(noise, 20, True)["xy"]
    assert len(cr.orb_border_keep(strict, noise.shape, 31)) > rank_tile
    cpu = cpu_backend.CpuBackend(net_height=64, net_width=96)
    try:
        r = cpu.orb(noise)
    finally:
        cpu.close()
    g = ctx.orb(noise)
    assert len(g["xy"]) == len(r["xy"]) > 500
    assert np.array_equal(g["octave"], r["octave"]) and np.array_equal(g["response"], r["response"])
    assert np.array_equal(g["xy"], r["xy"]) and np.array_equal(g["desc"], r["desc"])
    d = np.abs(g["angle"] - r["angle"])
    assert np.minimum(d, 2 * np.pi - d).max() <= 1e-5                  # (the angle's bound is tests/test_gpu_orb.py's)
