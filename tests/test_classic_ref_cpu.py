"""Properties of the numpy restatement of the classic front end's Shi-Tomasi and FAST detectors (tests/classic_ref.py) that do not
depend on a GPU: the kernels of csrc/classic_detect.hip.h are held to this restatement bit for bit (tests/test_gpu_classic_detectors.py),
so what the restatement itself computes is pinned here."""
import numpy as np
import pytest

from tests import classic_ref as cr


def test_gftt_finds_the_corners_of_isolated_squares():
    img = np.full((120, 200), 20, np.uint8)
    squares = [(20, 30), (20, 120), (70, 60), (70, 150)]          # top-left (y, x) of 24 x 24 squares, far more than 7.5 apart
    for y, x in squares:
        img[y:y + 24, x:x + 24] = 220
    r = cr.gftt(img)
    assert len(r["xy"]) == 4 * len(squares)
    corners = np.array([(x + dx, y + dy) for y, x in squares for dy in (0, 23) for dx in (0, 23)], np.float32)
    for p in r["xy"]:
        assert np.abs(corners - p).max(1).min() <= 2, p          # the eigenvalue peaks within the 5x5 window of the geometric corner
    for c in corners:
        assert np.abs(r["xy"] - c).max(1).min() <= 2, c
    assert np.all(r["xy"] == np.round(r["xy"])) and np.all(r["response"] > 0)


def test_gftt_box_sums_do_not_overflow_int32(sample_images):
    rng = np.random.RandomState(3)
    worst = (rng.randint(0, 2, (40, 56)) * 255).astype(np.uint8)  # gradients at their extremes
    for img in (worst, sample_images[0][100:180, 400:520]):
        a, b, c = cr.gftt_box_sums(img)
        I = np.pad(img.astype(np.int64), 1, mode="reflect")
        h, w = img.shape
        s = lambda dy, dx: I[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        ix = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
        iy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
        assert np.abs(ix).max() <= 1020 and np.abs(iy).max() <= 1020
        for got, prod in ((a, ix * ix), (b, ix * iy), (c, iy * iy)):
            P = np.pad(prod, 2, mode="reflect")
            ref = np.zeros((h, w), np.int64)
            for y in range(h):
                for x in range(w):
                    ref[y, x] = P[y:y + 5, x:x + 5].sum()
            assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), ref)
            assert np.abs(ref).max() < 2 ** 31
        rad = (a.astype(np.int64) - c) ** 2 + 4 * b.astype(np.int64) ** 2
        assert rad.max() < 2 ** 53                                  # exact in float64


def _noise():
    return np.random.RandomState(1).randint(0, 256, (200, 320)).astype(np.uint8)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_gftt_on_kitti_is_sorted_separated_and_maximal(sample_images, which):
    img = sample_images[which]
    r = cr.gftt(img)
    xy = r["xy"].astype(np.int64)
    n = len(xy)
    assert 100 < n < 1000                                           # the cap does not bind on the samples at their native size
    assert np.all(np.diff(r["response"].astype(np.float64)) <= 0)
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    d2[np.arange(n), np.arange(n)] = 10 ** 9
    assert d2.min() >= 57
    # maximal: every candidate that was not returned lies within the disc of a returned one that ranks before it
    w = img.shape[1]
    cand = r["candidates"]
    pos = {int(p): i for i, p in enumerate(cand.tolist())}
    kept = set((xy[:, 1] * w + xy[:, 0]).tolist())
    kept_rank = np.array([pos[int(p)] for p in (xy[:, 1] * w + xy[:, 0])])
    for i, p in enumerate(cand.tolist()):
        if p in kept:
            continue
        y, x = divmod(p, w)
        near = (xy[:, 0] - x) ** 2 + (xy[:, 1] - y) ** 2 <= 56
        assert (near & (kept_rank < i)).any(), (x, y)


def test_gftt_ties_put_the_later_raster_position_first():
    img = np.full((64, 64), 10, np.uint8)
    img[10:20, 10:20] = 200
    img[40:50, 40:50] = 200                                         # the same square twice: equal responses
    r = cr.gftt(img)
    resp = r["response"]
    idx = (r["xy"][:, 1] * 64 + r["xy"][:, 0]).astype(int)
    for i in range(len(resp) - 1):
        if resp[i] == resp[i + 1]:
            assert idx[i] > idx[i + 1]
    assert (resp[:-1] == resp[1:]).any()


@pytest.mark.parametrize("case", ["kitti0", "kitti1", "noise"])
def test_the_monotone_iteration_reaches_the_greedy_set(sample_images, case):
    """UNDECIDED -> SUPPRESSED if a KEPT candidate is in the disc, UNDECIDED -> KEPT if no KEPT and no better-ranked UNDECIDED one is:
    the fixed point is the sequential greedy loop's set (the kernel iterates this rule with stale reads allowed; here every round
    sees exactly the round before it)."""
    img = _noise() if case == "noise" else sample_images[int(case[-1])]
    lam = cr.gftt_response(img)
    cand = cr.gftt_candidates(lam)
    assert len(cand) > 1000
    _, greedy = cr.greedy_min_distance(cand, img.shape, 7.5, 1000)
    it, rounds = cr.iterative_min_distance(cand, img.shape, 7.5)
    assert np.array_equal(it, greedy)
    assert 1 < rounds < 64
    # and for another radius (min_distance 3 -> d2 <= 8)
    _, greedy3 = cr.greedy_min_distance(cand, img.shape, 3.0, 10 ** 9)
    it3, _ = cr.iterative_min_distance(cand, img.shape, 3.0)
    assert np.array_equal(it3, greedy3) and len(greedy3) > len(greedy)


def test_disc_limit_is_the_strict_comparison_on_integers():
    assert cr.disc_limit(7.5) == 56 and cr.disc_limit(3.0) == 8 and cr.disc_limit(1.0) == 0 and cr.disc_limit(15.0) == 224


def _ring(center, values):
    img = np.full((9, 9), center, np.uint8)
    for (dx, dy), v in zip(cr._CIRCLE, values):
        img[4 + dy, 4 + dx] = v
    return img


def test_fast_needs_an_arc_of_nine():
    nine = _ring(100, [150] * 9 + [100] * 7)
    eight = _ring(100, [150] * 8 + [100] * 8)
    assert cr.fast_score(nine, 10)[4, 4] == 50                      # the score is the smallest difference on the best arc (orb_fast_kernel's definition)
    assert cr.fast_score(eight, 10)[4, 4] == 0
    assert cr.fast_score(nine, 49)[4, 4] == 50 and cr.fast_score(nine, 50)[4, 4] == 0   # a corner while the difference EXCEEDS the threshold
    dark = _ring(100, [100] * 5 + [30] * 10 + [100])
    assert cr.fast_score(dark, 10)[4, 4] == 70
    wrap = _ring(100, [150] * 4 + [100] * 7 + [150] * 5)            # the arc runs across the start of the circle
    assert cr.fast_score(wrap, 10)[4, 4] == 50
    r = cr.fast(nine, 10, True)
    assert np.array_equal(r["xy"], [[4, 4]]) and np.array_equal(r["response"], [50])
    assert cr.fast_score(nine[2:, 2:], 10).max() == 0    # the corner now lies in the 3-pixel border


def test_fast_suppression_drops_both_of_two_equal_neighbours():
    score = np.zeros((12, 12), np.uint8)
    img = np.zeros((12, 12), np.uint8)
    # the rule is applied to a score map: use the restatement's suppression on a crafted one
    score[5, 5] = score[5, 6] = 30                                   # equal neighbours: both go
    score[8, 3] = 40; score[8, 4] = 39                               # the larger stays
    orig = cr.fast_score
    try:
        cr.fast_score = lambda im, t, border=3: score
        r = cr.fast(img, 10, True)
        assert np.array_equal(r["xy"], [[3, 8]]) and np.array_equal(r["response"], [40])
        r = cr.fast(img, 10, False)
        assert np.array_equal(r["xy"], [[5, 5], [6, 5], [3, 8], [4, 8]])   # raster order, everything kept
    finally:
        cr.fast_score = orig


def test_fast_on_noise_is_dense_and_never_keeps_neighbours():
    r = cr.fast(_noise(), 10, True)
    xy = r["xy"].astype(int)
    assert len(xy) > 2048
    occ = np.zeros((200, 320), bool)
    occ[xy[:, 1], xy[:, 0]] = True
    P = np.pad(occ, 1)
    nb = sum(P[1 + dy:201 + dy, 1 + dx:321 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
    assert not (occ & (nb > 0)).any()
    key = xy[:, 1] * 320 + xy[:, 0]
    assert np.all(np.diff(key) > 0)                                  # raster order
    assert xy[:, 0].min() >= 3 and xy[:, 0].max() < 317 and xy[:, 1].min() >= 3 and xy[:, 1].max() < 197
