"""Numpy restatement of the classic front end's Shi-Tomasi (GFTT) and FAST detectors as csrc/classic_detect.hip.h builds them
(cv::GFTTDetector::create(1000, 0.03, 7.5, 5, false, 0.04) and cv::FastFeatureDetector::create(10, true),
feature_detection_classic.cpp:32-47).  No OpenCV exists in this build to pin either against: this is the published algorithm with the
reference's parameters and OpenCV's tie / border rules as far as they are known, written once here and reproduced by the kernels
bit for bit.  The choices:

  1. gradients: 3x3 Sobel on the u8 image, border reflect-101; box sums of the three products over 5x5, border reflect-101 of the
     PRODUCT images; all exact int32.
  2. lambda2 = (a + c) - sqrt((a - c)^2 + 4 b^2): radicand exact in int64, one float64 square root, one float64 subtraction,
     clamp at 0, one rounding to float32.  OpenCV's scale factor (0.5 / (255 * 4 * 5)^2) is a positive constant: it is applied only to
     the reported response (one float32 multiplication).
  3. candidates: lambda2 > float32(float64(max) * quality) (strict), >= all eight neighbours (ties all kept), not in the outermost frame.
  4. order: response descending, of equal responses the LATER raster position first.
  5. minimum distance: greedy in that order, keep iff no kept one has dx^2 + dy^2 < min_distance^2 (strict); the first max_corners kept.
  6. FAST-9/16 score = orb_fast_kernel's: the smallest |difference| on the best arc of 9 (0 if no arc exceeds threshold t), 3-pixel border;
     suppression keeps a corner iff its score is strictly greater than all eight neighbours'; output in raster order.
  7. keypoint coordinates are integers stored as float32.
"""
import numpy as np

GFTT_SCALE = np.float32(0.5 / (5100.0 * 5100.0))     # 255 * 2^(3-1) * block_size, squared (products of two gradients), and the 1/2 of the eigenvalue

_CIRCLE = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3)]   # (dx, dy)


def _pad101(a, p):
    return np.pad(a, p, mode="reflect")


def gftt_box_sums(img):
    """a = sum Ix^2, b = sum Ix Iy, c = sum Iy^2 over 5x5, int32."""
    I = _pad101(np.ascontiguousarray(img, np.uint8).astype(np.int32), 1)
    h, w = img.shape
    s = lambda dy, dx: I[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    ix = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    iy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    out = []
    for prod in (ix * ix, ix * iy, iy * iy):
        P = _pad101(prod.astype(np.int32), 2)
        acc = np.zeros((h, w), np.int32)
        for dy in range(5):
            for dx in range(5):
                acc += P[dy:dy + h, dx:dx + w]
        out.append(acc)
    return out


def gftt_response(img):
    """lambda2 as float32 [h, w] (unscaled)."""
    a, b, c = [v.astype(np.int64) for v in gftt_box_sums(img)]
    rad = (a - c) * (a - c) + 4 * b * b
    lam = (a + c).astype(np.float64) - np.sqrt(rad.astype(np.float64))
    return np.maximum(lam, 0.0).astype(np.float32)


def gftt_candidates(lam, quality=0.03):
    """Raster indices of the candidates, in rank order (choice 3 and 4)."""
    h, w = lam.shape
    thr = np.float32(np.float64(lam.max()) * np.float64(quality))
    ok = np.zeros((h, w), bool)
    if h < 3 or w < 3:
        return np.zeros(0, np.int64)
    c = lam[1:-1, 1:-1]
    m = c > thr
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                m &= c >= lam[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    ok[1:-1, 1:-1] = m
    idx = np.flatnonzero(ok)
    v = lam.ravel()[idx]
    order = np.lexsort((-idx, -v.astype(np.float64)))
    return idx[order]


def disc_limit(min_distance):
    """largest integer d2 with d2 < min_distance^2 is ceil(min_distance^2) - 1"""
    md = float(np.float32(min_distance))
    return int(np.ceil(md * md)) - 1


def _disc_offsets(lim):
    r = int(np.floor(np.sqrt(max(lim, 0))))
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= lim], r


def greedy_min_distance(cand, shape, min_distance, max_corners):
    """The sequential loop (choice 5): candidates in rank order -> (kept raster indices in rank order, capped; all kept)."""
    h, w = shape
    lim = disc_limit(min_distance)
    offs, r = _disc_offsets(lim)
    dy = np.array([o[0] for o in offs]); dx = np.array([o[1] for o in offs])
    blocked = np.zeros((h + 2 * r, w + 2 * r), bool)
    kept = []
    for p in cand.tolist():
        y, x = divmod(p, w)
        if blocked[y + r, x + r]:
            continue
        kept.append(p)
        blocked[y + r + dy, x + r + dx] = True
    kept = np.asarray(kept, np.int64)
    return kept[:max_corners], kept


def iterative_min_distance(cand, shape, min_distance):
    """The monotone UNDECIDED -> KEPT / SUPPRESSED rule the kernel iterates (csrc/post.hip.h), all candidates at once per round.
    Returns (kept raster indices in rank order, number of rounds)."""
    h, w = shape
    lim = disc_limit(min_distance)
    offs, r = _disc_offsets(lim)
    offs = [o for o in offs if o != (0, 0)]
    BIG = np.int64(1) << 40
    rank = np.full((h + 2 * r, w + 2 * r), BIG, np.int64)       # rank of an UNDECIDED candidate, BIG otherwise
    kept = np.zeros((h + 2 * r, w + 2 * r), bool)
    ys, xs = np.divmod(cand, w)
    ys = ys + r; xs = xs + r
    rank[ys, xs] = np.arange(len(cand))
    und = np.ones(len(cand), bool)
    rounds = 0
    while und.any():
        rounds += 1
        y, x, me = ys[und], xs[und], np.arange(len(cand))[und]
        any_kept = np.zeros(len(me), bool)
        any_better = np.zeros(len(me), bool)
        for dy, dx in offs:
            any_kept |= kept[y + dy, x + dx]
            any_better |= rank[y + dy, x + dx] < me
        sup = any_kept
        keep = ~any_kept & ~any_better
        kept[y[keep], x[keep]] = True
        done = sup | keep
        rank[y[done], x[done]] = BIG
        und[me[done]] = False
    k = kept[ys, xs]
    return cand[k], rounds


def gftt(img, max_corners=1000, quality=0.03, min_distance=7.5, block_size=5):
    """-> dict(xy float32 [n, 2], response float32 [n], lam, candidates, kept_all)."""
    assert block_size == 5
    img = np.ascontiguousarray(img, np.uint8)
    lam = gftt_response(img)
    cand = gftt_candidates(lam, quality)
    kept, kept_all = greedy_min_distance(cand, img.shape, min_distance, max_corners)
    w = img.shape[1]
    xy = np.stack([kept % w, kept // w], 1).astype(np.float32).reshape(-1, 2)
    resp = (lam.ravel()[kept] * GFTT_SCALE).astype(np.float32)
    return dict(xy=xy, response=resp, lam=lam, candidates=cand, kept_all=kept_all)


def fast_score(img, t, border=3):
    """uint8 [h, w]: the FAST-9/16 score of every pixel, 0 where it is no corner at threshold t or lies in the border."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros((h, w), np.uint8)
    if h <= 2 * border or w <= 2 * border:
        return out
    I = img.astype(np.int16)
    c = I[border:h - border, border:w - border]
    d = [I[border + dy:h - border + dy, border + dx:w - border + dx] - c for dx, dy in _CIRCLE]
    best = np.zeros(c.shape, np.int16)
    for s in range(16):
        mn = d[s].copy(); mx = d[s].copy()
        for k in range(1, 9):
            np.minimum(mn, d[(s + k) % 16], out=mn)
            np.maximum(mx, d[(s + k) % 16], out=mx)
        best = np.maximum(best, np.where(mn > t, mn, 0))
        best = np.maximum(best, np.where(-mx > t, -mx, 0))
    out[border:h - border, border:w - border] = best.astype(np.uint8)
    return out


def fast(img, threshold=10, nonmax_suppression=True):
    """-> dict(xy float32 [n, 2] in raster order, response float32 [n], score)."""
    score = fast_score(img, threshold)
    h, w = score.shape
    m = score > 0
    if nonmax_suppression:
        P = np.pad(score, 1).astype(np.int16)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    m &= score > P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    ys, xs = np.nonzero(m)
    return dict(xy=np.stack([xs, ys], 1).astype(np.float32).reshape(-1, 2), response=score[ys, xs].astype(np.float32), score=score)


def orb_border_keep(xy, shape, edge=31):
    """indices of the keypoints the ORB extractor keeps (at least `edge` pixels from every border), ascending"""
    h, w = shape
    xy = np.asarray(xy).reshape(-1, 2)
    ok = (xy[:, 0] >= edge) & (xy[:, 0] < w - edge) & (xy[:, 1] >= edge) & (xy[:, 1] < h - edge)
    return np.flatnonzero(ok).astype(np.int32)
