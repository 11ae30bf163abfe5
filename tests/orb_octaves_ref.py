"""Numpy restatement of the ORB extractor on given keypoints that carry an octave, as csrc/orb.hip.h builds it
(spvo_orb_describe_octaves): cv::ORB::create()->compute(img, keypoints, descriptors) (feature_detection_classic.cpp:66-68, 110-111) on
keypoints whose KeyPoint::octave names a pyramid level -- what BRISK + ORB and AKAZE + ORB run.  No OpenCV exists in this build to pin it
against: this file is the definition, and the kernels reproduce it bit for bit (the direction, which is only reported, to rounding level:
it passes through atan2).  Where an independent implementation exists -- the compiled oracle oracle/cpu/orb_cpu.inc on the keypoints of
its own detector, which never come near a level's border -- tests/test_orb_octaves_ref_cpu.py holds this file to it.  Every choice, and
whether it is OpenCV 4.x's rule as far as known ("OpenCV") or a decision of this project ("ours"):

  Levels
   1. OpenCV: level l has scale 1.2^l and the size round(rows / scale) x round(cols / scale); each level is resized (INTER_LINEAR, 8-bit)
      from the level below.  ours: exactly spvo_orb_detect's levels -- scale_0 = 1, scale_l = scale_(l-1) * 1.2f in float32;
      lround(rows / scale) with the division in float32; the resize is orb_resize_kernel's integer arithmetic on linear_coeffs' 11-bit
      tables (`resize_u8` below).  Only levels 0 .. the largest octave named are built.
   2. ours: the 7 x 7 Gaussian (sigma 2) of a level is orb_blur_h_kernel / orb_blur_v_kernel's: float32 sums in tap order, every
      multiplication and addition separately rounded, taps clamped at the level's border, floor(s + 0.5) clamped to 0..255.  Only levels
      that hold a kept keypoint are smoothed.
  Which keypoints, in which order
   3. OpenCV: KeyPointsFilter::runByImageBorder(keypoints, image size, 31) against the LEVEL-0 image whatever the octave.  ours: applied
      to the coordinates rounded half to even, xi = rint(x), yi = rint(y): kept iff 31 <= xi < cols - 31 and 31 <= yi < rows - 31.  For
      integer coordinates that is spvo_orb_describe's rule.
   4. OpenCV: a list that is not sorted by level is grouped by level, ascending, stable within a level.  `kept` holds the indices into
      the input in output order (ascending only when the input was already sorted by octave).
   5. ours: an octave outside 0..7, a coordinate that is not finite, and a named octave whose level is smaller than 32 pixels in either
      dimension are refused (ValueError here, SPVO_ERR_INVALID there) before anything is computed.  With levels of at least 32 pixels one
      reflection (8) always suffices.
  Per keypoint
   6. OpenCV: the position on the level is cvRound(pt / scale).  ours: cx = (int)rint(x / scale_l) with the division in float32, rint to
      even, clamped into the level; likewise cy.
   7. ours: direction and the 256 tests are orb_describe_kernel's arithmetic unchanged: integer moments m10, m01 over the 709 pixels of
      the disc of radius 15 on the level image; (cos, sin) = (m10, m01) / sqrt(m10^2 + m01^2) in float32, every operation separately
      rounded ((1, 0) for a zero vector); test point = centre + floor(x cos - y sin + 0.5), floor(x sin + y cos + 0.5); bit = blurred(p1)
      < blurred(p2); bit k of the descriptor is bit k % 8 of byte k / 8.  The direction is always recomputed; angle = atan2(sin, cos) in
      radians is reported.  The tables are spvo_orb_tables' (`tables` below restates them; the test-pair table is the documented
      deviation of oracle/cpu/orb_cpu.inc: OpenCV's learned bit_pattern_31_ cannot be restated, the pairs are the BRIEF Gaussian's with
      a fixed seed, clipped to +-13).
   8. DEVIATION, like the table: OpenCV copies each level into a buffer with a border of 32 pixels reflected (BORDER_REFLECT_101) from
      the UNBLURRED level and blurs the whole buffer, so beyond a level's border its tests read the blur of the reflection.  ours: both
      the level image (moments) and the blurred level (tests) are read at the BORDER_REFLECT_101 index of that level -- the reflection
      of the blur (whose own taps clamp, 2).  The reach is 15 for the disc and at most 19 for a rotated test point (the pattern is
      clipped to +-13: 13 sqrt 2 = 18.4), so only a keypoint within 19 pixels of its level's border can read beyond it: `zone` reports
      that per keypoint and border (it is what the kernel picks its indexing by), `outside` whether a read really fell beyond.
      Away from the zone nothing differs from OpenCV's rule but the table.
"""
import numpy as np

LEVELS, HALF, EDGE, REACH, MIN_LEVEL = 8, 15, 31, 19, 32


def level_scales():
    s = [np.float32(1.0)]
    for _ in range(1, LEVELS):
        s.append(np.float32(s[-1] * np.float32(1.2)))
    return s


def _lround(v):
    return int(np.floor(np.float64(v) + 0.5))


def level_shapes(rows, cols):
    return [(_lround(np.float32(rows) / s), _lround(np.float32(cols) / s)) for s in level_scales()]


def _hash32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def tables():
    """(pattern [1024] = 256 x (x1, y1, x2, y2), taps [7]) as orb_host_tables builds them (spvo_orb_tables)"""
    f = np.float32
    state = 0x9E3779B9
    pat = np.zeros(1024, f)

    def uni():
        nonlocal state
        state = _hash32((state + 0x6D2B79F5) & 0xFFFFFFFF)
        return f(f(f(state >> 8) + f(0.5)) / f(16777216.0))
    for i in range(1024):
        u1, u2 = uni(), uni()
        g = f(np.sqrt(f(f(-2.0) * np.log(u1))) * np.cos(f(f(6.2831853) * u2)))
        v = f(g * f(f(31) / f(5.0)))
        v = min(max(v, f(-13)), f(13))
        pat[i] = np.floor(np.abs(v) + f(0.5)) * np.sign(v)          # std::round: half away from zero
    # expf, correctly rounded: the double exponential rounded once (numpy's float32 exp is an ulp off for two taps)
    k = np.array([f(np.exp(np.float64(f(f(f(-0.5) * f((i - 3) * (i - 3))) / f(4.0))))) for i in range(7)], f)
    s = f(0)
    for i in range(7):
        s = f(s + k[i])
    return pat, (k / s).astype(f)


def linear_coeffs(dst, src):
    """cv::resize(INTER_LINEAR) on 8-bit data: source index and the two 11-bit weights per destination index (spvo_detect.hip)"""
    d = np.arange(dst, dtype=np.float64)
    fl = ((d + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5).astype(np.float32)
    s = np.floor(fl).astype(np.int64)
    fl = (fl - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    fl = np.where(lo | hi, np.float32(0), fl).astype(np.float32)
    a0 = np.rint((np.float32(1) - fl) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(fl * np.float32(2048)).astype(np.int64)
    return s, a0, a1


def resize_u8(src, dh, dw):
    sh, sw = src.shape
    xi, xa0, xa1 = linear_coeffs(dw, sw)
    yi, yb0, yb1 = linear_coeffs(dh, sh)
    x1, y1 = np.minimum(xi + 1, sw - 1), np.minimum(yi + 1, sh - 1)
    im = src.astype(np.int64)
    s0 = (im[yi][:, xi] * xa0 + im[yi][:, x1] * xa1) >> 4
    s1 = (im[y1][:, xi] * xa0 + im[y1][:, x1] * xa1) >> 4
    v = (((yb0[:, None] * s0) >> 16) + ((yb1[:, None] * s1) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def pyramid(img, top):
    """levels 0 .. top, each resized from the one below"""
    shapes = level_shapes(*img.shape)
    pyr = [np.ascontiguousarray(img, np.uint8)]
    for l in range(1, top + 1):
        pyr.append(resize_u8(pyr[-1], *shapes[l]))
    return pyr


def blur7(im, taps):
    h, w = im.shape
    f = im.astype(np.float32)
    xs, ys = np.arange(w), np.arange(h)
    s = np.zeros((h, w), np.float32)
    for i in range(-3, 4):
        s = s + taps[i + 3] * f[:, np.clip(xs + i, 0, w - 1)]
    t = np.zeros((h, w), np.float32)
    for i in range(-3, 4):
        t = t + taps[i + 3] * s[np.clip(ys + i, 0, h - 1), :]
    return np.clip(np.floor(t + np.float32(0.5)).astype(np.int64), 0, 255).astype(np.uint8)


def disc_offsets():
    """the 709 (dx, dy) of the disc of radius 15, row by row"""
    out = []
    for dy in range(-HALF, HALF + 1):
        lim = int(np.floor(np.sqrt(float(HALF * HALF - dy * dy))))
        out += [(dx, dy) for dx in range(-lim, lim + 1)]
    return np.array(out, np.int64)


def reflect101(i, n):
    """BORDER_REFLECT_101 index into 0 .. n - 1 (one reflection: |overshoot| < n)"""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def border_keep(xy, shape):
    """the indices that pass rule 3"""
    rows, cols = shape
    xi, yi = np.rint(xy[:, 0]), np.rint(xy[:, 1])
    return np.nonzero((xi >= EDGE) & (xi < cols - EDGE) & (yi >= EDGE) & (yi < rows - EDGE))[0]


def describe(img, xy, octave, tables_=None):
    """-> dict: kept [m] indices into xy in output order, octave [m], cxy [m, 2] positions on the level, angle [m] rad, desc [m, 32],
    zone [m, 4] / outside [m, 4] (left, right, top, bottom: within 19 pixels of that border of its level / a read fell beyond it)"""
    img = np.asarray(img)
    rows, cols = img.shape
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    octave = np.ascontiguousarray(octave, np.int32).reshape(-1)
    if len(octave) != len(xy):
        raise ValueError("one octave per keypoint")
    if ((octave < 0) | (octave >= LEVELS)).any():
        raise ValueError("octave outside 0..7")
    if not np.isfinite(xy).all():
        raise ValueError("a coordinate is not finite")
    shapes, scales = level_shapes(rows, cols), level_scales()
    for l in sorted(set(octave.tolist())):
        if min(shapes[l]) < MIN_LEVEL:
            raise ValueError("level %d is %d x %d: smaller than %d pixels" % (l, shapes[l][0], shapes[l][1], MIN_LEVEL))
    pattern, taps = tables() if tables_ is None else tables_
    pattern = np.asarray(pattern, np.float32).reshape(256, 4)
    taps = np.asarray(taps, np.float32)
    keep = border_keep(xy, (rows, cols))
    keep = keep[np.argsort(octave[keep], kind="stable")]
    m = len(keep)
    out = dict(kept=keep.astype(np.int32), octave=octave[keep], cxy=np.zeros((m, 2), np.int32), angle=np.zeros(m, np.float32), desc=np.zeros((m, 32), np.uint8),
               zone=np.zeros((m, 4), bool), outside=np.zeros((m, 4), bool))
    if m == 0:
        return out
    pyr = pyramid(img, int(octave.max()))
    disc = disc_offsets()
    f = np.float32
    for l in sorted(set(out["octave"].tolist())):
        rows_l = np.nonzero(out["octave"] == l)[0]
        im, (h, w) = pyr[l], shapes[l]
        blur = blur7(im, taps)
        p = xy[keep[rows_l]]
        cx = np.clip(np.rint(p[:, 0] / scales[l]).astype(np.int64), 0, w - 1)
        cy = np.clip(np.rint(p[:, 1] / scales[l]).astype(np.int64), 0, h - 1)
        px, py = cx[:, None] + disc[None, :, 0], cy[:, None] + disc[None, :, 1]
        v = im[reflect101(py, h), reflect101(px, w)].astype(np.int64)
        m10, m01 = (disc[None, :, 0] * v).sum(1), (disc[None, :, 1] * v).sum(1)
        fx, fy = m10.astype(f), m01.astype(f)
        nrm = np.sqrt((fx * fx + fy * fy).astype(f)).astype(f)
        ok = nrm > 0
        safe = np.where(ok, nrm, f(1))
        ca, sa = np.where(ok, fx / safe, f(1)).astype(f), np.where(ok, fy / safe, f(0)).astype(f)
        ca_, sa_ = ca[:, None], sa[:, None]

        def rot(a, b):   # floor(a cos - b sin + 0.5), floor(a sin + b cos + 0.5)
            x = np.floor((a * ca_ - b * sa_).astype(f) + f(0.5)).astype(np.int64)
            y = np.floor((a * sa_ + b * ca_).astype(f) + f(0.5)).astype(np.int64)
            return cx[:, None] + x, cy[:, None] + y
        x1, y1 = rot(pattern[None, :, 0], pattern[None, :, 1])
        x2, y2 = rot(pattern[None, :, 2], pattern[None, :, 3])
        bits = blur[reflect101(y1, h), reflect101(x1, w)] < blur[reflect101(y2, h), reflect101(x2, w)]
        out["desc"][rows_l] = np.packbits(bits, axis=1, bitorder="little")
        out["angle"][rows_l] = np.arctan2(sa, ca).astype(f)
        out["cxy"][rows_l] = np.stack([cx, cy], 1)
        out["zone"][rows_l] = np.stack([cx < REACH, cx >= w - REACH, cy < REACH, cy >= h - REACH], 1)
        ax, ay = np.concatenate([px, x1, x2], 1), np.concatenate([py, y1, y2], 1)
        out["outside"][rows_l] = np.stack([ax.min(1) < 0, ax.max(1) >= w, ay.min(1) < 0, ay.max(1) >= h], 1)
    return out
