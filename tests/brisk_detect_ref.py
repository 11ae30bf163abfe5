"""Numpy restatement of the BRISK keypoint detector as csrc/brisk_detect.hip.h builds it: cv::BRISK::create()->detect(img), i.e.
threshold 30, 3 octaves, pattern scale 1 (feature_detection_classic.cpp:9-11): BriskScaleSpace with 6 layers, basicSize_ = 12, safety
factor 1.  No OpenCV exists in this build to pin it against: this file is the definition, and the kernels reproduce it bit for bit in
every field.  Every choice, and whether it is OpenCV 4.x's rule as far as known ("OpenCV") or a decision of this project ("ours"):

  Pyramid
   1. OpenCV: layer 0 is the image; layer 1 is layer 0 two-thirds-sampled to 2 * (rows / 3) x 2 * (cols / 3); layer i >= 2 is layer
      i - 2 half-sampled to rows / 2 x cols / 2 (integer divisions).  scale(0) = 1, scale(1) = 1.5, scale(i) = 2 * scale(i - 2);
      offset = 0.5f * scale - 0.5f (float).
   2. OpenCV: both samplers are cv::resize(INTER_AREA).  When the source is exactly twice the destination in BOTH directions (rows and
      cols of the source even) that is the integer rule (a + b + c + d + 2) >> 2 over the 2 x 2 block.
   3. OpenCV: every other ratio (always for two-thirds; for a half whenever a source size is odd) takes the general area path: per
      axis, with scale = ssize / dsize in double, destination cell d covers [d * scale, (d + 1) * scale); sx1 = ceil(d * scale),
      sx2 = min(floor((d + 1) * scale), ssize - 1), sx1 = min(sx1, sx2); cell = min(scale, ssize - d * scale); the taps in this order:
      source sx1 - 1 with weight (sx1 - d * scale) / cell if sx1 - d * scale > 1e-3; sources sx1 .. sx2 - 1 with weight 1 / cell;
      source sx2 with weight min(min((d + 1) * scale - sx2, 1), cell) / cell if (d + 1) * scale - sx2 > 1e-3.  Weights are formed in
      DOUBLE and stored as FLOAT.  A destination pixel is accumulated in float: for every source row of its y taps, in order,
      buf = sum over the x taps in order of pixel * alpha (buf = 0, then buf = buf + pixel * alpha), then sum = beta * buf for the
      first row and sum = sum + beta * buf for the others; the result is sum rounded to the nearest integer, ties to EVEN
      (saturate_cast<uchar>(float) = cvRound), clamped to 0..255.
      ours: every float multiplication and addition is separately rounded (no fused multiply-add), in exactly that order.
  Scores
   4. OpenCV: a layer's AGAST 9-16 score is computed lazily and cached in a score image: getAgastScore(x, y, thr) returns 0 outside
      the 3-pixel interior (x < 3, y < 3, x >= cols - 3, y >= rows - 3), else a cached value if it is > 2, else it bisects for the
      score starting at thr - 1, stores it (0 if it is below thr) and returns it.  The AGAST 9-16 (OAST) corner criterion is the
      FAST-9/16 segment test: nine contiguous pixels of the 16-pixel Bresenham circle of radius 3 all brighter than centre + b or all
      darker than centre - b (strict).  The bisection returns the largest b at which that still holds: with M = the smallest
      |difference| on the best arc (orb_fast_kernel's value at threshold 0), the score is s = M - 1 (s = 0 when M <= 1).  It is ONE
      LESS than the FAST response of spvo_fast_detect, which moves both `score > threshold` and the reported response.
      ours: the read is the PURE function  s(x, y) >= thr ? s(x, y) : 0  of a dense, threshold-independent map s (0 outside the
      3-pixel interior).  That is what OpenCV's lazy read returns on a cold cache; a warm cache returns a value > 2 whatever thr is,
      and isMax2D (7) reads the cache as earlier keypoints happened to leave it.  The pure form is independent of the order in which
      keypoints are processed, which is what lets every candidate be refined in parallel.
   5. OpenCV: the virtual layer below layer 0 uses the AGAST 5-8 score of layer 0: five contiguous pixels of the 8-pixel ring of
      radius 1, same strict criterion, same bisection, 0 within 2 pixels of the border: s5 = M5 - 1.  Read with threshold 1.
   6. OpenCV: the sub-pixel read getAgastScore(xf, yf, thr, scale = 1) interpolates inside the layer: x = (int)xf, rx1 = xf - x,
      rx = 1 - rx1, likewise y; value = (uchar)(rx * ry * s(x, y) + rx1 * ry * s(x + 1, y) + rx * ry1 * s(x, y + 1) + rx1 * ry1 *
      s(x + 1, y + 1)) in float, truncated.  ours: products left to right, every operation separately rounded.  For scale > 1 OpenCV
      smooths the cached scores over a box with integer weights (`smoothed_value` below restates it: the bilinear branch with weights
      of 1024 for a half-width below 0.5, else the area branch with `scaling` weights); the detector never passes a scale, so every
      sub-pixel read of the detection takes the float branch above and the kernels build only that.  There is no sub-pixel 5-8 read.
  Detection
   7. OpenCV: the candidates of a layer are its AGAST points at the safe threshold (int)(threshold * 1.0f) = threshold: s >= threshold,
      in raster order.  isMax2D: the centre must be >= all eight neighbours; for every neighbour EQUAL to the centre the 3 x 3 sums
      smoothed with weights 1 2 1 / 2 4 2 / 1 2 1 are compared and the centre is rejected when the neighbour's is larger.
      ours: isMax2D reads s >= threshold ? s : 0 (the cache as getAgastPoints leaves it, see 4).
   8. OpenCV: top layer (5): getScoreMaxBelow with the centre's score as threshold, then subpixel2D on its own 3 x 3 patch (reads with
      threshold 1): x = (float(x) + dx) * scale + offset, response = the patch's refined maximum.  No score test.
   9. OpenCV: every other layer: refine3D -- getScoreMaxAbove, then below (layer 0: the 3 x 3 patch of 5-8 scores, its maximum and
      subpixel2D offsets; else getScoreMaxBelow), subpixel2D on the layer's own patch, refine1D (even layers > 0), refine1D_1 (odd
      layers), refine1D_2 (layer 0) over (below, max(centre, patch maximum), above), interpolation of the position between the
      layers, scale *= layer scale; kept iff the refined score > threshold.
  10. OpenCV: getScoreMaxAbove / getScoreMaxBelow search the window that the pixel covers in the other layer -- corners in float:
      above, even layer (4 x - 1 -/+ 2) / 6, odd layer (6 x - 1 -/+ 3) / 8; below, even layer (8 x + 1 -/+ 4) / 6, odd layer
      (6 x + 1 -/+ 3) / 4 -- at most 4 x 4 reads: the fractional first and last row / column through the sub-pixel read (6), the
      integer positions between.  A value above the centre's score in the first or a middle row rejects the candidate; the LAST row
      is only searched for the maximum (as OpenCV's code has it).  Below, an interior value equal to the running maximum moves the
      maximum there when its weighted ring sum (2 x edge neighbours + corner neighbours) is larger.  The maximum's 3 x 3 patch goes
      through subpixel2D; the offset is mapped back -- above, even: (rx * 6 + 1) / 4 - x in float, odd: (rx * 8 + 1) / 6 - x in
      DOUBLE, rounded to float; below, even: float((rx * 6 + 1) / 8 in double) - x, odd: float((rx * 4 - 1) / 6 in double) - x --
      and saturated to [-1, 1]; a saturated offset returns the unrefined maximum, else max(refined, unrefined).
  11. OpenCV: subpixel2D, refine1D*: integer coefficient tables as below; float steps separately rounded, left to right (ours).
  12. OpenCV: the record is (x, y, size = 12 * scale, angle = -1, response = refined score, octave = layer).
  Order
  13. OpenCV: layer by layer, within a layer in raster order of the candidate (row, then column).
  Out-of-range reads
  14. ours: every score read outside a layer, or inside its border, returns 0 (OpenCV: the same for getAgastScore; its smoothing of
      (6) indexes the score image without a check).  No window is ever indexed outside its layer.  A layer too small to have an
      interior contributes nothing.
"""
import numpy as np

f32, f64 = np.float32, np.float64
N_LAYERS = 6
BASIC_SIZE = f32(12.0)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])

CIRCLE16 = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
RING8 = ((0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1))


# ---------------------------------------------------------------- pyramid (choices 1-3)
def layer_shapes(rows, cols):
    shapes = [(rows, cols), (2 * (rows // 3), 2 * (cols // 3))]
    for i in range(2, N_LAYERS):
        shapes.append((shapes[i - 2][0] // 2, shapes[i - 2][1] // 2))
    return shapes


def layer_scales():
    s = [f32(1.0), f32(1.5)]
    for i in range(2, N_LAYERS):
        s.append(f32(s[i - 2] * f32(2.0)))
    return s


def layer_offsets():
    return [f32(f32(f32(0.5) * s) - f32(0.5)) for s in layer_scales()]


def area_tab(ssize, dsize):
    """choice 3: per destination index the list of (source index, float weight), in OpenCV's order"""
    scale = f64(ssize) / f64(dsize)
    tab = []
    for d in range(dsize):
        fsx1 = f64(d) * scale
        fsx2 = fsx1 + scale
        cell = min(scale, f64(ssize) - fsx1)
        sx1, sx2 = int(np.ceil(fsx1)), int(np.floor(fsx2))
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        taps = []
        if sx1 - fsx1 > 1e-3:
            taps.append((sx1 - 1, f32((sx1 - fsx1) / cell)))
        for sx in range(sx1, sx2):
            taps.append((sx, f32(1.0 / cell)))
        if fsx2 - sx2 > 1e-3:
            taps.append((sx2, f32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
        tab.append(taps)
    return tab


def _tab_arrays(tab):
    m = max(len(t) for t in tab)
    idx = np.zeros((len(tab), m), np.int64)
    w = np.zeros((len(tab), m), f32)
    n = np.array([len(t) for t in tab])
    for d, taps in enumerate(tab):
        for k, (s, a) in enumerate(taps):
            idx[d, k], w[d, k] = s, a
    return idx, w, n


def resize_area(src, dh, dw):
    """choices 2 and 3"""
    sh, sw = src.shape
    if dh == 0 or dw == 0:
        return np.zeros((dh, dw), np.uint8)
    if sh == 2 * dh and sw == 2 * dw:
        s = src.astype(np.int32)
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    xi, xw, xn = _tab_arrays(area_tab(sw, dw))
    yi, yw, yn = _tab_arrays(area_tab(sh, dh))
    S = src.astype(f32)
    buf = np.zeros((sh, dw), f32)
    for k in range(xi.shape[1]):
        live = xn > k
        buf[:, live] = buf[:, live] + S[:, xi[live, k]] * xw[live, k][None, :]     # float32 product, float32 sum: two roundings
    out = np.zeros((dh, dw), f32)
    for k in range(yi.shape[1]):
        live = yn > k
        term = yw[live, k][:, None] * buf[yi[live, k], :]
        out[live, :] = term if k == 0 else out[live, :] + term
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)                           # rint: ties to even


def pyramid(img):
    img = np.ascontiguousarray(img, np.uint8)
    shapes = layer_shapes(*img.shape)
    layers = [img, resize_area(img, *shapes[1])]
    for i in range(2, N_LAYERS):
        layers.append(resize_area(layers[i - 2], *shapes[i]))
    return layers


# ---------------------------------------------------------------- dense scores (choices 4, 5)
def _arc_score(im, ring, arc, border):
    """max over the arcs of `arc` contiguous ring pixels of min |difference| (all of one sign), minus one; 0 inside `border`"""
    h, w = im.shape
    out = np.zeros((h, w), np.uint8)
    if h <= 2 * border or w <= 2 * border:
        return out
    c = im[border:h - border, border:w - border].astype(np.int16)
    d = [im[border + dy:h - border + dy, border + dx:w - border + dx].astype(np.int16) - c for dx, dy in ring]
    n = len(ring)
    best = np.zeros(c.shape, np.int16)
    for s in range(n):
        mn, mx = d[s], d[s]
        for k in range(1, arc):
            mn = np.minimum(mn, d[(s + k) % n])
            mx = np.maximum(mx, d[(s + k) % n])
        best = np.maximum(best, np.maximum(mn, -mx))
    out[border:h - border, border:w - border] = np.maximum(best - 1, 0).astype(np.uint8)
    return out


def score_9_16(im):
    return _arc_score(im, CIRCLE16, 9, 3)


def score_5_8(im):
    return _arc_score(im, RING8, 5, 2)


def lazy_score_9_16(im, x, y, thr):
    """OpenCV's cold-cache read, literally (bounds, bisection from thr - 1, zero below thr): what the purity test holds `read` against"""
    h, w = im.shape
    if x < 3 or y < 3 or x >= w - 3 or y >= h - 3:
        return 0
    c = int(im[y, x])
    d = [int(im[y + dy, x + dx]) - c for dx, dy in CIRCLE16]

    def corner(b):
        for s in range(16):
            arc = [d[(s + k) % 16] for k in range(9)]
            if all(v > b for v in arc) or all(v < -b for v in arc):
                return True
        return False

    bmin, bmax = thr - 1, 255
    b = (bmax + bmin) // 2
    while True:
        if corner(b):
            bmin = b
        else:
            bmax = b
        if bmin == bmax - 1 or bmin == bmax:
            break
        b = (bmin + bmax) // 2
    return bmin if bmin >= thr else 0


class Layer:
    def __init__(self, im, scale, offset):
        self.im, self.scale, self.offset = im, scale, offset
        self.h, self.w = im.shape
        self.s = score_9_16(im)
        self.s5 = None

    def read(self, x, y, thr=1):
        """choice 4 / 14"""
        if x < 0 or y < 0 or x >= self.w or y >= self.h:
            return 0
        v = int(self.s[y, x])
        return v if v >= thr else 0

    def read5(self, x, y):
        if x < 0 or y < 0 or x >= self.w or y >= self.h:
            return 0
        return int(self.s5[y, x])

    def read_f(self, xf, yf):
        """choice 6 (threshold 1, scale 1)"""
        x, y = int(xf), int(yf)
        rx1 = f32(xf - f32(x)); rx = f32(f32(1.0) - rx1)
        ry1 = f32(yf - f32(y)); ry = f32(f32(1.0) - ry1)
        v = f32(f32(rx * ry) * f32(self.read(x, y)))
        v = f32(v + f32(f32(rx1 * ry) * f32(self.read(x + 1, y))))
        v = f32(v + f32(f32(rx * ry1) * f32(self.read(x, y + 1))))
        v = f32(v + f32(f32(rx1 * ry1) * f32(self.read(x + 1, y + 1))))
        return int(v) & 0xFF

    def patch(self, x, y):
        """s_0_0 .. s_2_2 as subpixel2D takes them: first index = column offset, second = row offset"""
        return [[self.read(x + i - 1, y + j - 1) for j in range(3)] for i in range(3)]


def smoothed_value(score, xf, yf, scale):
    """choice 6, the branch for scale > 1 (BriskLayer::value on the score image) with reads outside the layer = 0 (choice 14).  The
    detector never reaches it; restated for completeness."""
    h, w = score.shape

    def at(x, y):
        return int(score[y, x]) if 0 <= x < w and 0 <= y < h else 0

    xf, yf, scale = f32(xf), f32(yf), f32(scale)
    x, y = int(np.floor(xf)), int(np.floor(yf))
    sigma_half = f32(scale / f32(2.0))
    area = f32(f32(f32(4.0) * sigma_half) * sigma_half)
    if sigma_half < 0.5:
        r_x, r_y = int(f32(f32(xf - f32(x)) * f32(1024))), int(f32(f32(yf - f32(y)) * f32(1024)))
        r_x_1, r_y_1 = 1024 - r_x, 1024 - r_y
        ret = r_x_1 * r_y_1 * at(x, y) + r_x * r_y_1 * at(x + 1, y) + r_x * r_y * at(x + 1, y + 1) + r_x_1 * r_y * at(x, y + 1)
        return 0xFF & ((ret + 512) // 1024 // 1024)
    scaling = int(f32(f32(4194304.0) / area))
    scaling2 = int(f32(f32(f32(scaling) * area) / f32(1024.0)))
    x_1, x1, y_1, y1 = f32(xf - sigma_half), f32(xf + sigma_half), f32(yf - sigma_half), f32(yf + sigma_half)
    x_left, y_top, x_right, y_bottom = int(f64(x_1) + 0.5), int(f64(y_1) + 0.5), int(f64(x1) + 0.5), int(f64(y1) + 0.5)
    r_x_1 = f32(f32(f32(x_left) - x_1) + f32(0.5)); r_y_1 = f32(f32(f32(y_top) - y_1) + f32(0.5))
    r_x1 = f32(f32(x1 - f32(x_right)) + f32(0.5)); r_y1 = f32(f32(y1 - f32(y_bottom)) + f32(0.5))
    A, B = int(f32(f32(r_x_1 * r_y_1) * f32(scaling))), int(f32(f32(r_x1 * r_y_1) * f32(scaling)))
    C, D = int(f32(f32(r_x1 * r_y1) * f32(scaling))), int(f32(f32(r_x_1 * r_y1) * f32(scaling)))
    wx = [int(f32(r_x_1 * f32(scaling)))] + [scaling] * (x_right - x_left - 1) + [int(f32(r_x1 * f32(scaling)))]
    wy = [int(f32(r_y_1 * f32(scaling)))] + [scaling] * (y_bottom - y_top - 1) + [int(f32(r_y1 * f32(scaling)))]
    ret = 0
    for j, yy in enumerate(range(y_top, y_bottom + 1)):
        for i, xx in enumerate(range(x_left, x_right + 1)):
            ex, ey = i in (0, len(wx) - 1), j in (0, len(wy) - 1)
            if ex and ey:
                wgt = {(0, 0): A, (1, 0): B, (1, 1): C, (0, 1): D}[(int(i != 0), int(j != 0))]
            elif ey:
                wgt = wy[j]
            elif ex:
                wgt = wx[i]
            else:
                wgt = scaling
            ret += wgt * at(xx, yy)
    return 0xFF & ((ret + scaling2 // 2) // scaling2 // 1024)


# ---------------------------------------------------------------- refinement (choices 8-11)
def _cdiv(a, b):
    return f32(f32(a) / f32(b))


def _quad(c1, c2, c3, c4, c5, c6, dx, dy):
    v = f32(f32(f32(c1) * dx) * dx)
    v = f32(v + f32(f32(f32(c2) * dy) * dy))
    v = f32(v + f32(f32(c3) * dx))
    v = f32(v + f32(f32(c4) * dy))
    v = f32(v + f32(f32(f32(c5) * dx) * dy))
    v = f32(v + f32(c6))
    return f32(v / f32(18.0))


def _clamp1(v):
    return f32(1.0) if v > f32(1.0) else (f32(-1.0) if v < f32(-1.0) else v)


def subpixel2d(p):
    """p[i][j] = s_i_j.  -> (refined maximum, delta_x, delta_y)"""
    (s00, s01, s02), (s10, s11, s12), (s20, s21, s22) = p
    tmp1 = s00 + s02 - 2 * s11 + s20 + s22
    c1 = 3 * (tmp1 + s01 - ((s10 + s12) << 1) + s21)
    c2 = 3 * (tmp1 - ((s01 + s21) << 1) + s10 + s12)
    tmp2 = s02 - s20
    tmp3 = s00 + tmp2 - s22
    tmp4 = tmp3 - 2 * tmp2
    c3 = -3 * (tmp3 + s01 - s21)
    c4 = -3 * (tmp4 + s10 - s12)
    c5 = (s00 - s02 - s20 + s22) * 4
    c6 = -(s00 + s02 - ((s10 + s01 + s12 + s21) << 1) - 5 * s11 + s20 + s22) * 2
    hdet = 4 * c1 * c2 - c5 * c5
    one = f32(1.0)
    if hdet == 0:
        return _cdiv(c6, 18.0), f32(0.0), f32(0.0)
    if not (hdet > 0 and c1 < 0):
        tmax, dx, dy = c3 + c4 + c5, one, one
        t = -c3 + c4 - c5
        if t > tmax:
            tmax, dx, dy = t, -one, one
        t = c3 - c4 - c5
        if t > tmax:
            tmax, dx, dy = t, one, -one
        t = -c3 - c4 + c5
        if t > tmax:
            tmax, dx, dy = t, -one, -one
        return _cdiv(tmax + c1 + c2 + c6, 18.0), dx, dy
    dx = _cdiv(2 * c2 * c3 - c4 * c5, -hdet)
    dy = _cdiv(2 * c1 * c4 - c3 * c5, -hdet)
    tx, tx_ = dx > one, (not dx > one) and dx < -one
    ty, ty_ = dy > one, dy < -one
    if tx or tx_ or ty or ty_:
        dx1 = dx2 = dy1 = dy2 = f32(0.0)
        if tx:
            dx1, dy1 = one, _clamp1(_cdiv(-f32(c4 + c5), 2 * c2))
        elif tx_:
            dx1, dy1 = -one, _clamp1(_cdiv(-f32(c4 - c5), 2 * c2))
        if ty:
            dy2, dx2 = one, _clamp1(_cdiv(-f32(c3 + c5), 2 * c1))
        elif ty_:
            dy2, dx2 = -one, _clamp1(_cdiv(-f32(c3 - c5), 2 * c1))
        m1, m2 = _quad(c1, c2, c3, c4, c5, c6, dx1, dy1), _quad(c1, c2, c3, c4, c5, c6, dx2, dy2)
        return (m1, dx1, dy1) if m1 > m2 else (m2, dx2, dy2)
    return _quad(c1, c2, c3, c4, c5, c6, dx, dy), dx, dy


def _i1024(v):
    return int(f64(1024.0) * f64(v) + f64(0.5))


def _refine1d(s_05, s0, s05, ca, cb, cc, lo, hi, div):
    """(scale, max): a = ca . i, b = cb . i, c = cc . i on the scores x 1024; lo / hi the scales of the layer below / above"""
    i_05, i0, i05 = _i1024(s_05), _i1024(s0), _i1024(s05)
    a = ca[0] * i_05 + ca[1] * i0 + ca[2] * i05
    if a >= 0:
        if s0 >= s_05 and s0 >= s05:
            return f32(1.0), s0
        if s_05 >= s0 and s_05 >= s05:
            return lo, s_05
        return hi, s05
    b = cb[0] * i_05 + cb[1] * i0 + cb[2] * i05
    r = f32(-f32(b) / f32(2 * a))
    if r < lo:
        r = lo
    elif r > hi:
        r = hi
    c = cc[0] * i_05 + cc[1] * i0 + cc[2] * i05
    m = f32(f32(c) + f32(f32(f32(a) * r) * r))
    m = f32(m + f32(f32(b) * r))
    return r, f32(m / f32(div))


def refine1d(s_05, s0, s05):       # even layers above 0: the layers below / above lie at 0.75 / 1.5
    return _refine1d(s_05, s0, s05, (16, -24, 8), (-40, 54, -14), (24, -27, 6), f32(0.75), f32(1.5), 3072.0)


def refine1d_1(s_05, s0, s05):     # odd layers: 2 / 3 and 4 / 3
    return _refine1d(s_05, s0, s05, (9, -18, 9), (-21, 36, -15), (12, -16, 6), f32(0.6666666666666666), f32(1.3333333333333333), 2048.0)


def refine1d_2(s_05, s0, s05):     # layer 0: the virtual layer at 0.7, layer 1 at 1.5
    return _refine1d(s_05, s0, s05, (2, -4, 2), (-5, 8, -3), (3, -3, 1), f32(0.7), f32(1.5), 1024.0)


def _sat(d):
    if d > f32(1.0):
        return f32(1.0), False
    if d < f32(-1.0):
        return f32(-1.0), False
    return d, True


def _window(x, y, num, a, b, den):
    """corners ((num * x + a -/+ b) / den) of the window a pixel covers in the other layer, float"""
    return (_cdiv(num * x + a - b, den), _cdiv(num * x + a + b, den), _cdiv(num * y + a - b, den), _cdiv(num * y + a + b, den))


def _search(L, x_1, x1, y_1, y1, thr, ties):
    """the window search shared by getScoreMaxAbove / getScoreMaxBelow -> None (a larger value) or (max, max_x, max_y)"""
    xs = list(range(int(x_1) + 1, int(x1) + 1))
    max_x, max_y = int(x_1) + 1, int(y_1) + 1
    mx = L.read_f(x_1, y_1)
    if mx > thr:
        return None
    for x in xs:
        t = L.read_f(f32(x), y_1)
        if t > thr:
            return None
        if t > mx:
            mx, max_x = t, x
    t = L.read_f(x1, y_1)
    if t > thr:
        return None
    if t > mx:
        mx, max_x = t, int(x1)
    for y in range(int(y_1) + 1, int(y1) + 1):
        t = L.read_f(x_1, f32(y))
        if t > thr:
            return None
        if t > mx:
            mx, max_x, max_y = t, int(f32(x_1 + f32(1.0))), y
        for x in xs:
            t = L.read(x, y)
            if t > thr:
                return None
            if ties and t == mx:
                def ring(cx, cy):
                    return (2 * (L.read(cx - 1, cy) + L.read(cx + 1, cy) + L.read(cx, cy + 1) + L.read(cx, cy - 1))
                            + L.read(cx + 1, cy + 1) + L.read(cx - 1, cy + 1) + L.read(cx + 1, cy - 1) + L.read(cx - 1, cy - 1))
                if ring(x, y) > ring(max_x, max_y):
                    max_x, max_y = x, y
            if t > mx:
                mx, max_x, max_y = t, x, y
        t = L.read_f(x1, f32(y))
        if t > thr:
            return None
        if t > mx:
            mx, max_x, max_y = t, int(x1), y
    t = L.read_f(x_1, y1)
    if t > mx:
        mx, max_x, max_y = t, int(f32(x_1 + f32(1.0))), int(y1)
    for x in xs:
        t = L.read_f(f32(x), y1)
        if t > mx:
            mx, max_x, max_y = t, x, int(y1)
    t = L.read_f(x1, y1)
    if t > mx:
        mx, max_x, max_y = t, int(x1), int(y1)
    return mx, max_x, max_y


def score_max_above(layers, layer, x, y, thr):
    """-> None or (max, dx, dy)"""
    L = layers[layer + 1]
    win = _window(x, y, 4, -1, 2, 6.0) if layer % 2 == 0 else _window(x, y, 6, -1, 3, 8.0)
    r = _search(L, *win, thr, False)
    if r is None:
        return None
    mx, max_x, max_y = r
    refined, dx_1, dy_1 = subpixel2d(L.patch(max_x, max_y))
    real_x, real_y = f32(f32(max_x) + dx_1), f32(f32(max_y) + dy_1)
    if layer % 2 == 0:
        dx = f32(_cdiv(f32(f32(real_x * f32(6.0)) + f32(1.0)), 4.0) - f32(x))
        dy = f32(_cdiv(f32(f32(real_y * f32(6.0)) + f32(1.0)), 4.0) - f32(y))
    else:
        dx = f32((f64(real_x) * 8.0 + 1.0) / 6.0 - f64(x))
        dy = f32((f64(real_y) * 8.0 + 1.0) / 6.0 - f64(y))
    dx, okx = _sat(dx)
    dy, oky = _sat(dy)
    return (max(refined, f32(mx)) if okx and oky else f32(mx)), dx, dy


def score_max_below(layers, layer, x, y, thr):
    L = layers[layer - 1]
    win = _window(x, y, 8, 1, 4, 6.0) if layer % 2 == 0 else _window(x, y, 6, 1, 3, 4.0)
    r = _search(L, *win, thr, True)
    if r is None:
        return None
    mx, max_x, max_y = r
    refined, dx_1, dy_1 = subpixel2d(L.patch(max_x, max_y))
    real_x, real_y = f32(f32(max_x) + dx_1), f32(f32(max_y) + dy_1)
    if layer % 2 == 0:
        dx = f32(f32((f64(real_x) * 6.0 + 1.0) / 8.0) - f32(x))
        dy = f32(f32((f64(real_y) * 6.0 + 1.0) / 8.0) - f32(y))
    else:
        dx = f32(f32((f64(real_x) * 4.0 - 1.0) / 6.0) - f32(x))
        dy = f32(f32((f64(real_y) * 4.0 - 1.0) / 6.0) - f32(y))
    dx, okx = _sat(dx)
    dy, oky = _sat(dy)
    return (max(refined, f32(mx)) if okx and oky else f32(mx)), dx, dy


def _lerp_pos(r0, r1, d_layer, d_other, p, L, scaled=True):
    v = f32(f32(f32(r0 * d_layer) + f32(r1 * d_other)) + f32(p))
    return f32(f32(v * L.scale) + L.offset) if scaled else v


def refine3d(layers, layer, x, y):
    """-> None or (score, x, y, scale)"""
    L = layers[layer]
    center = L.read(x, y)
    above = score_max_above(layers, layer, x, y, center)
    if above is None:
        return None
    max_above, dxa, dya = above
    if layer == 0:
        p5 = [[L.read5(x + i - 1, y + j - 1) for j in range(3)] for i in range(3)]
        max_below = f32(max(max(c) for c in p5))
        _, dxb, dyb = subpixel2d(p5)
    else:
        below = score_max_below(layers, layer, x, y, center)
        if below is None:
            return None
        max_below, dxb, dyb = below
    max_layer, dxl, dyl = subpixel2d(L.patch(x, y))
    s0 = max(f32(center), max_layer)
    one = f32(1.0)
    if layer % 2 == 0:
        scale, mx = refine1d_2(max_below, s0, max_above) if layer == 0 else refine1d(max_below, s0, max_above)
        if scale > one:
            r0 = f32(f32(f32(1.5) - scale) / f32(0.5))
            r1 = f32(one - r0)
            px, py = _lerp_pos(r0, r1, dxl, dxa, x, L), _lerp_pos(r0, r1, dyl, dya, y, L)
        elif layer == 0:
            r0 = f32(f32(scale - f32(0.5)) / f32(0.5))
            r1 = f32(one - r0)
            px, py = _lerp_pos(r0, r1, dxl, dxb, x, L, False), _lerp_pos(r0, r1, dyl, dyb, y, L, False)
        else:
            r0 = f32(f32(scale - f32(0.75)) / f32(0.25))
            r1 = f32(one - r0)
            px, py = _lerp_pos(r0, r1, dxl, dxb, x, L), _lerp_pos(r0, r1, dyl, dyb, y, L)
    else:
        scale, mx = refine1d_1(max_below, s0, max_above)
        if scale > one:
            r0 = f32(f32(4.0) - f32(scale * f32(3.0)))
            r1 = f32(one - r0)
            px, py = _lerp_pos(r0, r1, dxl, dxa, x, L), _lerp_pos(r0, r1, dyl, dya, y, L)
        else:
            r0 = f32(f32(scale * f32(3.0)) - f32(2.0))
            r1 = f32(one - r0)
            px, py = _lerp_pos(r0, r1, dxl, dxb, x, L), _lerp_pos(r0, r1, dyl, dyb, y, L)
    return mx, px, py, f32(scale * L.scale)


# ---------------------------------------------------------------- detection (choices 7, 12, 13)
def is_max_2d(L, x, y, thr, stats=None):
    def at(xx, yy):
        return L.read(xx, yy, thr)

    c = at(x, y)
    nb = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
    v = [at(x + dx, y + dy) for dx, dy in nb]
    if any(c < t for t in v):
        return False

    def smooth(cx, cy):
        return (4 * at(cx, cy) + 2 * (at(cx - 1, cy) + at(cx + 1, cy) + at(cx, cy - 1) + at(cx, cy + 1))
                + at(cx - 1, cy - 1) + at(cx + 1, cy - 1) + at(cx - 1, cy + 1) + at(cx + 1, cy + 1))

    ties = [d for d, t in zip(nb, v) if t == c]
    if ties:
        if stats is not None:
            stats["ties"] = stats.get("ties", 0) + 1
        sc = smooth(x, y)
        for dx, dy in ties:
            if smooth(x + dx, y + dy) > sc:
                if stats is not None:
                    stats["tie_rejects"] = stats.get("tie_rejects", 0) + 1
                return False
    return True


def build_layers(img):
    ims = pyramid(img)
    layers = [Layer(im, s, o) for im, s, o in zip(ims, layer_scales(), layer_offsets())]
    layers[0].s5 = score_5_8(ims[0])
    return layers


def detect(img, threshold=30, stats=None, layers=None):
    """-> keypoints (KP_DTYPE), in OpenCV's order.  stats (a dict) receives counts of the branches taken."""
    layers = build_layers(img) if layers is None else layers
    out = []
    for li, L in enumerate(layers):
        ys, xs = np.nonzero(L.s >= threshold)
        for y, x in zip(ys.tolist(), xs.tolist()):
            if stats is not None:
                stats["candidates"] = stats.get("candidates", 0) + 1
            if not is_max_2d(L, x, y, threshold, stats):
                continue
            if li == N_LAYERS - 1:
                if score_max_below(layers, li, x, y, L.read(x, y, threshold)) is None:
                    continue
                mx, dx, dy = subpixel2d(L.patch(x, y))
                out.append((f32(f32(f32(f32(x) + dx) * L.scale) + L.offset), f32(f32(f32(f32(y) + dy) * L.scale) + L.offset),
                            f32(BASIC_SIZE * L.scale), f32(-1.0), mx, li))
            else:
                r = refine3d(layers, li, x, y)
                if r is None:
                    continue
                score, px, py, scale = r
                if score > f32(threshold):
                    out.append((px, py, f32(BASIC_SIZE * scale), f32(-1.0), score, li))
    kp = np.zeros(len(out), KP_DTYPE)
    for i, rec in enumerate(out):
        kp[i] = rec
    return kp
