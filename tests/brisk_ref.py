"""Numpy restatement of the BRISK descriptor extractor as csrc/brisk.hip.h builds it: cv::BRISK::create(30, 3, 1.0f)->compute(img,
keypoints, desc) on given keypoints (feature_detection_classic.cpp:56-65, 110-111).  No OpenCV exists in this build to pin it against:
this file is the definition, and the kernels reproduce it bit for bit when both run on the same tables.  Every choice, and whether it is
OpenCV 4.x's rule as far as known ("OpenCV") or a decision of this project ("ours"):

  Pattern
   1. OpenCV: pattern_scale = 1; ring radii 0.85 * {0, 2.9, 4.9, 7.4, 10.8}; points per ring {1, 10, 14, 15, 20}, 60 points in all.
      OpenCV: a radius is the double product 0.85f * r stored as float.
   2. OpenCV: 64 scales span a range of 30: scale_list[s] = (float)pow(2, s * log2(30) / 64); 1024 rotations.
   3. OpenCV: point (s, rot, ring, num) lies at scale_list[s] * r[ring] * (cos, sin)(num * 2 pi / n[ring] + rot * 2 pi / 1024), the
      angle computed in double, the result stored as float.
   4. OpenCV: sigma = 1.3 * scale_list[s] * 0.5 on ring 0 and 1.3 * scale_list[s] * r[ring] * sin(pi / n[ring]) on the others, stored as
      float (1.3 is the float 1.3f).
   5. OpenCV: size_list[s] = the maximum over rings of ceil(scale_list[s] * r[ring] + sigma) + 1.  ours: the sum is taken in double.
  Pairs
   6. OpenCV: enumerated from the scale-0, rotation-0 points (as stored: float), for i in 1..59: for j in 0..i-1, d = p[j] - p[i].
      |d|^2 > 8.2^2: a long pair with weighted_dx = (int)(dx / |d|^2 * 2048 + 0.5), weighted_dy likewise; else |d|^2 < 5.85^2: a short
      pair.  Enumeration order is descriptor bit order.  512 short and 870 long pairs (asserted).  ours: d and |d|^2 in double from the
      float points, the thresholds are the squares of the floats 8.2f and 5.85f.
   7. OpenCV has a bilinear branch for sigma < 0.5.  The table builder asserts that every sigma >= 0.5 (the minimum is 0.65, ring 0 at
      scale 0), so that branch is dead with this pattern and is left out.
  Per keypoint
   8. OpenCV: s = max((int)(64 / log2(30) * log2(size / 7.2) + 0.5), 0), capped at 63, in float arithmetic: lb = (float)log(30) /
      0.693147180559945f, 7.2 is the float product 12 * 0.6f, every quotient and product is a float, + 0.5 is added in double.
      ours: a float logarithm is the double logarithm rounded to float (a libm's logf may differ from that by one float step; it
      changes s only for a size within 1e-7 relative of a scale boundary).
   9. OpenCV: a keypoint is dropped when x < b || x >= cols - b || y < b || y >= rows - b with b = size_list[s]; dropping preserves
      order.  ours: a keypoint with a NaN coordinate is dropped too (OpenCV's comparison would keep it).
  Smoothed intensity (box mean of half-width sigma around (x + px, y + py), in integers)
  10. OpenCV: xf = px + x, yf = py + y as float; area = 4 sigma^2 (float); scaling = (int)(4194304.0 / area), scaling2 =
      (int)((float)scaling * area / 1024.0).  The box edges xf -/+ sigma, yf -/+ sigma (float) are rounded with + 0.5 (double) and
      truncated; the fractional edge weights r = edge distance + 0.5f (float), the four corner weights (int)(r_x * r_y * scaling) and
      the four edge weights (int)(r * scaling) are truncated, interior pixels weigh `scaling`; result (sum + scaling2 / 2) / scaling2.
  11. OpenCV takes the interior and edge sums from the integral image when the box is large (dx + dy > 2) and loops over the pixels
      otherwise.  Both give the same integer -- the same pixels with the same integer weights -- so one form is enough: here (and in the
      kernel) every box goes through the integral image, the four corner pixels are read from the image.
      The sum stays below 2^31: the weights along x add up to at most (r_x_1 + dx + r_x1) * scaling = (x1 - x_1) * scaling, along y
      likewise, truncation only lowers them, so the weighted pixel count is at most scaling * (2 sigma)^2 (1 + 1e-5) = scaling * area
      (1 + 1e-5) <= 4194304 (1 + 1e-5) (the 1e-5: x1 - x_1 is a float difference of two rounded floats), and with pixels <= 255 the
      sum is at most 255 * 4194304 * (1 + 1e-5) + scaling2 / 2 < 1.07e9 + 2048 < 2^31.  smoothed_intensity asserts it on every call.
  Orientation
  12. OpenCV: always recomputed (compute() overwrites the angle that came in).  60 intensities at rotation 0; over the long pairs
      dir0 += (v[i] - v[j]) * weighted_dx / 1024 and dir1 likewise, C integer division (towards zero).
  13. OpenCV: angle = (float)(atan2((float)dir1, (float)dir0) / pi * 180); theta = (int)(1024 * (angle / 360.0) + 0.5) (truncation
      towards zero), + 1024 if negative, - 1024 if >= 1024; after that a negative angle gets + 360 (float).  ours: atan2 is the double
      one of the two integers (OpenCV calls the float overload); OpenCV's special case "angle == -1 means theta = 0" cannot be told from
      a computed angle of exactly -1 degree and is left out.
  Descriptor
  14. OpenCV: 60 intensities at rotation theta; bit k = v[short[k].i] > v[short[k].j]; bit k lives in byte k / 8, bit k % 8; 64 bytes.

A row is a BOUNDARY row when 1024 * angle / 360 + 0.5 lies within 1e-4 of an integer: one float step of an angle below 360 degrees is
9e-5 rotation steps, so an atan2 that differs in the last place may pick the neighbouring rotation there.
"""
import functools

import numpy as np

f32, f64, i64 = np.float32, np.float64, np.int64

N_SCALES, N_ROT, N_POINTS = 64, 1024, 60
RING_N = (1, 10, 14, 15, 20)
RING_R = tuple(f32(f64(f32(0.85)) * r) for r in (0.0, 2.9, 4.9, 7.4, 10.8))
D_LONG_SQ = f64(f32(8.2)) ** 2
D_SHORT_SQ = f64(f32(5.85)) ** 2
BASIC_SIZE_06 = f32(f32(12.0) * f32(0.6))
LOG2_F = f32(0.693147180559945)
LB_SCALERANGE = f32(f32(np.log(f64(30.0))) / LOG2_F)


def scale_list():
    return np.array([2.0 ** (s * np.log2(30.0) / N_SCALES) for s in range(N_SCALES)], f64).astype(f32)


def build_points(scales=None):
    """points [64, 1024, 60, 3] float32 (x, y, sigma), built in float64 (choices 1-4); `scales`: only these slices are filled."""
    sl = scale_list().astype(f64)
    out = np.zeros((N_SCALES, N_ROT, N_POINTS, 3), f32)
    theta = np.arange(N_ROT, dtype=f64) * 2 * np.pi / N_ROT
    for s in (range(N_SCALES) if scales is None else scales):
        p = 0
        for ring, n in enumerate(RING_N):
            r = f64(RING_R[ring])
            alpha = np.arange(n, dtype=f64) * 2 * np.pi / n
            a = alpha[None, :] + theta[:, None]
            out[s, :, p:p + n, 0] = (sl[s] * r * np.cos(a)).astype(f32)
            out[s, :, p:p + n, 1] = (sl[s] * r * np.sin(a)).astype(f32)
            sigma = f64(f32(1.3)) * sl[s] * 0.5 if ring == 0 else f64(f32(1.3)) * sl[s] * r * np.sin(np.pi / n)
            out[s, :, p:p + n, 2] = f32(sigma)
            p += n
    return out


def size_list(sl=None):
    sl = (scale_list() if sl is None else np.asarray(sl, f32)).astype(f64)
    out = np.zeros(N_SCALES, np.int32)
    for s in range(N_SCALES):
        for ring, n in enumerate(RING_N):
            r = f64(RING_R[ring])
            sigma = f32(f64(f32(1.3)) * sl[s] * 0.5) if ring == 0 else f32(f64(f32(1.3)) * sl[s] * r * np.sin(np.pi / n))
            assert sigma >= 0.5                                                        # choice 7
            out[s] = max(out[s], int(np.ceil(sl[s] * r + f64(sigma))) + 1)
    return out


def build_pairs(points00):
    """(short [512, 2] = i, j; long [870, 4] = i, j, weighted_dx, weighted_dy) from the scale-0, rotation-0 points [60, 3] (choice 6)."""
    p = np.asarray(points00, f32).astype(f64)
    short, long_ = [], []
    for i in range(1, N_POINTS):
        for j in range(i):
            dx, dy = p[j, 0] - p[i, 0], p[j, 1] - p[i, 1]
            n2 = dx * dx + dy * dy
            if n2 > D_LONG_SQ:
                long_.append((i, j, int(dx / n2 * 2048.0 + 0.5), int(dy / n2 * 2048.0 + 0.5)))
            elif n2 < D_SHORT_SQ:
                short.append((i, j))
    assert len(short) == 512 and len(long_) == 870
    return np.array(short, np.int32), np.array(long_, np.int32)


@functools.lru_cache(maxsize=None)
def own_tables():
    """The restatement's own tables: dict of points, short_pairs, long_pairs, scale_list, size_list."""
    pts = build_points()
    short, long_ = build_pairs(pts[0, 0])
    return dict(points=pts, short_pairs=short, long_pairs=long_, scale_list=scale_list(), size_list=size_list())


def scale_index(size):
    """choice 8"""
    size = np.asarray(size, f32)
    q = size / BASIC_SIZE_06
    lq = np.log(q.astype(f64)).astype(f32)
    w = (f32(N_SCALES) / LB_SCALERANGE) * (lq / LOG2_F)
    s = np.trunc(w.astype(f64) + 0.5)
    return np.clip(s, 0, N_SCALES - 1).astype(np.int32)


def border_keep(xy, size, shape, sizes=None):
    """(indices that survive choice 9, ascending; scale index of every keypoint)"""
    xy = np.asarray(xy, f32).reshape(-1, 2)
    s = scale_index(size).reshape(-1)
    b = (own_tables()["size_list"] if sizes is None else np.asarray(sizes))[s].astype(f32)
    rows, cols = shape
    x, y = xy[:, 0], xy[:, 1]
    with np.errstate(invalid="ignore"):
        keep = (x >= b) & (x < f32(cols) - b) & (y >= b) & (y < f32(rows) - b)
    return np.nonzero(keep)[0].astype(np.int32), s


def integral(img):
    """(rows + 1) x (cols + 1), I[r, c] = sum of img[:r, :c]"""
    I = np.zeros((img.shape[0] + 1, img.shape[1] + 1), i64)
    I[1:, 1:] = np.cumsum(np.cumsum(img.astype(i64), 0), 1)
    return I


def smoothed_intensity(img, I, xf, yf, sigma):
    """choices 10, 11 on float32 arrays of one shape -> int64 array of that shape"""
    rows, cols = img.shape
    area = f32(4.0) * sigma * sigma
    scaling = np.trunc(4194304.0 / area.astype(f64)).astype(i64)
    scf = scaling.astype(f32)
    scaling2 = np.trunc((scf * area).astype(f64) / 1024.0).astype(i64)
    x_1, x1, y_1, y1 = xf - sigma, xf + sigma, yf - sigma, yf + sigma
    xl = np.trunc(x_1.astype(f64) + 0.5).astype(i64)
    yt = np.trunc(y_1.astype(f64) + 0.5).astype(i64)
    xr = np.trunc(x1.astype(f64) + 0.5).astype(i64)
    yb = np.trunc(y1.astype(f64) + 0.5).astype(i64)
    assert xl.min() >= 0 and yt.min() >= 0 and xr.max() < cols and yb.max() < rows and (xr > xl).all() and (yb > yt).all()
    r_x_1 = xl.astype(f32) - x_1 + f32(0.5)
    r_y_1 = yt.astype(f32) - y_1 + f32(0.5)
    r_x1 = x1 - xr.astype(f32) + f32(0.5)
    r_y1 = y1 - yb.astype(f32) + f32(0.5)
    tr = lambda v: np.trunc(v).astype(i64)
    A, B, C, D = tr((r_x_1 * r_y_1) * scf), tr((r_x1 * r_y_1) * scf), tr((r_x1 * r_y1) * scf), tr((r_x_1 * r_y1) * scf)
    wl, wt, wr, wb = tr(r_x_1 * scf), tr(r_y_1 * scf), tr(r_x1 * scf), tr(r_y1 * scf)
    S = lambda r0, r1, c0, c1: I[r1, c1] - I[r0, c1] - I[r1, c0] + I[r0, c0]          # sum of img[r0:r1, c0:c1]
    im = img.astype(i64)
    total = A * im[yt, xl] + B * im[yt, xr] + C * im[yb, xr] + D * im[yb, xl]
    total += S(yt, yt + 1, xl + 1, xr) * wt + S(yb, yb + 1, xl + 1, xr) * wb
    total += S(yt + 1, yb, xl, xl + 1) * wl + S(yt + 1, yb, xr, xr + 1) * wr
    total += S(yt + 1, yb, xl + 1, xr) * scaling
    total += scaling2 // 2
    assert total.size == 0 or (total.max() < 2 ** 31 and total.min() >= 0)
    return total // scaling2


def _cdiv1024(a):
    return np.sign(a) * (np.abs(a) // 1024)


def theta_of(angle):
    """choice 13 on the angle BEFORE the + 360 (float32 degrees) -> (theta, 1024 * angle / 360 + 0.5)"""
    v = 1024.0 * (np.asarray(angle, f32).astype(f64) / 360.0) + 0.5
    t = np.trunc(v).astype(i64)
    t = np.where(t < 0, t + N_ROT, t)
    return np.where(t >= N_ROT, t - N_ROT, t).astype(np.int32), v


def theta_from_reported(angle):
    """theta from the angle a caller receives (0 .. 360: negative angles got + 360): what lies above 180 was negative"""
    a = np.asarray(angle, f32).astype(f64)
    return theta_of(np.where(a > 180.0, a - 360.0, a).astype(f32))[0]


def describe(img, xy, size, tables=None, atan2_float32=False):
    """cv::BRISK::compute on keypoints xy [n, 2] with sizes size [n] (a scalar is broadcast).  tables: dict as own_tables() (default) or
    the library's.  -> dict of kept [m], scale [m], values0 [m, 60], dir [m, 2], angle [m] (degrees, 0 .. 360), theta [m], desc [m, 64],
    boundary [m] (bool)."""
    T = own_tables() if tables is None else tables
    img = np.ascontiguousarray(img, np.uint8)
    xy = np.asarray(xy, f32).reshape(-1, 2)
    size = np.broadcast_to(np.asarray(size, f32), (len(xy),))
    kept, s_all = border_keep(xy, size, img.shape, T["size_list"])
    s = s_all[kept]
    m = len(kept)
    I = integral(img)
    kx, ky = xy[kept, 0][:, None], xy[kept, 1][:, None]
    pts = T["points"]

    def sample(rot):
        p = pts[s, rot]                                                                # [m, 60, 3]
        return smoothed_intensity(img, I, p[:, :, 0] + kx, p[:, :, 1] + ky, p[:, :, 2])

    v0 = sample(np.zeros(m, np.int64)) if m else np.zeros((0, N_POINTS), i64)
    L = T["long_pairs"].astype(i64)
    delta = v0[:, L[:, 0]] - v0[:, L[:, 1]]
    dir0 = _cdiv1024(delta * L[:, 2]).sum(1)
    dir1 = _cdiv1024(delta * L[:, 3]).sum(1)
    if atan2_float32:
        ang = (np.arctan2(dir1.astype(f32), dir0.astype(f32)).astype(f64) / np.pi * 180.0).astype(f32)
    else:
        ang = (np.arctan2(dir1.astype(f64), dir0.astype(f64)) / np.pi * 180.0).astype(f32)
    theta, v = theta_of(ang)
    boundary = np.abs(v - np.round(v)) < 1e-4
    angle = np.where(ang < 0, ang + f32(360.0), ang).astype(f32)
    v1 = sample(theta.astype(np.int64)) if m else v0
    Sh = T["short_pairs"]
    bits = (v1[:, Sh[:, 0]] > v1[:, Sh[:, 1]]).astype(np.uint8)                        # [m, 512]
    desc = np.packbits(bits.reshape(m, 64, 8), axis=2, bitorder="little").reshape(m, 64)
    return dict(kept=kept, scale=s, values0=v0.astype(np.int32), dir=np.stack([dir0, dir1], 1), angle=angle, theta=theta, desc=desc, boundary=boundary)
