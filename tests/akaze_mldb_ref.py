"""Numpy restatement of the AKAZE orientation and MLDB descriptor as csrc/akaze_mldb.hip.h builds them: cv::AKAZE::create()->compute,
i.e. Compute_Main_Orientation followed by the full 486-bit MLDB descriptor (pattern size 10, 3 channels, 61 bytes;
feature_detection_classic.cpp:69-70).  It continues tests/akaze_ref.py (imported, unchanged), whose scale space it reads.  No OpenCV
exists in this build to pin it against: this file is the definition.  Every float operation is rounded separately to float32, in the
order written, with no fused multiply-add, and NO TRANSCENDENTAL FUNCTION appears anywhere: only +, -, x, /, sqrt and comparisons.
The kernel is therefore held to it bit for bit in every angle and every byte, with no boundary rows.  Every rule, and whether it is
OpenCV's as far as known ("OpenCV") or a decision of this project ("ours"):

  Inputs: the levels of akaze_ref.scale_space; per level the planes Lt (diffused) and Lx = Dx Lsmooth, Ly = Dy Lsmooth of akaze_ref's
  rule 9 (`derivatives`); keypoint records of akaze_ref.KP_DTYPE.  Per keypoint level = class_id, ratio = (float)2^octave(level),
  s = cvRound(0.5f * size / ratio) (round half to even), xf = x / ratio, yf = y / ratio.
      ours: s is kept as the FLOAT cvRound leaves (rintf) and every product (float)(j * s) below is formed as (float)j * s.  Both j and
      s are integers a float holds exactly, so the one rounding of the float product is the rounding of (float)(j * s): the same value
      wherever OpenCV's int product does not overflow, and a defined one where it would (a size of 1e30 is a legal record here).
      ours: cvRound of a coordinate is rintf, compared with the plane's bounds AS A FLOAT; only a coordinate inside the plane is ever
      converted to an integer (an infinite or NaN coordinate, which huge sizes produce, is outside).
  Orientation (OpenCV Compute_Main_Orientation; always recomputed, the angle that came in is ignored)
   O1. OpenCV: for i = -6..6 (outer), j = -6..6 (inner) with i i + j j < 36 -- 109 samples, in this order -- iy = cvRound(yf +
       (float)(j s)), ix = cvRound(xf + (float)(i s)), resX = g * Lx[iy][ix], resY = g * Ly[iy][ix], g = gauss25[|i|][|j|]: SURF's
       7 x 7 table, symmetric, its 28 distinct constants written out below (exp(-(i^2 + j^2) / 12.5) / (12.5 pi) to eight decimals).
       ours: a sample outside the plane reads Lx = Ly = 0 (OpenCV reads out of bounds).
   O2. OpenCV (fastAtan32f, then radians): Ang = A(resY, resX) * (float)(pi / 180), where A(y, x) in degrees is: ax = |x|, ay = |y|;
       if ax >= ay: c = ay / (ax + (float)DBL_EPSILON), c2 = c c, a = (((p7 c2 + p5) c2 + p3) c2 + p1) c; else c = ax / (ay +
       (float)DBL_EPSILON), a = 90 - (the same polynomial); x < 0: a = 180 - a; y < 0: a = 360 - a.  p1, p3, p5, p7 are the float
       products of 0.9997878412794807f, -0.3258083974640975f, 0.1555786518463281f, -0.04432655554792128f with (float)(180 / pi).
   O3. OpenCV: windows ang1 = 0; ang1 < (float)(2 pi); ang1 += 0.15f by float accumulation (42 of them), ang2 = ang1 + (float)(pi / 3)
       > (float)(2 pi) ? ang1 - (float)(5 pi / 3) : ang1 + (float)(pi / 3).  sumX, sumY are sequential sums over k = 0..108 of the
       samples with (ang1 < ang2 && ang1 < Ang && Ang < ang2) || (ang2 < ang1 && ((Ang > 0 && Ang < ang2) || (Ang > ang1 && Ang <
       (float)(2 pi)))).  The first window whose sumX sumX + sumY sumY is strictly above the running maximum (initially 0) wins.
   O4. ours: the reported angle = A(sumY, sumX) of the winner, in degrees (cv::KeyPoint's unit); co = sumX / n, si = sumY / n with
       n = sqrt(sumX sumX + sumY sumY), correctly rounded.  No winner (all sums zero): angle = 0, co = 1, si = 0.
       OpenCV reports A's angle too (in radians inside, degrees on the keypoint) but rotates the descriptor grid by cos / sin of that
       APPROXIMATE angle; this project rotates by the direction (sumX, sumY) itself, so that no libm enters.  The size of that
       deviation is the polynomial's error against atan2: at most 0.00956 degrees (0.009552 on the diagonals, where c = 1 and a = p1 + p3 + p5 +
       p7 = 44.99045; measured over 3600 directions and five magnitudes by tests/test_akaze_mldb_ref_cpu.py, which prints it
       and uses the measured value as the bar of the ramp test).
  Descriptor (OpenCV 4.x MLDB_Full_Descriptor_Invoker; pattern size 10, 3 channels)
   D1. OpenCV: three grids with step = 10, 7, 5: i = -10; i < 10; i += step (outer) and j likewise (inner) give 2 x 2, 3 x 3, 4 x 4
       cells.  Per cell di, dx, dy are sequential sums over k = i..i + step - 1 (outer) and l = j..j + step - 1 (inner):
       sample_y = yf + (((float)l co) s + ((float)k si) s), sample_x = xf + (((float)(-l) si) s + ((float)k co) s), y1, x1 = cvRound of
       these; a sample outside the plane is skipped (4.x); otherwise di += Lt[y1][x1] and with rx = Lx[y1][x1], ry = Ly[y1][x1]:
       dx += -rx si + ry co, dy += rx co + ry si ((-rx) si is the float product, then the sum).  nsamples counts the samples taken;
       if positive, all three sums are divided by (float)nsamples.  values = [di, dx, dy] per cell, cells in loop order.
   D2. OpenCV: bits, grid by grid: for channel 0, 1, 2, for a < b over the grid's cells (a outer, b inner), the bit is set iff
       value[a] > value[b] as floats (OpenCV compares the toggled integer images: ours differs only between +0 and -0).  Bit p lives
       in byte p >> 3, bit p & 7: 18 + 108 + 360 = 486 bits, bits 6 and 7 of byte 60 are zero.
  No keypoint is dropped: n rows in, n rows out.
"""
import math

import numpy as np

from tests import akaze_ref as ak

f32, f64 = np.float32, np.float64
DESC_BYTES, DESC_BITS = 61, 486
NSAMPLES, NWINDOWS = 109, 42

# the 28 distinct constants of SURF's gauss25, G[a][b] with a <= b
_G = {(0, 0): 0.02546481, (0, 1): 0.02350698, (0, 2): 0.01849125, (0, 3): 0.01239505, (0, 4): 0.00708017, (0, 5): 0.00344629, (0, 6): 0.00142946,
      (1, 1): 0.02169968, (1, 2): 0.01706957, (1, 3): 0.01144208, (1, 4): 0.00653582, (1, 5): 0.00318132, (1, 6): 0.00131956,
      (2, 2): 0.01342740, (2, 3): 0.00900066, (2, 4): 0.00514126, (2, 5): 0.00250252, (2, 6): 0.00103800,
      (3, 3): 0.00603332, (3, 4): 0.00344629, (3, 5): 0.00167749, (3, 6): 0.00069579,
      (4, 4): 0.00196855, (4, 5): 0.00095820, (4, 6): 0.00039744,
      (5, 5): 0.00046640, (5, 6): 0.00019346,
      (6, 6): 0.00008024}
GAUSS25 = np.array([[_G[(min(a, b), max(a, b))] for b in range(7)] for a in range(7)], f64)

SAMPLES = [(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 36]      # O1's order
assert len(SAMPLES) == NSAMPLES
GRIDS = (10, 7, 5)
CELLS = [[(i, j) for i in range(-10, 10, step) for j in range(-10, 10, step)] for step in GRIDS]   # D1's order
assert [len(c) for c in CELLS] == [4, 9, 16]

_ATAN_C = (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128)


def _consts(ft):
    """every constant of O2 / O3 in the working precision (float32: the C expressions' values)"""
    scale = ft(180.0 / math.pi)
    p = [ft(ft(c) * scale) for c in _ATAN_C]
    return dict(p1=p[0], p3=p[1], p5=p[2], p7=p[3], eps=ft(2.220446049250313e-16), rad=ft(math.pi / 180.0), two_pi=ft(2.0 * math.pi),
                third=ft(math.pi / 3.0), five_thirds=ft(5.0 * math.pi / 3.0), step=ft(0.15))


def fast_atan(y, x, ft=f32):
    """O2's A(y, x) in degrees, elementwise"""
    C = _consts(ft)
    y, x = np.asarray(y, ft), np.asarray(x, ft)
    ax, ay = np.abs(x), np.abs(y)
    first = ax >= ay
    c = np.where(first, ay, ax) / (np.where(first, ax, ay) + C["eps"])
    c2 = c * c
    a = (((C["p7"] * c2 + C["p5"]) * c2 + C["p3"]) * c2 + C["p1"]) * c
    a = np.where(first, a, ft(90) - a)
    a = np.where(x < 0, ft(180) - a, a)
    return np.where(y < 0, ft(360) - a, a)


def windows(ft=f32):
    """O3 -> (ang1 [42], ang2 [42])"""
    C = _consts(ft)
    a1 = []
    ang1 = ft(0)
    while ang1 < C["two_pi"]:
        a1.append(ang1)
        ang1 = ft(ang1 + C["step"])
    a1 = np.array(a1, ft)
    wrap = a1 + C["third"] > C["two_pi"]
    return a1, np.where(wrap, a1 - C["five_thirds"], a1 + C["third"])


def derivatives(levels):
    """per level (Lx, Ly) of akaze_ref's rule 9: the scaled Scharr first derivatives of Lsmooth"""
    return [(ak._dx(L["Lsmooth"], L["sigma_size"]), ak._dy(L["Lsmooth"], L["sigma_size"])) for L in levels]


def _gather(plane, yr, xr):
    """plane[cvRound y][cvRound x] where the rounded coordinate (already rint'ed, float) is inside, and the inside mask"""
    h, w = plane.shape
    inside = (yr >= 0) & (yr < h) & (xr >= 0) & (xr < w)            # (False for NaN)
    yi = np.where(inside, yr, 0).astype(np.int64)
    xi = np.where(inside, xr, 0).astype(np.int64)
    return plane[yi, xi], inside


def describe(levels, kp, derivs=None, ft=f32, debug=None):
    """-> (angle [n] float32 degrees, desc [n][61] uint8).  `levels` of akaze_ref.scale_space in precision `ft`; `derivs`:
    derivatives(levels), computed when None.  debug: a dict that receives nsamples [n][29] (D1's counts, cells of the three grids in
    order), co, si."""
    n = len(kp)
    angle, desc = np.zeros(n, f32), np.zeros((n, DESC_BYTES), np.uint8)
    nsamp = np.zeros((n, 29), np.int64)
    co_all, si_all = np.ones(n, ft), np.zeros(n, ft)
    if derivs is None:
        derivs = derivatives(levels)
    for level in sorted(set(int(v) for v in kp["class_id"])):
        rows = np.nonzero(kp["class_id"] == level)[0]
        L = levels[level]
        lx, ly = derivs[level]
        with np.errstate(over="ignore", invalid="ignore"):
            a, d, ns, co, si = _describe_level(L["Lt"].astype(ft, copy=False), lx.astype(ft, copy=False), ly.astype(ft, copy=False), ft(2 ** L["octave"]), kp[rows], ft)
        angle[rows], desc[rows], nsamp[rows], co_all[rows], si_all[rows] = a, d, ns, co, si
    if debug is not None:
        debug.update(nsamples=nsamp, co=co_all, si=si_all)
    return angle, desc


def _describe_level(lt, lx, ly, ratio, kp, ft):
    C = _consts(ft)
    n = len(kp)
    x, y, size = kp["x"].astype(ft), kp["y"].astype(ft), kp["size"].astype(ft)
    s = np.rint(ft(0.5) * size / ratio)
    xf, yf = x / ratio, y / ratio
    # ---- O1, O2
    resx, resy = np.zeros((n, NSAMPLES), ft), np.zeros((n, NSAMPLES), ft)
    for k, (i, j) in enumerate(SAMPLES):
        yr, xr = np.rint(yf + ft(j) * s), np.rint(xf + ft(i) * s)
        g = ft(GAUSS25[abs(i)][abs(j)])
        vx, inside = _gather(lx, yr, xr)
        vy, _ = _gather(ly, yr, xr)
        resx[:, k] = g * np.where(inside, vx, ft(0))
        resy[:, k] = g * np.where(inside, vy, ft(0))
    ang = fast_atan(resy, resx, ft) * C["rad"]
    # ---- O3
    a1, a2 = windows(ft)
    assert len(a1) == NWINDOWS
    a1, a2 = a1[None, :, None], a2[None, :, None]
    A = ang[:, None, :]
    take = ((a1 < a2) & (a1 < A) & (A < a2)) | ((a2 < a1) & (((A > 0) & (A < a2)) | ((A > a1) & (A < C["two_pi"]))))
    sx, sy = np.zeros((n, NWINDOWS), ft), np.zeros((n, NWINDOWS), ft)
    for k in range(NSAMPLES):                                       # sequential; a sample not taken adds +0, which changes no sum that started at +0
        sx = sx + np.where(take[:, :, k], resx[:, k, None], ft(0))
        sy = sy + np.where(take[:, :, k], resy[:, k, None], ft(0))
    m = sx * sx + sy * sy
    best = np.zeros(n, ft)
    win = np.full(n, -1)
    for w in range(NWINDOWS):
        better = m[:, w] > best
        best = np.where(better, m[:, w], best)
        win = np.where(better, w, win)
    # ---- O4
    has = win >= 0
    r = np.arange(n)
    wx, wy = sx[r, np.maximum(win, 0)], sy[r, np.maximum(win, 0)]
    norm = np.sqrt(np.where(has, wx * wx + wy * wy, ft(1)))
    co = np.where(has, wx / norm, ft(1))
    si = np.where(has, wy / norm, ft(0))
    angle = np.where(has, fast_atan(wy, wx, ft), ft(0)).astype(f32)
    # ---- D1
    values, counts = [], []
    for step, cells in zip(GRIDS, CELLS):
        ci = np.array([c[0] for c in cells])[None, :]
        cj = np.array([c[1] for c in cells])[None, :]
        di, dx, dy = (np.zeros((n, len(cells)), ft) for _ in range(3))
        ns = np.zeros((n, len(cells)), np.int64)
        X, Y, S, CO, SI = xf[:, None], yf[:, None], s[:, None], co[:, None], si[:, None]
        for dk in range(step):
            for dl in range(step):
                k, l, ml = (ci + dk).astype(ft), (cj + dl).astype(ft), (-(cj + dl)).astype(ft)     # (float)(-l): +0 for l = 0
                sample_y = Y + ((l * CO) * S + (k * SI) * S)
                sample_x = X + ((ml * SI) * S + (k * CO) * S)
                yr, xr = np.rint(sample_y), np.rint(sample_x)
                ri, inside = _gather(lt, yr, xr)
                rx, _ = _gather(lx, yr, xr)
                ry, _ = _gather(ly, yr, xr)
                di = np.where(inside, di + ri, di)
                dx = np.where(inside, dx + ((-rx) * SI + ry * CO), dx)
                dy = np.where(inside, dy + (rx * CO + ry * SI), dy)
                ns += inside
        den = np.maximum(ns, 1).astype(ft)
        pos = ns > 0
        values.append([np.where(pos, v / den, v) for v in (di, dx, dy)])
        counts.append(ns)
    # ---- D2
    bits = np.zeros((n, DESC_BYTES * 8), np.uint8)
    p = 0
    for vals, cells in zip(values, CELLS):
        for v in vals:
            for a in range(len(cells)):
                for b in range(a + 1, len(cells)):
                    bits[:, p] = v[:, a] > v[:, b]
                    p += 1
    assert p == DESC_BITS
    desc = np.packbits(bits, axis=1, bitorder="little")
    return angle, desc, np.concatenate(counts, 1), co, si
