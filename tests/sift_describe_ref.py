"""Numpy restatement of the classic front end's SIFT extractor on GIVEN keypoints as csrc/sift.hip.h builds it (spvo_sift_describe:
cv::SIFT::create()->compute, feature_detection_classic.cpp:71-73, i.e. SIFT::detectAndCompute with useProvidedKeypoints).  No OpenCV
exists in this build to pin it against: this is OpenCV 4.5.4 as far as known, written once here on top of tests/sift_ref.py, whose
taps, pass rule, decimation and stage 6 it uses.  The choices:

  1. unpacking, per keypoint, from its packed `octave` field p: o = p & 255, sign-extended when >= 128; layer = (p >> 8) & 255;
     scale = 1 / 2^o for o >= 0 and 2^-o for o < 0, as float32 (exact powers of two).  Detectors that leave octave = 0 (Shi-Tomasi, FAST)
     give o = 0, layer = 0; BRISK's layer number 0..5 and AKAZE's octave 0..3 are read as o; ORB's level 0..7 likewise.
  2. pyramid extent: first = min(0, min o); n_oct = max o - first + 1 (no keypoint: no pyramid).
  3. base image.  first == -1: sift_ref's (2x upsampling, BASE_SIGMA): the Gaussian levels are sift_ref.pyramid's bit for bit.
     first == 0: u8 -> float32 at the image's own size, one blur with sigma sqrt(max(1.6^2 - 0.5^2, 0.01)), the same taps and pass rule.
  4. layers 1..5 of an octave and the decimation (every second pixel of layer 3, sizes halved rounding down) are sift_ref's.  No
     difference of Gaussians is built.
  5. per keypoint: level gauss[o - first][layer]; point (x * scale, y * scale), each a float32 product, rounded half to even;
     scl = (size * scale) * 0.5, each product rounded to float32; orientation 360 - angle, 0 when within FLT_EPSILON of 360 (the
     detectors' angle = -1 gives 361, which is legal: only differences of angles enter).  Then sift_ref.descriptor's stage 6 with this
     scl: histogram width 3 scl, radius round(width * sqrt(2) * 5 / 2) capped by the level's diagonal, Gaussian weight, trilinear bins,
     0.2 clamp, x512, round half to even, saturate.  Stage 6 wraps the orientation bin ONCE (o0 < 0: + 8): with orientation 361 a
     gradient angle below one degree gives o0 = -9 + 8 = -1, and the flat index ((r0 + 1) * 6 + c0 + 1) * 10 + o0 then names slot 9 of
     the cell before, which the final fold adds to orientation 1 of column c0 - 1 (the border cells are discarded).  OpenCV's
     calcSIFTDescriptor indexes the same way; the kernels reproduce it (sift_share_bin).
  6. output: no keypoint is erased and none is re-ordered: row i belongs to keypoint i.  A patch with no valid sample gives a row of zeros.
  7. refused (spvo_sift_describe: SPVO_ERR_INVALID): x, y, size or angle not finite, size <= 0, o < -1, layer > 5, an octave whose level
     would be empty (min(rows, cols) >> o < 1) or beyond 16 octaves, an image smaller than 6 x 6.
"""
import math

import numpy as np

from tests import sift_ref as sr

F = sr.F
MAX_OCT = 16
BASE_SIGMA_0 = math.sqrt(max(sr.SIGMA * sr.SIGMA - 0.5 * 0.5, 0.01))      # the base image at its own size (first octave 0)


def unpack(p):
    """packed octave field(s) -> (o, layer, scale float32)"""
    p = np.asarray(p).astype(np.int64)
    o = p & 255
    o = np.where(o >= 128, o - 256, o)
    layer = (p >> 8) & 255
    scale = np.where(o >= 0, 1.0 / np.exp2(np.maximum(o, 0).astype(np.float64)), np.exp2(-np.minimum(o, 0).astype(np.float64))).astype(F)
    return o, layer, scale


def pack(o, layer):
    """the packed field of (o, layer) with a zero xi byte"""
    return int((o & 255) | (layer << 8))


def extent(kp):
    """-> (first, n_oct) of a non-empty list"""
    o, _, _ = unpack(kp["octave"])
    first = min(0, int(o.min()))
    return first, int(o.max()) - first + 1


def check(shape, kp):
    """choice 7: raises ValueError for what spvo_sift_describe refuses"""
    rows, cols = shape
    if min(rows, cols) < sr.MIN_SIDE:
        raise ValueError("image below the minimum size")
    o, layer, _ = unpack(kp["octave"])
    for name in ("x", "y", "size", "angle"):
        if not np.isfinite(kp[name]).all():
            raise ValueError("a %s is not finite" % name)
    if not (kp["size"] > 0).all():
        raise ValueError("a size is not positive")
    if len(kp) and (o.min() < -1 or layer.max() > sr.N_LAYERS + 2):
        raise ValueError("octave below -1 or layer above 5")
    if len(kp):
        first, n_oct = extent(kp)
        if n_oct > MAX_OCT or (int(o.max()) > 0 and (min(rows, cols) >> int(o.max())) < 1):
            raise ValueError("an octave without a level")


def level_shapes(rows, cols, first, n_oct):
    h, w = (2 * rows, 2 * cols) if first == -1 else (rows, cols)
    out = []
    for _ in range(n_oct):
        out.append((h, w))
        h, w = h // 2, w // 2
    return out


def pyramid(img, first, n_oct):
    """-> gauss[k][i]: octave first + k, layers 0..5, float32"""
    img = np.ascontiguousarray(img, np.uint8)
    sig = sr.layer_sigmas()
    gauss = []
    for k in range(n_oct):
        if k == 0:
            g = [sr.blur(sr.upsample2(img), sr.BASE_SIGMA) if first == -1 else sr.blur(img.astype(F), BASE_SIGMA_0)]
        else:
            below = gauss[-1]
            g = [np.ascontiguousarray(below[sr.N_LAYERS][::2, ::2][:below[0].shape[0] // 2, :below[0].shape[1] // 2])]
        for i in range(1, sr.N_LAYERS + 3):
            g.append(sr.blur(g[-1], sig[i]))
        gauss.append(g)
    return gauss


def descriptor(G, scl, px, py, angle, T=F):
    """sift_ref.descriptor's stage 6 with the scale handed over: 128 integers (float32) at the integer point (px, py) of level G"""
    H, W = G.shape
    d, n = 4, 8
    ori = T(360) - T(angle)
    if abs(ori - T(360)) < sr.FLT_EPSILON:
        ori = T(0)
    scl = T(scl)
    cos_t, sin_t = np.cos(ori * T(math.pi / 180)), np.sin(ori * T(math.pi / 180))
    hist_width = T(3) * scl
    radius = int(np.rint(hist_width * T(1.4142135623730951) * T(d + 1) * T(0.5)))
    radius = min(radius, int(math.sqrt(float(W) * W + float(H) * H)))
    cos_t, sin_t = cos_t / hist_width, sin_t / hist_width
    # (rows and columns that cannot hold a valid sample are left out of the grid: the same samples in the same order, a smaller array)
    i0, i1 = max(-radius, 1 - py), min(radius, H - 2 - py)
    j0, j1 = max(-radius, 1 - px), min(radius, W - 2 - px)
    if i0 > i1 or j0 > j1:
        return np.zeros(d * d * n, F)
    ii, jj = np.mgrid[i0:i1 + 1, j0:j1 + 1]
    ii, jj = ii.ravel(), jj.ravel()
    iT, jT = ii.astype(T), jj.astype(T)
    c_rot = jT * cos_t - iT * sin_t
    r_rot = jT * sin_t + iT * cos_t
    rbin = r_rot + T(d / 2 - 0.5)
    cbin = c_rot + T(d / 2 - 0.5)
    y, x = py + ii, px + jj
    ok = (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d) & (y > 0) & (y < H - 1) & (x > 0) & (x < W - 1)
    y, x, rbin, cbin, c_rot, r_rot = y[ok], x[ok], rbin[ok], cbin[ok], c_rot[ok], r_rot[ok]
    GT = G if T is F else G.astype(T)
    dx = GT[y, x + 1] - GT[y, x - 1]
    dy = GT[y - 1, x] - GT[y + 1, x]
    w = np.exp((c_rot * c_rot + r_rot * r_rot) * T(-1.0 / (d * d * 0.5)))
    ang = np.arctan2(dy, dx) * T(180.0 / math.pi)
    ang = np.where(ang < 0, ang + T(360), ang)
    mag = np.sqrt(dx * dx + dy * dy) * w
    obin = (ang - ori) * T(n / 360.0)
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    rbin, cbin, obin = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    o0 = np.where(o0 < 0, o0 + n, o0)
    o0 = np.where(o0 >= n, o0 - n, o0)
    v_r1 = mag * rbin
    v_r0 = mag - v_r1
    v_rc11 = v_r1 * cbin
    v_rc10 = v_r1 - v_rc11
    v_rc01 = v_r0 * cbin
    v_rc00 = v_r0 - v_rc01
    hist = np.zeros((d + 2) * (d + 2) * (n + 2), T)
    idx = ((r0 + 1) * (d + 2) + c0 + 1) * (n + 2) + o0
    for v, base in ((v_rc00, 0), (v_rc01, n + 2), (v_rc10, (d + 2) * (n + 2)), (v_rc11, (d + 3) * (n + 2))):
        v1 = v * obin
        np.add.at(hist, idx + base, v - v1)
        np.add.at(hist, idx + base + 1, v1)
    hist = hist.reshape(d + 2, d + 2, n + 2)
    hist[:, :, 0] += hist[:, :, n]
    hist[:, :, 1] += hist[:, :, n + 1]
    dst = hist[1:d + 1, 1:d + 1, :n].reshape(-1).copy()
    thr = np.sqrt(np.sum(dst * dst, dtype=T)) * T(0.2)
    dst = np.minimum(dst, thr)
    nrm = T(512) / max(np.sqrt(np.sum(dst * dst, dtype=T)), T(sr.FLT_EPSILON))
    return np.clip(np.rint(dst * nrm), 0, 255).astype(F)


def point(k):
    """choice 5 for one record: -> (o, layer, px, py, scl float32)"""
    o, layer, scale = unpack(k["octave"])
    scale = F(scale)
    px, py = int(np.rint(F(k["x"]) * scale)), int(np.rint(F(k["y"]) * scale))
    scl = (F(k["size"]) * scale) * F(0.5)
    return int(o), int(layer), px, py, scl


def describe(img, kp, dtype=F, gauss=None):
    """-> desc [n, 128] float32, row i for record i of kp (sift_ref.KP_DTYPE)"""
    T = np.float64 if dtype in (np.float64, "float64") else F
    img = np.ascontiguousarray(img, np.uint8)
    kp = np.asarray(kp, sr.KP_DTYPE)
    check(img.shape, kp)
    desc = np.zeros((len(kp), 128), F)
    if not len(kp):
        return desc
    first, n_oct = extent(kp)
    if gauss is None:
        gauss = pyramid(img, first, n_oct)
    for i, k in enumerate(kp):
        o, layer, px, py, scl = point(k)
        desc[i] = descriptor(gauss[o - first][layer], scl, px, py, k["angle"], T)
    return desc
