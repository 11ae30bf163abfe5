"""Numpy restatement of the classic front end's SIFT detector + descriptor as csrc/sift.hip.h builds them (cv::SIFT::create(),
feature_detection_classic.cpp: nfeatures 0, nOctaveLayers 3, contrastThreshold 0.04, edgeThreshold 10, sigma 1.6).  No OpenCV exists in
this build to pin it against: this is Lowe 2004 with OpenCV 4.5.4's conventions as far as they are known, written once here.  Stages 1-4
are explicit single-rounded float32 operations in one stated order (no fused multiply-add): the kernels reproduce them bit for bit.
Stages 5-6 use exp / atan2 / sin / cos and are not bit-exact; they run in `dtype` (float32, or float64 as the yardstick of how much
their rounding matters).  The choices:

  1. base image: u8 -> float32; 2x bilinear upsampling (first octave -1): destination pixel d samples source (d + 0.5) / 2 - 0.5, i.e.
     weights 0.25 / 0.75 on the two nearest source pixels, indices clamped to the image (all sums exact in float32); then one blur with
     sigma = sqrt(1.6^2 - 4 * 0.5^2).  Octaves: round(log2(smaller side of the upsampled image) - 2) + 1.
  2. blur: layer i (1..5) of an octave = blur(layer i - 1, sig[i]), sig[i] = sqrt((1.6 k^i)^2 - (1.6 k^(i-1))^2), k = 2^(1/3), in double.
     Separable, rows then columns.  Taps: radius r = ((round(8 sigma + 1) | 1) - 1) / 2; t[j] = exp(-j^2 / (2 sigma^2)) for j = -r..r in
     double, summed left to right in double, each divided by the sum and rounded to float32 once.  One pass at pixel p:
     acc = t[0] * x[p]; for j = 1..r: acc = acc + t[j] * (x[m(p - j)] + x[m(p + j)]) -- one multiplication and two additions per j, each
     rounded.  Border reflect-101 as the index map m(i) = i mod (2n - 2), mirrored when >= n (0 when n = 1): valid for any radius.
     Layer 0 of the next octave = every second pixel (even indices) of layer 3, sizes halved rounding down.  DoG i = layer i+1 - layer i.
  3. extrema: DoG layers 1..3, 5-pixel border, |v| > floor(0.5 * 0.04 / 3 * 255) = 1, and v > 0 and >= all 26 neighbours, or v < 0 and <=
     all 26 (ties kept).
  4. refinement (at most 5 steps): derivatives by central differences scaled by 1/255 (float32(1) / float32(255)), x0.5 first, x0.25
     cross; the 3x3 system by Cramer's rule in the order of _solve below (determinant 0 rejects); offset = -solution.  All three
     |offsets| < 0.5: done.  Any |offset| not <= INT_MAX / 3: rejected.  Otherwise move by the offsets rounded half to even; leaving
     layers 1..3 or the 5-pixel border rejects; not done after 5 solves rejects.  contrast = v / 255 + 0.5 * ((dx xc + dy xr) + ds xi);
     |contrast| * 3 < 0.04 rejects; det = dxx dyy - dxy^2 <= 0 or tr^2 * 10 >= 121 det rejects.
     x = ((c + xc) * 2^o) * 0.5, y alike; size = float32(1.6 * 2^((layer + xi) / 3) * 2^o) evaluated in double (pow);
     response = |contrast|; octave = ((o - 1) & 255) | layer << 8 | round((xi + 0.5) * 255) << 16.
  5. orientation on Gaussian layer `layer` of the octave at (r, c): scl = 1.6 * 2^((layer + xi) / 3), radius round(4.5 scl), weight
     exp(-(i^2 + j^2) / (2 (1.5 scl)^2)), pixels with 0 < y < rows - 1, 0 < x < cols - 1; dx = I[y][x+1] - I[y][x-1],
     dy = I[y-1][x] - I[y+1][x]; angle = atan2(dy, dx) in degrees in [0, 360) (true arctangent, not cv::fastAtan2); bin =
     round(0.1 angle) mod 36; histogram += weight * magnitude.  Smoothing (h[i-2] + h[i+2]) / 16 + (h[i-1] + h[i+1]) * 4 / 16 + h[i] * 6 / 16,
     circular.  Peaks: h[j] > both neighbours and >= 0.8 max; bin = j + 0.5 (h[l] - h[r]) / (h[l] - 2 h[j] + h[r]) wrapped to [0, 36);
     angle = 360 - 10 bin, 0 when within FLT_EPSILON of 360.  One keypoint per peak.
  6. descriptor on the same layer at (round(c + xc), round(r + xr)), orientation 360 - angle: 4x4x8 bins, histogram width 3 scl, radius
     round(width * sqrt(2) * 5 / 2) capped by the level's diagonal, Gaussian weight exp(-(r_rot^2 + c_rot^2) / 8), trilinear in
     (row, column, orientation); normalise, clamp at 0.2 x norm, normalise to 512, round half to even, saturate to 0..255: integers
     stored as float32.
  7. order: ascending (x, y, size, angle, response, octave); of records equal in (x, y, size, angle) the first stays (what
     cv::KeyPointsFilter::removeDuplicatedSorted does).
"""
import math

import numpy as np

F = np.float32
N_LAYERS, SIGMA, BORDER, MAX_STEPS = 3, 1.6, 5, 5
KP_DTYPE = np.dtype([("x", F), ("y", F), ("size", F), ("angle", F), ("response", F), ("octave", np.int32)])
MIN_SIDE = 6                        # 2 x 6 = 12 >= 2 x BORDER + 1: the first octave has an interior
FLT_EPSILON = float(np.finfo(F).eps)
INT_LIMIT = F(2147483647 // 3)


def octave_count(rows, cols):
    return int(round(math.log2(2 * min(rows, cols)) - 2)) + 1


def level_shapes(rows, cols):
    out, h, w = [], 2 * rows, 2 * cols
    for _ in range(octave_count(rows, cols)):
        out.append((h, w))
        h, w = h // 2, w // 2
    return out


def layer_sigmas():
    k = 2.0 ** (1.0 / 3.0)
    sig = [SIGMA]
    for i in range(1, N_LAYERS + 3):
        prev = k ** (i - 1) * SIGMA
        total = prev * k
        sig.append(math.sqrt(total * total - prev * prev))
    return sig


BASE_SIGMA = math.sqrt(max(SIGMA * SIGMA - 4 * 0.5 * 0.5, 0.01))


def blur_taps(sigma):
    """t[0..r] (centre first; the kernel is symmetric), float32"""
    r = ((int(round(sigma * 8 + 1)) | 1) - 1) // 2
    t = [math.exp(-(j * j) / (2.0 * sigma * sigma)) for j in range(-r, r + 1)]
    s = 0.0
    for v in t:
        s += v
    return np.array([t[r + j] / s for j in range(r + 1)], np.float64).astype(F)


def reflect101(i, n):
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    m = i % p
    return np.where(m >= n, p - m, m)


def _pass(x, t, axis):
    n = x.shape[axis]
    idx = np.arange(n)
    acc = t[0] * x
    for j in range(1, len(t)):
        acc = acc + t[j] * (np.take(x, reflect101(idx - j, n), axis=axis) + np.take(x, reflect101(idx + j, n), axis=axis))
    return acc


def blur(x, sigma):
    t = blur_taps(sigma)
    return _pass(_pass(np.ascontiguousarray(x, F), t, 1), t, 0)


def upsample2(img):
    I = np.ascontiguousarray(img, np.uint8).astype(F)

    def axis_maps(n):
        d = np.arange(2 * n)
        k = d >> 1
        even = (d & 1) == 0
        a = np.where(even, np.maximum(k - 1, 0), k)
        b = np.where(even, k, np.minimum(k + 1, n - 1))
        wa = np.where(even, F(0.25), F(0.75)).astype(F)
        return a, b, wa, (F(1) - wa).astype(F)
    ay, by, way, wby = axis_maps(I.shape[0])
    ax, bx, wax, wbx = axis_maps(I.shape[1])
    rows = lambda yy: wax[None, :] * I[yy][:, ax] + wbx[None, :] * I[yy][:, bx]
    return way[:, None] * rows(ay) + wby[:, None] * rows(by)


def pyramid(img):
    """-> (gauss, dog): gauss[o][i] (6 layers), dog[o][i] (5 layers), float32"""
    rows, cols = img.shape
    sig = layer_sigmas()
    gauss, dog = [], []
    for o in range(octave_count(rows, cols)):
        g = [blur(upsample2(img), BASE_SIGMA) if o == 0 else np.ascontiguousarray(gauss[-1][N_LAYERS][::2, ::2][:gauss[-1][0].shape[0] // 2, :gauss[-1][0].shape[1] // 2])]
        for i in range(1, N_LAYERS + 3):
            g.append(blur(g[-1], sig[i]))
        gauss.append(g)
        dog.append([g[i + 1] - g[i] for i in range(N_LAYERS + 2)])
    return gauss, dog


def _extrema(D):
    """D [5, H, W] -> (layer, r, c) of the candidates, raster order per layer"""
    _, H, W = D.shape
    if H <= 2 * BORDER or W <= 2 * BORDER:
        return np.zeros((0, 3), np.int64)
    out = []
    for l in range(1, N_LAYERS + 1):
        v = D[l, BORDER:H - BORDER, BORDER:W - BORDER]
        ge = np.ones(v.shape, bool)
        le = np.ones(v.shape, bool)
        for dl in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dl == 0 and dy == 0 and dx == 0:
                        continue
                    nb = D[l + dl, BORDER + dy:H - BORDER + dy, BORDER + dx:W - BORDER + dx]
                    ge &= v >= nb
                    le &= v <= nb
        m = (np.abs(v) > F(1.0)) & (((v > 0) & ge) | ((v < 0) & le))
        rr, cc = np.nonzero(m)
        out.append(np.stack([np.full(len(rr), l), rr + BORDER, cc + BORDER], 1))
    return np.concatenate(out).astype(np.int64)


IMG_SCALE = F(1) / F(255)
D1, D2, DC = IMG_SCALE * F(0.5), IMG_SCALE, IMG_SCALE * F(0.25)


def _derivs(D, l, r, c):
    I = lambda dl, dr, dc: D[l + dl, r + dr, c + dc]      # (l, r, c are arrays)
    dx = (I(0, 0, 1) - I(0, 0, -1)) * D1
    dy = (I(0, 1, 0) - I(0, -1, 0)) * D1
    ds = (I(1, 0, 0) - I(-1, 0, 0)) * D1
    v = I(0, 0, 0)
    v2 = v * F(2)
    dxx = ((I(0, 0, 1) + I(0, 0, -1)) - v2) * D2
    dyy = ((I(0, 1, 0) + I(0, -1, 0)) - v2) * D2
    dss = ((I(1, 0, 0) + I(-1, 0, 0)) - v2) * D2
    dxy = (((I(0, 1, 1) - I(0, 1, -1)) - I(0, -1, 1)) + I(0, -1, -1)) * DC
    dxs = (((I(1, 0, 1) - I(1, 0, -1)) - I(-1, 0, 1)) + I(-1, 0, -1)) * DC
    dys = (((I(1, 1, 0) - I(1, -1, 0)) - I(-1, 1, 0)) + I(-1, -1, 0)) * DC
    return v, dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys


def _solve(dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys):
    """H X = dD by Cramer's rule; -> (det, X0, X1, X2); every operation float32, in this order"""
    c00 = dyy * dss - dys * dys
    c01 = dxy * dss - dys * dxs
    c02 = dxy * dys - dyy * dxs
    det = (dxx * c00 - dxy * c01) + dxs * c02
    with np.errstate(all="ignore"):
        inv = F(1) / det
        m0 = dy * dss - dys * ds
        m1 = dy * dys - dyy * ds
        m2 = dxy * ds - dy * dxs
        X0 = inv * ((dx * c00 - dxy * m0) + dxs * m1)
        X1 = inv * ((dxx * m0 - dx * c01) + dxs * m2)
        X2 = inv * ((dxx * (dyy * ds - dy * dys) - dxy * m2) + dx * c02)
    return det, X0, X1, X2


def _refine(D, cand):
    """-> rows (layer, r, c) int64 and (xi, xr, xc, contrast) float32 of the candidates that survive, in candidate order"""
    _, H, W = D.shape
    l, r, c = cand[:, 0].copy(), cand[:, 1].copy(), cand[:, 2].copy()
    n = len(l)
    active = np.ones(n, bool)
    keep = np.zeros(n, bool)
    off = np.zeros((n, 4), F)
    for _ in range(MAX_STEPS):
        a = np.nonzero(active)[0]
        if not len(a):
            break
        v, dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys = _derivs(D, l[a], r[a], c[a])
        det, X0, X1, X2 = _solve(dx, dy, ds, dxx, dyy, dss, dxy, dxs, dys)
        xc, xr, xi = -X0, -X1, -X2
        ok = det != 0
        done = ok & (np.abs(xi) < F(0.5)) & (np.abs(xr) < F(0.5)) & (np.abs(xc) < F(0.5))
        with np.errstate(all="ignore"):
            sane = ok & (np.abs(xi) <= INT_LIMIT) & (np.abs(xr) <= INT_LIMIT) & (np.abs(xc) <= INT_LIMIT)
        # converged: contrast and edge tests
        t = (dx * xc + dy * xr) + ds * xi
        contr = v * IMG_SCALE + t * F(0.5)
        tr = dxx + dyy
        det2 = dxx * dyy - dxy * dxy
        good = done & ~(np.abs(contr) * F(N_LAYERS) < F(0.04)) & ~((det2 <= 0) | ((tr * tr) * F(10) >= F(121) * det2))
        keep[a[good]] = True
        off[a[good]] = np.stack([xi, xr, xc, contr], 1)[good]
        active[a[done | ~sane]] = False
        mv = ~done & sane
        am = a[mv]
        c[am] += np.rint(xc[mv]).astype(np.int64)
        r[am] += np.rint(xr[mv]).astype(np.int64)
        l[am] += np.rint(xi[mv]).astype(np.int64)
        inside = (l[am] >= 1) & (l[am] <= N_LAYERS) & (c[am] >= BORDER) & (c[am] < W - BORDER) & (r[am] >= BORDER) & (r[am] < H - BORDER)
        active[am[~inside]] = False
    k = np.nonzero(keep)[0]
    return np.stack([l[k], r[k], c[k]], 1), off[k]


def pack_octave(o, layer, xi):
    p = o + (layer << 8) + (int(np.rint((F(xi) + F(0.5)) * F(255))) << 16)
    return (p & ~255) | ((p - 1) & 255)


def unpack_octave(p):
    """-> (octave index 0.., layer)"""
    p = np.asarray(p).astype(np.int64)
    return ((p & 255) + 1) & 255, (p >> 8) & 255


def detect_candidates(img):
    """The bit-exact stages: -> dict(gauss, dog, cand) with cand = list of (o, layer, r, c, xi, xr, xc, contrast) that survive refinement"""
    gauss, dog = pyramid(img)
    cand = []
    for o in range(len(dog)):
        D = np.stack(dog[o])
        pos, off = _refine(D, _extrema(D))
        for (l, r, c), (xi, xr, xc, contr) in zip(pos, off):
            cand.append((o, int(l), int(r), int(c), F(xi), F(xr), F(xc), F(contr)))
    return dict(gauss=gauss, dog=dog, cand=cand)


def candidate_record(o, l, r, c, xi, xr, xc, contr):
    """(x, y, size, response, octave) of a refined candidate"""
    x = ((F(c) + xc) * F(2 ** o)) * F(0.5)
    y = ((F(r) + xr) * F(2 ** o)) * F(0.5)
    size = F(1.6 * 2.0 ** ((float(l) + float(xi)) / 3.0) * 2.0 ** o)
    return x, y, size, np.abs(contr), pack_octave(o, l, xi)


def _scl(l, xi, T):
    return T(1.6) * np.exp2((T(l) + T(xi)) / T(3))


def orientations(G, l, r, c, xi, T=F):
    """angles (degrees, float32) of the histogram peaks at (r, c) of Gaussian level G, ascending bin"""
    H, W = G.shape
    scl = _scl(l, xi, T)
    radius = int(np.rint(T(4.5) * scl))
    sigma = T(1.5) * scl
    escale = T(-1) / (T(2) * sigma * sigma)
    ii, jj = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    y, x = (r + ii).ravel(), (c + jj).ravel()
    ok = (y > 0) & (y < H - 1) & (x > 0) & (x < W - 1)
    y, x, ii, jj = y[ok], x[ok], ii.ravel()[ok], jj.ravel()[ok]
    GT = G if T is F else G.astype(T)
    dx = GT[y, x + 1] - GT[y, x - 1]
    dy = GT[y - 1, x] - GT[y + 1, x]
    w = np.exp((ii * ii + jj * jj).astype(T) * escale)
    ang = np.arctan2(dy, dx) * T(180.0 / math.pi)
    ang = np.where(ang < 0, ang + T(360), ang)
    mag = np.sqrt(dx * dx + dy * dy)
    b = np.rint(T(0.1) * ang).astype(np.int64)
    b = np.where(b >= 36, b - 36, b)
    b = np.where(b < 0, b + 36, b)
    t = np.zeros(36, T)
    np.add.at(t, b, w * mag)
    h = (np.roll(t, 2) + np.roll(t, -2)) * T(1.0 / 16) + (np.roll(t, 1) + np.roll(t, -1)) * T(4.0 / 16) + t * T(6.0 / 16)
    thr = h.max() * T(0.8)
    out = []
    for j in range(36):
        hl, hr = h[j - 1], h[(j + 1) % 36]
        if h[j] > hl and h[j] > hr and h[j] >= thr:
            b = T(j) + T(0.5) * (hl - hr) / (hl - T(2) * h[j] + hr)
            b = T(36) + b if b < 0 else (b - T(36) if b >= 36 else b)
            a = T(360) - T(10) * b
            if abs(a - T(360)) < FLT_EPSILON:
                a = T(0)
            out.append(F(a))
    return out


def descriptor(G, l, ptx, pty, xi, angle, T=F):
    """128 integers (float32) for a keypoint at (ptx, pty) (float32 level coordinates) of Gaussian level G with `angle` (degrees, float32)"""
    H, W = G.shape
    d, n = 4, 8
    ori = T(360) - T(angle)
    if abs(ori - T(360)) < FLT_EPSILON:
        ori = T(0)
    px, py = int(np.rint(F(ptx))), int(np.rint(F(pty)))
    scl = _scl(l, xi, T)
    cos_t, sin_t = np.cos(ori * T(math.pi / 180)), np.sin(ori * T(math.pi / 180))
    hist_width = T(3) * scl
    radius = int(np.rint(hist_width * T(1.4142135623730951) * T(d + 1) * T(0.5)))
    radius = min(radius, int(math.sqrt(float(W) * W + float(H) * H)))
    cos_t, sin_t = cos_t / hist_width, sin_t / hist_width
    ii, jj = np.mgrid[-radius:radius + 1, -radius:radius + 1]
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
    nrm = T(512) / max(np.sqrt(np.sum(dst * dst, dtype=T)), T(FLT_EPSILON))
    return np.clip(np.rint(dst * nrm), 0, 255).astype(F)


def sort_unique(kp):
    """indices of the records that stay, in output order"""
    order = np.lexsort((kp["octave"], kp["response"], kp["angle"], kp["size"], kp["y"], kp["x"]))
    keep = []
    for i in order:
        if keep:
            a, b = kp[keep[-1]], kp[i]
            if a["x"] == b["x"] and a["y"] == b["y"] and a["size"] == b["size"] and a["angle"] == b["angle"]:
                continue
        keep.append(i)
    return np.array(keep, np.int64)


def describe(stage, dtype=F):
    """The stages that are not bit-exact, on detect_candidates' output: -> dict(kp [n] KP_DTYPE, desc [n, 128] float32), sorted, duplicate-free"""
    T = np.float64 if dtype in (np.float64, "float64") else F
    recs, src = [], []
    for k, (o, l, r, c, xi, xr, xc, contr) in enumerate(stage["cand"]):
        x, y, size, resp, octv = candidate_record(o, l, r, c, xi, xr, xc, contr)
        for a in orientations(stage["gauss"][o][l], l, r, c, xi, T):
            recs.append((x, y, size, a, resp, octv))
            src.append(k)
    kp = np.array(recs, KP_DTYPE) if recs else np.zeros(0, KP_DTYPE)
    keep = sort_unique(kp)
    kp = kp[keep]
    desc = np.zeros((len(kp), 128), F)
    for i, k in enumerate(np.array(src, np.int64)[keep]):
        o, l, r, c, xi, xr, xc, _ = stage["cand"][k]
        desc[i] = descriptor(stage["gauss"][o][l], l, F(c) + xc, F(r) + xr, xi, kp["angle"][i], T)
    return dict(kp=kp, desc=desc)


def detect(img, dtype=F):
    img = np.ascontiguousarray(img, np.uint8)
    if min(img.shape) < MIN_SIDE:
        raise ValueError("image below the minimum size")
    return describe(detect_candidates(img), dtype)


def keys(kp, angle_bin=True):
    """(octave index, layer, integer row, integer column[, orientation bin of 10 degrees]) of every record"""
    o, l = unpack_octave(kp["octave"])
    s = np.exp2(o.astype(np.float64))
    c = np.rint(kp["x"].astype(np.float64) * 2 / s).astype(np.int64)
    r = np.rint(kp["y"].astype(np.float64) * 2 / s).astype(np.int64)
    cols = [o, l, r, c]
    if angle_bin:
        cols.append(np.floor(kp["angle"].astype(np.float64) / 10).astype(np.int64) % 36)
    return [tuple(int(v) for v in row) for row in zip(*cols)]
