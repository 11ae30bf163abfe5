"""Numpy restatement of the AKAZE keypoint detector as csrc/akaze.hip.h builds it: cv::AKAZE::create()->detect(img), i.e. threshold
0.001 (floor min_dthreshold 1e-5), 4 octaves, 4 sublevels, diffusivity PM_G2, soffset 1.6, derivative_factor 1.5, contrast percentile
0.7 over 300 bins, MLDB descriptor with pattern size 10 (feature_detection_classic.cpp:26-28).  No OpenCV exists in this build to pin
it against: this file is the definition, and the kernels reproduce it bit for bit in every plane and every field.  Every rule, and
whether it is OpenCV's as far as known ("OpenCV") or a decision of this project ("ours"):

  Levels and tables
   1. OpenCV: octave o has size (int)(rows / 2^o) x (int)(cols / 2^o); octaves stop before the first o > 0 whose width is below 80 or
      whose height is below 40, and after 4.  Level (o, j), j = 0..3: esigma = 1.6f * powf(2, j / 4.f + o), sigma_size =
      cvRound(esigma * 1.5f / 2^o) (2, 3, 3, 4 on every octave), etime = 0.5f * esigma * esigma.  Transition i - 1 -> i takes
      fed_tau_by_process_time(etime_i - etime_(i-1), 1 cycle, tau_max 0.25, reordering on): n = ceil(sqrtf(3 t / tau_max + 0.25f) -
      0.5f - 1e-8f), scale = 3 t / (tau_max n (n + 1)), tau_k = scale * tau_max / 2 / cos^2(pi (2 k + 1) / (4 n + 2)), reordered
      with kappa = n / 2 over the next prime above n.  All of it in float.
   2. OpenCV: a Gaussian kernel of sigma s has size ceil(2 (1 + (s - 0.8) / 0.3)) made odd (9 for 1.6, 5 for 1); its taps are
      exp(-x^2 / (2 s^2)) normalised by their sum in DOUBLE, stored as FLOAT.
      Everything in 1 and 2 that passes through cos, exp, pow or sqrt is a TABLE: `make_tables` computes it here, spvo_akaze_tables in
      the library, and `detect(tables=...)` takes the library's, so that the planes can be compared bit for bit whatever the two
      math libraries do in the last place.
  Planes (every float operation separately rounded, in the order written; no fused multiply-add)
   3. ours: the u8 image is multiplied by the float 1.f / 255.f (OpenCV: convertTo with the double 1 / 255).
   4. ours: a blur is separable, rows then columns, each pass t = g0 * p[0], then t = t + gj * (p[-j] + p[j]) for j = 1 .. r; the
      border is reflect-101 (OpenCV 3.x's gaussian_2D_convolution; 4.x passes BORDER_REPLICATE as far as known -- the issue that
      introduced this file fixes reflect-101, which is also what every derivative below uses).  Level 0: Lt = Lsmooth = the image
      blurred with sigma 1.6.
   5. OpenCV: the contrast factor: the image blurred with sigma 1, Scharr 3 x 3 (7) of it, the magnitude sqrt(Lx^2 + Ly^2) over the
      interior (first and last row and column left out), hmax its maximum.  hmax == 0 (a flat image): k = 0.03.  Else the bin of a
      magnitude is (int)(magnitude * (299.f / hmax)) (ours: clamped to 299), nthreshold = (int)((float)(total - hist[0]) * 0.7f),
      and with nelements running over hist[1], hist[2], ... the first bin b >= 1 at which nelements >= nthreshold BEFORE hist[b] is
      added gives k = hmax * (float)b / 300.f; if no bin does, k = 0.03.  No NaN can arise: k > 0 always.
      On every new octave k is multiplied by 0.75f.
   6. OpenCV: level i > 0: Lt is the Lt of level i - 1; on a new octave it is half-sampled by cv::resize(INTER_AREA)'s arithmetic:
      ((a + b) + c) + d) * 0.25f over the 2 x 2 block (a b / c d) when the source is exactly twice the destination in both
      directions, else the general area path of brisk_detect_ref.py item 3 with a float source and no rounding at the end.
      Lsmooth = the blur of Lt with sigma 1 (taken BEFORE the diffusion steps), Lx, Ly = Scharr 3 x 3 of Lsmooth,
      Lflow = 1 / (1 + (Lx Lx + Ly Ly) / (k k)).
   7. OpenCV: Scharr 3 x 3, scale 1, reflect-101: with d(r) = p[r][c + 1] - p[r][c - 1], Lx = 10 d(r) + 3 (d(r - 1) + d(r + 1));
      with s(r) = 10 p[r][c] + 3 (p[r][c - 1] + p[r][c + 1]), Ly = s(r + 1) - s(r - 1).  ours: that order of operations.
   8. OpenCV: a diffusion step of size tau: Lt += (0.5f * tau) * S with S = ((R + L) + B) + A, where for the neighbour n to the
      right, left, below, above X = (Lflow + Lflow_n) * (Lt_n - Lt); a neighbour outside the image contributes nothing, and the four
      corner pixels do not move.  ours: a missing neighbour is the pixel itself, whose term is (2 Lflow) * 0 = +0 -- OpenCV leaves
      the term out, which differs in the sign of a zero sum at most.  All steps of a level read the level's one Lflow.
   9. OpenCV: the determinant: scaled Scharr kernels of size 3 + 2 (sigma_size - 1), i.e. three taps at 0 and +- s = sigma_size, with
      weights norm, w * norm, norm, w = 10.f / 3.f, norm = 1.f / (2.f * s * (w + 2.f)): with d(r) = p[r][c + s] - p[r][c - s],
      Dx p = wn d(r) + norm (d(r - s) + d(r + s)); with m(r) = wn p[r][c] + norm (p[r][c - s] + p[r][c + s]), Dy p = m(r + s) -
      m(r - s); reflect-101.  Lx = Dx Lsmooth, Ly = Dy Lsmooth, Lxx = Dx Lx, Lxy = Dy Lx, Lyy = Dy Ly (the second derivatives
      reflect the first-derivative PLANES at the border), Ldet = (Lxx Lyy - Lxy Lxy) * (float)(s^4).  The factor s^4 is OpenCV 4.x's
      sigma_size_quat; the issue's formula leaves it out, but without it responses fall as s^-4 and a blob's strongest level is not
      the one of its own scale.
  Keypoints
  10. OpenCV: a pixel of level i is a candidate when Ldet > threshold and Ldet >= 1e-5, it is strictly above all eight neighbours,
      and border <= row < rows - border, border <= col < cols - border with border = cvRound(10 * sqrtf(2) * sigma_size) + 1
      (29, 43, 58).  Candidates are listed level by level, in raster order.
  11. OpenCV (3.x's sequential Find_Scale_Space_Extrema; it depends on the order of 10): a list `aux` grows.  A candidate has
      size = esigma * 1.5f, ratio = 2^octave and the scaled position p = (col * ratio + h, row * ratio + h), h = 0.5f * (ratio - 1)
      (ours: in float).  It is compared with the FIRST entry of aux whose level is its own or the one below and whose scaled position
      q satisfies (col * ratio - q.x)^2 + (row * ratio - q.y)^2 <= size^2 (the candidate's position WITHOUT h, as OpenCV has it):
      if its response is larger it replaces that entry in place, else it is dropped; with no such entry it is appended.  Afterwards
      entry i is dropped when some entry j > i of the level above has (p_i - p_j)^2 <= size_i^2 and a larger response.
  12. OpenCV: refinement of a survivor on the 3 x 3 Ldet patch: Dx = 0.5 (r - l), Dy = 0.5 (d - u), Dxx = (r + l) - 2 c, Dyy = (d + u)
      - 2 c, Dxy = 0.25 (dr + ul) - 0.25 (ur + dl); the system [Dxx Dxy; Dxy Dyy] o = -[Dx Dy].  ours: Cramer's rule, det = Dxx Dyy -
      Dxy Dxy, ox = (Dy Dxy - Dx Dyy) / det, oy = (Dx Dxy - Dy Dxx) / det, and o = 0 when det == 0 (cv::solve leaves zeros).  Kept iff
      |ox| <= 1 and |oy| <= 1.  x = (col + ox) * ratio + h, y likewise (ours: float; OpenCV forms it in double).
  13. OpenCV: the record is (x, y, size = (esigma * 1.5f) * 2.f, angle = 0, response = Ldet, octave = o, class_id = level).
      angle: Do_Subpixel_Refinement sets 0 and detect() never computes the orientation (Compute_Descriptors does), so 0 and not
      cv::KeyPoint's default -1 is what detect leaves.
"""
import math

import numpy as np

from tests import brisk_detect_ref as bdr

f32, f64 = np.float32, np.float64
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
OMAX, NSUB = 4, 4
NBINS = 300
THRESHOLD = 0.001
MIN_DTHRESHOLD = f32(1e-5)


# ---------------------------------------------------------------- tables (rules 1, 2)
def octave_shapes(rows, cols):
    shapes = []
    for o in range(OMAX):
        h, w = int(rows / 2 ** o), int(cols / 2 ** o)
        if o > 0 and (w < 80 or h < 40):
            break
        shapes.append((h, w))
    return shapes


def _is_prime(n):
    return n >= 2 and all(n % d for d in range(2, int(math.isqrt(n)) + 1))


def fed_tau(t, tau_max=f32(0.25)):
    """fed_tau_by_process_time(t, 1, tau_max, reordering = true) in float -> the step sizes"""
    t = f32(t)
    root = f32(np.sqrt(f32(f32(f32(f32(3.0) * t) / tau_max) + f32(0.25))))
    n = int(math.ceil(f32(f32(root - f32(0.5)) - f32(1.0e-8))))
    if n <= 0:
        return np.zeros(0, f32)
    scale = f32(f32(f32(3.0) * t) / f32(tau_max * f32(n * (n + 1))))
    c = f32(f32(1.0) / f32(f32(4.0) * f32(n) + f32(2.0)))
    d = f32(f32(scale * tau_max) / f32(2.0))
    tauh = np.zeros(n, f32)
    for k in range(n):
        h = f32(np.cos(f32(f32(f32(np.pi) * f32(f32(2.0) * f32(k) + f32(1.0))) * c)))
        tauh[k] = f32(d / f32(h * h))
    kappa = n // 2
    prime = n + 1
    while not _is_prime(prime):
        prime += 1
    tau = np.zeros(n, f32)
    k = 0
    for l in range(n):
        while True:
            index = ((k + 1) * kappa) % prime - 1
            if index < n:
                break
            k += 1
        tau[l] = tauh[index]
        k += 1
    return tau


def gaussian_taps(sigma):
    """rule 2 -> (g0, g1 .. gr) as float32"""
    ksize = int(math.ceil(2.0 * (1.0 + (sigma - 0.8) / 0.3))) | 1
    r = ksize // 2
    x = np.arange(-r, r + 1, dtype=f64)
    t = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(f32)[r:]


def make_tables(rows, cols):
    shapes = octave_shapes(rows, cols)
    levels = []
    for o in range(len(shapes)):
        for j in range(NSUB):
            esigma = f32(f32(1.6) * f32(np.power(f32(2.0), f32(f32(j) / f32(NSUB) + f32(o)))))
            levels.append((o, esigma, int(np.rint(f32(f32(esigma * f32(1.5)) / f32(2 ** o))))))
    etime = [f32(f32(f32(0.5) * e) * e) for _, e, _ in levels]
    tau = [fed_tau(f32(etime[i] - etime[i - 1])) for i in range(1, len(levels))]
    return dict(octave=np.array([l[0] for l in levels], np.int32), esigma=np.array([l[1] for l in levels], f32),
                sigma_size=np.array([l[2] for l in levels], np.int32), nsteps=np.array([len(t) for t in tau], np.int32),
                tau=(np.concatenate(tau) if tau else np.zeros(0, f32)), g0=gaussian_taps(1.6), g1=gaussian_taps(1.0))


def level_border(sigma_size):
    return int(np.rint(f32(f32(f32(10.0) * f32(np.sqrt(f32(2.0)))) * f32(sigma_size)))) + 1


# ---------------------------------------------------------------- planes (rules 3-9)
def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def _pass(p, g, axis):
    """one pass of rule 4 along `axis`"""
    n, r = p.shape[axis], len(g) - 1
    idx = reflect101(np.arange(-r, n + r), n)
    q = np.take(p, idx, axis=axis)
    sl = lambda a: np.take(q, np.arange(a, a + n), axis=axis)
    t = g[0] * sl(r)
    for j in range(1, r + 1):
        t = t + g[j] * (sl(r - j) + sl(r + j))
    return t


def blur(p, g):
    g = g.astype(p.dtype)
    return _pass(_pass(p, g, 1), g, 0)


def _shift(p, dr, dc):
    h, w = p.shape
    return p[np.ix_(reflect101(np.arange(h) + dr, h), reflect101(np.arange(w) + dc, w))]


def scharr(p):
    """rule 7 -> Lx, Ly"""
    ft = p.dtype.type
    d = _shift(p, 0, 1) - _shift(p, 0, -1)
    lx = ft(10) * d + ft(3) * (_shift(d, -1, 0) + _shift(d, 1, 0))
    s = ft(10) * p + ft(3) * (_shift(p, 0, -1) + _shift(p, 0, 1))
    return lx, _shift(s, 1, 0) - _shift(s, -1, 0)


def contrast_factor(img01, g1):
    """rule 5: img01 is the scaled image"""
    ft = img01.dtype.type
    lx, ly = scharr(blur(img01, g1))
    lx, ly = lx[1:-1, 1:-1], ly[1:-1, 1:-1]
    mag = np.sqrt(lx * lx + ly * ly)
    hmax = mag.max() if mag.size else ft(0)
    if hmax == 0:
        return ft(0.03)
    bins = np.minimum((mag * (ft(NBINS - 1) / hmax)).astype(np.int64), NBINS - 1)
    hist = np.bincount(bins.ravel(), minlength=NBINS)
    nthreshold = int(ft(mag.size - hist[0]) * ft(0.7))
    nelements = 0
    for b in range(1, NBINS):
        if nelements >= nthreshold:
            return ft(ft(hmax * ft(b)) / ft(NBINS))
        nelements += int(hist[b])
    return ft(0.03)


def half_sample(p, dh, dw):
    """rule 6"""
    sh, sw = p.shape
    ft = p.dtype.type
    if sh == 2 * dh and sw == 2 * dw:
        return (((p[0::2, 0::2] + p[0::2, 1::2]) + p[1::2, 0::2]) + p[1::2, 1::2]) * ft(0.25)
    xi, xw, xn = bdr._tab_arrays(bdr.area_tab(sw, dw))
    yi, yw, yn = bdr._tab_arrays(bdr.area_tab(sh, dh))
    xw, yw = xw.astype(p.dtype), yw.astype(p.dtype)
    buf = np.zeros((sh, dw), p.dtype)
    for k in range(xi.shape[1]):
        live = xn > k
        buf[:, live] = buf[:, live] + p[:, xi[live, k]] * xw[live, k][None, :]
    out = np.zeros((dh, dw), p.dtype)
    for k in range(yi.shape[1]):
        live = yn > k
        term = yw[live, k][:, None] * buf[yi[live, k], :]
        out[live, :] = term if k == 0 else out[live, :] + term
    return out


def flow(lsmooth, k):
    lx, ly = scharr(lsmooth)
    ft = lsmooth.dtype.type
    return ft(1) / (ft(1) + (lx * lx + ly * ly) / ft(k * k))


def fed_step(lt, lf, tau):
    """rule 8"""
    h, w = lt.shape
    ft = lt.dtype.type
    R, L = np.minimum(np.arange(w) + 1, w - 1), np.maximum(np.arange(w) - 1, 0)
    B, A = np.minimum(np.arange(h) + 1, h - 1), np.maximum(np.arange(h) - 1, 0)
    s = (lf + lf[:, R]) * (lt[:, R] - lt)
    s = s + (lf + lf[:, L]) * (lt[:, L] - lt)
    s = s + (lf + lf[B, :]) * (lt[B, :] - lt)
    s = s + (lf + lf[A, :]) * (lt[A, :] - lt)
    step = s * ft(ft(0.5) * ft(tau))
    for r in (0, h - 1):
        for c in (0, w - 1):
            step[r, c] = 0
    return lt + step


def deriv_weights(s, ft=f32):
    w = ft(ft(10) / ft(3))
    norm = ft(ft(1) / ft(ft(ft(2) * ft(s)) * ft(w + ft(2))))
    return norm, ft(w * norm)


def _dx(p, s):
    norm, wn = deriv_weights(s, p.dtype.type)
    d = _shift(p, 0, s) - _shift(p, 0, -s)
    return wn * d + norm * (_shift(d, -s, 0) + _shift(d, s, 0))


def _dy(p, s):
    norm, wn = deriv_weights(s, p.dtype.type)
    m = wn * p + norm * (_shift(p, 0, -s) + _shift(p, 0, s))
    return _shift(m, s, 0) - _shift(m, -s, 0)


def determinant(lsmooth, s):
    """rule 9"""
    lx, ly = _dx(lsmooth, s), _dy(lsmooth, s)
    lxx, lxy, lyy = _dx(lx, s), _dy(lx, s), _dy(ly, s)
    return (lxx * lyy - lxy * lxy) * lsmooth.dtype.type(s ** 4)


def scale_space(img, tables=None, ft=f32):
    """-> (levels, k): levels[i] = dict(octave, esigma, sigma_size, Lt, Lsmooth, Lflow, Ldet), k[o] the contrast factor of octave o"""
    img = np.ascontiguousarray(img, np.uint8)
    T = tables or make_tables(*img.shape)
    shapes = octave_shapes(*img.shape)
    g0, g1 = T["g0"].astype(ft), T["g1"].astype(ft)
    img01 = img.astype(ft) * ft(ft(1) / ft(255))
    k = contrast_factor(img01, g1)
    ks = [k]
    levels = []
    t0 = 0
    for i in range(len(T["octave"])):
        o, s = int(T["octave"][i]), int(T["sigma_size"][i])
        if i == 0:
            lt = blur(img01, g0)
            lsm, lf = lt, np.zeros_like(lt)            # (level 0 has no flow: the plane reads as zeros)
        else:
            lt = levels[-1]["Lt"]
            if o > levels[-1]["octave"]:
                lt = half_sample(lt, *shapes[o])
                k = ft(k * ft(0.75))
                ks.append(k)
            lsm = blur(lt, g1)
            lf = flow(lsm, k)
            n = int(T["nsteps"][i - 1])
            for tau in T["tau"][t0:t0 + n]:
                lt = fed_step(lt, lf, tau)
            t0 += n
        levels.append(dict(octave=o, esigma=f32(T["esigma"][i]), sigma_size=s, Lt=lt, Lsmooth=lsm, Lflow=lf, Ldet=determinant(lsm, s)))
    return levels, np.array(ks, ft)


# ---------------------------------------------------------------- keypoints (rules 10-13)
def candidates(levels, threshold=THRESHOLD):
    """rules 10 and 12 -> one record array per level, in raster order: row, col, response, ox, oy, ok"""
    out = []
    for L in levels:
        d = L["Ldet"]
        ft = d.dtype.type
        h, w = d.shape
        b = level_border(L["sigma_size"])
        m = np.zeros((h, w), bool)
        if h - b > b and w - b > b:
            c = d[b:h - b, b:w - b]
            ok = (c > ft(f32(threshold))) & (c >= ft(MIN_DTHRESHOLD))
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    if dr or dc:
                        ok &= c > d[b + dr:h - b + dr, b + dc:w - b + dc]
            m[b:h - b, b:w - b] = ok
        r, c = np.nonzero(m)
        at = lambda dr, dc: d[r + dr, c + dc]
        ce = at(0, 0)
        Dx, Dy = ft(0.5) * (at(0, 1) - at(0, -1)), ft(0.5) * (at(1, 0) - at(-1, 0))
        Dxx, Dyy = (at(0, 1) + at(0, -1)) - ft(2) * ce, (at(1, 0) + at(-1, 0)) - ft(2) * ce
        Dxy = ft(0.25) * (at(1, 1) + at(-1, -1)) - ft(0.25) * (at(-1, 1) + at(1, -1))
        det = Dxx * Dyy - Dxy * Dxy
        safe = np.where(det == 0, ft(1), det)
        ox = np.where(det == 0, ft(0), (Dy * Dxy - Dx * Dyy) / safe)
        oy = np.where(det == 0, ft(0), (Dx * Dxy - Dy * Dxx) / safe)
        out.append(dict(row=r, col=c, response=ce, ox=ox, oy=oy, ok=(np.abs(ox) <= 1) & (np.abs(oy) <= 1)))
    return out


def suppress(levels, cand):
    """rule 11 -> the surviving (level, index within the level's candidates), in the list's order.  Always float32: it is the
    library's host loop."""
    n = sum(len(c["row"]) for c in cand)
    ax, ay, asz, aresp = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    alev, aidx = np.zeros(n, np.int64), np.zeros(n, np.int64)
    m = 0
    for lev, (L, C) in enumerate(zip(levels, cand)):
        ratio = f32(2 ** L["octave"])
        half = f32(f32(0.5) * f32(ratio - f32(1)))
        size = f32(L["esigma"] * f32(1.5))
        size2 = f32(size * size)
        for i in range(len(C["row"])):
            px, py, resp = f32(f32(C["col"][i]) * ratio), f32(f32(C["row"][i]) * ratio), f32(C["response"][i])
            dx, dy = px - ax[:m], py - ay[:m]
            near = ((alev[:m] == lev) | (alev[:m] == lev - 1)) & (dx * dx + dy * dy <= size2)
            slot = m
            if near.any():
                slot = int(np.argmax(near))
                if not resp > aresp[slot]:
                    continue
            else:
                m += 1
            ax[slot], ay[slot], asz[slot], aresp[slot], alev[slot], aidx[slot] = f32(px + half), f32(py + half), size, resp, lev, i
    keep = []
    for i in range(m):
        j = np.arange(i + 1, m)
        dx, dy = ax[i] - ax[j], ay[i] - ay[j]
        if not ((alev[j] == alev[i] + 1) & (dx * dx + dy * dy <= f32(asz[i] * asz[i])) & (aresp[i] < aresp[j])).any():
            keep.append((int(alev[i]), int(aidx[i])))
    return keep


def records(levels, cand, keep):
    """rules 12 and 13"""
    out = np.zeros(len(keep), KP_DTYPE)
    n = 0
    for lev, i in keep:
        L, C = levels[lev], cand[lev]
        if not C["ok"][i]:
            continue
        ratio = f32(2 ** L["octave"])
        half = f32(f32(0.5) * f32(ratio - f32(1)))
        x = f32(f32(f32(f32(C["col"][i]) + f32(C["ox"][i])) * ratio) + half)
        y = f32(f32(f32(f32(C["row"][i]) + f32(C["oy"][i])) * ratio) + half)
        out[n] = (x, y, f32(f32(L["esigma"] * f32(1.5)) * f32(2.0)), 0.0, f32(C["response"][i]), L["octave"], lev)
        n += 1
    return out[:n]


def detect(img, threshold=THRESHOLD, tables=None, ft=f32, levels=None):
    """-> KP_DTYPE records in the order rule 11 leaves them"""
    if levels is None:
        levels, _ = scale_space(img, tables, ft)
    cand = candidates(levels, threshold)
    return records(levels, cand, suppress(levels, cand))
