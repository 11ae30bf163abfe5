// sift.hip.h -- the classic front end's SIFT detector + descriptor on the GPU (ClassicFeatureFrontEnd with DetectorType::SIFT /
// DescriptorType::SIFT, feature_detection_classic.cpp: cv::SIFT::create() = nfeatures 0, 3 layers per octave, contrast 0.04, edge 10,
// sigma 1.6).  The reference obtains these from OpenCV; the algorithm built here is Lowe 2004 with OpenCV 4.5.4's conventions as far as
// they are known, in exactly the form tests/sift_ref.py restates it (its header lists every choice).  Two halves:
//   bit-exact   the Gaussian pyramid, the differences of Gaussians, the 26-neighbour extrema and the sub-pixel refinement are separately
//               rounded IEEE float operations in the restatement's order (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn: never contracted)
//   not exact   the orientation histogram and the 4x4x8 descriptor use expf / atan2f / sinf / cosf and sum in another order than the
//               restatement; they are deterministic (no float atomics: a lane adds into its own LDS column, lanes that share a column
//               take turns, columns are summed in a fixed order), so one image always gives the same bytes
// Data flow per image, enqueued without a host round trip: sift_blur_kernel x (1 + 5 per octave) -> sift_extrema_kernel per octave
// (candidates appended through one counter: their order depends on scheduling and nothing downstream depends on their order) ->
// sift_refine_kernel (a thread per candidate, in place) -> sift_describe_kernel (a wave per candidate: orientation peaks, one output row
// per peak through a second counter).  The host copies the records once, builds the keypoints, sorts them by OpenCV's total order and
// drops duplicates (spvo_sift.hip): n is a few thousand.  spvo_sift_detect_pair does that on the device instead (the ordering kernels at
// the end of this file) and keeps the features in a slot.
// The extractor on GIVEN keypoints (spvo_sift_describe, tests/sift_describe_ref.py): sift_blur_kernel x 6 per octave the list names, without
// the differences (MODE 3: the base at the image's own size when no record lies on octave -1) -> sift_describe_given_kernel, a wave per
// record with the per-sample device code of sift_describe_kernel (sift_patch, sift_patch_sample, sift_share_bin, sift_desc_store) and sums
// of its own that take no turns.  The same kernel behind a Shi-Tomasi / FAST detector (spvo_classic_sift_pair): its IO parameter reads the
// detector's list where it lies and writes the rows into a SIFT slot and the host's mirrors; only the base level is built for it.
// And behind the BRISK / AKAZE detector (spvo_brisk_sift_pair, spvo_akaze_sift_pair): SiftLinkIO reads records that carry an octave
// through a byte stride and field offsets; sift_link_compact_kernel turns BRISK's keep flags into the list of indices it walks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_mfma.hip.h"    // mul_rn, add_rn, sub_rn
#include "spvo_types.hip.h"   // SiftPyr
#include "list_steps.hip.h"   // stable_compact_walk

namespace spvo {

constexpr int SIFT_LAYERS = 3, SIFT_GAUSS = SIFT_LAYERS + 3, SIFT_DOG = SIFT_LAYERS + 2, SIFT_BORDER = 5, SIFT_STEPS = 5;
constexpr int SIFT_MAX_R = 13;        // the widest blur of the default parameters (layer 5: sigma 3.09, 27 taps)
constexpr int SIFT_TW = 64, SIFT_TH = 32;   // output tile of the blur
constexpr int SIFT_COLS = 16;         // LDS columns of a histogram bin (lanes l, l + 16, l + 32, l + 48 share one and take turns)

struct SiftTaps { float t[SIFT_MAX_R + 1]; int r; };   // t[0] = centre

// (SiftPyr, SIFT_MAX_OCT: spvo_types.hip.h)

// reflect-101 as an index map that stays valid for any i (a level may be smaller than the blur radius)
__device__ __forceinline__ int sift_reflect(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  int m = i % p;
  if (m < 0) m += p;
  return m >= n ? p - m : m;
}

// 2x bilinear upsampling of the u8 image at (y, x) of the doubled grid: weights 0.25 / 0.75, indices clamped; every sum is exact
__device__ __forceinline__ float sift_upsample(const uint8_t *img, int sh, int sw, int y, int x) {
  const int ky = y >> 1, kx = x >> 1;
  const bool ey = !(y & 1), ex = !(x & 1);
  const int ay = ey ? max(ky - 1, 0) : ky, by = ey ? ky : min(ky + 1, sh - 1);
  const int ax = ex ? max(kx - 1, 0) : kx, bx = ex ? kx : min(kx + 1, sw - 1);
  const float way = ey ? 0.25f : 0.75f, wax = ex ? 0.25f : 0.75f;
  const uint8_t *ra = img + (size_t)ay * sw, *rb = img + (size_t)by * sw;
  const float ta = add_rn(mul_rn(wax, (float)ra[ax]), mul_rn(1.f - wax, (float)ra[bx]));
  const float tb = add_rn(mul_rn(wax, (float)rb[ax]), mul_rn(1.f - wax, (float)rb[bx]));
  return add_rn(mul_rn(way, ta), mul_rn(1.f - way, tb));
}

// One separable blur, rows then columns, both from LDS.  MODE 0: src is a level of the same size.  MODE 1: src is layer 3 of the octave
// below (sh x sw), read at every second pixel; the decimated image itself is stored as layer 0 (g0).  MODE 2: src is the u8 image
// (sh x sw), upsampled 2x on the fly.  MODE 3: src is the u8 image at its own size (spvo_sift_describe on a list without octave -1).  dog (may
// be NULL) receives dst - source: the difference of Gaussians this layer completes.
template <int MODE>
__global__ __launch_bounds__(256) void sift_blur_kernel(const void *__restrict__ src_, int sh, int sw, float *__restrict__ dst, float *__restrict__ dog,
                                                        float *__restrict__ g0, int h, int w, SiftTaps tp) {
  __shared__ float tile[SIFT_TH + 2 * SIFT_MAX_R][SIFT_TW + 2 * SIFT_MAX_R + 1];
  __shared__ float rowf[SIFT_TH + 2 * SIFT_MAX_R][SIFT_TW + 1];
  const int r = tp.r, tid = threadIdx.x;
  const int x0 = blockIdx.x * SIFT_TW, y0 = blockIdx.y * SIFT_TH;
  const int tw2 = SIFT_TW + 2 * r, th2 = SIFT_TH + 2 * r;
  for (int idx = tid; idx < th2 * tw2; idx += 256) {
    const int ty = idx / tw2, tx = idx - ty * tw2;
    const int gy = sift_reflect(y0 + ty - r, h), gx = sift_reflect(x0 + tx - r, w);
    float v;
    if (MODE == 0) v = static_cast<const float *>(src_)[(size_t)gy * w + gx];
    else if (MODE == 1) v = static_cast<const float *>(src_)[(size_t)(2 * gy) * sw + 2 * gx];
    else if (MODE == 2) v = sift_upsample(static_cast<const uint8_t *>(src_), sh, sw, gy, gx);
    else v = (float)static_cast<const uint8_t *>(src_)[(size_t)gy * sw + gx];
    tile[ty][tx] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < th2 * SIFT_TW; idx += 256) {
    const int ty = idx / SIFT_TW, tx = idx - ty * SIFT_TW;
    const float *p = &tile[ty][tx + r];
    float acc = mul_rn(tp.t[0], p[0]);
    for (int j = 1; j <= r; ++j) acc = add_rn(acc, mul_rn(tp.t[j], add_rn(p[-j], p[j])));
    rowf[ty][tx] = acc;
  }
  __syncthreads();
  const int tx = tid & 63, gx = x0 + tx;
  for (int ty = tid >> 6; ty < SIFT_TH; ty += 4) {
    const int gy = y0 + ty;
    if (gx >= w || gy >= h) continue;
    float acc = mul_rn(tp.t[0], rowf[ty + r][tx]);
    for (int j = 1; j <= r; ++j) acc = add_rn(acc, mul_rn(tp.t[j], add_rn(rowf[ty + r - j][tx], rowf[ty + r + j][tx])));
    const size_t o = (size_t)gy * w + gx;
    const float centre = tile[ty + r][tx + r];
    dst[o] = acc;
    if (dog) dog[o] = sub_rn(acc, centre);
    if (MODE == 1) g0[o] = centre;
  }
}

// 26-neighbour extrema of DoG layers 1..3 of one octave (blockIdx.z = layer - 1) inside the 5-pixel border; the three layers of a
// 64 x 16 tile go through LDS.  Candidates {octave, layer, row, column} are appended through counter[0] (which keeps counting beyond cap).
__global__ __launch_bounds__(256) void sift_extrema_kernel(const float *__restrict__ dog, int h, int w, int octave, int4 *__restrict__ cand, int cap,
                                                           int *__restrict__ counter) {
  constexpr int EW = 64, EH = 16;
  __shared__ float t[3][EH + 2][EW + 2 + 1];
  const int layer = blockIdx.z + 1, tid = threadIdx.x;
  const int x0 = SIFT_BORDER + blockIdx.x * EW, y0 = SIFT_BORDER + blockIdx.y * EH;
  const size_t lvl = (size_t)h * w;
  for (int idx = tid; idx < 3 * (EH + 2) * (EW + 2); idx += 256) {
    const int l = idx / ((EH + 2) * (EW + 2)), rem = idx - l * (EH + 2) * (EW + 2), ty = rem / (EW + 2), tx = rem - ty * (EW + 2);
    const int gy = min(y0 + ty - 1, h - 1), gx = min(x0 + tx - 1, w - 1);   // (>= 4: never negative)
    t[l][ty][tx] = dog[(size_t)(layer - 1 + l) * lvl + (size_t)gy * w + gx];
  }
  __syncthreads();
  const int tx = tid & 63, gx = x0 + tx;
  for (int ty = tid >> 6; ty < EH; ty += 4) {
    const int gy = y0 + ty;
    if (gx >= w - SIFT_BORDER || gy >= h - SIFT_BORDER) continue;
    const float v = t[1][ty + 1][tx + 1];
    if (!(fabsf(v) > 1.0f)) continue;   // floor(0.5 * 0.04 / 3 * 255)
    bool ge = true, le = true;
    for (int l = 0; l < 3; ++l)
      for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
          const float nb = t[l][ty + dy][tx + dx];
          ge = ge && v >= nb;
          le = le && v <= nb;
        }
    if ((v > 0 && ge) || (v < 0 && le)) {
      const int pos = atomicAdd(counter, 1);
      if (pos < cap) cand[pos] = make_int4(octave, layer, gy, gx);
    }
  }
}

// Sub-pixel refinement, contrast and edge tests of every candidate, a thread each, in place: pos becomes the position the iteration
// ended at (layer 0: rejected), off = {xi, xr, xc, contrast}.  The arithmetic is tests/sift_ref.py's _derivs / _solve / _refine.
__global__ __launch_bounds__(256) void sift_refine_kernel(SiftPyr P, int4 *__restrict__ pos, float4 *__restrict__ off, const int *__restrict__ counter, int cap) {
  const int n = min(counter[0], cap);
  const float img_scale = __fdiv_rn(1.f, 255.f), d1 = mul_rn(img_scale, 0.5f), d2 = img_scale, dc = mul_rn(img_scale, 0.25f);
  const float lim = (float)(2147483647 / 3);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    int4 p = pos[i];
    const int o = p.x, h = P.h[o], w = P.w[o];
    const size_t lvl = (size_t)h * w;
    const float *D = P.pyr + P.d_off[o];
    int layer = p.y, r = p.z, c = p.w;
    bool keep = false;
    float4 res = make_float4(0, 0, 0, 0);
    for (int step = 0; step < SIFT_STEPS; ++step) {
      const float *img = D + (size_t)layer * lvl + (size_t)r * w + c, *prv = img - lvl, *nxt = img + lvl;
      const float v = img[0];
      const float dx = mul_rn(sub_rn(img[1], img[-1]), d1), dy = mul_rn(sub_rn(img[w], img[-w]), d1), ds = mul_rn(sub_rn(nxt[0], prv[0]), d1);
      const float v2 = mul_rn(v, 2.f);
      const float dxx = mul_rn(sub_rn(add_rn(img[1], img[-1]), v2), d2);
      const float dyy = mul_rn(sub_rn(add_rn(img[w], img[-w]), v2), d2);
      const float dss = mul_rn(sub_rn(add_rn(nxt[0], prv[0]), v2), d2);
      const float dxy = mul_rn(add_rn(sub_rn(sub_rn(img[w + 1], img[w - 1]), img[-w + 1]), img[-w - 1]), dc);
      const float dxs = mul_rn(add_rn(sub_rn(sub_rn(nxt[1], nxt[-1]), prv[1]), prv[-1]), dc);
      const float dys = mul_rn(add_rn(sub_rn(sub_rn(nxt[w], nxt[-w]), prv[w]), prv[-w]), dc);
      const float c00 = sub_rn(mul_rn(dyy, dss), mul_rn(dys, dys));
      const float c01 = sub_rn(mul_rn(dxy, dss), mul_rn(dys, dxs));
      const float c02 = sub_rn(mul_rn(dxy, dys), mul_rn(dyy, dxs));
      const float det = add_rn(sub_rn(mul_rn(dxx, c00), mul_rn(dxy, c01)), mul_rn(dxs, c02));
      if (det == 0.f) break;
      const float inv = __fdiv_rn(1.f, det);
      const float m0 = sub_rn(mul_rn(dy, dss), mul_rn(dys, ds));
      const float m1 = sub_rn(mul_rn(dy, dys), mul_rn(dyy, ds));
      const float m2 = sub_rn(mul_rn(dxy, ds), mul_rn(dy, dxs));
      const float X0 = mul_rn(inv, add_rn(sub_rn(mul_rn(dx, c00), mul_rn(dxy, m0)), mul_rn(dxs, m1)));
      const float X1 = mul_rn(inv, add_rn(sub_rn(mul_rn(dxx, m0), mul_rn(dx, c01)), mul_rn(dxs, m2)));
      const float X2 = mul_rn(inv, add_rn(sub_rn(mul_rn(dxx, sub_rn(mul_rn(dyy, ds), mul_rn(dy, dys))), mul_rn(dxy, m2)), mul_rn(dx, c02)));
      const float xc = -X0, xr = -X1, xi = -X2;
      if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) {
        const float t = add_rn(add_rn(mul_rn(dx, xc), mul_rn(dy, xr)), mul_rn(ds, xi));
        const float contr = add_rn(mul_rn(v, img_scale), mul_rn(t, 0.5f));
        const float tr = add_rn(dxx, dyy), det2 = sub_rn(mul_rn(dxx, dyy), mul_rn(dxy, dxy));
        keep = !(mul_rn(fabsf(contr), (float)SIFT_LAYERS) < 0.04f) && !(det2 <= 0.f || mul_rn(mul_rn(tr, tr), 10.f) >= mul_rn(121.f, det2));
        res = make_float4(xi, xr, xc, contr);
        break;
      }
      if (!(fabsf(xi) <= lim && fabsf(xr) <= lim && fabsf(xc) <= lim)) break;
      c += __float2int_rn(xc); r += __float2int_rn(xr); layer += __float2int_rn(xi);
      if (layer < 1 || layer > SIFT_LAYERS || c < SIFT_BORDER || c >= w - SIFT_BORDER || r < SIFT_BORDER || r >= h - SIFT_BORDER) break;
    }
    pos[i] = make_int4(o, keep ? layer : 0, r, c);
    off[i] = res;
  }
}

__device__ __forceinline__ float sift_wave_sum(float v) {   // every lane gets the same sum, in a fixed order
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// ---- stage 6 of tests/sift_ref.py, the device code both describe kernels share: the frame of a patch, one sample of it, and the last
// step from the 128 sums to the stored row.  How the samples' eight contributions are ADDED is each kernel's own business.
struct SiftPatch { int px, py, radius; float ori, cos_t, sin_t; };

// the patch of a keypoint at (px, py) of an h x w level with scale scl and `angle` (degrees, cv::KeyPoint's)
__device__ __forceinline__ SiftPatch sift_patch(float scl, float angle, int px, int py, int h, int w) {
  SiftPatch t;
  float ori = 360.f - angle;
  if (fabsf(ori - 360.f) < 1.1920929e-7f) ori = 0.f;
  const float hist_width = 3.f * scl;
  int radius = (int)rintf(hist_width * 1.4142135623730951f * 5.f * 0.5f);
  radius = min(radius, (int)sqrt((double)w * w + (double)h * h));
  t.px = px; t.py = py; t.radius = radius; t.ori = ori;
  t.cos_t = cosf(ori * 0.017453292519943295f) / hist_width;
  t.sin_t = sinf(ori * 0.017453292519943295f) / hist_width;
  return t;
}

// the sample at offset (di, dj): false when it contributes nothing; else the bins (r0, c0 in -1..3, o0 in -1..7) and the eight trilinear
// shares v[e], share e for sift_share_bin(r0, c0, o0, e)
__device__ __forceinline__ bool sift_patch_sample(const float *__restrict__ G, int h, int w, const SiftPatch &t, bool in_range, int di, int dj, int &r0, int &c0, int &o0,
                                                  float (&v)[8]) {
  const int y = t.py + di, x = t.px + dj;
  const float cos_t = t.cos_t, sin_t = t.sin_t, ori = t.ori;
  const float c_rot = dj * cos_t - di * sin_t, r_rot = dj * sin_t + di * cos_t;
  float rbin = r_rot + 1.5f, cbin = c_rot + 1.5f;
  const bool ok = in_range && rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f && y > 0 && y < h - 1 && x > 0 && x < w - 1;
  r0 = 0; c0 = 0; o0 = 0;
  if (ok) {
    const float *g = G + (size_t)y * w + x;
    const float dx = g[1] - g[-1], dy = g[-w] - g[w];
    float ang = atan2f(dy, dx) * 57.29577951308232f;
    if (ang < 0.f) ang += 360.f;
    const float mag = sqrtf(dx * dx + dy * dy) * expf((c_rot * c_rot + r_rot * r_rot) * -0.125f);
    float obin = (ang - ori) * (8.f / 360.f);
    const float fr = floorf(rbin), fc = floorf(cbin), fo = floorf(obin);
    rbin -= fr; cbin -= fc; obin -= fo;
    r0 = (int)fr; c0 = (int)fc; o0 = (int)fo;
    if (o0 < 0) o0 += 8;
    if (o0 >= 8) o0 -= 8;
    // (one wrap, as the rule has it: an orientation of 361 -- angle -1 -- leaves o0 = -1 for gradient angles below one degree, see
    // sift_share_bin; an orientation outside -360 .. 720, for which the rule defines nothing, is wrapped all the way)
    if (o0 < -1 || o0 > 7) o0 &= 7;
    const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
    const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11, v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
    v[1] = v_rc00 * obin; v[0] = v_rc00 - v[1];
    v[3] = v_rc01 * obin; v[2] = v_rc01 - v[3];
    v[5] = v_rc10 * obin; v[4] = v_rc10 - v[5];
    v[7] = v_rc11 * obin; v[6] = v_rc11 - v[7];
  }
  return ok;
}

// the bin (0 .. 127) share e of a sample is added to, or -1 when it falls into the border the rule discards.  The rule's histogram is
// hist[(r + 1) * 6 + (c + 1)][o] with TEN orientation slots per cell, slots 8 and 9 folded into 0 and 1 at the end: o0 = -1 makes the
// first share of a pair land in slot 9 of the cell BEFORE (r, c) -- orientation 1 of column c - 1, or nowhere when that is the border --
// and the second in slot 0 of (r, c).  tests/sift_ref.py and OpenCV index the same way; with an orientation below 360 o0 is 0 .. 7.
__device__ __forceinline__ int sift_share_bin(int r0, int c0, int o0, int e) {
  const int rr = r0 + (e >> 2);
  int cc = c0 + ((e >> 1) & 1), oo = o0 + (e & 1);
  if (oo < 0) { cc -= 1; oo = 1; }
  else oo &= 7;
  return rr >= 0 && rr < 4 && cc >= 0 && cc < 4 ? (rr * 4 + cc) * 8 + oo : -1;
}

// bins `lane` (d0) and `lane + 64` (d1) of the 128 sums -> the row's columns `lane` and `lane + 64`: 0.2 clamp, x512, round, saturate
__device__ __forceinline__ void sift_desc_finish(float &d0, float &d1) {
  const float thr2 = sqrtf(sift_wave_sum(d0 * d0 + d1 * d1)) * 0.2f;
  d0 = fminf(d0, thr2); d1 = fminf(d1, thr2);
  const float nrm = 512.f / fmaxf(sqrtf(sift_wave_sum(d0 * d0 + d1 * d1)), 1.1920929e-7f);
  d0 = fminf(fmaxf(rintf(d0 * nrm), 0.f), 255.f);
  d1 = fminf(fmaxf(rintf(d1 * nrm), 0.f), 255.f);
}
__device__ __forceinline__ void sift_desc_store(float d0, float d1, float *__restrict__ row, int lane) {
  sift_desc_finish(d0, d1);
  row[lane] = d0;
  row[64 + lane] = d1;
}

// Orientation and descriptor of every surviving candidate: one wave (= one workgroup) per candidate, lanes over the patch.  A peak of the
// smoothed 36-bin histogram is one keypoint: row `slot` (counter[1], which keeps counting beyond kp_cap) of kp = {candidate, angle bits}
// and of desc (128 integers 0..255 as float).
// DESCRIBE = false (spvo_sift_brisk_pair: another extractor describes the keypoints): histogram, peaks and the raw rows {candidate, angle
// bits} as above -- one row per peak -- without the per-peak patch loop and the row store; `desc` is not touched.
template <bool DESCRIBE = true>
__global__ __launch_bounds__(64) void sift_describe_kernel(SiftPyr P, const int4 *__restrict__ pos, const float4 *__restrict__ off, int *__restrict__ counter, int cap,
                                                           int2 *__restrict__ kp, float *__restrict__ desc, int kp_cap) {
  __shared__ float hist[128 * SIFT_COLS];
  __shared__ float sm_t[36], sm_h[36];
  __shared__ int sm_base;
  const int n = min(counter[0], cap), lane = threadIdx.x, col = lane & (SIFT_COLS - 1), turn = lane >> 4;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int4 p = pos[i];
    if (p.y == 0) continue;   // (the same in every lane)
    const float4 f = off[i];
    const int o = p.x, layer = p.y, r = p.z, c = p.w, h = P.h[o], w = P.w[o];
    const float *G = P.pyr + P.g_off[o] + (size_t)layer * h * w;
    const float scl = 1.6f * exp2f(((float)layer + f.x) / 3.f);
    // ---- orientation histogram
    {
      const int radius = (int)rintf(4.5f * scl), side = 2 * radius + 1, total = side * side;
      const float sigma = 1.5f * scl, escale = -1.f / (2.f * sigma * sigma);
      for (int k = lane; k < 36 * SIFT_COLS; k += 64) hist[k] = 0.f;
      __syncthreads();
      for (int k0 = 0; k0 < total; k0 += 64) {
        const int k = k0 + lane, di = k / side - radius, dj = k % side - radius, y = r + di, x = c + dj;
        const bool ok = k < total && y > 0 && y < h - 1 && x > 0 && x < w - 1;
        int bin = 0;
        float val = 0.f;
        if (ok) {
          const float *q = G + (size_t)y * w + x;
          const float dx = q[1] - q[-1], dy = q[-w] - q[w];
          float ang = atan2f(dy, dx) * 57.29577951308232f;
          if (ang < 0.f) ang += 360.f;
          bin = (int)rintf(0.1f * ang);
          if (bin >= 36) bin -= 36;
          if (bin < 0) bin += 36;
          val = expf((float)(di * di + dj * dj) * escale) * sqrtf(dx * dx + dy * dy);
        }
        for (int tn = 0; tn < 4; ++tn) {
          if (ok && turn == tn) hist[bin * SIFT_COLS + col] += val;
          __syncthreads();
        }
      }
      if (lane < 36) {
        float s = 0.f;
        for (int k = 0; k < SIFT_COLS; ++k) s += hist[lane * SIFT_COLS + k];
        sm_t[lane] = s;
      }
      __syncthreads();
      if (lane < 36) {
        const float a2 = sm_t[(lane + 34) % 36], a1 = sm_t[(lane + 35) % 36], b1 = sm_t[(lane + 1) % 36], b2 = sm_t[(lane + 2) % 36];
        sm_h[lane] = (a2 + b2) * (1.f / 16.f) + (a1 + b1) * (4.f / 16.f) + sm_t[lane] * (6.f / 16.f);
      }
      __syncthreads();
    }
    float hmax = sm_h[0];
    for (int k = 1; k < 36; ++k) hmax = fmaxf(hmax, sm_h[k]);
    const float thr = hmax * 0.8f;
    bool peak = false;
    if (lane < 36) {
      const float hl = sm_h[(lane + 35) % 36], hr = sm_h[(lane + 1) % 36], hj = sm_h[lane];
      peak = hj > hl && hj > hr && hj >= thr;
    }
    unsigned long long mask = __ballot(peak);
    const int n_peaks = __popcll(mask);
    if (n_peaks == 0) continue;
    if (lane == 0) sm_base = atomicAdd(counter + 1, n_peaks);
    __syncthreads();
    const int base = sm_base;
    // ---- one descriptor per peak, ascending bin
    for (int q = 0; q < n_peaks; ++q) {
      const int j = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int slot = base + q;
      if (slot >= kp_cap) break;
      const float hl = sm_h[(j + 35) % 36], hr = sm_h[(j + 1) % 36], hj = sm_h[j];
      float b = (float)j + 0.5f * (hl - hr) / (hl - 2.f * hj + hr);
      b = b < 0.f ? 36.f + b : (b >= 36.f ? b - 36.f : b);
      float angle = 360.f - 10.f * b;
      if (fabsf(angle - 360.f) < 1.1920929e-7f) angle = 0.f;
      if constexpr (!DESCRIBE) {
        if (lane == 0) kp[slot] = make_int2(i, __float_as_int(angle));
        continue;
      }
      const int px = __float2int_rn(add_rn((float)c, f.z)), py = __float2int_rn(add_rn((float)r, f.y));
      const SiftPatch pt = sift_patch(scl, angle, px, py, h, w);
      const int radius = pt.radius, side = 2 * radius + 1, total = side * side;
      for (int k = lane; k < 128 * SIFT_COLS; k += 64) hist[k] = 0.f;
      __syncthreads();
      for (int k0 = 0; k0 < total; k0 += 64) {
        const int k = k0 + lane, di = k / side - radius, dj = k % side - radius;
        int r0, c0, o0;
        float v[8];
        const bool ok = sift_patch_sample(G, h, w, pt, k < total, di, dj, r0, c0, o0, v);
        for (int tn = 0; tn < 4; ++tn) {
          if (ok && turn == tn) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int bin = sift_share_bin(r0, c0, o0, e);
              if (bin >= 0) hist[bin * SIFT_COLS + col] += v[e];
            }
          }
          __syncthreads();
        }
      }
      float d0 = 0.f, d1 = 0.f;
      for (int k = 0; k < SIFT_COLS; ++k) { d0 += hist[lane * SIFT_COLS + k]; d1 += hist[(lane + 64) * SIFT_COLS + k]; }
      sift_desc_store(d0, d1, desc + (size_t)slot * 128, lane);
      if (lane == 0) kp[slot] = make_int2(i, __float_as_int(angle));
      __syncthreads();   // (hist is cleared for the next peak / candidate)
    }
    __syncthreads();   // (sm_base, sm_h are rewritten by the next candidate)
  }
}

// The descriptor of GIVEN keypoints (spvo_sift_describe: tests/sift_describe_ref.py): one wave (= one workgroup) per record, row i for
// record i.  The pyramid is Gaussian-only and starts at octave `first` (0 or -1): a record's level is octave o - first, layer `layer` of
// its packed field; point, scale and orientation by the restatement's choice 5 in separately rounded operations.  The patch is walked in
// tiles of 16 x 4 samples over the rows and columns that lie inside the level (a radius reaches the level's diagonal: no sample index is
// ever formed, so nothing overflows), and the samples are those of sift_patch_sample.  The sums are deterministic and take no turns:
//   FORM 0   a lane adds into a column of its own, hist[bin][lane] (128 x 64 floats = 32 KB; bank = lane: never a conflict); at the end lane b
//            sums row b and row b + 64 starting at column b (bank b + l: no conflict either), a fixed order per bin
//   FORM 1   the tile's samples are staged in LDS (bins packed in a word, eight shares), lane b owns bins b and b + 64 in registers and
//            walks the tile's valid samples in lane order, adding the share that falls into its bin (the measurement's other form)
// Where the records come from and where the rows go is the kernel's IO parameter:
//   SiftGivenIO     spvo_sift_describe: the caller's records, rows of 128 floats back to back
//   SiftDetectorIO  spvo_classic_sift_pair: the list a Shi-Tomasi / FAST detector left on the device (xy, resp, counters[2]) as records
//                   {x, y, size, -1, response, 0}, the count read here; row i goes into a SIFT slot in the L2 matcher's format (pitch 256,
//                   columns 128.. zero, the squared norm: integers <= 255, exact in any order) with its record, the same to the host's
//                   pinned mirrors (pitch 128) -- sift_gather_kernel's part for spvo_sift_detect_pair.  The slot takes min(count, slot_cap)
//                   rows; the host is told the detector's full count and its overflow flag
struct SiftGivenIO {
  const SiftKey *kp;
  int n;
  float *desc;
  __device__ __forceinline__ int begin() const { return n; }
  __device__ __forceinline__ SiftKey record(int i) const { return kp[i]; }
  __device__ __forceinline__ void store(int i, const SiftKey &, float d0, float d1, int lane) const { sift_desc_store(d0, d1, desc + (size_t)i * 128, lane); }
};
struct SiftDetectorIO {
  const float *xy, *resp;   // [n][2], [n]
  const int *counters;      // the detector's block: [2] keypoints, [3] overflow flag
  SiftKey proto;            // what every record of the list shares: size, angle, octave (kernel arguments, so that nothing of a record is a compile-time
                            // constant the optimiser could fold sift_patch's cosf / sinf with: the arithmetic stays spvo_sift_describe's)
  int slot_cap;
  float *s_desc, *s_sqn;
  SiftKey *s_rec;
  int *d_n;
  float *h_desc;
  SiftKey *h_rec;
  int *h_n;                 // {keypoints (may exceed slot_cap), overflow flag, 0}
  __device__ __forceinline__ int begin() const {   // the rows this launch describes; the counts to the slot and the host
    const int n_all = counters[2], n = min(n_all, slot_cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) { *d_n = n; h_n[0] = n_all; h_n[1] = counters[3]; h_n[2] = 0; }
    return n;
  }
  __device__ __forceinline__ SiftKey record(int i) const { return SiftKey{xy[2 * i], xy[2 * i + 1], proto.size, proto.angle, resp[i], proto.octave}; }
  __device__ __forceinline__ void store(int i, const SiftKey &k, float d0, float d1, int lane) const {
    sift_desc_finish(d0, d1);
    float *row = s_desc + (size_t)i * 256, *hrow = h_desc + (size_t)i * 128;
    row[lane] = d0; row[64 + lane] = d1; row[128 + lane] = 0.f; row[192 + lane] = 0.f;
    hrow[lane] = d0; hrow[64 + lane] = d1;
    const float sq = sift_wave_sum(d0 * d0 + d1 * d1);
    if (lane == 0) { s_sqn[i] = sq; s_rec[i] = k; h_rec[i] = k; }
  }
};
//   SiftLinkIO      spvo_brisk_sift_pair, spvo_akaze_sift_pair, spvo_sift_link_debug: the records of a detector that reports an octave,
//                   read where they lie through SiftLinkSrc's byte stride and field offsets (kernel arguments: nothing of a record is a
//                   compile-time constant, as above).  Row r describes record kept[r] (sift_link_compact_kernel's list: BRISK's keep
//                   flags, the hook's) or record r (kept = NULL: AKAZE's suppression left a compacted list); the count is read here.
//                   The sink is SiftDetectorIO's -- slot rows, squared norms, SiftKey records, the count; pinned rows and h_n = {rows in
//                   all, the detector's overflow flag, 0} -- except that the host's mirror receives the detector's OWN record, all
//                   `stride` bytes of it, unchanged (AKAZE: with class_id; its contrast factors go to h_k).  The hook has no slot and
//                   no mirror of records: s_desc, h_rec and h_n are NULL, h_desc is its device buffer
struct SiftLinkIO {
  SiftLinkSrc s;
  const int *kept, *n_kept;   // sift_link_compact_kernel's list and its length, or NULL
  int max_octave, slot_cap;   // the last octave of the pyramid the launch reads
  float *s_desc, *s_sqn;
  SiftKey *s_rec;
  int *d_n;
  float *h_desc;
  char *h_rec;                // [slot_cap][s.stride]
  int *h_n, *h_k;
  __device__ __forceinline__ int begin() const {
    const int n_all = kept ? *n_kept : min(max(*s.n_ptr, 0), s.n_cap), n = min(n_all, slot_cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (d_n) *d_n = n;
      if (h_n) {
        h_n[0] = n_all; h_n[2] = 0;
        if (s.stat) {
          h_n[1] = s.stat[AKAZE_STAT_OVERFLOW] || s.stat[AKAZE_STAT_NCAND] > s.cand_cap;
          for (int o = 0; o < AKAZE_MAX_OCTAVES; ++o) h_k[o] = s.stat[AKAZE_STAT_K + o];
        } else {
          h_n[1] = s.det_counters ? s.det_counters[3] : 0;
        }
      }
    }
    return n;
  }
  __device__ __forceinline__ const char *at(int i) const { return s.rec + (size_t)(kept ? kept[i] : i) * s.stride; }
  __device__ __forceinline__ SiftKey record(int i) const {
    const char *p = at(i);
    int oct = *reinterpret_cast<const int *>(p + s.off_octave);
    // (no detector reports another octave or a layer, and the hook refuses them: nothing may name a level that was not built)
    if ((oct & 255) > max_octave || ((oct >> 8) & 255) != 0) oct = 0;
    return SiftKey{*reinterpret_cast<const float *>(p + s.off_x),    *reinterpret_cast<const float *>(p + s.off_y),        *reinterpret_cast<const float *>(p + s.off_size),
                   *reinterpret_cast<const float *>(p + s.off_angle), *reinterpret_cast<const float *>(p + s.off_response), oct};
  }
  __device__ __forceinline__ void store(int i, const SiftKey &k, float d0, float d1, int lane) const {
    sift_desc_finish(d0, d1);
    float *hrow = h_desc + (size_t)i * 128;
    hrow[lane] = d0; hrow[64 + lane] = d1;
    if (s_desc) {
      float *row = s_desc + (size_t)i * 256;
      row[lane] = d0; row[64 + lane] = d1; row[128 + lane] = 0.f; row[192 + lane] = 0.f;
      const float sq = sift_wave_sum(d0 * d0 + d1 * d1);
      if (lane == 0) { s_sqn[i] = sq; s_rec[i] = k; }
    }
    if (h_rec && lane < (s.stride >> 2)) reinterpret_cast<int *>(h_rec + (size_t)i * s.stride)[lane] = reinterpret_cast<const int *>(at(i))[lane];
  }
};

// kept[0 .. *n_out) = the indices i < min(*n_ptr, n_cap) with keep[i] != 0 (keep = NULL: every index), ascending: ONE workgroup walks the
// list (stable_compact_walk, list_steps.hip.h, of indices)
__global__ __launch_bounds__(1024) void sift_link_compact_kernel(const int *__restrict__ keep, const int *__restrict__ n_ptr, int n_cap, int *__restrict__ kept,
                                                                 int *__restrict__ n_out) {
  const int base = stable_compact_walk(
      min(max(*n_ptr, 0), n_cap), [&](int i) { return !keep || keep[i] != 0; }, [&](int off, int i) { kept[off] = i; });   // (off <= i < n_cap)
  if (threadIdx.x == 0) *n_out = base;
}

template <int FORM, class IO>
__global__ __launch_bounds__(64) void sift_describe_given_kernel(SiftPyr P, int first, IO io) {
  constexpr int TW = 16, TH = 4;
  __shared__ float lds[FORM == 0 ? 128 * 64 : 8 * 64];
  __shared__ int code[64];
  const int lane = threadIdx.x, n = io.begin();
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const SiftKey k = io.record(i);
    int o = k.octave & 255;
    if (o >= 128) o -= 256;
    const int layer = (k.octave >> 8) & 255, lvl = o - first, h = P.h[lvl], w = P.w[lvl];
    const float scale = __int_as_float((127 - o) << 23);   // 1 / 2^o, 2^-o: exact
    const float *G = P.pyr + P.g_off[lvl] + (size_t)layer * h * w;
    const int px = __float2int_rn(mul_rn(k.x, scale)), py = __float2int_rn(mul_rn(k.y, scale));
    const float scl = mul_rn(mul_rn(k.size, scale), 0.5f);
    const SiftPatch pt = sift_patch(scl, k.angle, px, py, h, w);
    // rows and columns of the patch that hold pixels with all four neighbours (64-bit: a point may lie anywhere)
    const long long i0 = max(-(long long)pt.radius, 1ll - py), i1 = min((long long)pt.radius, (long long)h - 2 - py);
    const long long j0 = max(-(long long)pt.radius, 1ll - px), j1 = min((long long)pt.radius, (long long)w - 2 - px);
    const int ni = i0 <= i1 ? (int)(i1 - i0 + 1) : 0, nj = j0 <= j1 ? (int)(j1 - j0 + 1) : 0;   // (<= h, <= w)
    const int di0 = ni ? (int)i0 : 0, dj0 = nj ? (int)j0 : 0, ly = lane >> 4, lx = lane & 15;
    float d0 = 0.f, d1 = 0.f;
    if (FORM == 0) {
      for (int q = lane; q < 128 * 64; q += 64) lds[q] = 0.f;
      __syncthreads();
    }
    for (int ty = 0; ty < ni && nj > 0; ty += TH)
      for (int tx = 0; tx < nj; tx += TW) {
        const int a = ty + ly, b = tx + lx;
        int r0, c0, o0;
        float v[8];
        const bool ok = sift_patch_sample(G, h, w, pt, a < ni && b < nj, di0 + a, dj0 + b, r0, c0, o0, v);
        if (FORM == 0) {
          if (ok) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int bin = sift_share_bin(r0, c0, o0, e);
              if (bin >= 0) lds[bin * 64 + lane] += v[e];
            }
          }
        } else {
          unsigned long long m = __ballot(ok);
          if (m == 0) continue;   // (the same in every lane)
          code[lane] = (r0 + 1) | ((c0 + 1) << 4) | ((o0 + 1) << 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) lds[e * 64 + lane] = ok ? v[e] : 0.f;
          __syncthreads();
          while (m) {
            const int s = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int cd = code[s], sr = (cd & 15) - 1, sc = ((cd >> 4) & 15) - 1, so = (cd >> 8) - 1, O = lane & 7;
            // (sift_share_bin read backwards: which share of sample s falls into orientation O of this lane's column)
            const int dO = so >= 0 ? ((O - so) & 7) : (O == 0 ? 1 : (O == 1 ? 0 : 2)), dc = ((lane >> 3) & 3) - sc + (so < 0 && O == 1 ? 1 : 0);
            const int dr0 = (lane >> 5) - sr, dr1 = dr0 + 2;
            if ((unsigned)dc < 2u && dO < 2) {
              const int e = dc * 2 + dO;
              if ((unsigned)dr0 < 2u) d0 += lds[(dr0 * 4 + e) * 64 + s];
              if ((unsigned)dr1 < 2u) d1 += lds[(dr1 * 4 + e) * 64 + s];
            }
          }
          __syncthreads();   // (the staging is rewritten by the next tile)
        }
      }
    if (FORM == 0) {
      __syncthreads();
      for (int l = 0; l < 64; ++l) {
        const int cidx = (lane + l) & 63;
        d0 += lds[lane * 64 + cidx];
        d1 += lds[(lane + 64) * 64 + cidx];
      }
      __syncthreads();   // (the columns are cleared for the next record)
    }
    io.store(i, k, d0, d1, lane);
  }
}

// ---------------------------------------------------------------- the final ordering on the device (spvo_sift_detect_pair)
// sift_describe_kernel leaves raw rows {candidate, angle bits} + 128 floats in the order its waves happened to append them.  Four
// launches turn them into OpenCV's output order without the host -- what spvo_sift_detect's std::sort + duplicate loop do:
//   sift_key_kernel     a thread per raw row: its key (x, y, size, angle, response, octave) from the candidate, with the arithmetic of
//                       spvo_sift.hip's sift_record (separately rounded float operations; `size` through a double pow -- a SORT KEY only:
//                       rows of one candidate get one size, so ties and duplicates are those of the host's keys)
//   sift_rank_kernel    rank by counting: a tile of keys in LDS, every row counts the rows in front of it under
//                       the host comparator (float != and <, so -0 = 0); rows equal in all six fields go by raw index: a permutation
//   sift_unique_kernel  cv::KeyPointsFilter::removeDuplicatedSorted: a sorted row whose (x, y, size, angle) equal its predecessor's is
//                       dropped (equality is transitive and equal rows are adjacent: the predecessor stands for the last kept row);
//                       order-preserving, by one workgroup (stable_compact_walk, list_steps.hip.h)
//   sift_gather_kernel  a wave per final row: descriptor (pitch 256, columns 128.. zero), squared norm (an exact integer < 2^24) and source
//                       into the slot, the same to the host's pinned mirrors, the counts to both
// Every length is read from device memory and clamped to the list's capacity (the counters keep counting beyond it).
constexpr int SIFT_ORD_TILE = 1024;

__global__ __launch_bounds__(256) void sift_key_kernel(const int4 *__restrict__ pos, const float4 *__restrict__ off, const int2 *__restrict__ kp, const int *__restrict__ counter,
                                                       int kp_cap, SiftKey *__restrict__ keys) {
  const int n = min(counter[1], kp_cap);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int2 row = kp[i];
    const int4 p = pos[row.x];
    const float4 f = off[row.x];
    const int o = p.x, layer = p.y;
    const float scale = __int_as_float((127 + o) << 23);   // 2^o
    SiftKey k;
    k.x = mul_rn(mul_rn(add_rn((float)p.w, f.z), scale), 0.5f);
    k.y = mul_rn(mul_rn(add_rn((float)p.z, f.y), scale), 0.5f);
    k.size = (float)(1.6 * pow(2.0, ((double)layer + (double)f.x) / 3.0) * (double)scale);
    k.angle = __int_as_float(row.y);
    k.response = fabsf(f.w);
    const int packed = o + (layer << 8) + (__float2int_rn(mul_rn(add_rn(f.x, 0.5f), 255.f)) << 16);
    k.octave = (packed & ~255) | ((packed - 1) & 255);
    keys[i] = k;
  }
}

// (not list_steps.hip.h's rank_by_counting: the order is a six-field comparison with a tie rule, not a 64-bit key)
// sorted[rank of raw row i] = i.  A workgroup takes 256 rows and walks all keys in LDS tiles; every lane reads the same tile entry (a broadcast)
__global__ __launch_bounds__(256) void sift_rank_kernel(const SiftKey *__restrict__ keys, const int *__restrict__ n_ptr, int cap, int *__restrict__ sorted) {
  __shared__ float tx[SIFT_ORD_TILE], ty[SIFT_ORD_TILE], ts[SIFT_ORD_TILE], ta[SIFT_ORD_TILE], tr[SIFT_ORD_TILE];
  __shared__ int to[SIFT_ORD_TILE];
  const int n = min(*n_ptr, cap);
  const int nbi = (n + 255) / 256;
  for (int bi = blockIdx.x; bi < nbi; bi += gridDim.x) {
    const int i = bi * 256 + (int)threadIdx.x;
    SiftKey k = {0.f, 0.f, 0.f, 0.f, 0.f, 0};
    if (i < n) k = keys[i];
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += SIFT_ORD_TILE) {
      const int m = min(SIFT_ORD_TILE, n - j0);
      __syncthreads();   // (the previous tile has been read)
      for (int t = threadIdx.x; t < m; t += 256) {
        const SiftKey q = keys[j0 + t];
        tx[t] = q.x; ty[t] = q.y; ts[t] = q.size; ta[t] = q.angle; tr[t] = q.response; to[t] = q.octave;
      }
      __syncthreads();
      for (int t = 0; t < m; ++t) {
        const float qx = tx[t];
        bool before;
        if (qx != k.x) before = qx < k.x;
        else if (ty[t] != k.y) before = ty[t] < k.y;
        else if (ts[t] != k.size) before = ts[t] < k.size;
        else if (ta[t] != k.angle) before = ta[t] < k.angle;
        else if (tr[t] != k.response) before = tr[t] < k.response;
        else if (to[t] != k.octave) before = to[t] < k.octave;
        else before = j0 + t < i;
        cnt += before ? 1 : 0;
      }
    }
    if (i < n) sorted[cnt] = i;
  }
}

// order[0 .. *n_out) = the raw rows that stay, in output order
__global__ __launch_bounds__(1024) void sift_unique_kernel(const SiftKey *__restrict__ keys, const int *__restrict__ sorted, const int *__restrict__ n_ptr, int cap,
                                                           int *__restrict__ order, int *__restrict__ n_out) {
  int raw = 0;   // the raw row at sorted position s, from keep(s) to put(o, s)
  const int base = stable_compact_walk(
      min(*n_ptr, cap),
      [&](int s) {
        raw = sorted[s];
        if (s == 0) return true;
        const SiftKey a = keys[sorted[s - 1]], b = keys[raw];
        return !(a.x == b.x && a.y == b.y && a.size == b.size && a.angle == b.angle);
      },
      [&](int o, int) { order[o] = raw; });   // (o <= s < n)
  if (threadIdx.x == 0) *n_out = base;
}

// h_n = {rows kept (may exceed slot_cap), candidates counted, raw rows counted}; the slot holds min(kept, slot_cap) rows
__global__ __launch_bounds__(256) void sift_gather_kernel(const int *__restrict__ order, const int *__restrict__ n_kept, const int *__restrict__ counter, const int2 *__restrict__ kp,
                                                          const int4 *__restrict__ pos, const float4 *__restrict__ off, const float *__restrict__ desc, int slot_cap,
                                                          float *__restrict__ s_desc, float *__restrict__ s_sqn, SiftSrc *__restrict__ s_src, int *__restrict__ d_n,
                                                          float *__restrict__ h_desc, SiftSrc *__restrict__ h_src, int *__restrict__ h_n) {
  const int n_all = *n_kept, n = min(n_all, slot_cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) { *d_n = n; h_n[0] = n_all; h_n[1] = counter[0]; h_n[2] = counter[1]; }
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += gridDim.x * 4) {
    const int raw = order[r];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < 32) v = *reinterpret_cast<const float4 *>(desc + (size_t)raw * 128 + lane * 4);
    *reinterpret_cast<float4 *>(s_desc + (size_t)r * 256 + lane * 4) = v;
    if (lane < 32) *reinterpret_cast<float4 *>(h_desc + (size_t)r * 128 + lane * 4) = v;
    const float sq = sift_wave_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);   // integers: exact in any order
    if (lane == 0) {
      const int2 row = kp[raw];
      SiftSrc src;
      src.pos = pos[row.x]; src.off = off[row.x]; src.angle = __int_as_float(row.y);
      src.pad[0] = src.pad[1] = src.pad[2] = 0;
      s_sqn[r] = sq;
      s_src[r] = src;
      h_src[r] = src;
    }
  }
}

// spvo_sift_brisk_pair, in sift_gather_kernel's place: the ordered list in the form brisk_pair_chain_enqueue reads a detector's list (SiftKey
// is BriskDetKeypoint's layout) --
//   rec[r]  = keys[order[r]], the final row r's key: here its `size` picks the BRISK scale index and lands in the record, so the host checks it
//   keep[r] = 1
//   cnt     = a BRISK detector's counter block: [1] = the final rows (cnt[2] as well), [3] = the SIFT lists overflowed (candidates or raw rows
//             counted above list_cap: the call grows the lists and runs again)
// and to the host's pinned mirrors every final row's source with the bits of the size used in pad[0], and h_n = {final rows, candidates
// counted, raw rows counted}.  order / n_kept come from sift_unique_kernel: n <= min(raw rows, list_cap).
__global__ __launch_bounds__(256) void sift_records_kernel(const int *__restrict__ order, const int *__restrict__ n_kept, const int *__restrict__ counter, int list_cap,
                                                           const SiftKey *__restrict__ keys, const int2 *__restrict__ kp, const int4 *__restrict__ pos,
                                                           const float4 *__restrict__ off, BriskDetKeypoint *__restrict__ rec, int *__restrict__ keep, int *__restrict__ cnt,
                                                           SiftSrc *__restrict__ h_src, int *__restrict__ h_n) {
  const int n = min(max(*n_kept, 0), list_cap);
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  if (tid == 0) {
    cnt[0] = 0; cnt[1] = n; cnt[2] = n; cnt[3] = counter[0] > list_cap || counter[1] > list_cap;
    h_n[0] = n; h_n[1] = counter[0]; h_n[2] = counter[1];
  }
  for (int r = tid; r < n; r += nth) {
    const int raw = order[r];
    const SiftKey k = keys[raw];
    BriskDetKeypoint d;
    d.x = k.x; d.y = k.y; d.size = k.size; d.angle = k.angle; d.response = k.response; d.octave = k.octave;
    rec[r] = d;
    keep[r] = 1;
    const int2 row = kp[raw];
    SiftSrc src;
    src.pos = pos[row.x]; src.off = off[row.x]; src.angle = __int_as_float(row.y);
    src.pad[0] = __float_as_int(k.size); src.pad[1] = src.pad[2] = 0;
    h_src[r] = src;
  }
}

}  // namespace spvo
