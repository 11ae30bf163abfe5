// akaze.hip.h -- the classic front end's AKAZE keypoint detector (cv::AKAZE::create()->detect, feature_detection_classic.cpp:26-28): the
// nonlinear scale space, the Hessian-determinant response of every level and its extrema with their sub-pixel offsets.  The definition is
// tests/akaze_ref.py (its header numbers the rules these comments cite); the kernels reproduce it bit for bit in every plane and field.
//   blur          separable Gaussian, rows then columns, through an LDS tile with a halo of the kernel's radius (rule 4); one
//                 instantiation reads u8 and scales by 1 / 255 (rule 3), one reads float
//   half / area   a new octave's Lt: the exact 2 x 2 mean, or cv::resize(INTER_AREA)'s general path with the tap runs of a shape (rule 6)
//   contrast      gradient maximum (bits of a non-negative float: an integer atomicMax), histogram (integer atomics, LDS first), and one
//                 lane that walks the histogram and writes k of every octave to device memory, where the flow kernel reads it (rule 5)
//   flow          Scharr 3 x 3 of Lsmooth and the PM_G2 conductivity in one launch; Lx and Ly are not stored (rules 6, 7)
//   FED step      one launch per step, out of place: a tile reads its neighbours' old values, so the two buffers of a level alternate (rule 8)
//   determinant   the scaled first derivatives as planes, then the second derivatives of those planes and Ldet in one launch (rule 9)
//   extrema       threshold, strict 8-neighbour maximum, border rule -> keys (level << 32 | raster index), one atomic per wave; ranked by
//                 counting (cls_rank_kernel) so that a candidate's record lands at its raster position within its level; the record
//                 carries the refinement of rule 12.  The order-dependent suppression of rule 11 runs on the host over that list.
// Every float operation is a separately rounded IEEE one in the restatement's order (mul_rn / add_rn / sub_rn, __fdiv_rn, sqrtf):
// no contraction, no fast-math.  Every index is reflected or clamped into its plane before it is used.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_mfma.hip.h"    // mul_rn, add_rn, sub_rn
#include "spvo_types.hip.h"   // AkazeLevel(s), AkazeTaps, AkazeCand, BriskAreaTap, AKAZE_*
#include "list_steps.hip.h"   // wave_append

namespace spvo {

constexpr int AKAZE_TW = 64, AKAZE_TH = 16;   // the blur's output tile

// reflect-101 as an index map: any i, any n >= 1
__device__ __forceinline__ int akaze_reflect(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  i %= p;
  if (i < 0) i += p;
  return i >= n ? p - i : i;
}

template <typename T>
__global__ __launch_bounds__(256) void akaze_blur_kernel(const T *__restrict__ src, float *__restrict__ dst, float *__restrict__ dst2, int h, int w, const AkazeTaps tp) {
  __shared__ float s_in[AKAZE_TH + 2 * AKAZE_BLUR_R][AKAZE_TW + 2 * AKAZE_BLUR_R];
  __shared__ float s_row[AKAZE_TH + 2 * AKAZE_BLUR_R][AKAZE_TW];
  const int r = tp.r, x0 = blockIdx.x * AKAZE_TW, y0 = blockIdx.y * AKAZE_TH;
  const int iw = AKAZE_TW + 2 * r, ih = AKAZE_TH + 2 * r;
  const float inv255 = __fdiv_rn(1.f, 255.f);
  for (int i = threadIdx.x; i < ih * iw; i += 256) {
    const int ty = i / iw, tx = i - ty * iw;
    const size_t at = (size_t)akaze_reflect(y0 + ty - r, h) * w + akaze_reflect(x0 + tx - r, w);
    if constexpr (sizeof(T) == 1) s_in[ty][tx] = mul_rn((float)src[at], inv255);
    else s_in[ty][tx] = src[at];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ih * AKAZE_TW; i += 256) {
    const int ty = i / AKAZE_TW, tx = i % AKAZE_TW;
    const float *p = &s_in[ty][tx + r];
    float acc = mul_rn(tp.g[0], p[0]);
    for (int j = 1; j <= r; ++j) acc = add_rn(acc, mul_rn(tp.g[j], add_rn(p[-j], p[j])));
    s_row[ty][tx] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < AKAZE_TH * AKAZE_TW; i += 256) {
    const int ty = i / AKAZE_TW, tx = i % AKAZE_TW, x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) continue;
    float acc = mul_rn(tp.g[0], s_row[ty + r][tx]);
    for (int j = 1; j <= r; ++j) acc = add_rn(acc, mul_rn(tp.g[j], add_rn(s_row[ty + r - j][tx], s_row[ty + r + j][tx])));
    dst[(size_t)y * w + x] = acc;
    if (dst2) dst2[(size_t)y * w + x] = acc;
  }
}

#define AKAZE_XY(W, H)                                                                             \
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);     \
  if (x >= (W) || y >= (H)) return

// rule 6, the exact half: the source is 2 dh x 2 dw
__global__ __launch_bounds__(256) void akaze_half_kernel(const float *__restrict__ src, float *__restrict__ dst, int sw, int dh, int dw) {
  AKAZE_XY(dw, dh);
  const float *r0 = src + (size_t)(2 * y) * sw + 2 * x, *r1 = r0 + sw;
  dst[(size_t)y * dw + x] = mul_rn(add_rn(add_rn(add_rn(r0[0], r0[1]), r1[0]), r1[1]), 0.25f);
}

// rule 6, every other ratio: brisk_area_kernel's accumulation on a float source, not rounded at the end
__global__ __launch_bounds__(256) void akaze_area_kernel(const float *__restrict__ src, float *__restrict__ dst, int sw, int dh, int dw, const BriskAreaTap *__restrict__ xtab,
                                                         const BriskAreaTap *__restrict__ ytab) {
  AKAZE_XY(dw, dh);
  const BriskAreaTap tx = xtab[x], ty = ytab[y];
  float sum = 0.f;
  for (int j = 0; j < ty.n; ++j) {
    const float *row = src + (size_t)(ty.start + j) * sw + tx.start;
    float buf = 0.f;
    for (int i = 0; i < tx.n; ++i) buf = add_rn(buf, mul_rn(row[i], tx.a[i]));
    const float term = mul_rn(ty.a[j], buf);
    sum = j == 0 ? term : add_rn(sum, term);
  }
  dst[(size_t)y * dw + x] = sum;
}

// rule 7: Scharr 3 x 3 of plane p at (y, x)
__device__ __forceinline__ void akaze_scharr(const float *__restrict__ p, int h, int w, int y, int x, float &lx, float &ly) {
  const float *rm = p + (size_t)akaze_reflect(y - 1, h) * w, *rc = p + (size_t)y * w, *rp = p + (size_t)akaze_reflect(y + 1, h) * w;
  const int xm = akaze_reflect(x - 1, w), xp = akaze_reflect(x + 1, w);
  lx = add_rn(mul_rn(10.f, sub_rn(rc[xp], rc[xm])), mul_rn(3.f, add_rn(sub_rn(rm[xp], rm[xm]), sub_rn(rp[xp], rp[xm]))));
  const float sm = add_rn(mul_rn(10.f, rm[x]), mul_rn(3.f, add_rn(rm[xm], rm[xp])));
  const float sp = add_rn(mul_rn(10.f, rp[x]), mul_rn(3.f, add_rn(rp[xm], rp[xp])));
  ly = sub_rn(sp, sm);
}

__device__ __forceinline__ float akaze_magnitude(const float *__restrict__ p, int h, int w, int y, int x) {
  float lx, ly;
  akaze_scharr(p, h, w, y, x, lx, ly);
  return sqrtf(add_rn(mul_rn(lx, lx), mul_rn(ly, ly)));   // correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt, which the Makefile passes for this unit; __fsqrt_rn is the native instruction here: 1 ulp)
}

// rule 5: the maximum gradient magnitude over the interior.  Magnitudes are non-negative, so their bit patterns order as the values do.
__global__ __launch_bounds__(256) void akaze_gradmax_kernel(const float *__restrict__ p, int h, int w, int *__restrict__ stat) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  unsigned bits = 0;
  if (x >= 1 && y >= 1 && x < w - 1 && y < h - 1) bits = __float_as_uint(akaze_magnitude(p, h, w, y, x));
  for (int o = 32; o > 0; o >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, o));
  if ((threadIdx.x & 63) == 0 && bits) atomicMax((unsigned *)stat + AKAZE_STAT_MAX, bits);
}

__global__ __launch_bounds__(256) void akaze_hist_kernel(const float *__restrict__ p, int h, int w, int *__restrict__ stat) {
  __shared__ int s_hist[AKAZE_NBINS];
  for (int i = threadIdx.x; i < AKAZE_NBINS; i += 256) s_hist[i] = 0;
  __syncthreads();
  const float hmax = __uint_as_float((unsigned)stat[AKAZE_STAT_MAX]);
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (hmax != 0.f && x >= 1 && y >= 1 && x < w - 1 && y < h - 1) {
    const float scale = __fdiv_rn((float)(AKAZE_NBINS - 1), hmax);
    atomicAdd(&s_hist[min((int)mul_rn(akaze_magnitude(p, h, w, y, x), scale), AKAZE_NBINS - 1)], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < AKAZE_NBINS; i += 256)
    if (s_hist[i]) atomicAdd(&stat[AKAZE_STAT_HIST + i], s_hist[i]);
}

// rule 5's walk over the histogram, and k of every octave (one lane: 300 bins)
__global__ void akaze_contrast_finish_kernel(int h, int w, int octaves, int *__restrict__ stat) {
  if (threadIdx.x | blockIdx.x) return;
  const float hmax = __uint_as_float((unsigned)stat[AKAZE_STAT_MAX]);
  float k = 0.03f;
  if (hmax != 0.f) {
    const int total = (h - 2) * (w - 2);
    const int nthreshold = (int)mul_rn((float)(total - stat[AKAZE_STAT_HIST]), 0.7f);
    int nelements = 0;
    for (int b = 1; b < AKAZE_NBINS; ++b) {
      if (nelements >= nthreshold) { k = __fdiv_rn(mul_rn(hmax, (float)b), (float)AKAZE_NBINS); break; }
      nelements += stat[AKAZE_STAT_HIST + b];
    }
  }
  for (int o = 0; o < octaves; ++o) {
    stat[AKAZE_STAT_K + o] = (int)__float_as_uint(k);
    k = mul_rn(k, 0.75f);
  }
}

// rules 6 and 7: Lflow = 1 / (1 + (Lx^2 + Ly^2) / k^2) with k of the level's octave from device memory
__global__ __launch_bounds__(256) void akaze_flow_kernel(const float *__restrict__ ls, float *__restrict__ lflow, int h, int w, const int *__restrict__ k_bits) {
  AKAZE_XY(w, h);
  const float k = __uint_as_float((unsigned)*k_bits);
  float lx, ly;
  akaze_scharr(ls, h, w, y, x, lx, ly);
  lflow[(size_t)y * w + x] = __fdiv_rn(1.f, add_rn(1.f, __fdiv_rn(add_rn(mul_rn(lx, lx), mul_rn(ly, ly)), mul_rn(k, k))));
}

// rule 8: one diffusion step, out of place (half_tau = 0.5f * tau)
__global__ __launch_bounds__(256) void akaze_fed_kernel(const float *__restrict__ lt, const float *__restrict__ lf, float *__restrict__ out, int h, int w, float half_tau) {
  AKAZE_XY(w, h);
  const size_t row = (size_t)y * w, rb = (size_t)min(y + 1, h - 1) * w, ra = (size_t)max(y - 1, 0) * w;
  const int xr = min(x + 1, w - 1), xl = max(x - 1, 0);
  const float c = lt[row + x], f = lf[row + x];
  const float tr = mul_rn(add_rn(f, lf[row + xr]), sub_rn(lt[row + xr], c));
  const float tl = mul_rn(add_rn(f, lf[row + xl]), sub_rn(lt[row + xl], c));
  const float tb = mul_rn(add_rn(f, lf[rb + x]), sub_rn(lt[rb + x], c));
  const float ta = mul_rn(add_rn(f, lf[ra + x]), sub_rn(lt[ra + x], c));
  float step = mul_rn(add_rn(add_rn(add_rn(tr, tl), tb), ta), half_tau);
  if ((x == 0 || x == w - 1) && (y == 0 || y == h - 1)) step = 0.f;
  out[row + x] = add_rn(c, step);
}

// rule 9: the scaled Scharr derivatives of plane p at (y, x), taps at 0 and +- s
__device__ __forceinline__ float akaze_dx(const float *__restrict__ p, int h, int w, int y, int x, int s, float norm, float wn) {
  const float *rm = p + (size_t)akaze_reflect(y - s, h) * w, *rc = p + (size_t)y * w, *rp = p + (size_t)akaze_reflect(y + s, h) * w;
  const int xm = akaze_reflect(x - s, w), xp = akaze_reflect(x + s, w);
  return add_rn(mul_rn(wn, sub_rn(rc[xp], rc[xm])), mul_rn(norm, add_rn(sub_rn(rm[xp], rm[xm]), sub_rn(rp[xp], rp[xm]))));
}
__device__ __forceinline__ float akaze_dy(const float *__restrict__ p, int h, int w, int y, int x, int s, float norm, float wn) {
  const float *rm = p + (size_t)akaze_reflect(y - s, h) * w, *rp = p + (size_t)akaze_reflect(y + s, h) * w;
  const int xm = akaze_reflect(x - s, w), xp = akaze_reflect(x + s, w);
  const float mm = add_rn(mul_rn(wn, rm[x]), mul_rn(norm, add_rn(rm[xm], rm[xp])));
  const float mp = add_rn(mul_rn(wn, rp[x]), mul_rn(norm, add_rn(rp[xm], rp[xp])));
  return sub_rn(mp, mm);
}

__global__ __launch_bounds__(256) void akaze_deriv_kernel(const float *__restrict__ ls, float *__restrict__ lx, float *__restrict__ ly, int h, int w, int s, float norm, float wn) {
  AKAZE_XY(w, h);
  lx[(size_t)y * w + x] = akaze_dx(ls, h, w, y, x, s, norm, wn);
  ly[(size_t)y * w + x] = akaze_dy(ls, h, w, y, x, s, norm, wn);
}

__global__ __launch_bounds__(256) void akaze_det_kernel(const float *__restrict__ lx, const float *__restrict__ ly, float *__restrict__ ldet, int h, int w, int s, float norm, float wn,
                                                        float quat) {
  AKAZE_XY(w, h);
  const float lxx = akaze_dx(lx, h, w, y, x, s, norm, wn), lxy = akaze_dy(lx, h, w, y, x, s, norm, wn), lyy = akaze_dy(ly, h, w, y, x, s, norm, wn);
  ldet[(size_t)y * w + x] = mul_rn(sub_rn(mul_rn(lxx, lyy), mul_rn(lxy, lxy)), quat);
}

// rule 10: the candidates of the levels first_level + blockIdx.z (the levels of one octave: one grid size) as keys, one atomic per wave.
// border >= 1, so the eight neighbours are inside.
__global__ __launch_bounds__(256) void akaze_extrema_kernel(const AkazeLevels lv, int first_level, float threshold, float floor_threshold, unsigned long long *__restrict__ keys, int cap,
                                                            int *__restrict__ stat) {
  const int level = first_level + (int)blockIdx.z;
  const AkazeLevel L = lv.l[level];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (y >= L.h) return;   // (whole waves: a wave is 64 consecutive x of one row)
  bool keep = x >= L.border && x < L.w - L.border && y >= L.border && y < L.h - L.border;
  if (keep) {
    const float *p = L.Ldet + (size_t)y * L.w + x;
    const float v = p[0];
    const int w = L.w;
    keep = v > threshold && v >= floor_threshold && v > p[-1] && v > p[1] && v > p[-w - 1] && v > p[-w] && v > p[-w + 1] && v > p[w - 1] && v > p[w] && v > p[w + 1];
  }
  const int slot = wave_append(keep, &stat[AKAZE_STAT_NCAND]);
  if (!keep) return;
  if (slot >= cap) { stat[AKAZE_STAT_OVERFLOW] = 1; return; }
  keys[slot] = ((unsigned long long)level << 32) | (unsigned)(y * L.w + x);
}

// rules 12 and 13: a candidate's record at its rank (rank is left zero for the next call)
__global__ __launch_bounds__(256) void akaze_refine_kernel(const AkazeLevels lv, const unsigned long long *__restrict__ keys, int *__restrict__ rank, int cap, const int *__restrict__ stat,
                                                           AkazeCand *__restrict__ rec) {
  const int n = min(stat[AKAZE_STAT_NCAND], cap);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned long long key = keys[i];
    const int r = rank[i], level = (int)(key >> 32), at = (int)(key & 0xFFFFFFFFu);
    rank[i] = 0;
    if (r < 0 || r >= n || level >= lv.n) continue;   // (cannot happen: keys are unique)
    const AkazeLevel L = lv.l[level];
    const int w = L.w, row = at / w, col = at - row * w;
    const float *p = L.Ldet + at;
    const float c = p[0];
    const float Dx = mul_rn(0.5f, sub_rn(p[1], p[-1])), Dy = mul_rn(0.5f, sub_rn(p[w], p[-w]));
    const float Dxx = sub_rn(add_rn(p[1], p[-1]), mul_rn(2.f, c)), Dyy = sub_rn(add_rn(p[w], p[-w]), mul_rn(2.f, c));
    const float Dxy = sub_rn(mul_rn(0.25f, add_rn(p[w + 1], p[-w - 1])), mul_rn(0.25f, add_rn(p[-w + 1], p[w - 1])));
    const float det = sub_rn(mul_rn(Dxx, Dyy), mul_rn(Dxy, Dxy));
    float ox = 0.f, oy = 0.f;
    if (det != 0.f) {
      ox = __fdiv_rn(sub_rn(mul_rn(Dy, Dxy), mul_rn(Dx, Dyy)), det);
      oy = __fdiv_rn(sub_rn(mul_rn(Dx, Dxy), mul_rn(Dy, Dxx)), det);
    }
    const float ratio = (float)(1 << L.octave), half = mul_rn(0.5f, sub_rn(ratio, 1.f));
    AkazeCand k;
    k.x = add_rn(mul_rn(add_rn((float)col, ox), ratio), half);
    k.y = add_rn(mul_rn(add_rn((float)row, oy), ratio), half);
    k.size = mul_rn(mul_rn(L.esigma, 1.5f), 2.f);
    k.angle = 0.f;
    k.response = c;
    k.octave = L.octave;
    k.class_id = level;
    k.row = row;
    k.col = col;
    k.ok = fabsf(ox) <= 1.f && fabsf(oy) <= 1.f;
    rec[r] = k;
  }
}

#undef AKAZE_XY

}  // namespace spvo
