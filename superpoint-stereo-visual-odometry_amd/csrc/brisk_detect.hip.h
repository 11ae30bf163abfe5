// brisk_detect.hip.h -- the classic front end's BRISK keypoint detector on the GPU (ClassicFeatureFrontEnd with DetectorType::BRISK,
// feature_detection_classic.cpp:9-11: cv::BRISK::create() -> detect(): threshold 30, 3 octaves, pattern scale 1, i.e. BriskScaleSpace with
// six layers).  The reference obtains it from OpenCV, which does not exist in this build: what is built here is OpenCV 4.x's algorithm as
// far as it is known, restated once on the CPU (tests/brisk_detect_ref.py: its header lists every choice, numbered) and reproduced by
// these kernels bit for bit in every field of every keypoint.  The stages, one launch each for ALL six layers where the data allow it
// (layer in blockIdx.z, as orb.hip.h: the chain is launch-bound):
//   pyramid     layer 1 = two-thirds of layer 0, layer i >= 2 = half of layer i - 2: brisk_half_kernel where the source is exactly twice
//               the destination (integers), brisk_area_kernel for every other ratio (cv::resize(INTER_AREA)'s float taps from tables).
//               A layer depends on the layer two below: three launches (layer 1; layers 2, 3; layers 4, 5).
//   scores      the dense, threshold-independent AGAST 9-16 score of every layer (fast916_arc_score at threshold 0, less one: choice 4)
//               and the 5-8 score of layer 0 (the virtual layer below it)
//   candidates  score >= threshold and isMax2D, one atomic per wave; keys (layer, raster index) ordered by cls_rank_kernel, so the
//               output order does not depend on the order of the atomics
//   refinement  ONE CANDIDATE PER LANE: the windows searched in the layers above and below hold at most 4 x 4 positions of 4 bytes each
//               (choice 10) and the search is sequential by nature (running maximum, tie rule in raster order): there is nothing for a
//               wave to share.  refine3D / the top layer's path -> a record and a keep flag at the candidate's rank
//   compaction  order-preserving, one workgroup (list_steps.hip.h's walk)
// Integer stages are exact by nature; every float operation is a separately rounded IEEE one in the restatement's order (mul_rn /
// add_rn / __fdiv_rn, the three double steps of choice 10 with __dmul_rn / __dadd_rn / __ddiv_rn): no contraction, no fast-math.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_mfma.hip.h"    // mul_rn, add_rn
#include "spvo_types.hip.h"   // fast916_arc_score, BriskDetLayers, BriskDetKeypoint
#include "list_steps.hip.h"   // wave_append, stable_compact_walk

namespace spvo {

// (BriskDetLayer, BriskDetLayers, BriskAreaTap, BriskDetKeypoint, BRISK_DET_*: spvo_types.hip.h)

// exact 2:1 in both directions: (a + b + c + d + 2) >> 2.  blockIdx.z picks one of up to two (source, destination) pairs
__global__ __launch_bounds__(256) void brisk_half_kernel(const BriskResizeJobs jobs) {
  const BriskResizeJob J = jobs.j[blockIdx.z];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (J.xtab || x >= J.dw || y >= J.dh) return;
  const uint8_t *r0 = J.src + (size_t)(2 * y) * J.sw + 2 * x, *r1 = r0 + J.sw;
  J.dst[(size_t)y * J.dw + x] = (uint8_t)(((int)r0[0] + (int)r0[1] + (int)r1[0] + (int)r1[1] + 2) >> 2);
}

// every other ratio (two-thirds always; a half whose source size is odd): cv::resize(INTER_AREA)'s general path, choice 3.  Per
// destination column / row a run of at most BRISK_DET_TAPS consecutive sources with float weights (built on the host in double).
__global__ __launch_bounds__(256) void brisk_area_kernel(const BriskResizeJobs jobs) {
  const BriskResizeJob J = jobs.j[blockIdx.z];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (!J.xtab || x >= J.dw || y >= J.dh) return;
  const BriskAreaTap tx = J.xtab[x], ty = J.ytab[y];
  float sum = 0.f;
  for (int j = 0; j < ty.n; ++j) {
    const uint8_t *row = J.src + (size_t)(ty.start + j) * J.sw + tx.start;
    float buf = 0.f;
    for (int i = 0; i < tx.n; ++i) buf = add_rn(buf, mul_rn((float)row[i], tx.a[i]));
    const float term = mul_rn(ty.a[j], buf);
    sum = j == 0 ? term : add_rn(sum, term);
  }
  J.dst[(size_t)y * J.dw + x] = (uint8_t)min(max((int)rintf(sum), 0), 255);   // ties to even, as cvRound
}

// choice 4: s = M - 1 with M = fast916_arc_score at threshold 0; 0 outside the 3-pixel interior
__global__ __launch_bounds__(256) void brisk_score916_kernel(const BriskDetLayers lv) {
  const BriskDetLayer L = lv.l[blockIdx.z];
  const int h = L.h, w = L.w;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  int s = 0;
  if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) s = max(fast916_arc_score(L.im + (size_t)y * w + x, w, 0) - 1, 0);
  L.score[(size_t)y * w + x] = (uint8_t)s;
}

// choice 5: the 5-8 score of layer 0 -- five contiguous pixels of the ring of radius 1 -- 0 within 2 pixels of the border
__global__ __launch_bounds__(256) void brisk_score58_kernel(const BriskDetLayers lv) {
  const BriskDetLayer L = lv.l[0];
  const int h = L.h, w = L.w;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  int best = 0;
  if (x >= 2 && x < w - 2 && y >= 2 && y < h - 2) {
    const uint8_t *p = L.im + (size_t)y * w + x;
    const int c = *p;
    const int off[8] = {-w, -w + 1, 1, w + 1, w, w - 1, -1, -w - 1};
    int d[12];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = (int)p[off[i]] - c;
#pragma unroll
    for (int i = 8; i < 12; ++i) d[i] = d[i - 8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      int mn = 255, mx = -255;
#pragma unroll
      for (int k = 0; k < 5; ++k) { mn = min(mn, d[s + k]); mx = max(mx, d[s + k]); }
      best = max(best, max(mn, -mx));
    }
    best = max(best - 1, 0);
  }
  lv.score58[(size_t)y * w + x] = (uint8_t)best;
}

// choice 7: candidates (score >= threshold, isMax2D on the thresholded map) -> keys (layer << 32 | raster index), one atomic per wave.
// A candidate lies in the 3-pixel interior (the map is 0 outside it), so the 5 x 5 pixels isMax2D may touch are inside the layer.
__global__ __launch_bounds__(256) void brisk_collect_kernel(const BriskDetLayers lv, int thr, unsigned long long *__restrict__ keys, int cap, int *__restrict__ counters) {
  const BriskDetLayer L = lv.l[blockIdx.z];
  const int h = L.h, w = L.w;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (y >= h) return;   // (whole waves: a wave is 64 consecutive x of one row)
  const uint8_t *score = L.score;
  const int c = x < w ? score[(size_t)y * w + x] : 0;
  bool keep = c >= thr;
  if (keep) {
    auto at = [&](int dx, int dy) { const int v = score[(size_t)(y + dy) * w + x + dx]; return v >= thr ? v : 0; };
    int sc = 4 * c;
    bool tie[9];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (!(dy | dx)) { tie[4] = false; continue; }
        const int v = at(dx, dy);
        if (v > c) keep = false;
        tie[(dy + 1) * 3 + dx + 1] = v == c;
        sc += ((dy == 0 || dx == 0) ? 2 : 1) * v;
      }
    if (keep) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        if (!tie[k]) continue;
        const int ox = k % 3 - 1, oy = k / 3 - 1;
        int so = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) so += ((dy == 0 ? 2 : 1) * (dx == 0 ? 2 : 1)) * at(ox + dx, oy + dy);
        if (so > sc) keep = false;
      }
    }
  }
  const int slot = wave_append(keep, &counters[1]);
  if (!keep) return;
  if (slot < cap) keys[slot] = ((unsigned long long)blockIdx.z << 32) | (unsigned)(y * w + x);
  else counters[3] = 1;
}

// ---- refinement: the device forms of the restatement's functions (same names)
__device__ __forceinline__ int bd_read(const BriskDetLayer &L, int x, int y) {   // choice 4 at threshold 1, choice 14
  return (x < 0 || y < 0 || x >= L.w || y >= L.h) ? 0 : (int)L.score[(size_t)y * L.w + x];
}
// choice 6.  At an integer position the weights are 1, 0, 0, 0 and the value is the score itself: the interior positions of a window
// go through here too.
__device__ __forceinline__ int bd_read_f(const BriskDetLayer &L, float xf, float yf) {
  const int x = (int)xf, y = (int)yf;
  const float rx1 = add_rn(xf, -(float)x), rx = add_rn(1.f, -rx1), ry1 = add_rn(yf, -(float)y), ry = add_rn(1.f, -ry1);
  float v = mul_rn(mul_rn(rx, ry), (float)bd_read(L, x, y));
  v = add_rn(v, mul_rn(mul_rn(rx1, ry), (float)bd_read(L, x + 1, y)));
  v = add_rn(v, mul_rn(mul_rn(rx, ry1), (float)bd_read(L, x, y + 1)));
  v = add_rn(v, mul_rn(mul_rn(rx1, ry1), (float)bd_read(L, x + 1, y + 1)));
  return (int)v & 0xFF;
}

struct BdPatch { int s00, s01, s02, s10, s11, s12, s20, s21, s22; };   // s_i_j: i = column offset, j = row offset
struct BdPeak { float m, dx, dy; };

__device__ __forceinline__ BdPatch bd_patch(const BriskDetLayer &L, int x, int y) {
  return BdPatch{bd_read(L, x - 1, y - 1), bd_read(L, x - 1, y), bd_read(L, x - 1, y + 1), bd_read(L, x, y - 1), bd_read(L, x, y),
                 bd_read(L, x, y + 1),     bd_read(L, x + 1, y - 1), bd_read(L, x + 1, y), bd_read(L, x + 1, y + 1)};
}
__device__ __forceinline__ float bd_quad(int c1, int c2, int c3, int c4, int c5, int c6, float dx, float dy) {
  float v = mul_rn(mul_rn((float)c1, dx), dx);
  v = add_rn(v, mul_rn(mul_rn((float)c2, dy), dy));
  v = add_rn(v, mul_rn((float)c3, dx));
  v = add_rn(v, mul_rn((float)c4, dy));
  v = add_rn(v, mul_rn(mul_rn((float)c5, dx), dy));
  v = add_rn(v, (float)c6);
  return __fdiv_rn(v, 18.f);
}
__device__ __forceinline__ float bd_clamp1(float v) { return v > 1.f ? 1.f : (v < -1.f ? -1.f : v); }

__device__ BdPeak bd_subpixel2d(const BdPatch &p) {
  const int tmp1 = p.s00 + p.s02 - 2 * p.s11 + p.s20 + p.s22;
  const int c1 = 3 * (tmp1 + p.s01 - ((p.s10 + p.s12) * 2) + p.s21);
  const int c2 = 3 * (tmp1 - ((p.s01 + p.s21) * 2) + p.s10 + p.s12);
  const int tmp2 = p.s02 - p.s20;
  const int tmp3 = p.s00 + tmp2 - p.s22;
  const int tmp4 = tmp3 - 2 * tmp2;
  const int c3 = -3 * (tmp3 + p.s01 - p.s21);
  const int c4 = -3 * (tmp4 + p.s10 - p.s12);
  const int c5 = (p.s00 - p.s02 - p.s20 + p.s22) * 4;
  const int c6 = -(p.s00 + p.s02 - ((p.s10 + p.s01 + p.s12 + p.s21) * 2) - 5 * p.s11 + p.s20 + p.s22) * 2;
  const int hdet = 4 * c1 * c2 - c5 * c5;
  if (hdet == 0) return BdPeak{__fdiv_rn((float)c6, 18.f), 0.f, 0.f};
  if (!(hdet > 0 && c1 < 0)) {
    int tmax = c3 + c4 + c5;
    float dx = 1.f, dy = 1.f;
    int t = -c3 + c4 - c5;
    if (t > tmax) { tmax = t; dx = -1.f; dy = 1.f; }
    t = c3 - c4 - c5;
    if (t > tmax) { tmax = t; dx = 1.f; dy = -1.f; }
    t = -c3 - c4 + c5;
    if (t > tmax) { tmax = t; dx = -1.f; dy = -1.f; }
    return BdPeak{__fdiv_rn((float)(tmax + c1 + c2 + c6), 18.f), dx, dy};
  }
  const float dx = __fdiv_rn((float)(2 * c2 * c3 - c4 * c5), (float)(-hdet)), dy = __fdiv_rn((float)(2 * c1 * c4 - c3 * c5), (float)(-hdet));
  const bool tx = dx > 1.f, tx_ = !tx && dx < -1.f, ty = dy > 1.f, ty_ = dy < -1.f;
  if (tx || tx_ || ty || ty_) {
    float dx1 = 0.f, dx2 = 0.f, dy1 = 0.f, dy2 = 0.f;
    if (tx) { dx1 = 1.f; dy1 = bd_clamp1(__fdiv_rn(-(float)(c4 + c5), (float)(2 * c2))); }
    else if (tx_) { dx1 = -1.f; dy1 = bd_clamp1(__fdiv_rn(-(float)(c4 - c5), (float)(2 * c2))); }
    if (ty) { dy2 = 1.f; dx2 = bd_clamp1(__fdiv_rn(-(float)(c3 + c5), (float)(2 * c1))); }
    else if (ty_) { dy2 = -1.f; dx2 = bd_clamp1(__fdiv_rn(-(float)(c3 - c5), (float)(2 * c1))); }
    const float m1 = bd_quad(c1, c2, c3, c4, c5, c6, dx1, dy1), m2 = bd_quad(c1, c2, c3, c4, c5, c6, dx2, dy2);
    return m1 > m2 ? BdPeak{m1, dx1, dy1} : BdPeak{m2, dx2, dy2};
  }
  return BdPeak{bd_quad(c1, c2, c3, c4, c5, c6, dx, dy), dx, dy};
}

__device__ __forceinline__ int bd_i1024(float v) { return (int)__dadd_rn(__dmul_rn(1024.0, (double)v), 0.5); }

// refine1D (variant 0: even layers above 0), refine1D_1 (1: odd layers), refine1D_2 (2: layer 0) -> scale; *mx = the refined score
__device__ float bd_refine1d(int variant, float s_05, float s0, float s05, float *mx) {
  const int ca[3][3] = {{16, -24, 8}, {9, -18, 9}, {2, -4, 2}}, cb[3][3] = {{-40, 54, -14}, {-21, 36, -15}, {-5, 8, -3}}, cc[3][3] = {{24, -27, 6}, {12, -16, 6}, {3, -3, 1}};
  const float lo = variant == 0 ? 0.75f : (variant == 1 ? 0.6666666666666666f : 0.7f), hi = variant == 1 ? 1.3333333333333333f : 1.5f;
  const float div = variant == 0 ? 3072.f : (variant == 1 ? 2048.f : 1024.f);
  const int i_05 = bd_i1024(s_05), i0 = bd_i1024(s0), i05 = bd_i1024(s05);
  const int a = ca[variant][0] * i_05 + ca[variant][1] * i0 + ca[variant][2] * i05;
  if (a >= 0) {
    if (s0 >= s_05 && s0 >= s05) { *mx = s0; return 1.f; }
    if (s_05 >= s0 && s_05 >= s05) { *mx = s_05; return lo; }
    *mx = s05;
    return hi;
  }
  const int b = cb[variant][0] * i_05 + cb[variant][1] * i0 + cb[variant][2] * i05;
  float r = __fdiv_rn(-(float)b, (float)(2 * a));
  if (r < lo) r = lo;
  else if (r > hi) r = hi;
  const int c = cc[variant][0] * i_05 + cc[variant][1] * i0 + cc[variant][2] * i05;
  float m = add_rn((float)c, mul_rn(mul_rn((float)a, r), r));
  m = add_rn(m, mul_rn((float)b, r));
  *mx = __fdiv_rn(m, div);
  return r;
}

// choice 10, the window search shared by getScoreMaxAbove / getScoreMaxBelow over the window (x_1 .. x1) x (y_1 .. y1) of layer L: false if
// a value above thr lies in any row but the last.  Positions in raster order; column / row 0 is the fractional first one, the last the
// fractional last one, the integers between.
__device__ bool bd_search(const BriskDetLayer &L, float x_1, float x1, float y_1, float y1, int thr, bool ties, int *mx_out, int *max_x_out, int *max_y_out) {
  const int ix_1 = (int)x_1, ix1 = (int)x1, iy_1 = (int)y_1, iy1 = (int)y1;
  const int nx = ix1 - ix_1 + 2, ny = iy1 - iy_1 + 2;   // positions per row / column
  int mx = -1, max_x = ix_1 + 1, max_y = iy_1 + 1;
  auto ring = [&](int cx, int cy) {
    return 2 * (bd_read(L, cx - 1, cy) + bd_read(L, cx + 1, cy) + bd_read(L, cx, cy + 1) + bd_read(L, cx, cy - 1)) + bd_read(L, cx + 1, cy + 1) + bd_read(L, cx - 1, cy + 1) +
           bd_read(L, cx + 1, cy - 1) + bd_read(L, cx - 1, cy - 1);
  };
  for (int j = 0; j < ny; ++j) {
    const bool first_row = j == 0, last_row = j == ny - 1;
    const float yf = first_row ? y_1 : (last_row ? y1 : (float)(iy_1 + j));
    const int ly = first_row ? iy_1 + 1 : (last_row ? iy1 : iy_1 + j);
    for (int i = 0; i < nx; ++i) {
      const bool first_col = i == 0, last_col = i == nx - 1;
      const float xf = first_col ? x_1 : (last_col ? x1 : (float)(ix_1 + i));
      const int lx = first_col ? (first_row ? ix_1 + 1 : (int)add_rn(x_1, 1.f)) : (last_col ? ix1 : ix_1 + i);
      const int t = bd_read_f(L, xf, yf);
      if (!last_row && t > thr) return false;
      if (ties && t == mx && !first_row && !last_row && !first_col && !last_col && ring(lx, ly) > ring(max_x, max_y)) { max_x = lx; max_y = ly; }
      if (t > mx) { mx = t; max_x = lx; max_y = ly; }
    }
  }
  *mx_out = mx; *max_x_out = max_x; *max_y_out = max_y;
  return true;
}

__device__ __forceinline__ float bd_sat(float d, bool *ok) {
  if (d > 1.f) { *ok = false; return 1.f; }
  if (d < -1.f) { *ok = false; return -1.f; }
  return d;
}
__device__ __forceinline__ float bd_corner(int v, float den) { return __fdiv_rn((float)v, den); }

// getScoreMaxAbove of layer `layer` (< 5) at (x, y): false = not a maximum; else *mx, *dx, *dy
__device__ bool bd_max_above(const BriskDetLayers &lv, int layer, int x, int y, int thr, float *mx, float *dx, float *dy) {
  const BriskDetLayer &L = lv.l[layer + 1];
  const bool even = !(layer & 1);
  const int num = even ? 4 : 6, b = even ? 2 : 3;
  const float den = even ? 6.f : 8.f;
  int m, max_x, max_y;
  if (!bd_search(L, bd_corner(num * x - 1 - b, den), bd_corner(num * x - 1 + b, den), bd_corner(num * y - 1 - b, den), bd_corner(num * y - 1 + b, den), thr, false, &m, &max_x, &max_y)) return false;
  const BdPeak pk = bd_subpixel2d(bd_patch(L, max_x, max_y));
  const float real_x = add_rn((float)max_x, pk.dx), real_y = add_rn((float)max_y, pk.dy);
  float ddx, ddy;
  if (even) {
    ddx = add_rn(__fdiv_rn(add_rn(mul_rn(real_x, 6.f), 1.f), 4.f), -(float)x);
    ddy = add_rn(__fdiv_rn(add_rn(mul_rn(real_y, 6.f), 1.f), 4.f), -(float)y);
  } else {
    ddx = (float)__dadd_rn(__ddiv_rn(__dadd_rn(__dmul_rn((double)real_x, 8.0), 1.0), 6.0), -(double)x);
    ddy = (float)__dadd_rn(__ddiv_rn(__dadd_rn(__dmul_rn((double)real_y, 8.0), 1.0), 6.0), -(double)y);
  }
  bool ok = true;
  *dx = bd_sat(ddx, &ok);
  *dy = bd_sat(ddy, &ok);
  *mx = ok ? fmaxf(pk.m, (float)m) : (float)m;
  return true;
}

// getScoreMaxBelow of layer `layer` (> 0)
__device__ bool bd_max_below(const BriskDetLayers &lv, int layer, int x, int y, int thr, float *mx, float *dx, float *dy) {
  const BriskDetLayer &L = lv.l[layer - 1];
  const bool even = !(layer & 1);
  const int num = even ? 8 : 6, b = even ? 4 : 3;
  const float den = even ? 6.f : 4.f;
  int m, max_x, max_y;
  if (!bd_search(L, bd_corner(num * x + 1 - b, den), bd_corner(num * x + 1 + b, den), bd_corner(num * y + 1 - b, den), bd_corner(num * y + 1 + b, den), thr, true, &m, &max_x, &max_y)) return false;
  const BdPeak pk = bd_subpixel2d(bd_patch(L, max_x, max_y));
  const float real_x = add_rn((float)max_x, pk.dx), real_y = add_rn((float)max_y, pk.dy);
  const double mul = even ? 6.0 : 4.0, add = even ? 1.0 : -1.0, div = even ? 8.0 : 6.0;
  const float ddx = add_rn((float)__ddiv_rn(__dadd_rn(__dmul_rn((double)real_x, mul), add), div), -(float)x);
  const float ddy = add_rn((float)__ddiv_rn(__dadd_rn(__dmul_rn((double)real_y, mul), add), div), -(float)y);
  bool ok = true;
  *dx = bd_sat(ddx, &ok);
  *dy = bd_sat(ddy, &ok);
  *mx = ok ? fmaxf(pk.m, (float)m) : (float)m;
  return true;
}

__device__ __forceinline__ float bd_lerp(float r0, float r1, float d_layer, float d_other, int p) { return add_rn(add_rn(mul_rn(r0, d_layer), mul_rn(r1, d_other)), (float)p); }
__device__ __forceinline__ float bd_to_image(float v, const BriskDetLayer &L) { return add_rn(mul_rn(v, L.scale), L.offset); }

// choices 8, 9, 12: candidate i (key order = output order through `rank`) -> rec[rank], keep[rank]
__global__ __launch_bounds__(256) void brisk_refine_kernel(const BriskDetLayers lv, int thr, const unsigned long long *__restrict__ keys, int *__restrict__ rank, int cap,
                                                           const int *__restrict__ counters, BriskDetKeypoint *__restrict__ rec, int *__restrict__ keep) {
  const int n = min(counters[1], cap);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {   // (a fixed grid: the count lies on the device, as fast_write_kernel)
    const int r = rank[i];
    rank[i] = 0;
    const unsigned long long key = keys[i];
    const int layer = (int)(key >> 32), p = (int)(key & 0xFFFFFFFFull);
    const BriskDetLayer &L = lv.l[layer];
    const int y = p / L.w, x = p - y * L.w;
    const int center = bd_read(L, x, y);
    BriskDetKeypoint k;
    k.angle = -1.f;
    k.octave = layer;
    bool ok = true;
    if (layer == BRISK_DET_LAYERS - 1) {
      float mb, dxb, dyb;
      ok = bd_max_below(lv, layer, x, y, center, &mb, &dxb, &dyb);
      if (ok) {
        const BdPeak pk = bd_subpixel2d(bd_patch(L, x, y));
        k.x = bd_to_image(add_rn((float)x, pk.dx), L);
        k.y = bd_to_image(add_rn((float)y, pk.dy), L);
        k.size = mul_rn(12.f, L.scale);
        k.response = pk.m;
      }
    } else {
      float max_above, dxa, dya, max_below = 0.f, dxb = 0.f, dyb = 0.f;
      ok = bd_max_above(lv, layer, x, y, center, &max_above, &dxa, &dya);
      if (ok) {
        if (layer == 0) {
          const uint8_t *s5 = lv.score58;
          auto r5 = [&](int xx, int yy) { return (xx < 0 || yy < 0 || xx >= L.w || yy >= L.h) ? 0 : (int)s5[(size_t)yy * L.w + xx]; };
          const BdPatch p5{r5(x - 1, y - 1), r5(x - 1, y), r5(x - 1, y + 1), r5(x, y - 1), r5(x, y), r5(x, y + 1), r5(x + 1, y - 1), r5(x + 1, y), r5(x + 1, y + 1)};
          max_below = (float)max(max(max(max(p5.s00, p5.s01), max(p5.s02, p5.s10)), max(max(p5.s11, p5.s12), max(p5.s20, p5.s21))), p5.s22);
          const BdPeak pk = bd_subpixel2d(p5);
          dxb = pk.dx; dyb = pk.dy;
        } else {
          ok = bd_max_below(lv, layer, x, y, center, &max_below, &dxb, &dyb);
        }
      }
      if (ok) {
        const BdPeak pl = bd_subpixel2d(bd_patch(L, x, y));
        const float s0 = fmaxf((float)center, pl.m);
        float score, r0, r1, px, py;
        const float scale = bd_refine1d((layer & 1) ? 1 : (layer == 0 ? 2 : 0), max_below, s0, max_above, &score);
        const bool up = scale > 1.f;
        if (layer & 1) r0 = up ? add_rn(4.f, -mul_rn(scale, 3.f)) : add_rn(mul_rn(scale, 3.f), -2.f);
        else if (up) r0 = __fdiv_rn(add_rn(1.5f, -scale), 0.5f);
        else if (layer == 0) r0 = __fdiv_rn(add_rn(scale, -0.5f), 0.5f);
        else r0 = __fdiv_rn(add_rn(scale, -0.75f), 0.25f);
        r1 = add_rn(1.f, -r0);
        px = bd_lerp(r0, r1, pl.dx, up ? dxa : dxb, x);
        py = bd_lerp(r0, r1, pl.dy, up ? dya : dyb, y);
        if (up || layer != 0) { px = bd_to_image(px, L); py = bd_to_image(py, L); }
        k.x = px; k.y = py;
        k.size = mul_rn(12.f, mul_rn(scale, L.scale));
        k.response = score;
        ok = score > (float)thr;
      }
    }
    keep[r] = ok ? 1 : 0;
    if (ok) rec[r] = k;
  }
}

// the kept records, order-preserving: ONE workgroup walks the list (stable_compact_walk, list_steps.hip.h).  counters[2] = the number kept.
__global__ __launch_bounds__(1024) void brisk_det_compact_kernel(const BriskDetKeypoint *__restrict__ rec, const int *__restrict__ keep, int cap, int *__restrict__ counters,
                                                                 BriskDetKeypoint *__restrict__ out) {
  const int base = stable_compact_walk(min(counters[1], cap), [&](int i) { return keep[i] != 0; }, [&](int off, int i) { out[off] = rec[i]; });
  if (threadIdx.x == 0) counters[2] = base;
}

}  // namespace spvo
