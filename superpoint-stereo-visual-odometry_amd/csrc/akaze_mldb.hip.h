// akaze_mldb.hip.h -- the classic front end's AKAZE orientation and MLDB descriptor (cv::AKAZE::create()->compute,
// feature_detection_classic.cpp:69-70): Compute_Main_Orientation and the full 486-bit descriptor (pattern size 10, 3 channels, 61 bytes) on
// the scale space akaze.hip.h leaves resident (per level Lt and the scaled first derivatives Lx, Ly of rule 9).  The definition is
// tests/akaze_mldb_ref.py (its header names the rules O1 - O4, D1, D2 these comments cite); the kernel reproduces it bit for bit in every
// angle and every byte.  One launch, one wave per keypoint:
//   gather       109 weighted samples (O1) and their angle by fastAtan32f's polynomial (O2) into LDS, two samples per lane at most
//   windows      42 lanes each sum one sliding window over the samples IN ORDER k (O3); a wave reduction finds the first maximum
//   direction    (co, si) = the winning sum normalised (O4): no cos, no sin -- nothing transcendental runs anywhere in this file
//   cells        29 lanes each sum one cell of the 2 x 2, 3 x 3 and 4 x 4 grids in D1's order (k outer, l inner) -> 87 values in LDS
//   bytes        61 lanes each form one byte from the pair table (D2)
// Every float operation is a separately rounded IEEE one in the restatement's order (mul_rn / add_rn / sub_rn, __fdiv_rn, sqrtf: the unit's
// Makefile line states the correctly rounded division and square root).  A rounded coordinate is compared with the plane's bounds as a
// float and converted to an index only when it is inside, so no record, however large its size, reads outside a plane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_mfma.hip.h"    // mul_rn, add_rn, sub_rn
#include "spvo_types.hip.h"   // AkazeLevel(s), AkazeCand

namespace spvo {

constexpr int AKAZE_ORI_SAMPLES = 109, AKAZE_ORI_WINDOWS = 42, AKAZE_MLDB_CELLS = 29, AKAZE_MLDB_BITS = 486, AKAZE_MLDB_BYTES = 61;

// O1's sample order and weights, D1's cells in loop order, D2's pairs as indices into the 87 values (channel * 29 + cell)
struct AkazeMldbTab {
  signed char si[AKAZE_ORI_SAMPLES], sj[AKAZE_ORI_SAMPLES];
  float g[AKAZE_ORI_SAMPLES];
  signed char ci[AKAZE_MLDB_CELLS], cj[AKAZE_MLDB_CELLS], cstep[AKAZE_MLDB_CELLS];
  unsigned char pa[AKAZE_MLDB_BITS], pb[AKAZE_MLDB_BITS];
};

constexpr AkazeMldbTab akaze_mldb_make_tab() {
  // SURF's gauss25
  constexpr float G[7][7] = {{0.02546481f, 0.02350698f, 0.01849125f, 0.01239505f, 0.00708017f, 0.00344629f, 0.00142946f},
                             {0.02350698f, 0.02169968f, 0.01706957f, 0.01144208f, 0.00653582f, 0.00318132f, 0.00131956f},
                             {0.01849125f, 0.01706957f, 0.01342740f, 0.00900066f, 0.00514126f, 0.00250252f, 0.00103800f},
                             {0.01239505f, 0.01144208f, 0.00900066f, 0.00603332f, 0.00344629f, 0.00167749f, 0.00069579f},
                             {0.00708017f, 0.00653582f, 0.00514126f, 0.00344629f, 0.00196855f, 0.00095820f, 0.00039744f},
                             {0.00344629f, 0.00318132f, 0.00250252f, 0.00167749f, 0.00095820f, 0.00046640f, 0.00019346f},
                             {0.00142946f, 0.00131956f, 0.00103800f, 0.00069579f, 0.00039744f, 0.00019346f, 0.00008024f}};
  AkazeMldbTab t{};
  int k = 0;
  for (int i = -6; i <= 6; ++i)
    for (int j = -6; j <= 6; ++j)
      if (i * i + j * j < 36) {
        t.si[k] = (signed char)i; t.sj[k] = (signed char)j;
        t.g[k] = G[i < 0 ? -i : i][j < 0 ? -j : j];
        ++k;
      }
  const int steps[3] = {10, 7, 5};
  int cell = 0, p = 0;
  for (int g = 0; g < 3; ++g) {
    const int base = cell;
    for (int i = -10; i < 10; i += steps[g])
      for (int j = -10; j < 10; j += steps[g]) {
        t.ci[cell] = (signed char)i; t.cj[cell] = (signed char)j; t.cstep[cell] = (signed char)steps[g];
        ++cell;
      }
    const int nc = cell - base;
    for (int ch = 0; ch < 3; ++ch)
      for (int a = 0; a < nc; ++a)
        for (int b = a + 1; b < nc; ++b) {
          t.pa[p] = (unsigned char)(ch * AKAZE_MLDB_CELLS + base + a);
          t.pb[p] = (unsigned char)(ch * AKAZE_MLDB_CELLS + base + b);
          ++p;
        }
  }
  return t;
}
static __constant__ const AkazeMldbTab akaze_mldb_tab = akaze_mldb_make_tab();

// O2: fastAtan32f, degrees
__device__ __forceinline__ float akaze_fast_atan(float y, float x) {
  const float scale = (float)(180.0 / 3.14159265358979323846);
  const float p1 = mul_rn(0.9997878412794807f, scale), p3 = mul_rn(-0.3258083974640975f, scale), p5 = mul_rn(0.1555786518463281f, scale), p7 = mul_rn(-0.04432655554792128f, scale);
  const float eps = (float)2.220446049250313e-16;
  const float ax = fabsf(x), ay = fabsf(y);
  const bool first = ax >= ay;
  const float c = __fdiv_rn(first ? ay : ax, add_rn(first ? ax : ay, eps)), c2 = mul_rn(c, c);
  float a = mul_rn(add_rn(mul_rn(add_rn(mul_rn(add_rn(mul_rn(p7, c2), p5), c2), p3), c2), p1), c);
  if (!first) a = sub_rn(90.f, a);
  if (x < 0.f) a = sub_rn(180.f, a);
  if (y < 0.f) a = sub_rn(360.f, a);
  return a;
}

// the index of the rounded coordinate (yr, xr) in an h x w plane, or -1 outside (NaN included)
__device__ __forceinline__ int akaze_inside(float yr, float xr, int h, int w) {
  if (!(yr >= 0.f && yr < (float)h && xr >= 0.f && xr < (float)w)) return -1;
  return (int)yr * w + (int)xr;
}

// n_ptr == NULL: the n records of the host's list.  Otherwise the list was left on the device (spvo_akaze_detect_pair) and the first
// min(*n_ptr, n) records are described, n being what the buffers hold.
__global__ __launch_bounds__(64) void akaze_describe_kernel(const AkazeLevels lv, const AkazeKp *__restrict__ kp, int n, const int *__restrict__ n_ptr, float *__restrict__ angle,
                                                            uint8_t *__restrict__ desc) {
  if (n_ptr) n = min(n, *n_ptr);
  __shared__ float s_rx[AKAZE_ORI_SAMPLES], s_ry[AKAZE_ORI_SAMPLES], s_ang[AKAZE_ORI_SAMPLES], s_val[3 * AKAZE_MLDB_CELLS];
  const int lane = threadIdx.x;
  const AkazeMldbTab &T = akaze_mldb_tab;
  const float rad = (float)(3.14159265358979323846 / 180.0), two_pi = (float)(2.0 * 3.14159265358979323846);
  const float third = (float)(3.14159265358979323846 / 3.0), five_thirds = (float)(5.0 * 3.14159265358979323846 / 3.0);
  for (int q = blockIdx.x; q < n; q += gridDim.x) {
    const AkazeKp r = kp[q];
    const int level = min(max(r.class_id, 0), lv.n - 1);   // (the host has checked it)
    const AkazeLevel L = lv.l[level];
    const int h = L.h, w = L.w;
    const float ratio = (float)(1 << L.octave);
    const float s = rintf(__fdiv_rn(mul_rn(0.5f, r.size), ratio)), xf = __fdiv_rn(r.x, ratio), yf = __fdiv_rn(r.y, ratio);
    // O1, O2
    for (int k = lane; k < AKAZE_ORI_SAMPLES; k += 64) {
      const float yr = rintf(add_rn(yf, mul_rn((float)T.sj[k], s))), xr = rintf(add_rn(xf, mul_rn((float)T.si[k], s)));
      const int at = akaze_inside(yr, xr, h, w);
      const float rx = mul_rn(T.g[k], at >= 0 ? L.Lx[at] : 0.f), ry = mul_rn(T.g[k], at >= 0 ? L.Ly[at] : 0.f);
      s_rx[k] = rx; s_ry[k] = ry;
      s_ang[k] = mul_rn(akaze_fast_atan(ry, rx), rad);
    }
    __syncthreads();
    // O3: lane t sums window t
    float sx = 0.f, sy = 0.f, m = 0.f;
    if (lane < AKAZE_ORI_WINDOWS) {
      float ang1 = 0.f;
      for (int t = 0; t < lane; ++t) ang1 = add_rn(ang1, 0.15f);
      const float up = add_rn(ang1, third);
      const float ang2 = up > two_pi ? sub_rn(ang1, five_thirds) : up;
      for (int k = 0; k < AKAZE_ORI_SAMPLES; ++k) {
        const float a = s_ang[k];
        if ((ang1 < ang2 && ang1 < a && a < ang2) || (ang2 < ang1 && ((a > 0.f && a < ang2) || (a > ang1 && a < two_pi)))) {
          sx = add_rn(sx, s_rx[k]);
          sy = add_rn(sy, s_ry[k]);
        }
      }
      m = add_rn(mul_rn(sx, sx), mul_rn(sy, sy));
      if (!(m > 0.f)) m = 0.f;
    }
    float mx = m;
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const unsigned long long won = __ballot(mx > 0.f && m == mx);
    // O4
    float co = 1.f, si = 0.f, ang = 0.f;
    if (won) {
      const int win = __ffsll((long long)won) - 1;   // the first window that reaches the maximum
      const float wx = __shfl(sx, win), wy = __shfl(sy, win);
      const float norm = sqrtf(add_rn(mul_rn(wx, wx), mul_rn(wy, wy)));
      co = __fdiv_rn(wx, norm);
      si = __fdiv_rn(wy, norm);
      ang = akaze_fast_atan(wy, wx);
    }
    // D1: lane c sums cell c
    if (lane < AKAZE_MLDB_CELLS) {
      const int ci = T.ci[lane], cj = T.cj[lane], step = T.cstep[lane];
      float di = 0.f, dx = 0.f, dy = 0.f;
      int ns = 0;
      for (int k = ci; k < ci + step; ++k)
        for (int l = cj; l < cj + step; ++l) {
          const float sample_y = add_rn(yf, add_rn(mul_rn(mul_rn((float)l, co), s), mul_rn(mul_rn((float)k, si), s)));
          const float sample_x = add_rn(xf, add_rn(mul_rn(mul_rn((float)(-l), si), s), mul_rn(mul_rn((float)k, co), s)));
          const int at = akaze_inside(rintf(sample_y), rintf(sample_x), h, w);
          if (at < 0) continue;
          const float rx = L.Lx[at], ry = L.Ly[at];
          di = add_rn(di, L.Lt[at]);
          dx = add_rn(dx, add_rn(mul_rn(-rx, si), mul_rn(ry, co)));
          dy = add_rn(dy, add_rn(mul_rn(rx, co), mul_rn(ry, si)));
          ++ns;
        }
      if (ns > 0) {
        const float fn = (float)ns;
        di = __fdiv_rn(di, fn); dx = __fdiv_rn(dx, fn); dy = __fdiv_rn(dy, fn);
      }
      s_val[lane] = di; s_val[AKAZE_MLDB_CELLS + lane] = dx; s_val[2 * AKAZE_MLDB_CELLS + lane] = dy;
    }
    __syncthreads();
    // D2
    if (lane < AKAZE_MLDB_BYTES) {
      unsigned byte = 0;
      for (int b = 0; b < 8; ++b) {
        const int p = 8 * lane + b;
        if (p < AKAZE_MLDB_BITS && s_val[T.pa[p]] > s_val[T.pb[p]]) byte |= 1u << b;
      }
      desc[(size_t)q * AKAZE_MLDB_BYTES + lane] = (uint8_t)byte;
    }
    if (lane == 0) angle[q] = ang;
    __syncthreads();   // the next keypoint reuses the LDS arrays
  }
}

}  // namespace spvo
