// classic_detect.hip.h -- the classic front end's other two detectors on the GPU: Shi-Tomasi (cv::GFTTDetector::create(1000, 0.03,
// 7.5, 5, false, 0.04)) and FAST (cv::FastFeatureDetector::create(10, true)), feature_detection_classic.cpp:32-47 -- SURVEY.md
// section 8a row U.  Together with the ORB extractor for given keypoints (spvo_orb_describe: orb.hip.h's blur and describe kernels
// on a one-level OrbLevels) they make ClassicFeatureFrontEnd's ShiTomasi + ORB (its default constructor) and FAST + ORB run.
// The reference obtains both detectors from OpenCV, which does not exist in this build: what is built here is the published
// algorithm with the reference's parameters and OpenCV's tie / border rules as far as they are known, restated once on the CPU
// (tests/classic_ref.py) and reproduced by these kernels bit for bit -- it agrees with the build's own definition; OpenCV is unpinned.
// The choices (the same list heads tests/classic_ref.py):
//   1. 3x3 Sobel on the u8 image (reflect-101), 5x5 un-normalised box sums of Ix^2, IxIy, Iy^2 (reflect-101 of the product images): exact
//      int32 (|Sobel| <= 1020, 25 products <= 2.7e7).
//   2. lambda2 = (a + c) - sqrt((a - c)^2 + 4 b^2): radicand exact in int64 (< 2^53), ONE __dsqrt_rn, ONE __dsub_rn, clamp at 0, one
//      rounding to fp32.  OpenCV's scale 0.5 / (255 * 4 * 5)^2 is a positive constant that changes no comparison: it is applied
//      only to the reported response (one mul_rn).
//   3. candidates: lambda2 > fp32(fp64(max) * quality) (strict, THRESH_TOZERO), >= all eight neighbours (val == dilate(val): ties all
//      kept), not in the outermost 1-pixel frame.
//   4. order: response descending, of equal responses the LATER raster position first (greaterThanPtr compares addresses).
//   5. minimum distance: greedy in that order, keep iff no kept one has dx^2 + dy^2 < min_distance^2 (strict); the first max_corners
//      kept.  The lexicographically first maximal independent set again: the monotone UNDECIDED -> KEPT / SUPPRESSED iteration of
//      post.hip.h (K8-K10, proof there) over a state map, the window being a disc instead of a Chebyshev square.
//   6. FAST-9/16: orb_fast_kernel's score with a 3-pixel border; suppression keeps a corner iff its score is STRICTLY greater than all
//      eight neighbours' (two equal neighbours both go: cv::FAST's rule, not ORB's "first of equals wins"); raster order; no cap.
//   7. keypoint coordinates are integers stored as float.
// 256-thread groups of 64x4 pixels, as orb.hip.h.  All of it is latency- / launch-bound integer and byte work: no MFMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "orb.hip.h"
#include "list_steps.hip.h"   // workgroup_append, wave_append, rank_by_counting, stable_compact_walk

namespace spvo {

constexpr int CLS_PAD = 16;              // state-map padding: >= the largest supported disc radius (min_distance <= 15 -> 14)
constexpr int CLS_COUNTER_INTS = 16;     // 0 candidates, 1 kept / survivors, 2 written, 3 overflow, 4 max(lambda2) bits, 5 rounds of the finish kernel, 8.. undecided after launch k
constexpr int CLS_ROUND_LAUNCHES = 3;    // grid-wide round launches before the one-workgroup finish
__host__ __device__ inline int cls_state_pitch(int w) { return ((w + 2 * CLS_PAD + 3) / 4) * 4; }

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// Choice 1 + 2 in one launch: the u8 tile with a 3-pixel halo goes to LDS once, the three products of the tile with a 2-pixel halo to
// LDS, box sums from LDS.  A product OUTSIDE the image is the product at the reflected position (the box filter reflects the product
// images, not the u8 image), so those few are computed from global memory at the reflected position.  The image-wide maximum is one
// atomicMax on the float's bit pattern per workgroup (lambda2 >= 0: bit patterns order like the values).
__global__ __launch_bounds__(256) void gftt_response_kernel(const uint8_t *__restrict__ im, int h, int w, float *__restrict__ lam, int *__restrict__ counters) {
  constexpr int TW = 64 + 6, TH = 4 + 6, PW = 64 + 4, PH = 4 + 4;
  __shared__ int s_im[TH * TW];
  __shared__ int s_xx[PH * PW], s_xy[PH * PW], s_yy[PH * PW];
  __shared__ unsigned s_max[4];
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 4;
  for (int i = threadIdx.x; i < TH * TW; i += 256) {
    const int ty = i / TW, tx = i - ty * TW;
    const int gy = min(max(reflect101(y0 + ty - 3, h), 0), h - 1), gx = min(max(reflect101(x0 + tx - 3, w), 0), w - 1);   // (the clamp only guards tiles that hang over the image: their values are never used)
    s_im[i] = im[(size_t)gy * w + gx];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < PH * PW; i += 256) {
    const int py = i / PW, px = i - py * PW;
    const int gy = y0 + py - 2, gx = x0 + px - 2;
    int ix, iy;
    if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
      const int *p = s_im + (py + 1) * TW + px + 1;   // tile coordinates of (gy, gx)
      ix = (p[-TW + 1] + 2 * p[1] + p[TW + 1]) - (p[-TW - 1] + 2 * p[-1] + p[TW - 1]);
      iy = (p[TW - 1] + 2 * p[TW] + p[TW + 1]) - (p[-TW - 1] + 2 * p[-TW] + p[-TW + 1]);
    } else {
      const int ry = min(max(reflect101(gy, h), 0), h - 1), rx = min(max(reflect101(gx, w), 0), w - 1);
      const int ym = reflect101(ry - 1, h), yp = reflect101(ry + 1, h), xm = reflect101(rx - 1, w), xp = reflect101(rx + 1, w);
      auto at = [&](int yy, int xx) { return (int)im[(size_t)yy * w + xx]; };
      ix = (at(ym, xp) + 2 * at(ry, xp) + at(yp, xp)) - (at(ym, xm) + 2 * at(ry, xm) + at(yp, xm));
      iy = (at(yp, xm) + 2 * at(yp, rx) + at(yp, xp)) - (at(ym, xm) + 2 * at(ym, rx) + at(ym, xp));
    }
    s_xx[i] = ix * ix; s_xy[i] = ix * iy; s_yy[i] = iy * iy;
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int x = x0 + lx, y = y0 + ly;
  float v = 0.f;
  if (x < w && y < h) {
    int a = 0, b = 0, c = 0;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const int k = (ly + dy) * PW + lx + dx;
        a += s_xx[k]; b += s_xy[k]; c += s_yy[k];
      }
    const long long d = (long long)a - c, rad = d * d + 4ll * b * b;
    const double l2 = __dsub_rn((double)(a + c), __dsqrt_rn((double)rad));
    v = (float)fmax(l2, 0.0);
    lam[(size_t)y * w + x] = v;
  }
  unsigned m = __float_as_uint(v);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  if (lx == 0) s_max[ly] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned mm = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    if (mm) atomicMax((unsigned *)&counters[4], mm);
  }
}

// Choice 3: candidates -> state map (UNDECIDED / NONE for every pixel of the image) + candidate list, one atomic per workgroup
// (workgroup_append, list_steps.hip.h)
__global__ __launch_bounds__(256) void gftt_collect_kernel(const float *__restrict__ lam, int h, int w, double quality, uint8_t *__restrict__ state, int *__restrict__ cand,
                                                           int *__restrict__ counters) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const float thr = (float)((double)__uint_as_float((unsigned)counters[4]) * quality);
  bool c = false;
  if (x >= 1 && x < w - 1 && y >= 1 && y < h - 1) {
    const float *p = lam + (size_t)y * w + x;
    const float v = *p;
    c = v > thr && v >= p[-w - 1] && v >= p[-w] && v >= p[-w + 1] && v >= p[-1] && v >= p[1] && v >= p[w - 1] && v >= p[w] && v >= p[w + 1];
  }
  if (x < w && y < h) state[(size_t)(y + CLS_PAD) * cls_state_pitch(w) + x + CLS_PAD] = c ? ST_UNDECIDED : ST_NONE;
  const int slot = workgroup_append(c, &counters[0]);
  if (c) cand[slot] = y * w + x;   // (at most (h - 2)(w - 2) candidates: the list holds h w)
}

// Choice 4 as a key: smaller = earlier.  Higher response first; of equal responses the later raster position first.
__device__ __forceinline__ unsigned long long gftt_key(float v, int p) {
  return ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(v)) << 32) | (0xFFFFFFFFu - (unsigned)p);
}

// the decision for one undecided candidate (nms_decide of post.hip.h with a disc for a window): ST_KEPT / ST_SUPPRESSED / ST_UNDECIDED
__device__ __forceinline__ uint8_t gftt_decide(const float *__restrict__ lam, const uint8_t *state, int w, int pitch, int radius, int lim, int p, int x, int y) {
  const unsigned long long key = gftt_key(lam[p], p);
  bool any_kept = false, any_better = false;
  for (int dy = -radius; dy <= radius; ++dy) {
    const volatile uint8_t *row = state + (size_t)(y + dy + CLS_PAD) * pitch + x + CLS_PAD;
    for (int dx = -radius; dx <= radius; ++dx) {
      if (dy * dy + dx * dx > lim || !(dy | dx)) continue;
      const uint8_t s = row[dx];
      if (s == ST_KEPT) any_kept = true;
      else if (s == ST_UNDECIDED && gftt_key(lam[p + dy * w + dx], p + dy * w + dx) < key) any_better = true;
    }
  }
  return any_kept ? ST_SUPPRESSED : (any_better ? ST_UNDECIDED : ST_KEPT);
}

__device__ __forceinline__ void gftt_survive(const float *__restrict__ lam, int p, unsigned long long *__restrict__ keys, int cap, int *__restrict__ counters) {
  const int s = atomicAdd(&counters[1], 1);
  if (s < cap) keys[s] = gftt_key(lam[p], p);
  else counters[3] = 1;
}

// Choice 5, grid-wide rounds (nms_round_kernel).  Decisions are final and equal the greedy outcome whatever staleness the neighbour
// states are observed with; a kept candidate enters the survivor list on the spot.  counters[8 + launch] = undecided after this launch.
template <int INNER>
__global__ __launch_bounds__(256) void gftt_round_kernel(const float *__restrict__ lam, int w, int radius, int lim, uint8_t *state, const int *__restrict__ cand,
                                                         unsigned long long *__restrict__ keys, int key_cap, int *__restrict__ counters, int launch) {
  if (launch > 0 && counters[8 + launch - 1] == 0) return;
  const int n = counters[0];
  const int pitch = cls_state_pitch(w);
  const int stride = gridDim.x * 256;
  for (int it = 0; it < INNER; ++it) {
    bool live = false;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
      const int p = cand[i];
      const int y = p / w, x = p - y * w;
      volatile uint8_t *sp = state + (size_t)(y + CLS_PAD) * pitch + x + CLS_PAD;
      if (*sp != ST_UNDECIDED) continue;
      const uint8_t d = gftt_decide(lam, state, w, pitch, radius, lim, p, x, y);
      if (d == ST_UNDECIDED) { live = true; continue; }
      *sp = d;
      if (d == ST_KEPT) gftt_survive(lam, p, keys, key_cap, counters);
    }
    __threadfence();
    if (!__syncthreads_or(live)) break;
  }
  int rem = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int p = cand[i];
    const int y = p / w, x = p - y * w;
    rem += ((volatile uint8_t *)state)[(size_t)(y + CLS_PAD) * pitch + x + CLS_PAD] == ST_UNDECIDED ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) rem += __shfl_xor(rem, o);
  if ((threadIdx.x & 63) == 0 && rem) atomicAdd(&counters[8 + launch], rem);
}

// The stragglers (nms_finish_kernel): ONE workgroup iterates rounds with workgroup barriers between them until nothing is undecided.
// Every round decides at least the best undecided candidate of the image, so the loop ends.  counters[5] = rounds it took.
__global__ __launch_bounds__(1024) void gftt_finish_kernel(const float *__restrict__ lam, int w, int radius, int lim, uint8_t *state, const int *__restrict__ cand,
                                                           unsigned long long *__restrict__ keys, int key_cap, int *__restrict__ counters, int launch) {
  if (counters[8 + launch - 1] == 0) return;
  const int n = counters[0];
  const int pitch = cls_state_pitch(w);
  int rounds = 0;
  for (;;) {
    bool live = false;
    for (int i = threadIdx.x; i < n; i += 1024) {
      const int p = cand[i];
      const int y = p / w, x = p - y * w;
      volatile uint8_t *sp = state + (size_t)(y + CLS_PAD) * pitch + x + CLS_PAD;
      if (*sp != ST_UNDECIDED) continue;
      const uint8_t d = gftt_decide(lam, state, w, pitch, radius, lim, p, x, y);
      if (d == ST_UNDECIDED) { live = true; continue; }
      *sp = d;
      if (d == ST_KEPT) gftt_survive(lam, p, keys, key_cap, counters);
    }
    ++rounds;
    __threadfence();
    if (!__syncthreads_or(live)) break;
  }
  if (threadIdx.x == 0) counters[5] = rounds;
}

// rank by counting (rank_by_counting, list_steps.hip.h) over one key list whose length lies in device memory
__global__ __launch_bounds__(256) void cls_rank_kernel(const unsigned long long *__restrict__ keys, int *__restrict__ rank, const int *__restrict__ n_ptr, int cap) {
  rank_by_counting(keys, rank, min(*n_ptr, cap));
}

// the first max_corners kept in rank order -> xy (float), response (lambda2 x scale); counters[2] = how many
__global__ __launch_bounds__(256) void gftt_write_kernel(const float *__restrict__ lam, int w, const unsigned long long *__restrict__ keys, int *__restrict__ rank, int key_cap,
                                                         int max_corners, float scale, float *__restrict__ xy, float *__restrict__ resp, int *__restrict__ counters) {
  const int n = min(counters[1], key_cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) counters[2] = min(n, max_corners);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int r = rank[i];
    rank[i] = 0;
    if (r < max_corners) {
      const int p = (int)(0xFFFFFFFFu - (unsigned)(keys[i] & 0xFFFFFFFFull));
      const int y = p / w, x = p - y * w;
      xy[2 * r] = (float)x;
      xy[2 * r + 1] = (float)y;
      resp[r] = mul_rn(lam[p], scale);
    }
  }
}

// Choice 6: FAST corners of the score map -> keys (raster index << 32 | score), one atomic per wave (wave_append, list_steps.hip.h;
// the suppression rule differs from orb_collect_kernel's: strictly greater than all eight neighbours).  The score map is 0 in the 3-pixel border.
__global__ __launch_bounds__(256) void fast_collect_kernel(const uint8_t *__restrict__ score, int h, int w, int nonmax, unsigned long long *__restrict__ keys, int cap,
                                                           int *__restrict__ counters) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (y >= h) return;   // (whole waves)
  const bool inside = x >= 3 && x < w - 3 && y >= 3 && y < h - 3;
  const int s = inside ? score[(size_t)y * w + x] : 0;
  bool keep = s != 0;
  if (keep && nonmax) {
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx)
        if ((dy || dx) && (int)score[(size_t)(y + dy) * w + x + dx] >= s) keep = false;
  }
  const int slot = wave_append(keep, &counters[1]);
  if (!keep) return;
  if (slot < cap) keys[slot] = ((unsigned long long)(unsigned)(y * w + x) << 32) | (unsigned)s;
  else counters[3] = 1;
}

// raster order: position = rank of the key
__global__ __launch_bounds__(256) void fast_write_kernel(int w, const unsigned long long *__restrict__ keys, int *__restrict__ rank, int key_cap, float *__restrict__ xy,
                                                         float *__restrict__ resp, int *__restrict__ counters) {
  const int n = min(counters[1], key_cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) counters[2] = n;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int r = rank[i];
    rank[i] = 0;
    const int p = (int)(keys[i] >> 32);
    const int y = p / w, x = p - y * w;
    xy[2 * r] = (float)x;
    xy[2 * r + 1] = (float)y;
    resp[r] = (float)(unsigned)(keys[i] & 0xFFull);
  }
}

// ---- spvo_classic_detect: detector -> extractor -> feature slot without the host in between
// cv::ORB::compute's border rule on the device (what spvo_orb_describe does on the host around its launch): of the n = counters[2] keypoints
// in xy, those at least `edge` pixels from every border, ORDER-PRESERVING, as the extractor's integer list + the detector's responses.
// ONE workgroup walks the list (stable_compact_walk, list_steps.hip.h).  out_cnt[0] = kept in all, out_cnt[2] = min(kept, cap) = what
// orb_describe_kernel describes.
__global__ __launch_bounds__(1024) void cls_compact_kernel(const float *__restrict__ xy, const float *__restrict__ resp, const int *__restrict__ counters, int h, int w, int edge,
                                                           int *__restrict__ kxy, float *__restrict__ kresp, int cap, int *__restrict__ out_cnt) {
  int x = 0, y = 0;   // keypoint i's integer coordinates, from keep(i) to put(off, i)
  const int base = stable_compact_walk(
      counters[2],
      [&](int i) {
        x = (int)xy[2 * i]; y = (int)xy[2 * i + 1];
        return !(x < edge || x >= w - edge || y < edge || y >= h - edge);
      },
      [&](int off, int i) {
        if (off >= cap) return;
        kxy[2 * off] = x; kxy[2 * off + 1] = y;
        kresp[off] = resp[i];
      });
  if (threadIdx.x == 0) { out_cnt[0] = base; out_cnt[2] = min(base, cap); }
}

// The last launch of an image: the slot's count on the device, and the host's copy of the slot -- count, keypoint records and descriptors
// go to pinned memory from here, n rows instead of a capacity-sized copy whose length the host cannot know yet.
//   ORB (n_levels = 8):  n = min(sum of the levels' written counts, kp_cap) as spvo_orb_detect computes it; overflow = any level's flag
//   extractor (n_levels = 0): n = ext_cnt[0] (all that passed the border rule); the record's response becomes the DETECTOR's (kresp)
// h_n = {n, overflow}; the slot holds min(n, cap) rows (n > cap: the caller reports SPVO_ERR_CAPACITY and the slot stays unfilled).
__global__ __launch_bounds__(256) void classic_finish_kernel(const int *__restrict__ orb_counters, int n_levels, int counter_stride, int kp_cap, const int *__restrict__ det_counters,
                                                             const int *__restrict__ ext_cnt, const float *__restrict__ kresp, OrbKeypoint *__restrict__ kps,
                                                             const uint4 *__restrict__ desc, int cap, int *__restrict__ d_n, int *__restrict__ h_n,
                                                             OrbKeypoint *__restrict__ h_kp, uint4 *__restrict__ h_desc) {
  int n_all = 0, overflow = 0;
  if (n_levels > 0) {
    for (int l = 0; l < n_levels; ++l) { n_all += orb_counters[l * counter_stride + 2]; overflow |= orb_counters[l * counter_stride + 3]; }
    n_all = min(n_all, kp_cap);
  } else {
    n_all = ext_cnt[0];
    overflow = det_counters[3];
  }
  const int n = min(n_all, cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) { *d_n = n; h_n[0] = n_all; h_n[1] = overflow; }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    OrbKeypoint k = kps[i];
    if (n_levels == 0) { k.response = kresp[i]; kps[i] = k; }
    h_kp[i] = k;
    h_desc[2 * i] = desc[2 * i];
    h_desc[2 * i + 1] = desc[2 * i + 1];
  }
}

}  // namespace spvo
