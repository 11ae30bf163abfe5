// brisk.hip.h -- the BRISK descriptor extractor of the classic front end on given keypoints (cv::BRISK::create(30, 3, 1.0f)->compute,
// feature_detection_classic.cpp:56-65, 110-111) as tests/brisk_ref.py restates it; its header lists every choice, the kernels reproduce
// it bit for bit on the same tables.  Everything numeric here is integer or a fixed sequence of single float operations (no contraction,
// no atomics on floats, no order-dependent sums): two calls return identical bytes.
//   brisk_integral_rows_kernel / _cols_kernel   the (rows + 1) x (cols + 1) int32 integral image: a wave-level scan along every row, then
//                                               a running sum down every column (exact integers: any order gives the same image)
//   brisk_compact_kernel                        the border rule as an order-preserving compaction (list_steps.hip.h's walk): the kept
//                                               indices and their scale index
//   brisk_compact_list_kernel                   the same walk on a detector's list whose length is on the device, one size for all
//                                               (spvo_classic_detect's chain); brisk_slot_finish_kernel closes that chain
//   brisk_pair_compact_kernel                   the walk on the BRISK detector's own records where brisk_refine_kernel left them: the keep flag
//                                               and the border rule of EVERY record's own scale index in one launch
//                                               (spvo_brisk_detect_pair's chain); brisk_pair_finish_kernel closes that chain
//   brisk_describe_kernel                       one wave64 per kept keypoint at a time, four per workgroup: 60 box means at rotation 0, direction
//                                               from the 870 long pairs, 60 box means at rotation theta, 512 short-pair bits
//   brisk_finish_kernel                         count and results to pinned host memory, n_kept rows instead of a capacity-sized copy
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "spvo_types.hip.h"   // OrbKeypoint
#include "list_steps.hip.h"   // stable_compact_walk

namespace spvo {

constexpr int BRISK_DESCRIBE_BLOCKS = 512;   // workgroups of brisk_describe_kernel at most (two per CU): beyond 2048 keypoints a wave takes several
constexpr int BRISK_SCALES = 64, BRISK_ROT = 1024, BRISK_POINTS = 60, BRISK_SHORT = 512, BRISK_LONG = 870, BRISK_BYTES = 64;

struct BriskLongPair { unsigned char i, j; short wdx, wdy; short pad; };   // 8 bytes
struct BriskShortPair { unsigned char i, j; };

// what the per-keypoint rules need besides the tables: size_list, and the two float constants of the scale index (brisk_ref.py choice 8)
struct BriskParams {
  int size_list[BRISK_SCALES];
  float basic_size_06;     // 12 * 0.6f
  float scales_over_lb;    // 64 / lb, lb = (float)log(30) / 0.693147180559945f
};

// I[r + 1][c + 1] of row r = the prefix sums of the row itself; row 0 and column 0 are zero.  One wave per row, four rows per workgroup.
__global__ __launch_bounds__(256) void brisk_integral_rows_kernel(const uint8_t *__restrict__ im, int rows, int cols, int *__restrict__ integ) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int pitch = cols + 1;
  if (r == 0)
    for (int c = lane; c < pitch; c += 64) integ[c] = 0;
  if (r >= rows) return;
  int *out = integ + (size_t)(r + 1) * pitch;
  const uint8_t *src = im + (size_t)r * cols;
  if (lane == 0) out[0] = 0;
  int carry = 0;
  for (int c0 = 0; c0 < cols; c0 += 64) {   // (wave-uniform trip count: the shuffles below are executed by all 64 lanes)
    const int c = c0 + lane;
    int v = c < cols ? (int)src[c] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(v, d);
      if (lane >= d) v += t;
    }
    if (c < cols) out[c + 1] = carry + v;
    carry += __shfl(v, 63);
  }
}

// a running sum down every column of rows 1 .. rows (one thread per column: neighbouring threads read and write neighbouring ints)
__global__ __launch_bounds__(256) void brisk_integral_cols_kernel(int rows, int cols, int *__restrict__ integ) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int pitch = cols + 1;
  if (c >= pitch) return;
  int acc = 0;
  for (int r = 1; r <= rows; ++r) {
    acc += integ[(size_t)r * pitch + c];
    integ[(size_t)r * pitch + c] = acc;
  }
}

// brisk_ref.py choice 8
__device__ inline int brisk_scale_index(float size, const BriskParams &P) {
  const float q = __fdiv_rn(size, P.basic_size_06);
  const float lq = (float)log((double)q);
  const float w = __fmul_rn(P.scales_over_lb, __fdiv_rn(lq, 0.693147180559945f));
  const double s = (double)w + 0.5;
  if (!(s >= 1.0)) return 0;
  return s >= (double)BRISK_SCALES ? BRISK_SCALES - 1 : (int)s;
}

// choice 9 as an order-preserving compaction by ONE workgroup (stable_compact_walk, list_steps.hip.h): the border rule on top of the walk.
// Keypoint i's coordinates are xy[stride * i], xy[stride * i + 1]; live(i) says whether it takes part at all (a
// dead one's coordinates are not read), scale_of(i) is its scale index; of the survivors the first `cap` are handed to put(k, i, s) -- the
// k-th survivor is keypoint i at scale s -- and ALL are counted: the return value (the same in every thread).
template <typename Live, typename ScaleOf, typename Put>
__device__ __forceinline__ int brisk_compact_walk_if(const float *__restrict__ xy, int stride, int n, int h, int w, const BriskParams &P, int cap, Live live, ScaleOf scale_of, Put put) {
  int s = 0;   // keypoint i's scale index, from the rule to put
  return stable_compact_walk(
      n,
      [&](int i) {
        if (!live(i)) return false;
        const float x = xy[(size_t)stride * i], y = xy[(size_t)stride * i + 1];
        s = scale_of(i);
        const float b = (float)P.size_list[s];
        return x >= b && x < (float)w - b && y >= b && y < (float)h - b;   // (a NaN coordinate is dropped)
      },
      [&](int k, int i) { if (k < cap) put(k, i, s); });
}
// ... on a packed [n][2] list of which every keypoint takes part
template <typename ScaleOf, typename Put>
__device__ __forceinline__ int brisk_compact_walk(const float *__restrict__ xy, int n, int h, int w, const BriskParams &P, int cap, ScaleOf scale_of, Put put) {
  return brisk_compact_walk_if(xy, 2, n, h, w, P, cap, [](int) { return true; }, scale_of, put);
}

// spvo_brisk_describe: n and a size per keypoint from the host.  kept[k] = index into xy of the k-th survivor, kscale[k] its scale index;
// out_cnt[0] = their number (at most n survive: nothing is cut).
__global__ __launch_bounds__(1024) void brisk_compact_kernel(const float *__restrict__ xy, const float *__restrict__ size, int n, int h, int w, BriskParams P,
                                                             int *__restrict__ kept, int *__restrict__ kscale, int *__restrict__ out_cnt) {
  const int base = brisk_compact_walk(xy, n, h, w, P, n, [&](int i) { return brisk_scale_index(size[i], P); }, [&](int k, int i, int s) { kept[k] = i; kscale[k] = s; });
  if (threadIdx.x == 0) out_cnt[0] = base;
}

// spvo_classic_detect: the detector's list as it lies on the device -- n = det_counters[2] keypoints in xy, their responses in resp -- and ONE
// size for all of them (5: Shi-Tomasi, 7: FAST).  The detector's response goes along (kresp[k]), as in cls_compact_kernel, and overflow is
// that kernel's too: survivors at or beyond `cap` are counted and not written.  out_cnt[0] = survivors in all (reaches the host),
// out_cnt[2] = min(that, cap) = what brisk_describe_kernel describes.
__global__ __launch_bounds__(1024) void brisk_compact_list_kernel(const float *__restrict__ xy, const float *__restrict__ resp, const int *__restrict__ det_counters, float size,
                                                                  int h, int w, BriskParams P, int cap, int *__restrict__ kept, int *__restrict__ kscale,
                                                                  float *__restrict__ kresp, int *__restrict__ out_cnt) {
  const int s_all = brisk_scale_index(size, P);
  const int base = brisk_compact_walk(xy, det_counters[2], h, w, P, cap, [&](int) { return s_all; }, [&](int k, int i, int s) { kept[k] = i; kscale[k] = s; kresp[k] = resp[i]; });
  if (threadIdx.x == 0) { out_cnt[0] = base; out_cnt[2] = min(base, cap); }
}

// spvo_brisk_detect_pair: the BRISK detector's records as brisk_refine_kernel left them -- rec[i] and keep[i] of the min(det_counters[1],
// det_cap) candidates, in output order -- instead of brisk_det_compact_kernel, a download, an upload and brisk_compact_kernel: a record
// survives iff its keep flag is set AND it passes the border rule of ITS OWN scale index (a BRISK keypoint carries its own size).  The k-th
// survivor leaves what brisk_describe_kernel reads -- its coordinates in the packed list kxy[k], kept[k] = k, kscale[k] -- and its record
// crec[k] for brisk_pair_finish_kernel.  Overflow and out_cnt as brisk_compact_list_kernel.
static_assert(sizeof(BriskDetKeypoint) == 6 * sizeof(float), "a record is six words: x, y lead it");
__global__ __launch_bounds__(1024) void brisk_pair_compact_kernel(const BriskDetKeypoint *__restrict__ rec, const int *__restrict__ keep, const int *__restrict__ det_counters,
                                                                  int det_cap, int h, int w, BriskParams P, int cap, float *__restrict__ kxy, int *__restrict__ kept,
                                                                  int *__restrict__ kscale, BriskDetKeypoint *__restrict__ crec, int *__restrict__ out_cnt) {
  const int n = min(det_counters[1], det_cap);
  const int base = brisk_compact_walk_if(
      &rec->x, 6, n, h, w, P, cap, [&](int i) { return keep[i] != 0; }, [&](int i) { return brisk_scale_index(rec[i].size, P); },
      [&](int k, int i, int s) {
        const float x = rec[i].x, y = rec[i].y, size = rec[i].size, angle = rec[i].angle, response = rec[i].response;
        const int32_t octave = rec[i].octave;
        kxy[2 * k] = x; kxy[2 * k + 1] = y;
        kept[k] = k; kscale[k] = s;
        crec[k].x = x; crec[k].y = y; crec[k].size = size; crec[k].angle = angle; crec[k].response = response; crec[k].octave = octave;
      });
  if (threadIdx.x == 0) { out_cnt[0] = base; out_cnt[2] = min(base, cap); }
}

// choices 10 and 11: the box mean of half-width sigma around (xf, yf).  Every index is clamped into the image: for a keypoint that passed
// the border rule no clamp binds (brisk_ref.py asserts it), and nothing else may read out of bounds.
__device__ inline int brisk_smoothed(const uint8_t *__restrict__ im, const int *__restrict__ integ, int rows, int cols, float xf, float yf, float sigma) {
#pragma clang fp contract(off)
  const float area = 4.0f * sigma * sigma;
  const int scaling = (int)(4194304.0 / (double)area);
  const float scf = (float)scaling;
  int scaling2 = (int)((double)(scf * area) / 1024.0);
  scaling2 = scaling2 > 0 ? scaling2 : 1;
  const float x_1 = xf - sigma, x1 = xf + sigma, y_1 = yf - sigma, y1 = yf + sigma;
  const int xl = min(max((int)((double)x_1 + 0.5), 0), cols - 1), yt = min(max((int)((double)y_1 + 0.5), 0), rows - 1);
  const int xr = min(max((int)((double)x1 + 0.5), xl), cols - 1), yb = min(max((int)((double)y1 + 0.5), yt), rows - 1);
  const float r_x_1 = (float)xl - x_1 + 0.5f, r_y_1 = (float)yt - y_1 + 0.5f;
  const float r_x1 = x1 - (float)xr + 0.5f, r_y1 = y1 - (float)yb + 0.5f;
  const int A = (int)((r_x_1 * r_y_1) * scf), B = (int)((r_x1 * r_y_1) * scf), C = (int)((r_x1 * r_y1) * scf), D = (int)((r_x_1 * r_y1) * scf);
  const int wl = (int)(r_x_1 * scf), wt = (int)(r_y_1 * scf), wr = (int)(r_x1 * scf), wb = (int)(r_y1 * scf);
  const int pitch = cols + 1;
  const int *r0 = integ + (size_t)yt * pitch, *r1 = r0 + pitch, *r2 = integ + (size_t)yb * pitch, *r3 = r2 + pitch;
  // the integral image at the four rows yt, yt + 1, yb, yb + 1 and the four columns xl, xl + 1, xr, xr + 1
  const int a0 = r0[xl + 1], a1 = r0[xr];
  const int b0 = r1[xl], b1 = r1[xl + 1], b2 = r1[xr], b3 = r1[xr + 1];
  const int c0 = r2[xl], c1 = r2[xl + 1], c2 = r2[xr], c3 = r2[xr + 1];
  const int d0 = r3[xl + 1], d1 = r3[xr];
  int total = A * (int)im[(size_t)yt * cols + xl] + B * (int)im[(size_t)yt * cols + xr] + C * (int)im[(size_t)yb * cols + xr] + D * (int)im[(size_t)yb * cols + xl];
  total += (b2 - a1 - b1 + a0) * wt + (d1 - c2 - d0 + c1) * wb;     // the rows yt and yb between the corners
  total += (c1 - b1 - c0 + b0) * wl + (c3 - b3 - c2 + b2) * wr;     // the columns xl and xr between the corners
  total += (c2 - b2 - c1 + b1) * scaling;                           // the interior
  return (total + scaling2 / 2) / scaling2;
}

__device__ inline int brisk_wave_sum(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// One wave per kept keypoint at a time (a wave strides over the list when there are more keypoints than waves, so a workgroup loads the pair
// tables once for all of its keypoints).  The 60 intensities stay in the registers of lanes 0 .. 59 and a pair reads its two through __shfl (every
// shuffle is executed by all 64 lanes with an index below 60); the pair tables are in LDS, loaded once per workgroup.
//   angle [n] degrees (0 .. 360), desc [n][64], values0 [n][60] (may be NULL): row k belongs to keypoint kept[k]
__global__ __launch_bounds__(256) void brisk_describe_kernel(const uint8_t *__restrict__ im, const int *__restrict__ integ, int rows, int cols, const float *__restrict__ xy,
                                                             const int *__restrict__ kept, const int *__restrict__ kscale, const int *__restrict__ cnt,
                                                             const float *__restrict__ points, const BriskLongPair *__restrict__ long_pairs,
                                                             const BriskShortPair *__restrict__ short_pairs, float *__restrict__ angle, uint8_t *__restrict__ desc,
                                                             int *__restrict__ values0) {
  __shared__ BriskLongPair s_long[BRISK_LONG];
  __shared__ BriskShortPair s_short[BRISK_SHORT];
  for (int p = threadIdx.x; p < BRISK_LONG; p += 256) s_long[p] = long_pairs[p];
  for (int p = threadIdx.x; p < BRISK_SHORT; p += 256) s_short[p] = short_pairs[p];
  __syncthreads();
  const int lane = threadIdx.x & 63, n_kept = cnt[0];
  for (int k = blockIdx.x * 4 + (threadIdx.x >> 6); k < n_kept; k += gridDim.x * 4) {   // (wave-uniform; no barrier inside)
    const int src = kept[k], s = kscale[k];
    const float kx = xy[2 * src], ky = xy[2 * src + 1];
    const int pt = lane < BRISK_POINTS ? lane : 0;
    const float *p0 = points + ((size_t)s * BRISK_ROT * BRISK_POINTS + pt) * 3;
    int v = brisk_smoothed(im, integ, rows, cols, p0[0] + kx, p0[1] + ky, p0[2]);
    if (values0 && lane < BRISK_POINTS) values0[(size_t)k * BRISK_POINTS + lane] = v;
    int dir0 = 0, dir1 = 0;
#pragma unroll 2
    for (int it = 0; it < (BRISK_LONG + 63) / 64; ++it) {
      const int p = it * 64 + lane;
      const BriskLongPair lp = s_long[p < BRISK_LONG ? p : 0];
      const int delta = __shfl(v, (int)lp.i) - __shfl(v, (int)lp.j);
      if (p < BRISK_LONG) {
        dir0 += delta * lp.wdx / 1024;   // (C division: towards zero)
        dir1 += delta * lp.wdy / 1024;
      }
    }
    dir0 = brisk_wave_sum(dir0);
    dir1 = brisk_wave_sum(dir1);
    // choice 13 (every lane computes the same numbers)
    float ang = (float)(atan2((double)dir1, (double)dir0) / 3.141592653589793 * 180.0);
    int theta = (int)(1024.0 * ((double)ang / 360.0) + 0.5);
    if (theta < 0) theta += BRISK_ROT;
    if (theta >= BRISK_ROT) theta -= BRISK_ROT;
    if (ang < 0) ang += 360.f;
    if (lane == 0) angle[k] = ang;
    const float *p1 = p0 + (size_t)theta * BRISK_POINTS * 3;
    v = brisk_smoothed(im, integ, rows, cols, p1[0] + kx, p1[1] + ky, p1[2]);
    unsigned byte = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const BriskShortPair sp = s_short[lane * 8 + b];
      const int t1 = __shfl(v, (int)sp.i), t2 = __shfl(v, (int)sp.j);
      byte |= (t1 > t2 ? 1u : 0u) << b;
    }
    desc[(size_t)k * BRISK_BYTES + lane] = (uint8_t)byte;
  }
}

// The last launch of a call: count and the rows that exist go to pinned host memory.  h_n[0] = n_kept.
__global__ __launch_bounds__(256) void brisk_finish_kernel(const int *__restrict__ cnt, const int *__restrict__ kept, const float *__restrict__ angle, const uint32_t *__restrict__ desc,
                                                           const int *__restrict__ values0, int *__restrict__ h_n, int *__restrict__ h_kept, float *__restrict__ h_angle,
                                                           uint32_t *__restrict__ h_desc, int *__restrict__ h_values0) {
  const int n = cnt[0];
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  if (tid == 0) h_n[0] = n;
  for (int i = tid; i < n; i += nth) { h_kept[i] = kept[i]; h_angle[i] = angle[i]; }
  for (int i = tid; i < n * (BRISK_BYTES / 4); i += nth) h_desc[i] = desc[i];
  if (h_values0)
    for (int i = tid; i < n * BRISK_POINTS; i += nth) h_values0[i] = values0[i];
}

// The last launch of an image in spvo_classic_detect's chain: the slot's count and keypoint records on the device -- x, y the detector's,
// the extractor's angle (degrees), the detector's response, octave 0 -- and the host's copy of the slot in pinned memory: count, records
// and 64-byte rows, n rows of each.  h_n = {rows that passed the border rule, overflow flag of the detector}; the slot holds min(n, cap)
// rows (n > cap: the caller reports SPVO_ERR_CAPACITY and the slot stays unfilled).
__global__ __launch_bounds__(256) void brisk_slot_finish_kernel(const int *__restrict__ det_counters, const int *__restrict__ ext_cnt, const float *__restrict__ xy,
                                                                const int *__restrict__ kept, const float *__restrict__ angle, const float *__restrict__ kresp,
                                                                const uint4 *__restrict__ desc, int cap, OrbKeypoint *__restrict__ kps, int *__restrict__ d_n,
                                                                int *__restrict__ h_n, OrbKeypoint *__restrict__ h_kp, uint4 *__restrict__ h_desc) {
  const int n_all = ext_cnt[0], n = min(n_all, cap);
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  if (tid == 0) { *d_n = n; h_n[0] = n_all; h_n[1] = det_counters[3]; }
  for (int i = tid; i < n; i += nth) {
    const int src = kept[i];
    OrbKeypoint k;
    k.x = xy[2 * src]; k.y = xy[2 * src + 1]; k.angle = angle[i]; k.response = kresp[i]; k.octave = 0;
    kps[i] = k;
    h_kp[i] = k;
  }
  for (int i = tid; i < n * (BRISK_BYTES / 16); i += nth) h_desc[i] = desc[i];
}

// The last launch of an image in spvo_brisk_detect_pair's chain: the slot's count and its 20-byte records (x, y, the extractor's angle,
// response, layer), and the host's copy in pinned memory: count, the detector's 24-byte records with the extractor's angle (degrees) in
// place of -1, and the 64-byte rows, n of each.  h_n and n as brisk_slot_finish_kernel.
__global__ __launch_bounds__(256) void brisk_pair_finish_kernel(const int *__restrict__ det_counters, const int *__restrict__ ext_cnt, const BriskDetKeypoint *__restrict__ crec,
                                                                const float *__restrict__ angle, const uint4 *__restrict__ desc, int cap, OrbKeypoint *__restrict__ kps,
                                                                int *__restrict__ d_n, int *__restrict__ h_n, BriskDetKeypoint *__restrict__ h_kp, uint4 *__restrict__ h_desc) {
  const int n_all = ext_cnt[0], n = min(n_all, cap);
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  if (tid == 0) { *d_n = n; h_n[0] = n_all; h_n[1] = det_counters[3]; }
  for (int i = tid; i < n; i += nth) {
    BriskDetKeypoint r = crec[i];
    r.angle = angle[i];
    h_kp[i] = r;
    OrbKeypoint k;
    k.x = r.x; k.y = r.y; k.angle = r.angle; k.response = r.response; k.octave = r.octave;
    kps[i] = k;
  }
  for (int i = tid; i < n * (BRISK_BYTES / 16); i += nth) h_desc[i] = desc[i];
}

}  // namespace spvo
