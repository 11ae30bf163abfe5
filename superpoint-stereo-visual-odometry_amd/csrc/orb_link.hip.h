// orb_link.hip.h -- the device link from a detector's record list to the octave-aware ORB extractor (spvo_brisk_orb_pair,
// spvo_akaze_orb_pair, spvo_orb_octaves_link_debug): what spvo_orb_describe_octaves does on the host between the caller's list and
// orb_describe_given_kernel -- the level-0 border rule, the stable grouping by octave, the (cx, cy, level) records, the per-level counts
// -- on a list that lies where a detector left it, with its length read on the device; the describe kernel with a grid that does not
// depend on the row count; and the kernel that closes an image of a pair (slot, pinned mirrors).  tests/orb_octaves_ref.py stays the
// definition: the same list gives the same bytes as the host path, whatever the scheduling (no atomics, one workgroup, fixed order).
#pragma once
#include "orb.hip.h"

namespace spvo {

// (OrbLinkSrc: spvo_types.hip.h)
struct OrbLinkGeom { int h[ORB_LEVELS], w[ORB_LEVELS]; float lscale[ORB_LEVELS]; };   // orb_prepare's levels, bit for bit
constexpr int ORB_LINK_TOTAL = ORB_LEVELS;        // cnt[0 .. 7]: rows per level, cnt[8]: rows in all (beyond the capacity: counted, not written)
constexpr int ORB_LINK_N = ORB_LEVELS + 1;        // cnt[9]: the list's length when the caller has none of its own on the device (the test hook)
constexpr int ORB_LINK_INTS = 16;

// does record i take part, and with what?  The keep flag, then cv::ORB::compute's border rule at level 0 on coordinates rounded half to
// even, compared in float as the host code compares them (a NaN passes no comparison here and is dropped; the host path refuses it)
__device__ __forceinline__ bool orb_link_pass(const OrbLinkSrc &s, int i, int n, int rows, int cols, int max_octave, float &x, float &y, int &o) {
  x = y = 0.f; o = 0;
  if (i >= n || (s.keep && s.keep[i] == 0)) return false;
  const char *p = s.rec + (size_t)i * s.stride;
  x = *reinterpret_cast<const float *>(p + s.off_x);
  y = *reinterpret_cast<const float *>(p + s.off_y);
  o = *reinterpret_cast<const int *>(p + s.off_octave);
  if (o < 0 || o > max_octave) { o = 0; return false; }   // (no detector reports such an octave and the hook refuses it: nothing may name a level that was not built)
  const float xi = rintf(x), yi = rintf(y);
  return xi >= (float)ORB_EDGE && xi < (float)(cols - ORB_EDGE) && yi >= (float)ORB_EDGE && yi < (float)(rows - ORB_EDGE);
}

// (not list_steps.hip.h's stable_compact_walk: a base per octave, which takes a counting walk before the placing one)
// ONE workgroup, two walks over the list in chunks of 1024 (that header's walk, per octave): the first counts the passing
// records of every octave, the second gives each passing record the row first[octave] + the number of earlier passing records of its
// octave -- per-wave ballots, a [16 waves][8 octaves] table in LDS per chunk, a running base per octave.  Row r: kept[r] = the record's
// index in the list, rec[3 r ..] = (cx, cy, level) clamped into the level.
__global__ __launch_bounds__(1024) void orb_link_group_kernel(const OrbLinkSrc s, int rows, int cols, int max_octave, const OrbLinkGeom g, int cap, int *__restrict__ kept,
                                                              int *__restrict__ rec, int *__restrict__ cnt) {
  __shared__ int s_wave[16][ORB_LEVELS];
  __shared__ int s_first[ORB_LEVELS];
  __shared__ int s_h[ORB_LEVELS], s_w[ORB_LEVELS];
  __shared__ float s_scale[ORB_LEVELS];
  const int n = min(max(*s.n_ptr, 0), s.n_cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < ORB_LEVELS) { s_h[threadIdx.x] = g.h[threadIdx.x]; s_w[threadIdx.x] = g.w[threadIdx.x]; s_scale[threadIdx.x] = g.lscale[threadIdx.x]; }
  // first walk: the counts (a wave's lane 0 keeps its wave's sums)
  int acc[ORB_LEVELS] = {0};
  for (int i0 = 0; i0 < n; i0 += 1024) {
    float x, y;
    int o;
    const bool pass = orb_link_pass(s, i0 + (int)threadIdx.x, n, rows, cols, max_octave, x, y, o);
#pragma unroll
    for (int l = 0; l < ORB_LEVELS; ++l) acc[l] += __popcll(__ballot(pass && o == l));
  }
  if (lane == 0) {
#pragma unroll
    for (int l = 0; l < ORB_LEVELS; ++l) s_wave[wave][l] = acc[l];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int at = 0;
    for (int l = 0; l < ORB_LEVELS; ++l) {
      int tot = 0;
      for (int k = 0; k < 16; ++k) tot += s_wave[k][l];
      s_first[l] = at;
      cnt[l] = tot;
      at += tot;
    }
    cnt[ORB_LINK_TOTAL] = at;
  }
  __syncthreads();
  // second walk: the rows
  int base[ORB_LEVELS];
#pragma unroll
  for (int l = 0; l < ORB_LEVELS; ++l) base[l] = s_first[l];
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + (int)threadIdx.x;
    float x, y;
    int o;
    const bool pass = orb_link_pass(s, i, n, rows, cols, max_octave, x, y, o);
    unsigned long long mine = 0;
    __syncthreads();   // (the previous chunk's table, and the first walk's, have been read)
#pragma unroll
    for (int l = 0; l < ORB_LEVELS; ++l) {
      const unsigned long long m = __ballot(pass && o == l);
      if (o == l) mine = m;
      if (lane == 0) s_wave[wave][l] = __popcll(m);
    }
    __syncthreads();
    int off = 0;
#pragma unroll
    for (int l = 0; l < ORB_LEVELS; ++l) {
      int before = 0, tot = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int v = s_wave[k][l];
        before += k < wave ? v : 0;
        tot += v;
      }
      if (o == l) off = base[l] + before;
      base[l] += tot;
    }
    off += __popcll(mine & ((1ull << lane) - 1ull));
    if (pass && off < cap) {
      kept[off] = i;
      rec[3 * off] = min(max((int)rintf(__fdiv_rn(x, s_scale[o])), 0), s_w[o] - 1);
      rec[3 * off + 1] = min(max((int)rintf(__fdiv_rn(y, s_scale[o])), 0), s_h[o] - 1);
      rec[3 * off + 2] = o;
    }
  }
}

// orb_describe_given_kernel with the row count read on the device: min(cnt[ORB_LINK_TOTAL], cap) rows, a wave per row at a time (the grid is
// fixed by the capacity and strides over the rows)
__global__ __launch_bounds__(256) void orb_link_describe_kernel(const OrbLevels lv, const int *__restrict__ rec, const int *__restrict__ cnt, int cap,
                                                                const signed char *__restrict__ disc, const float *__restrict__ pattern, float *__restrict__ angle,
                                                                uint8_t *__restrict__ desc) {
  const int lane = threadIdx.x & 63;
  const int n = min(cnt[ORB_LINK_TOTAL], cap);
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {   // (wave-uniform)
    const int cx = __builtin_amdgcn_readfirstlane(rec[3 * i]), cy = __builtin_amdgcn_readfirstlane(rec[3 * i + 1]);
    const int level = __builtin_amdgcn_readfirstlane(rec[3 * i + 2]) & (ORB_LEVELS - 1);
    const OrbLevel &L = lv.l[level];
    const int h = L.h, w = L.w;
    const bool near = cx < ORB_REACH || cx >= w - ORB_REACH || cy < ORB_REACH || cy >= h - ORB_REACH;   // (the same in every lane)
    if (near) orb_describe_given_one<true>(L.im, L.blur, h, w, cx, cy, lane, disc, pattern, angle + i, desc + (size_t)i * 32);
    else orb_describe_given_one<false>(L.im, L.blur, h, w, cx, cy, lane, disc, pattern, angle + i, desc + (size_t)i * 32);
  }
}

// The last launch of an image in an ORB pair's chain: the slot's count and its 20-byte records (x, y, the extractor's angle in radians, the
// detector's response and octave) -- its 32-byte rows are where the describe kernel put them -- and the host's copy in pinned memory: the
// detector's record at kept[r] in its own layout with the extractor's radians in `angle`, and the rows, n of each.  h_n = {rows in all,
// overflow flag of the detector's candidate list}; the slot holds min(n, cap) rows.  AKAZE (stat != NULL): the flag is
// akaze_pair_finish_kernel's, and the contrast factors go to h_k.
template <class Rec>
__global__ __launch_bounds__(256) void orb_link_finish_kernel(const Rec *__restrict__ src, const int *__restrict__ kept, const int *__restrict__ cnt, const float *__restrict__ angle,
                                                              const uint4 *__restrict__ desc, int cap, const int *__restrict__ det_counters, const int *__restrict__ stat,
                                                              int cand_cap, OrbKeypoint *__restrict__ kps, int *__restrict__ d_n, int *__restrict__ h_n, int *__restrict__ h_k,
                                                              Rec *__restrict__ h_kp, uint4 *__restrict__ h_desc) {
  const int n_all = cnt[ORB_LINK_TOTAL], n = min(n_all, cap);
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  if (tid == 0) {
    *d_n = n; h_n[0] = n_all;
    if (stat) {
      h_n[1] = stat[AKAZE_STAT_OVERFLOW] || stat[AKAZE_STAT_NCAND] > cand_cap;
      for (int o = 0; o < AKAZE_MAX_OCTAVES; ++o) h_k[o] = stat[AKAZE_STAT_K + o];
    } else {
      h_n[1] = det_counters[3];
    }
  }
  for (int i = tid; i < n; i += nth) {
    Rec r = src[kept[i]];
    r.angle = angle[i];
    h_kp[i] = r;
    OrbKeypoint k;
    k.x = r.x; k.y = r.y; k.angle = r.angle; k.response = r.response; k.octave = r.octave;
    kps[i] = k;
  }
  for (int i = tid; i < n * 2; i += nth) h_desc[i] = desc[i];
}

// The other direction (spvo_orb_brisk_pair, spvo_orb_sift_pair): the ORB DETECTOR's list, where orb_describe_kernel left it, in the form the
// BRISK extractor's chain and the SIFT link read a detector's list -- what spvo_orb_detect and the host's to_keypoint do between them.
//   n        = min(sum of the eight levels' counters[l][2], kp_cap), spvo_orb_detect's `base`
//   rec[i]   = {x, y, 31 * level_scale[octave], the angle in degrees, response, octave}: the bytes of the host's conversion -- ONE float
//              multiply each for size and angle, then + 360 for a negative angle, every operation rounded on its own (mul_rn / add_rn,
//              conv_mfma.hip.h: a contracted multiply-add differs in the last bit, and HIP's __fmul_rn / __fadd_rn do not prevent one)
//   keep[i]  = 1
//   cnt      = a BRISK detector's counter block: [1] = n, [3] = the OR of the levels' overflow flags (cnt[2] = n as well)
// level_scale: the host's repeated * 1.2f, passed by value.
struct OrbLevelScale { float s[ORB_LEVELS]; };
__global__ __launch_bounds__(256) void orb_records_kernel(const OrbKeypoint *__restrict__ kps, const int *__restrict__ counters, int kp_cap, const OrbLevelScale ls,
                                                          BriskDetKeypoint *__restrict__ rec, int *__restrict__ keep, int *__restrict__ cnt) {
  int total = 0, overflow = 0;
#pragma unroll
  for (int l = 0; l < ORB_LEVELS; ++l) {
    total += counters[l * NMS_COUNTER_INTS + 2];
    overflow |= counters[l * NMS_COUNTER_INTS + 3];
  }
  const int n = min(max(total, 0), kp_cap);
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  if (tid == 0) { cnt[0] = 0; cnt[1] = n; cnt[2] = n; cnt[3] = overflow != 0; }
  for (int i = tid; i < n; i += nth) {
    const OrbKeypoint k = kps[i];
    const float deg = mul_rn(k.angle, 57.29577951308232f);
    BriskDetKeypoint r;
    r.x = k.x; r.y = k.y;
    r.size = mul_rn(31.f, ls.s[k.octave & (ORB_LEVELS - 1)]);
    r.angle = deg < 0 ? add_rn(deg, 360.f) : deg;
    r.response = k.response;
    r.octave = k.octave;
    rec[i] = r;
    keep[i] = 1;
  }
}

}  // namespace spvo
