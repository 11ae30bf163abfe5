// akaze_suppress.hip.h -- rule 11 of the AKAZE detector (tests/akaze_ref.py) on the device: the order-dependent suppression between the
// candidates akaze_refine_kernel leaves (level by level, raster order within a level), the same survivors in the same order as the host
// loop of spvo_akaze_detect (ak_suppress, spvo_akaze.hip), and the keypoint records of those whose offsets passed rule 13.
//   first loop    ONE wave walks the candidates in order: each one sees the list as its predecessors left it, in-place replacements
//                 included.  The scan of a candidate -- "the first entry, in list order, of level L or L - 1 within size^2" -- is parallel:
//                 chunks of 64 entries, a ballot per chunk, the lowest set lane of the first chunk with a hit.  Lane 0 appends, replaces
//                 in place or drops.  The list is sized by the candidate capacity of the image, far beyond LDS: its first 3072 entries
//                 are kept in LDS while the walk runs, the rest in global memory.
//                 A slot can be raised level by level, so an entry of level L - 1 may lie far before the place where level L - 1's
//                 candidates began, and a lower bound for the scan has to come from what was WRITTEN.  In the LDS part every chunk of 64
//                 entries keeps the set of levels and the range of y ever written to it, and a scan visits only the chunks that held L or
//                 L - 1 at a y the candidate can reach; in global memory it starts at the lowest position ever written with one of the two.
//   second loop   one thread per entry i scans the entries j > i of the next level, tile by tile through LDS
//   compaction    list_steps.hip.h's walk: survivors whose candidate has `ok` set, as AkazeKp records, with their number
// The candidate's position goes in WITHOUT the half-pixel shift of its octave against stored positions that carry it, and with the
// candidate's size^2; the second loop compares stored positions with entry i's size^2.  Both asymmetries are the restatement's.
// Every float operation is a separately rounded IEEE one (mul_rn / add_rn / sub_rn), as the host loop under fp contract(off).
// Worst case: quadratic in the candidates, as the host loop (no hit: every candidate scans every entry of its two levels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_mfma.hip.h"    // mul_rn, add_rn, sub_rn
#include "spvo_types.hip.h"   // AkazeLevels, AkazeCand, AkazeKp
#include "list_steps.hip.h"   // stable_compact_walk

namespace spvo {

constexpr int AKAZE_SUP_UNROLL = 4;   // chunks of 64 entries whose loads are in flight together
constexpr int AKAZE_SUP_LDS = 3072;   // entries of the list the first loop keeps in LDS (20 bytes each: 60 KB); a multiple of 64
constexpr int AKAZE_SUP_LEN = 0, AKAZE_SUP_KEPT = 1, AKAZE_SUP_INTS = 4;   // cnt: entries the first loop leaves, records the compaction writes

// (an entry of the list is a float4: x, y with the half-pixel shift, response, level as integer bits; the candidate it came from is in idx[])

// size^2 of a level, as the host loop forms it
__device__ __forceinline__ float akaze_sup_size2(const AkazeLevels &lv, int level) {
  const float size = mul_rn(lv.l[level].esigma, 1.5f);
  return mul_rn(size, size);
}

// uniform lane index: one value of a wave's register for every lane
__device__ __forceinline__ int akaze_sup_lane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float akaze_sup_lane(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// n_ptr: the number of candidates (clamped to cap).  list / idx hold cap entries.  Only esigma of lv's levels is read.
// The first AKAZE_SUP_LDS entries of the list live in LDS while the walk runs and go to global memory in one sweep at its end; entries
// beyond that are read and written in global memory directly.
__global__ __launch_bounds__(64) void akaze_suppress_first_kernel(const AkazeLevels lv, const AkazeCand *__restrict__ rec, const int *__restrict__ n_ptr, int cap, float4 *list, int *idx,
                                                                  int *__restrict__ cnt) {
  __shared__ float4 s_list[AKAZE_SUP_LDS];
  __shared__ int s_idx[AKAZE_SUP_LDS];
  static_assert(AKAZE_SUP_LDS % 64 == 0 && AKAZE_SUP_LDS / 64 <= 64 && AKAZE_MAX_LEVELS <= 32, "one lane per chunk of the LDS part, one bit per level");
  const int lane = threadIdx.x;
  // per lane, in registers: size^2 and a radius no smaller than its root of level `lane`; of chunk `lane` (64 entries) of the LDS part the
  // levels ever written to it (bit = level) and the range of the y ever written to it.  Both only grow, so they cover what the chunk holds.
  const float my_size2 = akaze_sup_size2(lv, min(lane, AKAZE_MAX_LEVELS - 1));
  const float my_rad = add_rn(mul_rn(mul_rn(lv.l[min(lane, AKAZE_MAX_LEVELS - 1)].esigma, 1.5f), 1.001f), 0.01f);
  unsigned my_mask = 0u;
  float my_ylo = 3.0e38f, my_yhi = -3.0e38f;
  const int n = min(max(*n_ptr, 0), cap);
  int len = 0, cur = -1, low_cur = 0x7FFFFFFF, low_prev = 0x7FFFFFFF;   // low_*: lowest position written with level cur / cur - 1
  for (int i0 = 0; i0 < n; i0 += 64) {
    // 64 candidates at a time, one per lane; the walk below reads them lane by lane
    const AkazeCand *p = rec + min(i0 + lane, n - 1);
    const int my_level = min(max(p->class_id, 0), AKAZE_MAX_LEVELS - 1), my_oct = min(max(p->octave, 0), 30), my_row = p->row, my_col = p->col;
    const float my_resp = p->response;
    const int m = min(64, n - i0);
    for (int j = 0; j < m; ++j) {
      const int level = akaze_sup_lane(my_level, j);
      const float ratio = (float)(1 << akaze_sup_lane(my_oct, j)), half = mul_rn(0.5f, sub_rn(ratio, 1.f));
      const float px = mul_rn((float)akaze_sup_lane(my_col, j), ratio), py = mul_rn((float)akaze_sup_lane(my_row, j), ratio), resp = akaze_sup_lane(my_resp, j);
      const float size2 = akaze_sup_lane(my_size2, level), rad = akaze_sup_lane(my_rad, level);
      if (level != cur) {
        low_prev = level == cur + 1 ? low_cur : 0x7FFFFFFF;
        low_cur = 0x7FFFFFFF;
        cur = level;
      }
      int hit = -1;
      float hit_resp = 0.f;
      // every load below is unconditional, from a clamped index; whether the entry exists goes into the predicate
      auto within = [&](const float4 &e, bool exists) {
        const int el = __float_as_int(e.w);
        const float dx = sub_rn(px, e.x), dy = sub_rn(py, e.y);
        return __ballot(exists && (el == level || el == level - 1) && add_rn(mul_rn(dx, dx), mul_rn(dy, dy)) <= size2);
      };
      // the LDS part: only the chunks that ever held level L or L - 1 and a y within the radius of the candidate's (candidates come in
      // raster order within a level and a replacement stays near its place, so a chunk spans few rows), in list order, AKAZE_SUP_UNROLL at a time
      const unsigned want = (1u << level) | (level > 0 ? 1u << (level - 1) : 0u);
      unsigned long long todo = __ballot(lane * 64 < min(len, AKAZE_SUP_LDS) && (my_mask & want) != 0u && py >= sub_rn(my_ylo, rad) && py <= add_rn(my_yhi, rad));
      while (todo && hit < 0) {
        int c[AKAZE_SUP_UNROLL];
        float4 e[AKAZE_SUP_UNROLL];
#pragma unroll
        for (int u = 0; u < AKAZE_SUP_UNROLL; ++u) {
          c[u] = todo ? __ffsll((long long)todo) - 1 : -1;
          todo &= todo - 1ull;
          e[u] = s_list[min(max(c[u], 0) * 64 + lane, AKAZE_SUP_LDS - 1)];
        }
#pragma unroll
        for (int u = 0; u < AKAZE_SUP_UNROLL; ++u) {
          const unsigned long long b = within(e[u], c[u] >= 0 && c[u] * 64 + lane < len);
          if (b && hit < 0) {
            const int src = __ffsll((long long)b) - 1;
            hit = c[u] * 64 + src;
            hit_resp = akaze_sup_lane(e[u].z, src);
          }
        }
      }
      // the part in global memory, from the lowest position written with level L - 1 or L
      for (int k0 = max(min(low_cur, low_prev) & ~63, AKAZE_SUP_LDS); k0 < len && hit < 0; k0 += 64 * AKAZE_SUP_UNROLL) {   // (nothing written yet: k0 >= len)
        float4 e[AKAZE_SUP_UNROLL];
#pragma unroll
        for (int u = 0; u < AKAZE_SUP_UNROLL; ++u) e[u] = list[min(k0 + 64 * u + lane, len - 1)];
#pragma unroll
        for (int u = 0; u < AKAZE_SUP_UNROLL; ++u) {
          const unsigned long long b = within(e[u], k0 + 64 * u + lane < len);
          if (b && hit < 0) {
            const int src = __ffsll((long long)b) - 1;
            hit = k0 + 64 * u + src;
            hit_resp = akaze_sup_lane(e[u].z, src);
          }
        }
      }
      if (hit >= 0 && !(resp > hit_resp)) continue;   // dropped
      const int slot = hit >= 0 ? hit : len;
      if (lane == 0) {
        const float4 entry = make_float4(add_rn(px, half), add_rn(py, half), resp, __int_as_float(level));
        if (slot < AKAZE_SUP_LDS) { s_list[slot] = entry; s_idx[slot] = i0 + j; }
        else { list[slot] = entry; idx[slot] = i0 + j; }
      }
      if (lane == (slot >> 6)) {   // (slots beyond the LDS part have no lane: nothing is marked)
        const float ey = add_rn(py, half);
        my_mask |= 1u << level;
        my_ylo = fminf(my_ylo, ey); my_yhi = fmaxf(my_yhi, ey);
      }
      low_cur = min(low_cur, slot);
      if (hit < 0) ++len;
      __syncthreads();   // one wave: the later scans of every lane see lane 0's entry
    }
  }
  for (int k = lane; k < min(len, AKAZE_SUP_LDS); k += 64) { list[k] = s_list[k]; idx[k] = s_idx[k]; }
  if (lane == 0) cnt[AKAZE_SUP_LEN] = len;
}

// second loop and rule 13's flag: keep[i] = 1 if entry i survives and its candidate has `ok` set.  A workgroup takes 256 entries and walks
// the list from its own first entry on in tiles of 256 through LDS (every thread reads the same entry of a tile: a broadcast).
__global__ __launch_bounds__(256) void akaze_suppress_second_kernel(const AkazeLevels lv, const AkazeCand *__restrict__ rec, const float4 *__restrict__ list, const int *__restrict__ idx,
                                                                    const int *__restrict__ cnt, int cap, int *__restrict__ keep) {
  __shared__ float4 s_tile[256];
  const int len = min(cnt[AKAZE_SUP_LEN], cap), tid = threadIdx.x;
  for (int base = blockIdx.x * 256; base < len; base += gridDim.x * 256) {   // (workgroup-uniform: the barriers below are reached by all)
    const int i = base + tid;
    const bool valid = i < len;
    const float4 a = valid ? list[i] : make_float4(0.f, 0.f, 0.f, __int_as_float(0));
    const int level = __float_as_int(a.w);
    const float size2 = akaze_sup_size2(lv, min(max(level, 0), AKAZE_MAX_LEVELS - 1));
    bool repeated = false;
    for (int t0 = base; t0 < len; t0 += 256) {
      __syncthreads();   // (the previous tile has been read)
      s_tile[tid] = t0 + tid < len ? list[t0 + tid] : make_float4(0.f, 0.f, 0.f, __int_as_float(-100));
      __syncthreads();
      if (!valid || repeated) continue;
      const int end = min(256, len - t0);
      for (int jj = max(i + 1 - t0, 0); jj < end && !repeated; ++jj) {
        const float4 b = s_tile[jj];
        if (__float_as_int(b.w) != level + 1) continue;
        const float dx = sub_rn(a.x, b.x), dy = sub_rn(a.y, b.y);
        repeated = add_rn(mul_rn(dx, dx), mul_rn(dy, dy)) <= size2 && a.z < b.z;
      }
    }
    if (valid) keep[i] = !repeated && rec[idx[i]].ok ? 1 : 0;
  }
}

// the kept entries, order-preserving: ONE workgroup walks the list (stable_compact_walk, list_steps.hip.h).
// out[k]: the record of the k-th kept candidate (its first seven fields), src[k]: that candidate's index.  cnt[AKAZE_SUP_KEPT] = their number.
__global__ __launch_bounds__(1024) void akaze_suppress_compact_kernel(const AkazeCand *__restrict__ rec, const int *__restrict__ idx, const int *__restrict__ keep, int cap,
                                                                      int *__restrict__ cnt, AkazeKp *__restrict__ out, int *__restrict__ src) {
  const int base = stable_compact_walk(
      min(cnt[AKAZE_SUP_LEN], cap), [&](int i) { return keep[i] != 0; },
      [&](int off, int i) {
        const AkazeCand c = rec[idx[i]];
        out[off] = AkazeKp{c.x, c.y, c.size, c.angle, c.response, c.octave, c.class_id};
        src[off] = idx[i];
      });
  if (threadIdx.x == 0) cnt[AKAZE_SUP_KEPT] = base;
}

// The last launch of an image in spvo_akaze_detect_pair's chain: the slot's count, its 20-byte records (x, y, the descriptor's angle,
// response, level) and its rows in the wide matcher's format (16 words: 61 bytes, then zeros), and the host's copy in pinned memory:
// count, the detector's 28-byte records with the descriptor's angle (degrees) in place of 0, the packed 61-byte rows, n of each, and the
// contrast factors.  h_n = {records the compaction kept, overflow flag of the candidate list}; the slot holds min(n, cap) rows.
__global__ __launch_bounds__(256) void akaze_pair_finish_kernel(const int *__restrict__ stat, int cand_cap, const int *__restrict__ cnt, const AkazeKp *__restrict__ crec,
                                                                const float *__restrict__ angle, const uint8_t *__restrict__ desc, int cap, OrbKeypoint *__restrict__ kps,
                                                                uint32_t *__restrict__ rows16, int *__restrict__ d_n, int *__restrict__ h_n, int *__restrict__ h_k,
                                                                AkazeKp *__restrict__ h_kp, uint8_t *__restrict__ h_desc) {
  const int n_all = cnt[AKAZE_SUP_KEPT], n = min(n_all, cap);
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  if (tid == 0) {
    *d_n = n; h_n[0] = n_all; h_n[1] = stat[AKAZE_STAT_OVERFLOW] || stat[AKAZE_STAT_NCAND] > cand_cap;
    for (int o = 0; o < AKAZE_MAX_OCTAVES; ++o) h_k[o] = stat[AKAZE_STAT_K + o];
  }
  for (int i = tid; i < n; i += nth) {
    AkazeKp r = crec[i];
    r.angle = angle[i];
    h_kp[i] = r;
    OrbKeypoint k;
    k.x = r.x; k.y = r.y; k.angle = r.angle; k.response = r.response; k.octave = r.class_id;
    kps[i] = k;
  }
  for (int i = tid; i < n * 16; i += nth) {
    const int row = i >> 4, w = i & 15;
    const uint8_t *s = desc + (size_t)row * 61 + 4 * w;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (4 * w + b < 61) v |= (uint32_t)s[b] << (8 * b);
    rows16[i] = v;
  }
  for (int i = tid; i < n * 61; i += nth) h_desc[i] = desc[i];
}

// spvo_akaze_brisk_pair: the records the compaction kept, presented as a BRISK detector's list to brisk_pair_chain_enqueue -- 24-byte
// records (x, y, size, response, octave) with every keep flag set, and its counter block (1: the list's length, 3: the overflow flag of
// the candidate list).  A record's `angle` word carries the level (class_id) as integer bits: the chain copies the word untouched into its
// compacted record, its own mirror and the slot take the extractor's angle, and akaze_brisk_finish_kernel reads the level back.
__global__ __launch_bounds__(256) void akaze_present_brisk_kernel(const int *__restrict__ stat, int cand_cap, const int *__restrict__ cnt, const AkazeKp *__restrict__ kp, int cap,
                                                                  BriskDetKeypoint *__restrict__ rec, int *__restrict__ keep, int *__restrict__ det_counters) {
  const int n = min(max(cnt[AKAZE_SUP_KEPT], 0), cap);
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  if (tid == 0) {
    det_counters[0] = 0; det_counters[1] = n; det_counters[2] = 0;
    det_counters[3] = stat[AKAZE_STAT_OVERFLOW] || stat[AKAZE_STAT_NCAND] > cand_cap;
  }
  for (int i = tid; i < n; i += nth) {
    const AkazeKp r = kp[i];
    rec[i] = BriskDetKeypoint{r.x, r.y, r.size, __int_as_float(r.class_id), r.response, r.octave};
    keep[i] = 1;
  }
}

// ... and the last launch of an image in that chain, behind brisk_pair_finish_kernel: the host's 28-byte records -- the detector's, with the
// extractor's angle (degrees) in place of 0 -- for the rows the slot holds, and the contrast factors
__global__ __launch_bounds__(256) void akaze_brisk_finish_kernel(const int *__restrict__ stat, const int *__restrict__ ext_cnt, const BriskDetKeypoint *__restrict__ crec,
                                                                 const float *__restrict__ angle, int cap, int *__restrict__ h_k, AkazeKp *__restrict__ h_kp) {
  const int n = min(ext_cnt[0], cap);
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  if (tid == 0)
    for (int o = 0; o < AKAZE_MAX_OCTAVES; ++o) h_k[o] = stat[AKAZE_STAT_K + o];
  for (int i = tid; i < n; i += nth) {
    const BriskDetKeypoint r = crec[i];
    h_kp[i] = AkazeKp{r.x, r.y, r.size, angle[i], r.response, r.octave, __float_as_int(r.angle)};
  }
}

}  // namespace spvo
