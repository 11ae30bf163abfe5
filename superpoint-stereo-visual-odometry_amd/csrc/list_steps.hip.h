// list_steps.hip.h -- the steps every detector and extractor of the front ends ends with, written once: survivors are appended to a list
// (one atomic per wave, or one per workgroup), a key list is ranked by counting, one workgroup compacts a list in order.  Each step is a
// function a kernel calls with its own data: what is kept, what is stored, capacity cuts, overflow flags and the counters that report a
// length stay in the calling kernel.  The appends return a negative slot to a thread that keeps nothing; a caller that still has its own
// flag tests that (the compiler already holds it as a mask; the slot's sign is a second compare behind the merge).
//   stable_compact_walk   cls_compact_kernel, brisk_compact_kernel / _list_kernel / brisk_pair_compact_kernel (through brisk_compact_walk_if),
//                         brisk_det_compact_kernel, akaze_suppress_compact_kernel, sift_link_compact_kernel, sift_unique_kernel
//   rank_by_counting      nms_rank_kernel, orb_rank_kernel, cls_rank_kernel
//   wave_append           orb_collect_kernel, fast_collect_kernel, brisk_collect_kernel, akaze_extrema_kernel
//   workgroup_append      nms_threshold_kernel, gftt_collect_kernel
#pragma once
#include <hip/hip_runtime.h>
#include "spvo_types.hip.h"   // RANK_TILE

namespace spvo {

// Order-preserving compaction by ONE workgroup of 1024 threads: the list is walked in chunks of 1024 with a running base; inside a chunk a
// kept index's offset is the wave ballots' prefix (LDS, 16 waves) + its lane's prefix.  keep(i) is evaluated for i < n only, by thread
// i % 1024; put(off, i) is called by the same thread right after it for every kept i (off = the number of kept indices below i), so what
// keep(i) learned may be handed to put through the caller's own variables.  Returns the number kept, the same in every thread.
// Every thread of the workgroup must call it, and once per kernel (the LDS is not guarded against a second walk).
template <typename Keep, typename Put>
__device__ __forceinline__ int stable_compact_walk(int n, Keep keep, Put put) {
  __shared__ int s_wave[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 1024) {   // (workgroup-uniform: the barriers below are reached by all)
    const int i = i0 + (int)threadIdx.x;
    const bool kp = i < n && keep(i);
    const unsigned long long m = __ballot(kp);
    __syncthreads();   // (the previous chunk's sums have been read)
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = base, tot = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int v = s_wave[k];
      off += k < wave ? v : 0;
      tot += v;
    }
    off += __popcll(m & ((1ull << lane) - 1ull));
    if (kp) put(off, i);
    base += tot;
  }
  return base;
}

// Rank by counting over 64-bit keys: rank[i] += the number of keys smaller than keys[i], for i < n (rank is zero on entry; unique keys get a
// permutation).  2-D decomposition: block (bi, bj) counts 256 keys against a RANK_TILE-key LDS tile; the workgroups of the grid's x
// dimension (256 threads each) stride over the blocks n calls for, so the grid does not depend on a capacity.
__device__ __forceinline__ void rank_by_counting(const unsigned long long *keys, int *rank, int n) {
  __shared__ __attribute__((aligned(16))) unsigned long long tile[RANK_TILE];
  const int nbi = (n + 255) / 256, nbj = (n + RANK_TILE - 1) / RANK_TILE;
  for (int b = blockIdx.x; b < nbi * nbj; b += gridDim.x) {
    const int bi = b % nbi, j0 = (b / nbi) * RANK_TILE;
    __syncthreads();
    for (int t = threadIdx.x; t < RANK_TILE; t += 256) tile[t] = (j0 + t < n) ? keys[j0 + t] : ~0ull;
    __syncthreads();
    const int i = bi * 256 + threadIdx.x;
    if (i >= n) continue;
    const unsigned long long key = keys[i];
    int cnt = 0;
    const ulonglong2 *t2 = (const ulonglong2 *)tile;
#pragma unroll 8
    for (int t = 0; t < RANK_TILE / 2; ++t) {
      const ulonglong2 v = t2[t];
      cnt += (v.x < key ? 1 : 0) + (v.y < key ? 1 : 0);
    }
    if (cnt) atomicAdd(&rank[i], cnt);
  }
}

// Append with one atomic per wave: the keepers of a wave take consecutive slots from *counter.  Returns the lane's slot, negative if it does
// not keep; the slot may lie beyond the list's capacity (the counter keeps counting): the cut and the overflow flag are the caller's.  The
// atomic is the first keeper's, so lanes that left the kernel earlier do not matter; the lanes still there must call it together.
__device__ __forceinline__ int wave_append(bool keep, int *counter) {
  const unsigned long long m = __ballot(keep);
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (m) {   // (wave-uniform: a wave without a keeper issues no atomic)
    const int first = __ffsll((long long)m) - 1;
    if (lane == first) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, first);
  }
  return keep ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}

// Append with one atomic per workgroup of 256 threads (wave ballots + an LDS prefix over the 4 waves): the keepers of a workgroup take
// consecutive slots in thread order, so a list comes out grouped by workgroup.  Returns the thread's slot, negative if it does not keep.
// Every thread of the workgroup must call it, and once per kernel.
__device__ __forceinline__ int workgroup_append(bool keep, int *counter) {
  __shared__ int s_wave[4];
  __shared__ int s_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    s_base = tot ? atomicAdd(counter, tot) : 0;
  }
  __syncthreads();
  if (!keep) return -1;
  int off = s_base + __popcll(m & ((1ull << lane) - 1ull));
  for (int k = 0; k < wave; ++k) off += s_wave[k];
  return off;
}

}  // namespace spvo
