// Stand-alone device timing of the Hamming matchers for 64-byte rows (csrc/match.hip.h): the slot matcher match_hamming_tiled_kernel<16>
// (spvo_match_hamming_slots on two BRISK slots) against match_hamming_kernel<16> (spvo_match_hamming) on the same rows, NN and NN +
// cross-check, and a check that both give the same result on every row.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/hamming_bench.hip -o tools/hamming_bench
//   usage: hamming_bench [rounds = 7] [reps = 200] [n ...  = 2000 4500]
// Per size and mode: `rounds` rounds, each timing `reps` back-to-back launches of one matcher, then of the other (alternating, device
// events around the window); printed are every round's time per match, the median and the min .. max spread of each matcher.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../superpoint-stereo-visual-odometry_amd/csrc/match.hip.h"
using namespace spvo;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main(int argc, char **argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 7, reps = argc > 2 ? atoi(argv[2]) : 200;
  std::vector<int> sizes;
  for (int i = 3; i < argc; ++i) sizes.push_back(atoi(argv[i]));
  if (sizes.empty()) sizes = {2000, 4500};
  if (rounds < 1 || reps < 1) { printf("rounds and reps must be positive\n"); return 1; }
  for (int n : sizes)
    if (n < 2 || n > (1 << HAM_SHIFT)) { printf("n must be 2 .. %d\n", 1 << HAM_SHIFT); return 1; }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int n : sizes) {
    // query rows at random; half of the train rows are query rows with up to 40 bits flipped, the others unrelated (a frame's mix of matches and clutter)
    std::mt19937 rng(1);
    std::vector<uint32_t> ha((size_t)n * 16), hb((size_t)n * 16);
    for (auto &w : ha) w = rng();
    for (auto &w : hb) w = rng();
    for (int r = 0; r < n; r += 2) {
      for (int w = 0; w < 16; ++w) hb[(size_t)r * 16 + w] = ha[(size_t)((r * 7) % n) * 16 + w];
      for (int k = 0; k < (int)(rng() % 41); ++k) { const uint32_t bit = rng() % 512; hb[(size_t)r * 16 + bit / 32] ^= 1u << (bit % 32); }
    }
    uint32_t *da, *db;
    int *dn, *idx;
    float *dist;
    int2 *out;
    unsigned long long *vote;
    CK(hipMalloc(&da, ha.size() * 4)); CK(hipMalloc(&db, hb.size() * 4)); CK(hipMalloc(&dn, 4)); CK(hipMalloc(&idx, n * 4)); CK(hipMalloc(&dist, n * 4));
    CK(hipMalloc(&out, n * sizeof(int2))); CK(hipMalloc(&vote, n * sizeof(unsigned long long)));
    CK(hipMemcpy(da, ha.data(), ha.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(db, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dn, &n, 4, hipMemcpyHostToDevice));
    const dim3 g_tiled((n + HAM_QB<16> - 1) / HAM_QB<16>), g_wave((n + 3) / 4), g_cross((n + 255) / 256);
    for (int cross = 0; cross < 2; ++cross) {
      // what spvo_match_hamming_slots / spvo_match_hamming enqueue for one match (spvo_match.hip)
      auto tiled = [&]() {
        if (cross) {
          (void)hipMemsetAsync(vote, 0xFF, (size_t)n * sizeof(unsigned long long), 0);
          hipLaunchKernelGGL(match_hamming_tiled_kernel<16>, g_tiled, dim3(256), 0, 0, db, dn, da, dn, n, 2, 0.8f, out, vote);
          hipLaunchKernelGGL(match_hamming_cross_slots_kernel, g_cross, dim3(256), 0, 0, vote, dn, n, out);
        } else {
          hipLaunchKernelGGL(match_hamming_tiled_kernel<16>, g_tiled, dim3(256), 0, 0, da, dn, db, dn, n, 0, 0.8f, out, vote);
        }
      };
      auto wave = [&]() {
        if (cross) {
          (void)hipMemsetAsync(vote, 0xFF, (size_t)n * sizeof(unsigned long long), 0);
          hipLaunchKernelGGL(match_hamming_kernel<16>, g_wave, dim3(256), 0, 0, db, n, da, n, 2, 0.8f, idx, dist, vote);
          hipLaunchKernelGGL(match_hamming_cross_kernel, g_cross, dim3(256), 0, 0, vote, n, idx, dist);
        } else {
          hipLaunchKernelGGL(match_hamming_kernel<16>, g_wave, dim3(256), 0, 0, da, n, db, n, 0, 0.8f, idx, dist, vote);
        }
      };
      // same result on every row
      tiled(); wave();
      CK(hipDeviceSynchronize());
      std::vector<int2> ho(n);
      std::vector<int> hi(n);
      std::vector<float> hd(n);
      CK(hipMemcpy(ho.data(), out, n * sizeof(int2), hipMemcpyDeviceToHost)); CK(hipMemcpy(hi.data(), idx, n * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(hd.data(), dist, n * 4, hipMemcpyDeviceToHost));
      int differ = 0, kept = 0;
      for (int i = 0; i < n; ++i) {
        float d;
        std::memcpy(&d, &ho[i].y, 4);
        differ += ho[i].x != hi[i] || d != hd[i];
        kept += hi[i] >= 0;
      }
      std::vector<float> t_tiled, t_wave;
      for (int r = -1; r < rounds; ++r) {   // round -1 warms up
        float ms[2];
        for (int which = 0; which < 2; ++which) {
          CK(hipEventRecord(e0));
          for (int i = 0; i < reps; ++i) { if (which == 0) wave(); else tiled(); }
          CK(hipEventRecord(e1));
          CK(hipEventSynchronize(e1));
          CK(hipEventElapsedTime(&ms[which], e0, e1));
        }
        CK(hipGetLastError());
        if (r < 0) continue;
        t_wave.push_back(1e3f * ms[0] / reps); t_tiled.push_back(1e3f * ms[1] / reps);
        printf("n=%d %s round %d: match_hamming_kernel<16> %.2f us, match_hamming_tiled_kernel<16> %.2f us per match\n", n, cross ? "NN+cross" : "NN", r, t_wave.back(), t_tiled.back());
      }
      auto stat = [&](std::vector<float> v, const char *name) {
        std::sort(v.begin(), v.end());
        printf("n=%d %-8s %-34s median %8.2f us  (min %.2f, max %.2f over %d rounds of %d matches)\n", n, cross ? "NN+cross" : "NN", name, v[v.size() / 2], v.front(), v.back(), rounds, reps);
        return v[v.size() / 2];
      };
      const float mw = stat(t_wave, "match_hamming_kernel<16>"), mt = stat(t_tiled, "match_hamming_tiled_kernel<16>");
      printf("n=%d %-8s slot matcher / one-wave-per-row matcher = %.3f; rows kept %d, rows that differ between the two: %d\n", n, cross ? "NN+cross" : "NN", mt / mw, kept, differ);
      if (differ) return 2;
    }
    CK(hipFree(da)); CK(hipFree(db)); CK(hipFree(dn)); CK(hipFree(idx)); CK(hipFree(dist)); CK(hipFree(out)); CK(hipFree(vote));
  }
  return 0;
}
