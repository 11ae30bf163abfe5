// Stand-alone timing of the matcher's kernels (csrc/match.hip.h) in the pipeline's configuration: two jobs (stereo and
// temporal match) per launch.  hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/match_bench.hip -o tools/match_bench -ldl
// usage: match_bench [n = 1000] [jobs = 2] [reps = 200] [spread = 0]   -- times the unfused form (K12a writes dt, K12b reads it back) and the
// fused form (K12a reduces each tile per row in LDS, K12m merges) and checks that both give the same matches
// usage: match_bench u8 <path of libspvo.so> [rounds = 7] [reps = 20]   -- the byte-L2 leg (MatcherType::FLANN on binary descriptors, K12u), per shape
// (2000 x 2000 and 500 x 500 rows of 32 and of 64 bytes, NN and KNN):
//   * one match through the C ABI, host wall clock, upload and result copy included: spvo_match_l2_u8 on the bytes against the route that gave the
//     same answer before it existed -- the rows expanded to float on the host (inside the timed window), then spvo_match_l2.  The library is loaded
//     with dlopen, so the other legs need no library.  Both routes must agree on every row, indices and distance bits.
//   * the kernels alone on device-resident rows (device events around `reps` x 10 launches, counts read on the device as the slot routes do):
//     match_l2u8_kernel against match_hamming_tiled_kernel on the same rows, as context -- another norm, another answer.
//   Rounds alternate between the routes; printed are the median and min .. max of every route.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <random>
#include <vector>
#include "../include/spvo.h"
#include "../superpoint-stereo-visual-odometry_amd/csrc/match.hip.h"
using namespace spvo;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

static double wall_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void print_stat(const char *what, std::vector<double> v, double *median) {
  std::sort(v.begin(), v.end());
  *median = v[v.size() / 2];
  printf("    %-58s median %9.2f us  (min %.2f, max %.2f over %zu rounds)\n", what, *median, v.front(), v.back(), v.size());
}

static int u8_leg(const char *libpath, int rounds, int reps) {
  void *lib = dlopen(libpath, RTLD_NOW | RTLD_LOCAL);
  if (!lib) { printf("dlopen %s: %s\n", libpath, dlerror()); return 1; }
  auto f_default = (decltype(&spvo_default_config))dlsym(lib, "spvo_default_config");
  auto f_create = (decltype(&spvo_create))dlsym(lib, "spvo_create");
  auto f_destroy = (decltype(&spvo_destroy))dlsym(lib, "spvo_destroy");
  auto f_l2 = (decltype(&spvo_match_l2))dlsym(lib, "spvo_match_l2");
  auto f_u8 = (decltype(&spvo_match_l2_u8))dlsym(lib, "spvo_match_l2_u8");
  if (!f_default || !f_create || !f_destroy || !f_l2 || !f_u8) { printf("%s lacks an entry point\n", libpath); return 1; }
  spvo_config cfg;
  f_default(&cfg);
  spvo_ctx *ctx = nullptr;
  if (f_create(&cfg, &ctx) != SPVO_OK) { printf("spvo_create failed\n"); return 1; }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int sizes[2] = {2000, 500}, widths[2] = {32, 64};
  for (int n : sizes)
    for (int W : widths) {
      // query rows at random; half of the train rows are query rows with a few bytes moved by a little, the others unrelated
      std::mt19937 rng(1);
      std::vector<uint8_t> ha((size_t)n * W), hb((size_t)n * W);
      for (auto &v : ha) v = (uint8_t)rng();
      for (auto &v : hb) v = (uint8_t)rng();
      for (int r = 0; r < n; r += 2) {
        std::memcpy(&hb[(size_t)r * W], &ha[(size_t)((r * 7) % n) * W], W);
        for (int k = 0; k < (int)(rng() % 9); ++k) hb[(size_t)r * W + rng() % W] += (uint8_t)(rng() % 7);
      }
      uint32_t *da, *db;
      int *dn;
      int2 *out;
      unsigned long long *vote;
      CK(hipMalloc(&da, ha.size())); CK(hipMalloc(&db, hb.size())); CK(hipMalloc(&dn, 4)); CK(hipMalloc(&out, n * sizeof(int2))); CK(hipMalloc(&vote, n * 8));
      CK(hipMemcpy(da, ha.data(), ha.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(db, hb.data(), hb.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(dn, &n, 4, hipMemcpyHostToDevice));
      for (int knn = 0; knn < 2; ++knn) {
        printf("byte-L2 %d x %d rows of %d bytes, %s\n", n, n, W, knn ? "KNN 0.8" : "NN");
        std::vector<int32_t> i_u8(n), i_f(n);
        std::vector<float> d_u8(n), d_f(n), fa((size_t)n * W), fb((size_t)n * W);
        auto route_u8 = [&]() { return f_u8(ctx, ha.data(), n, hb.data(), n, W, knn, 0, 0.8f, i_u8.data(), d_u8.data()); };
        auto route_f = [&]() {
          for (size_t i = 0; i < ha.size(); ++i) fa[i] = (float)ha[i];
          for (size_t i = 0; i < hb.size(); ++i) fb[i] = (float)hb[i];
          return f_l2(ctx, fa.data(), n, fb.data(), n, W, knn, 0, 0.8f, i_f.data(), d_f.data());
        };
        if (route_u8() != SPVO_OK || route_f() != SPVO_OK) { printf("a match failed\n"); return 1; }
        int differ = 0, kept = 0;
        for (int i = 0; i < n; ++i) { differ += i_u8[i] != i_f[i] || std::memcmp(&d_u8[i], &d_f[i], 4) != 0; kept += i_u8[i] >= 0; }
        const dim3 g_u8((n + U8L2_QT - 1) / U8L2_QT), g_ham(W == 32 ? (n + HAM_QB<8> - 1) / HAM_QB<8> : (n + HAM_QB<16> - 1) / HAM_QB<16>);
        auto kern_u8 = [&]() {
          if (W == 32) hipLaunchKernelGGL(match_l2u8_kernel<32>, g_u8, dim3(256), 0, 0, da, n, dn, db, n, dn, n, W, knn, 0.8f, out, vote);
          else hipLaunchKernelGGL(match_l2u8_kernel<64>, g_u8, dim3(256), 0, 0, da, n, dn, db, n, dn, n, W, knn, 0.8f, out, vote);
        };
        auto kern_ham = [&]() {
          if (W == 32) hipLaunchKernelGGL(match_hamming_tiled_kernel<8>, g_ham, dim3(256), 0, 0, da, dn, db, dn, n, knn, 0.8f, out, vote);
          else hipLaunchKernelGGL(match_hamming_tiled_kernel<16>, g_ham, dim3(256), 0, 0, da, dn, db, dn, n, knn, 0.8f, out, vote);
        };
        std::vector<double> t_u8, t_f, k_u8, k_ham;
        for (int r = -1; r < rounds; ++r) {   // round -1 warms up
          double t[2];
          float ms[2];
          for (int which = 0; which < 2; ++which) {
            const double t0 = wall_us();
            for (int i = 0; i < reps; ++i)
              if ((which ? route_f() : route_u8()) != SPVO_OK) { printf("a match failed\n"); return 1; }
            t[which] = (wall_us() - t0) / reps;
          }
          for (int which = 0; which < 2; ++which) {
            CK(hipEventRecord(e0));
            for (int i = 0; i < 10 * reps; ++i) { if (which) kern_ham(); else kern_u8(); }
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms[which], e0, e1));
          }
          CK(hipGetLastError());
          if (r < 0) continue;
          t_u8.push_back(t[0]); t_f.push_back(t[1]); k_u8.push_back(1e3 * ms[0] / (10 * reps)); k_ham.push_back(1e3 * ms[1] / (10 * reps));
        }
        double m_u8, m_f, mk_u8, mk_ham;
        print_stat("spvo_match_l2_u8, upload and result copy included", t_u8, &m_u8);
        print_stat("float expansion on the host + spvo_match_l2, the same", t_f, &m_f);
        print_stat("match_l2u8_kernel alone, rows resident", k_u8, &mk_u8);
        print_stat("match_hamming_tiled_kernel alone, the same rows (context)", k_ham, &mk_ham);
        printf("    float route / byte route = %.2f; byte-L2 kernel / Hamming kernel = %.2f; rows kept %d, rows on which the two routes differ: %d\n", m_f / m_u8, mk_u8 / mk_ham, kept, differ);
        if (differ) return 2;
      }
      CK(hipFree(da)); CK(hipFree(db)); CK(hipFree(dn)); CK(hipFree(out)); CK(hipFree(vote));
    }
  f_destroy(ctx);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "u8") == 0) {
    if (argc < 3) { printf("usage: match_bench u8 <path of libspvo.so> [rounds = 7] [reps = 20]\n"); return 1; }
    return u8_leg(argv[2], argc > 3 ? std::max(atoi(argv[3]), 1) : 7, argc > 4 ? std::max(atoi(argv[4]), 1) : 20);
  }
  const int n = argc > 1 ? atoi(argv[1]) : 1000, njobs = argc > 2 ? atoi(argv[2]) : 2, reps = argc > 3 ? atoi(argv[3]) : 200;
  const float spread = argc > 4 ? (float)atof(argv[4]) : 0.f;   // > 0: every descriptor = one common vector + spread x noise (near-duplicates: many rows inside every window)
  const int ldt = match_ldt(n);
  std::mt19937 rng(1);
  std::normal_distribution<float> nd;
  std::vector<float> h((size_t)4 * n * 256);
  for (int r = 0; r < 4 * n; ++r) {
    double s = 0;
    for (int k = 0; k < 256; ++k) { float v = nd(rng); if (spread > 0.f) v = std::sin(0.37f * k) + spread * v; h[(size_t)r * 256 + k] = v; s += (double)v * v; }
    for (int k = 0; k < 256; ++k) h[(size_t)r * 256 + k] /= (float)std::sqrt(s);
  }
  float *d, *sq, *dt, *bd;
  int *bi;
  int2 *out, *cand;
  int4 *meta;
  const int nt = (n + MATCH_TT - 1) / MATCH_TT;
  CK(hipMalloc(&cand, (size_t)2 * n * nt * MATCH_C * sizeof(int2))); CK(hipMalloc(&meta, (size_t)2 * n * nt * sizeof(int4)));
  CK(hipMalloc(&d, h.size() * 4)); CK(hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  CK(hipMalloc(&sq, 4 * n * 4 + 64)); CK(hipMalloc(&dt, (size_t)2 * n * ldt * 4)); CK(hipMalloc(&bd, 4 * n * 4)); CK(hipMalloc(&bi, 4 * n * 4));
  CK(hipMalloc(&out, 2 * n * sizeof(int2)));
  hipLaunchKernelGGL(row_sqnorm_kernel, dim3(n), dim3(256), 0, 0, d, 4 * n, nullptr, sq);
  MatchJobs jobs;
  for (int k = 0; k < 2; ++k) {
    MatchJob &j = jobs.j[k];
    j.A = d + (size_t)(2 * k) * n * 256; j.B = d + (size_t)(2 * k + 1) * n * 256; j.na = j.nb = n; j.na_ptr = j.nb_ptr = nullptr;
    j.nA = sq + (2 * k) * n; j.nB = sq + (2 * k + 1) * n; j.dt = dt + (size_t)k * n * ldt; j.best_d2 = bd + 2 * k * n; j.best_idx = bi + 2 * k * n;
    j.cand = cand + (size_t)k * n * nt * MATCH_C; j.meta = meta + (size_t)k * n * nt;
    j.A8 = j.B8 = nullptr; j.qA8 = j.qB8 = nullptr; j.train_best = nullptr; j.out = out + k * n;
  }
  CK(hipFuncSetAttribute((const void *)match_gemm_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, MATCH_LDS_BYTES));
  CK(hipFuncSetAttribute((const void *)match_gemm_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, MATCH_LDS_BYTES));
  const int gx = (n + MATCH_TT - 1) / MATCH_TT, gy = (n + MATCH_QT - 1) / MATCH_QT;
  const dim3 gg(8 * ((gx * gy * njobs + 7) / 8)), gr((n + 3) / 4, njobs);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  float ms;
  std::vector<int2> ho[2];
  for (int fused = 0; fused < 2; ++fused) {
    CK(hipMemset(out, 0xFF, 2 * n * sizeof(int2)));
    for (int phase = 0; phase < 3; ++phase) {
      for (int w = 0; w < 2; ++w) {   // w = 0 warms up
        CK(hipEventRecord(e0));
        for (int i = 0; i < reps; ++i) {
          if (phase != 1) {
            if (fused) hipLaunchKernelGGL((match_gemm_kernel<false, true>), gg, dim3(256), MATCH_LDS_BYTES, 0, jobs, ldt, MATCH_ERR_REL, nt, gx, gy, njobs);
            else hipLaunchKernelGGL((match_gemm_kernel<false, false>), gg, dim3(256), MATCH_LDS_BYTES, 0, jobs, ldt, 0.f, 0, gx, gy, njobs);
          }
          if (phase != 0) {
            if (fused) hipLaunchKernelGGL(match_merge_kernel<>, gr, dim3(256), sizeof(MatchRerankLds<0>), 0, jobs, nt, ldt, MATCH_ERR_REL, 1, 0, 0.8f);
            else if (n <= 1024) hipLaunchKernelGGL(match_rerank_kernel<4>, gr, dim3(256), sizeof(MatchRerankLds<4>), 0, jobs, ldt, MATCH_ERR_REL, 1, 0, 0.8f);
            else hipLaunchKernelGGL(match_rerank_kernel<0>, gr, dim3(256), sizeof(MatchRerankLds<0>), 0, jobs, ldt, MATCH_ERR_REL, 1, 0, 0.8f);
          }
        }
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
      }
      const double us = ms * 1e3 / reps, fl = 2.0 * n * n * 256 * njobs;
      const char *form = fused ? "fused  " : "unfused";
      if (phase == 0) printf("%s n=%d jobs=%d  gemm   %7.2f us  %6.1f TFLOP/s = %.3f of the fp32 MFMA peak (%d workgroups)\n", form, n, njobs, us, fl / us / 1e6, fl / us / 1e6 / 157.3, gx * gy * njobs);
      if (phase == 1) printf("%s n=%d jobs=%d  %s %7.2f us\n", form, n, njobs, fused ? "merge " : "rerank", us);
      if (phase == 2) printf("%s n=%d jobs=%d  both   %7.2f us\n", form, n, njobs, us);
    }
    ho[fused].resize(2 * n);
    CK(hipMemcpy(ho[fused].data(), out, ho[fused].size() * sizeof(int2), hipMemcpyDeviceToHost));
  }
  long cs = 0, diff = 0;
  for (int i = 0; i < njobs * n; ++i) { cs += ho[1][i].x; diff += ho[0][i].x != ho[1][i].x || ho[0][i].y != ho[1][i].y; }
  printf("checksum %ld, rows on which the two forms differ: %ld\n", cs, diff);
  return 0;
}
