// Stand-alone check of csrc/launch_segments.hip.h: plain launches through launch_kernel(), and a recorded segment flushed as plain launches.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -I superpoint-stereo-visual-odometry_amd/csrc tools/launch_wrap_test.hip -o tools/launch_wrap_test
#include "launch_segments.hip.h"
#include <cstdio>
struct Args { const float *in; float *out; int n; float k; };
template <int ADD> __global__ __launch_bounds__(256) void k_struct(const Args a) { const int i = blockIdx.x * 256 + threadIdx.x; if (i < a.n) a.out[i] = a.in[i] * a.k + ADD; }
__global__ void k_plain(const float *__restrict__ in, float *__restrict__ out, int n, float k, const int *opt) { const int i = blockIdx.x * 256 + threadIdx.x; if (i < n) out[i] = in[i] + k + (opt ? 1 : 0); }
namespace spvo_int { __thread LaunchRecorder *t_rec = nullptr; }
int main() {
  const int n = 1000;
  float *a, *b, *c2;
  hipMalloc(&a, n * 4); hipMalloc(&b, n * 4); hipMalloc(&c2, n * 4);
  std::vector<float> h(n, 1.f);
  hipMemcpy(a, h.data(), n * 4, hipMemcpyHostToDevice);
  hipStream_t s; hipStreamCreate(&s);
  std::printf("plain launch...\n"); std::fflush(stdout);
  hipLaunchKernelGGL(k_plain, dim3(4), dim3(256), 0, s, a, b, n, 2.f, nullptr);
  hipLaunchKernelGGL((k_struct<3>), dim3(4), dim3(256), 0, s, Args{b, c2, n, 2.f});
  hipStreamSynchronize(s);
  hipMemcpy(h.data(), c2, n * 4, hipMemcpyDeviceToHost);
  std::printf("plain: %g (expect 9) err %s\n", h[5], hipGetErrorString(hipGetLastError()));
  spvo_int::LaunchRecorder r; r.active = true; r.stream = s; spvo_int::t_rec = &r;
  hipLaunchKernelGGL(k_plain, dim3(4), dim3(256), 0, s, a, b, n, 5.f, (const int *)nullptr);
  hipLaunchKernelGGL((k_struct<1>), dim3(4), dim3(256), 0, s, Args{b, c2, n, 3.f});
  std::printf("recorded %zu nodes\n", r.rec.nodes.size());
  spvo_int::rec_poison(); spvo_int::t_rec = nullptr;
  hipStreamSynchronize(s);
  hipMemcpy(h.data(), c2, n * 4, hipMemcpyDeviceToHost);
  std::printf("segment flushed: %g (expect 19) err %s\n", h[5], hipGetErrorString(hipGetLastError()));
  return 0;
}
