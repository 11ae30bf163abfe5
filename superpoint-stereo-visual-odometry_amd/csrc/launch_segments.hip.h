// launch_segments.hip.h -- runs of kernel launches recorded and replayed from HIP graphs (included by spvo_internal.hip.h; see below).
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include <type_traits>
// ---------------------------------------------------------------------------------------------------------------- launch segments
// The frame loop of the small engines (FP16 / INT8: BASELINE configs 3 and 5) is bound by the HOST: ~20 kernel launches per frame at
// 2.6-4 us each against ~0.1 ms of network (NOTES.md round 6; tools/graph_bench.hip: ONE hipGraphLaunch costs the host 4.7 us whatever the
// number of kernel nodes).  So a run of kernel launches on one stream between two event operations -- a SEGMENT: a group's trunk, its heads,
// a pair's heat map + NMS + sampling, its two matches -- is recorded instead of launched (the launch macro below lands here), and when the
// segment closes it is either replayed from the HIP graph its entry holds -- when the recorded launches are identical to the ones that graph
// was built from: kernels, launch dimensions, LDS sizes and argument bytes -- or launched kernel by kernel and, when it recorded the same
// launches as the last time, turned into a graph for the next time.  The enqueueing code is unchanged: every hipLaunchKernelGGL of the
// library goes through launch_kernel(), which launches at once unless a segment is open on that stream.  Anything that is not a kernel
// launch (event record / wait, copies, memsets -- also the profiler's events) inside an open segment flushes it and falls back to plain
// launches for the rest of that segment (rec_poison), so ordering is never at risk.
#include <tuple>
#include <utility>
namespace spvo_int {
struct LaunchNode { const void *func; dim3 grid, block; unsigned lds; int n_args; unsigned arg_off[32]; };
// a segment's launches as recorded: the nodes and the argument copies they point into (arg_off).  Every byte of `args` is written -- the
// gaps in front of the 16-byte aligned arguments are zero, and the argument structs have no implicit padding -- so two recordings of the
// same launches are equal byte for byte.
struct Recording {
  std::vector<LaunchNode> nodes;
  std::vector<char> args;
  void clear() { nodes.clear(); args.clear(); }
  void params(const LaunchNode &n, void **p) const {
    for (int i = 0; i < n.n_args; ++i) p[i] = const_cast<char *>(args.data()) + n.arg_off[i];
  }
  hipError_t launch(const LaunchNode &n, hipStream_t stream) const {
    void *p[32];
    params(n, p);
    return hipLaunchKernel(n.func, n.grid, n.block, p, n.lds, stream);
  }
};
inline bool operator==(const LaunchNode &a, const LaunchNode &b) {
  auto same = [](dim3 x, dim3 y) { return x.x == y.x && x.y == y.y && x.z == y.z; };
  return a.func == b.func && same(a.grid, b.grid) && same(a.block, b.block) && a.lds == b.lds && a.n_args == b.n_args &&
         std::memcmp(a.arg_off, b.arg_off, a.n_args * sizeof(unsigned)) == 0;
}
inline bool operator==(const Recording &a, const Recording &b) { return a.nodes == b.nodes && a.args == b.args; }
struct GraphEntry {
  bool never = false;          // instantiation failed once: this segment stays plain launches
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  Recording rec;               // the launches `exec` was built from; without one, the launches that went out plainly the last time
};
struct LaunchRecorder {
  bool active = false, poisoned = false;
  hipStream_t stream = nullptr;
  GraphEntry *entry = nullptr;
  Recording rec;               // the open segment
};
extern __thread LaunchRecorder *t_rec;   // (__thread, not thread_local: no dynamic-initialisation wrapper between the translation units of the library)
// the open segment's recorded launches go out one by one, in order, and what comes behind them as plain launches (not held against the
// entry: the profiler's events come and go)
inline void rec_poison() {
  LaunchRecorder *r = t_rec;
  if (!r || !r->active) return;
  for (const LaunchNode &n : r->rec.nodes) (void)r->rec.launch(n, r->stream);
  r->rec.clear();
  r->poisoned = true;
  r->active = false;
}
template <typename T> inline void rec_put_arg(Recording &r, LaunchNode &n, const T &v, bool &ok) {
  static_assert(std::is_trivially_copyable<T>::value, "kernel arguments are plain data");
  if (n.n_args >= 32) { ok = false; return; }
  const size_t at = (r.args.size() + 15) & ~(size_t)15;
  r.args.resize(at + sizeof(T));   // (zero-fills the gap in front of the argument)
  std::memcpy(r.args.data() + at, &v, sizeof(T));
  n.arg_off[n.n_args++] = (unsigned)at;
}
template <typename... KArgs, typename... Args>
inline void launch_kernel(void (*k)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args &&...a) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "kernel argument count");
  std::tuple<std::decay_t<KArgs>...> vals{static_cast<std::decay_t<KArgs>>(std::forward<Args>(a))...};
  LaunchRecorder *r = t_rec;
  if (r && r->active) {
    if (stream == r->stream) {
      LaunchNode n{(const void *)k, grid, block, (unsigned)lds, 0, {}};
      bool ok = true;
      std::apply([&](const auto &...v) { (rec_put_arg(r->rec, n, v, ok), ...); }, vals);
      if (ok) { r->rec.nodes.push_back(n); return; }
    }
    rec_poison();   // another stream inside the segment, or more than 32 arguments: plain launches from here on
  }
  void *params[sizeof...(KArgs) + 1];
  int i = 0;
  std::apply([&](auto &...v) { ((params[i++] = (void *)&v), ...); }, vals);
  (void)hipLaunchKernel((const void *)k, grid, block, params, lds, stream);
}
// stream operations that are not kernel launches close an open segment first (defined before the macros below rename the calls)
template <typename... A> inline hipError_t guarded_memset_async(A &&...a) { rec_poison(); return hipMemsetAsync(std::forward<A>(a)...); }
template <typename... A> inline hipError_t guarded_memcpy_async(A &&...a) { rec_poison(); return hipMemcpyAsync(std::forward<A>(a)...); }
template <typename... A> inline hipError_t guarded_event_record(A &&...a) { rec_poison(); return hipEventRecord(std::forward<A>(a)...); }
template <typename... A> inline hipError_t guarded_stream_wait_event(A &&...a) { rec_poison(); return hipStreamWaitEvent(std::forward<A>(a)...); }
template <typename... A> inline hipError_t guarded_stream_synchronize(A &&...a) { rec_poison(); return hipStreamSynchronize(std::forward<A>(a)...); }
}  // namespace spvo_int
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) ::spvo_int::launch_kernel(kernel, grid, block, lds, stream, ##__VA_ARGS__)
#define hipMemsetAsync ::spvo_int::guarded_memset_async
#define hipMemcpyAsync ::spvo_int::guarded_memcpy_async
#define hipEventRecord ::spvo_int::guarded_event_record
#define hipStreamWaitEvent ::spvo_int::guarded_stream_wait_event
#define hipStreamSynchronize ::spvo_int::guarded_stream_synchronize

