// spvo_core.hip -- context and submission-set life cycle, tuning switches, launch segments, profiling.  No kernel header: an edit of a
// kernel does not rebuild this unit (engine files: engine_file.h, spvo_plan.hip).
// Part of the extern "C" shim declared in include/spvo.h; the kernels live in the headers next to this file.
#include "spvo_internal.hip.h"
#include <mutex>

namespace spvo_int {

thread_local std::string g_error;  // for calls without a context
HostDiag g_diag;

int fail(spvo_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->error = buf;
  g_error = buf;
  return code;
}

int stage_id(spvo_ctx *c, const std::string &name) {
  for (size_t i = 0; i < c->stages.size(); ++i)
    if (c->stages[i].name == name) return (int)i;
  Stage s;
  s.name = name;
  c->stages.push_back(s);
  return (int)c->stages.size() - 1;
}

// ---- diagnostic switches (include/spvo.h: spvo_set_tuning).  One process-wide table, filled by explicit calls only.
namespace {
const char *const kTuningNames[] = {"winograd", "wino4", "wino4_item", "wino_narrow", "wino_dynamic", "winograd_min_tiles", "wino4_min_tiles", "merge_siblings", "heads_fused",
                                    "heads_on_net", "heads_split", "match_fused", "fp32_split", "prematch", "spin_wait", "trunk_timing", "solve_timing", "nms_first", "upload_side", "inject_launch_failure", "int8_fused", "pair_always", "preprocess_fused", "heads_keep_raw", "tail_streams", "solve_collect_first", "graphs", "solve_fuse", "solve_keep", "sift_describe_form", "sift_pair_waves_per_cu", "sift_brisk_recheck", "conv_variant", "int8_general"};
constexpr int kTuningCount = sizeof kTuningNames / sizeof kTuningNames[0];
std::mutex g_tuning_mutex;
bool g_tuning_set[kTuningCount] = {};
int g_tuning_value[kTuningCount] = {};
int tuning_index(const char *name) {
  for (int i = 0; name && i < kTuningCount; ++i)
    if (std::strcmp(name, kTuningNames[i]) == 0) return i;
  return -1;
}
}  // namespace
int tuning(const char *name, int dflt) {
  const int i = tuning_index(name);
  if (i < 0) return dflt;
  std::lock_guard<std::mutex> lock(g_tuning_mutex);
  return g_tuning_set[i] ? g_tuning_value[i] : dflt;
}

// tuning "spin_wait" = 1: the waits of the per-frame path poll their event instead of sleeping in the driver (a sleeping host thread
// pays the wake-up latency of its core at every wait).  Off by default: on the bench box it changed nothing (the waits are
// dominated by GPU time), and a ROS node should not burn a core while it waits.
bool spin_wait_enabled() { return tuning("spin_wait", 0) != 0; }
hipError_t wait_event(hipEvent_t ev) {
  if (spin_wait_enabled()) {
    for (long spins = 0; spins < 20000000; ++spins) {   // far longer than any wait of this library; then fall back to the blocking form
      const hipError_t e = hipEventQuery(ev);
      if (e != hipErrorNotReady) return e;
      __builtin_ia32_pause();
    }
  }
  return hipEventSynchronize(ev);
}

hipEvent_t get_event(spvo_ctx *c) {
  if (!c->free_events.empty()) {
    hipEvent_t e = c->free_events.back();
    c->free_events.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

void resolve_pending(spvo_ctx *c) {
  if (c->pending.empty()) return;
  for (auto &p : c->pending) {
    float ms = 0;
    (void)hipEventSynchronize(p.e1);
    if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
      c->stages[p.stage].total_ms += ms;
      c->stages[p.stage].calls += 1;
      c->stages[p.stage].flops_sum += p.flops;
      c->stages[p.stage].bytes_sum += p.bytes;
    }
    c->free_events.push_back(p.e0);
    c->free_events.push_back(p.e1);
  }
  c->pending.clear();
}

// ---------------------------------------------------------------------------------------------------------------- launch segments
// (launch_segments.hip.h, top: what they are and why)
__thread LaunchRecorder *t_rec = nullptr;

static void seg_drop(GraphEntry &e) {
  if (e.exec) (void)hipGraphExecDestroy(e.exec);
  if (e.graph) (void)hipGraphDestroy(e.graph);
  e = GraphEntry();
}

void set_release_segments(SubmitSet &s) {
  for (GraphEntry *e : {&s.seg_T[0], &s.seg_T[1], &s.seg_H[0], &s.seg_H[1], &s.seg_A, &s.seg_B}) seg_drop(*e);
}
void seg_free_all(spvo_ctx *c) {
  for (SubmitSet &s : c->sets) set_release_segments(s);
}

void seg_abort(spvo_ctx *c) {
  LaunchRecorder &r = c->rec;
  if (t_rec == &r) t_rec = nullptr;
  r.active = false; r.poisoned = false;
  r.rec.clear();
}

bool seg_begin(spvo_ctx *c, GraphEntry *e, hipStream_t stream) {
  LaunchRecorder &r = c->rec;
  if (t_rec == &r) seg_abort(c);   // (an error return between a begin and its end left it open: what it held was never launched and belongs to a failed submission)
  if (!c->use_graphs || !e || e->never || t_rec) return false;   // (with the profiler on, a segment that holds a timed stage is flushed by the stage's first event)
  r.active = true; r.poisoned = false; r.stream = stream; r.entry = e;
  r.rec.clear();
  t_rec = &r;
  return true;
}

int seg_end(spvo_ctx *c) {
  LaunchRecorder &r = c->rec;
  if (t_rec != &r) return SPVO_OK;
  t_rec = nullptr;
  const bool was_active = r.active;
  r.active = false;
  if (r.poisoned || !was_active) return SPVO_OK;   // (flushed already; what came behind went out as plain launches)
  GraphEntry &e = *r.entry;
  const size_t n = r.rec.nodes.size();
  if (n == 0) return SPVO_OK;
  if (e.exec && r.rec == e.rec) {   // the very launches the graph was built from
    if (::hipGraphLaunch(e.exec, r.stream) == hipSuccess) {
      c->stages[stage_id(c, "segment_graph_launch")].calls += 1;   // (counted with profiling off too: tests and bench.py read it)
      r.rec.clear();
      return SPVO_OK;
    }
    seg_drop(e);   // the replay failed: plain launches now, a new graph next time
  }
  // plain launches; and a graph for the next time when the same launches come by the second time in a row for this entry (launches that
  // keep changing would pay an instantiation per segment)
  const bool build = n >= 2 && r.rec == e.rec;
  if (!build) {
    if (e.exec) seg_drop(e);   // built from other launches
    e.rec = r.rec;
  }
  c->stages[stage_id(c, "segment_plain_launch")].calls += 1;
  hipError_t first_err = hipSuccess;
  for (const LaunchNode &q : r.rec.nodes) {
    const hipError_t le = r.rec.launch(q, r.stream);
    if (le != hipSuccess && first_err == hipSuccess) first_err = le;
  }
  if (first_err != hipSuccess) {   // what the enqueueing code's own hipGetLastError checks would have seen with plain launches
    r.rec.clear();
    return fail(c, SPVO_ERR_DEVICE, "kernel launch failed (%s) in a launch segment", hipGetErrorString(first_err));
  }
  if (build) {
    bool ok = ::hipGraphCreate(&e.graph, 0) == hipSuccess;
    hipGraphNode_t prev = nullptr;
    for (size_t i = 0; i < n && ok; ++i) {
      const LaunchNode &q = e.rec.nodes[i];
      void *params[32];
      e.rec.params(q, params);
      hipKernelNodeParams kp{};
      kp.func = const_cast<void *>(q.func);
      kp.gridDim = q.grid; kp.blockDim = q.block; kp.sharedMemBytes = q.lds;
      kp.kernelParams = params; kp.extra = nullptr;
      hipGraphNode_t node = nullptr;
      ok = ::hipGraphAddKernelNode(&node, e.graph, prev ? &prev : nullptr, prev ? 1 : 0, &kp) == hipSuccess;
      prev = node;
    }
    if (ok) ok = ::hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      seg_drop(e);
      e.never = true;   // this segment cannot be a graph here: never try again
    }
  }
  r.rec.clear();
  return SPVO_OK;
}

// ---------------------------------------------------------------------------------------------------------------- submission sets
// (SubmitSet, spvo_internal.hip.h.)  What every set has from spvo_create on; the rest is allocated on first use (ensure_host_sets, ensure_match, seg_end)
int set_alloc(spvo_ctx *c, int index) {
  SubmitSet &s = c->sets[index];
  const size_t hw = (size_t)c->H * c->W;
  const int cap = c->cfg.max_keypoints;
  for (hipEvent_t *e : {&s.ev_net, &s.ev_tail, &s.ev_feat, &s.ev_copy, &s.ev_pre, &s.ev_res, &s.ev_up, &s.ev_heads})
    if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return fail(c, SPVO_ERR_DEVICE, "cannot create events on device %d", c->cfg.device);
  s.d_counters = c->d_counters_all + (size_t)index * 2 * NMS_COUNTER_INTS;
  int rc = dev_alloc(c, &s.d_heat_base, 2 * hw + 128);
  if (rc) return rc;
  s.d_heat = s.d_heat_base + 64;   // K10 reads aligned float4 rows that may start left of column 0
  for (NmsBuffers &b : s.nms) {
    if ((rc = dev_alloc(c, &b.state, (size_t)(c->H + 2 * NMS_PAD) * nms_state_pitch(c->W)))) return rc;
    if ((rc = dev_alloc(c, &b.cand, hw))) return rc;
    b.counters = nullptr;   // set per submission (nms_pair)
    if ((rc = dev_alloc(c, &b.surv_key, c->surv_cap))) return rc;
    if ((rc = dev_alloc(c, &b.rank, c->surv_cap))) return rc;
    if ((rc = dev_alloc(c, &b.out_xy, (size_t)cap * 2))) return rc;
  }
  if (hipHostMalloc((void **)&s.h_counters, 2 * NMS_COUNTER_INTS * sizeof(int)) != hipSuccess ||
      hipHostMalloc((void **)&s.h_xy, (size_t)2 * cap * 2 * sizeof(float)) != hipSuccess) return fail(c, SPVO_ERR_DEVICE, "hipHostMalloc failed");
  return SPVO_OK;
}

void set_release_images(SubmitSet &s) {
  dev_free(s.d_img);
  host_free(s.h_img);
}
void set_release_match(SubmitSet &s) {
  host_free(s.h_match_out);
  s.mcache.invalidate();
}
void set_release(SubmitSet &s) {
  set_release_images(s); set_release_match(s); set_release_segments(s);
  for (NmsBuffers &b : s.nms) dev_free(b.state, b.cand, b.surv_key, b.rank, b.out_xy);
  dev_free(s.d_heat_base, s.d_resized);   // (d_heat and d_counters point into other allocations)
  host_free(s.h_counters, s.h_xy, s.h_resized, s.h_desc);
  for (hipEvent_t e : {s.ev_net, s.ev_tail, s.ev_feat, s.ev_copy, s.ev_pre, s.ev_res, s.ev_up, s.ev_heads}) if (e) (void)hipEventDestroy(e);
  s = SubmitSet();
}

}  // namespace spvo_int

// tuning "trunk_timing" = 1 (diagnostic): how long the network stream works per trunk launch and how long it stands idle between two,
// from timing events at both ends of the trunk (printed every 200 launches); > 1: one line per launch from that launch on (80 of
// them), with the host clock.  The switch is read when the context is created (spvo_create), the timing events and sums belong to the context.
void TrunkDiag::launch_begin(spvo_ctx *c, int npairs) {
  const int trace_lo = c->trunk_timing;
  const double tnow = diag_now_us();
  const bool found_idle = c->last_launch_ring >= 0 && hipEventQuery(c->sets[c->last_launch_ring].ev_net) == hipSuccess;
  if (found_idle) ++g_diag.late;   // the trunk before this one is done already: the stream is idle
  if (trace_lo > 1 && g_diag.launches + 1 >= trace_lo && g_diag.launches + 1 < trace_lo + 80)
    std::fprintf(stderr, "T %.0f launch %ld: %d pairs, stream %s, submissions so far %u, in flight %zu\n", tnow, g_diag.launches + 1, npairs, found_idle ? "IDLE" : "busy", c->submit_count, c->pendq.size());
  if (++g_diag.launches > 100 && g_diag.iv_printed < 16 && (found_idle || g_diag.iv_printed % 4 != 0)) {   // an idle launch and the three behind it
    std::fprintf(stderr, "[spvo]   launch %ld (%d pairs, stream %s): %.0f us since the previous launch, of which the host waited %.0f us for features, %.0f us for matches, %.0f us for the solver; %zu submissions in flight\n",
                 g_diag.launches, npairs, found_idle ? "IDLE" : "busy", tnow - g_diag.t_last_submit, g_diag.iv_tail, g_diag.iv_match, g_diag.iv_solve, c->pendq.size());
    ++g_diag.iv_printed;
  }
  g_diag.iv_tail = g_diag.iv_match = g_diag.iv_solve = 0;
  g_diag.depth_sum += (int)c->pendq.size();
  if (g_diag.t_last_submit > 0) g_diag.max_interval = std::max(g_diag.max_interval, tnow - g_diag.t_last_submit);
  g_diag.t_last_submit = tnow;
  if (n == 0)
    for (int r = 0; r < TT; ++r) { (void)hipEventCreate(&b[r]); (void)hipEventCreate(&e[r]); (void)hipEventCreate(&tb[r]); (void)hipEventCreate(&te[r]); }
  if (n >= TT) {   // the launches before those that may be in flight are complete: ring slots (n-8) and (n-9)
    const int r2 = (int)((n - 8) % TT), r3 = (int)((n - 9) % TT);
    float busy_ms = 0, idle_ms = 0;
    if (hipEventElapsedTime(&busy_ms, b[r2], e[r2]) == hipSuccess && hipEventElapsedTime(&idle_ms, e[r3], b[r2]) == hipSuccess) {
      busy += busy_ms; idle += idle_ms;
      late += idle_ms > 0.05f ? 1 : 0;
      max_idle = std::max(max_idle, idle_ms);
    }
    pat += (char)('0' + np[r2]);
    if (idle_ms > 0.05f) pat += idle_ms > 0.3f ? 'I' : 'i';
    if (n % 200 == 0) { std::fprintf(stderr, "[spvo]   pairs per launch (i / I: the stream stood idle > 50 / > 300 us in front of it): %s\n", pat.c_str()); pat.clear(); }
    if (trace_lo > 1) {   // device-side times of launch (n - 8), relative to the first trace line's moment
      if (!base && g_diag.launches >= trace_lo - 8) { (void)hipEventCreate(&base); (void)hipEventRecord(base, c->stream_t); (void)hipEventSynchronize(base); base_host = diag_now_us(); }
      float b0 = 0, e0 = 0, tb0 = 0, te0 = 0;
      if (base && g_diag.launches - 8 >= trace_lo && g_diag.launches - 8 < trace_lo + 80 && hipEventElapsedTime(&b0, base, b[r2]) == hipSuccess &&
          hipEventElapsedTime(&e0, base, e[r2]) == hipSuccess && hipEventElapsedTime(&tb0, base, tb[r2]) == hipSuccess && hipEventElapsedTime(&te0, base, te[r2]) == hipSuccess)
        std::fprintf(stderr, "G launch %ld (%d pairs): trunk %.0f .. %.0f, tail %.0f .. %.0f (host clock)\n", g_diag.launches - 8, np[r2], base_host + b0 * 1e3, base_host + e0 * 1e3,
                     base_host + tb0 * 1e3, base_host + te0 * 1e3);
    }
    float tail_ms = 0, lag_ms = 0;
    if (hipEventElapsedTime(&tail_ms, tb[r2], te[r2]) == hipSuccess && hipEventElapsedTime(&lag_ms, e[r2], te[r2]) == hipSuccess) { tail += tail_ms; lag += lag_ms; }
    if (n % 200 == 0) {
      std::fprintf(stderr, "[spvo] trunk timing over 200 launches (%.0f pairs): network stream busy %.1f us, idle %.1f us per launch (%d gaps above 50 us, longest %.0f us)\n",
                   pairs, busy * 1e3 / 200, idle * 1e3 / 200, late, max_idle * 1e3);
      std::fprintf(stderr, "[spvo]   NMS continuations driven by the host so far: %lld\n", c->stages[stage_id(c, "nms_redo")].calls);
      std::fprintf(stderr, "[spvo]   tail stream: %.1f us per launch from its first kernel to its last, which ends %.1f us behind the trunk\n", tail * 1e3 / 200, lag * 1e3 / 200);
      tail = lag = 0;
      std::fprintf(stderr, "[spvo]   host: longest interval between launches %.0f us, longest wait for a tail %.0f us, for a solve %.0f us, matches not served from the cache %d; "
                           "launches that found the network stream idle %d, mean submissions in flight at launch %.2f\n",
                   g_diag.max_interval, g_diag.max_tail_wait, g_diag.max_solve_wait, g_diag.match_miss, g_diag.late, g_diag.depth_sum / 200.0);
      g_diag.max_interval = g_diag.max_tail_wait = g_diag.max_solve_wait = 0; g_diag.match_miss = 0; g_diag.late = 0; g_diag.depth_sum = 0;
      busy = idle = pairs = 0; late = 0; max_idle = 0;
    }
  }
  pairs += npairs;
  np[n % TT] = npairs;
  (void)hipEventRecord(b[n % TT], c->stream);
}

// ===========================================================================
extern "C" {

void spvo_default_config(spvo_config *cfg) {
  if (!cfg) return;
  cfg->device = 0;
  cfg->net_height = 360;
  cfg->net_width = 1176;
  cfg->max_batch = 2;
  cfg->conf_thresh = 0.015f;
  cfg->dist_thresh = 4;
  cfg->border_remove = 4;
  cfg->max_keypoints = 1000;
  cfg->bug_compat_p = 1;
}

const char *spvo_last_error(const spvo_ctx *ctx) { return ctx ? ctx->error.c_str() : g_error.c_str(); }
void spvo_internal_set_error(const char *msg) { g_error = msg ? msg : ""; }   // spvo_comm.hip reports through the same channel

int spvo_create(const spvo_config *cfg, spvo_ctx **out) {
  if (!cfg || !out) return fail(nullptr, SPVO_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->net_height <= 0 || cfg->net_width <= 0 || cfg->net_height % 8 || cfg->net_width % 8)
    return fail(nullptr, SPVO_ERR_INVALID, "net size %dx%d must be positive multiples of 8 (feature_detection.hpp:296)", cfg->net_height, cfg->net_width);
  if (cfg->max_batch != 1 && cfg->max_batch != 2)
    return fail(nullptr, SPVO_ERR_INVALID, "Wrong batch size (%d)", cfg->max_batch);  // nn.cpp:490
  if (cfg->max_keypoints <= 0 || cfg->dist_thresh < 0 || cfg->dist_thresh > NMS_PAD || cfg->border_remove < 0)
    return fail(nullptr, SPVO_ERR_INVALID, "bad post-processing parameters (dist_thresh must be in [0, %d])", NMS_PAD);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, SPVO_ERR_DEVICE, "no HIP device visible: this library has no CPU path");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, SPVO_ERR_DEVICE, "device %d out of range (%d visible)", cfg->device, ndev);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return fail(nullptr, SPVO_ERR_DEVICE, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, SPVO_ERR_DEVICE, "device %d is %s; the kernels are built for gfx950 only", cfg->device, prop.gcnArchName);
  spvo_ctx *c = new spvo_ctx();
  c->cfg = *cfg;
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  c->H = cfg->net_height; c->W = cfg->net_width; c->Hc = c->H / 8; c->Wc = c->W / 8;
  c->nms_first = std::min(std::max(tuning("nms_first", 4), 1), NMS_MAX_LAUNCH);   // (diagnostic override)
  c->pair_always = tuning("pair_always", 1) != 0;
  c->trunk_timing = tuning("trunk_timing", 0);
  c->solve_timing = tuning("solve_timing", 0);
  c->inject_launch_failure = tuning("inject_launch_failure", 0);
  c->solve_fuse = tuning("solve_fuse", 1) != 0 ? 1 : 0;
  c->B = 4;   // images the activation buffers hold: two stereo pairs per trunk launch (spvo_set_trunk_pairing)
  // Non-blocking streams: work the caller puts on the NULL stream (a framework's default stream, a blocking hipMemcpy) must not
  // serialise the three streams of the pipeline against each other.  Device pointers handed to the *_dev entry points
  // have to be complete when the call is made (include/spvo.h).
  if (hipSetDevice(cfg->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&c->stream_t, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->stream_tb, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(nullptr, SPVO_ERR_DEVICE, "cannot create a stream on device %d", cfg->device);
  }
  c->post = c->stream;
  c->split_req = tuning("fp32_split", 0) != 0;
  c->int8_general_req = tuning("int8_general", 0) != 0;
  int rc = SPVO_OK;
  const size_t hw = (size_t)c->H * c->W;
  const int cap = cfg->max_keypoints;
  // one survivor per (dist+1)^2 cell at most
  const int cell = cfg->dist_thresh + 1;
  c->surv_cap = ((c->H + cell - 1) / cell) * ((c->W + cell - 1) / cell) + 64;
  do {
    if ((rc = dev_check(c, hipEventCreateWithFlags(&c->ev_post, hipEventDisableTiming), "hipEventCreate")) || (rc = dev_check(c, hipEventCreateWithFlags(&c->ev_post_b, hipEventDisableTiming), "hipEventCreate"))) break;
    if ((rc = grow(c, wait_for_nothing(), {zeroed(c->d_dense_in, c->B * hw), zeroed(c->d_det_dense, (size_t)c->B * 65 * c->Hc * c->Wc),
                                           zeroed(c->d_counters_all, (size_t)(RING + 1) * 2 * NMS_COUNTER_INTS)})))   // RING submission sets, stand-alone
      break;
    c->d_counters_alone = c->d_counters_all + (size_t)RING * 2 * NMS_COUNTER_INTS;
    for (int r = 0; r < RING && !rc; ++r) rc = set_alloc(c, r);
    if (rc) break;
    // (two lists, around the sets: the order of allocation decides where the buffers land, and is kept)
    std::vector<GrowEntry> list{zeroed(c->d_resized, 2 * hw), zeroed(c->d_tab, (size_t)3 * (c->H + c->W))};
    for (FeatureSlot &sl : c->slots)
      list.insert(list.end(), {zeroed(sl.d_xy, (size_t)cap * 2), zeroed(sl.d_desc, (size_t)cap * 256), zeroed(sl.d_n, 1), zeroed(sl.d_sqn, cap + 4)});   // K12b reads the norms four at a time
    list.insert(list.end(), {zeroed(c->d_xy_tmp, (size_t)cap * 2), zeroed(c->d_desc_tmp, (size_t)cap * 256)});
    if ((rc = grow(c, wait_for_nothing(), list))) break;
    if ((rc = ensure_match(c, cap, cap))) break;
  } while (0);
  if (rc) {
    g_error = c->error;
    spvo_destroy(c);
    return rc;
  }
  (void)hipStreamSynchronize(c->stream);
  *out = c;
  return SPVO_OK;
}

void spvo_destroy(spvo_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->cfg.device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  if (c->stream_t) (void)hipStreamSynchronize(c->stream_t);
  if (c->stream_tb) (void)hipStreamSynchronize(c->stream_tb);
  for (hipEvent_t e : c->ev_solve) if (e) (void)hipEventDestroy(e);
  if (c->ev_post) (void)hipEventDestroy(c->ev_post);
  if (c->ev_post_b) (void)hipEventDestroy(c->ev_post_b);
  resolve_pending(c);
  for (int r = 0; r < TrunkDiag::TT; ++r)
    for (hipEvent_t e : {c->tdiag.b[r], c->tdiag.e[r], c->tdiag.tb[r], c->tdiag.te[r]}) if (e) (void)hipEventDestroy(e);
  if (c->tdiag.base) (void)hipEventDestroy(c->tdiag.base);
  for (auto e : c->free_events) (void)hipEventDestroy(e);
  free_plan(c);
  for (SubmitSet &s : c->sets) set_release(s);
  classic_release(c);
  sift_release(c);
  if (c->stream_t) (void)hipStreamDestroy(c->stream_t);
  if (c->stream_tb) (void)hipStreamDestroy(c->stream_tb);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  delete c;   // frees every buffer the context owns (DevBuf / PinBuf members), its device still current
}

int spvo_set_fp32_split(spvo_ctx *c, int enable) {
  if (!c) return SPVO_ERR_INVALID;
  c->split_req = enable != 0;
  return SPVO_OK;
}

int spvo_set_int8_general(spvo_ctx *c, int enable) {
  if (!c) return SPVO_ERR_INVALID;
  c->int8_general_req = enable != 0;
  return SPVO_OK;
}

int spvo_engine_precision(const spvo_ctx *c) {
  if (!c || !c->weights) return SPVO_ERR_STATE;
  return c->int8 ? 2 : c->fp16 ? 1 : 0;
}

void *spvo_stream(spvo_ctx *c) { return c ? (void *)c->stream : nullptr; }

int spvo_synchronize(spvo_ctx *c) {
  if (!c) return fail(c, SPVO_ERR_INVALID, "null context");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream_t));
  HIP_TRY(c, hipStreamSynchronize(c->stream_tb));
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  return SPVO_OK;
}

int spvo_profile_enable(spvo_ctx *c, int on) {
  if (!c) return fail(c, SPVO_ERR_INVALID, "null context");
  if (!on) resolve_pending(c);
  c->prof = on != 0;
  return SPVO_OK;
}

int spvo_profile_only(spvo_ctx *c, const char *stage) {
  if (!c) return fail(c, SPVO_ERR_INVALID, "null context");
  resolve_pending(c);
  c->prof_only = (stage && *stage) ? stage_id(c, stage) : -1;
  return SPVO_OK;
}

int spvo_profile_reset(spvo_ctx *c) {
  if (!c) return fail(c, SPVO_ERR_INVALID, "null context");
  resolve_pending(c);
  for (auto &s : c->stages) { s.total_ms = 0; s.calls = 0; s.flops_sum = 0; s.bytes_sum = 0; }
  return SPVO_OK;
}

int spvo_profile_count(spvo_ctx *c) {
  if (!c) return 0;
  resolve_pending(c);
  return (int)c->stages.size();
}

int spvo_profile_get(spvo_ctx *c, int i, char *name, size_t name_cap, double *total_ms, long long *calls, double *flops_per_call, double *bytes_per_call) {
  if (!c || i < 0 || i >= (int)c->stages.size()) return fail(c, SPVO_ERR_INVALID, "bad stage index");
  resolve_pending(c);
  const Stage &s = c->stages[i];
  if (name && name_cap) { std::strncpy(name, s.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (total_ms) *total_ms = s.total_ms;
  if (calls) *calls = s.calls;
  // per call = the MEAN over the timed calls (so that flops / (total_ms / calls) is the rate also when launches of different batch mix)
  if (flops_per_call) *flops_per_call = s.calls ? s.flops_sum / s.calls : s.flops;
  if (bytes_per_call) *bytes_per_call = s.calls ? s.bytes_sum / s.calls : s.bytes;
  return SPVO_OK;
}

int spvo_set_tuning(const char *name, int value) {
  const int i = tuning_index(name);
  if (i < 0) return SPVO_ERR_INVALID;
  std::lock_guard<std::mutex> lock(g_tuning_mutex);
  g_tuning_set[i] = true;
  g_tuning_value[i] = value;
  return SPVO_OK;
}

int spvo_get_tuning(const char *name, int dflt) { return tuning(name, dflt); }

void spvo_clear_tuning(void) {
  std::lock_guard<std::mutex> lock(g_tuning_mutex);
  for (int i = 0; i < kTuningCount; ++i) g_tuning_set[i] = false;
}

int spvo_profile_stage_kernel(spvo_ctx *c, const char *stage, char *name, size_t name_cap, double *executed_per_algorithmic) {
  if (!c || !stage) return fail(c, SPVO_ERR_INVALID, "null argument");
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const Op &op = c->ops[i];
    if (op.stage < 0 || op.stage >= (int)c->stages.size() || c->stages[op.stage].name != stage) continue;
    const char *k = "other";
    double f = 1.0;
    if (op.type == OP_CONV) {
      if (c->int8) k = (op.fused_dw >= 0 || op.fused_stem) ? "dwpw_i8_kernel" : "conv_i8_kernel";   // (the fused block: depthwise 3x3 + pointwise 1x1 in one launch)
      else if (c->fp16) k = "conv_f16_kernel";
      else if (c->s3) { k = "conv_s3_kernel"; f = 6.0; }
      else if (op.wino4) { k = "conv_wino4_kernel"; f = 0.25; }
      else if (op.wino) { k = "conv_wino2_kernel"; f = 4.0 / 9.0; }
      else k = "conv_mfma_kernel";
    }
    if (op.type == OP_MAXPOOL && c->int8) k = "maxpool2_i8_kernel";   // (int8_general)
    if (op.type == OP_DWCONV) k = c->int8 ? "dwconv3x3_i8_kernel" : c->fp16 ? "dwconv3x3_f16_kernel" : "dwconv3x3_kernel";
    if (name && name_cap) { std::strncpy(name, k, name_cap - 1); name[name_cap - 1] = 0; }
    if (executed_per_algorithmic) *executed_per_algorithmic = f;
    return SPVO_OK;
  }
  return fail(c, SPVO_ERR_INVALID, "no layer of the loaded engine is timed under that stage name");
}

int spvo_profile_stage_variant(spvo_ctx *c, const char *stage, int info[7]) {
  if (!c || !stage || !info) return fail(c, SPVO_ERR_INVALID, "null argument");
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const Op &op = c->ops[i];
    if (op.type != OP_CONV || op.stage < 0 || op.stage >= (int)c->stages.size() || c->stages[op.stage].name != stage) continue;
    for (int q = 0; q < 7; ++q) info[q] = 0;
    const bool in_heads = c->heads_fused && i >= c->head_start;
    // (the layers that run no instance of the tiled kernels: spvo_net_*.hip, launch_conv*)
    if (op.cin > 1 && !op.merged && !op.wino && !op.wino4 && op.fused_dw < 0 && !op.fused_away && !in_heads) {
      info[0] = op.ks; info[1] = op.ck; info[2] = op.wr; info[3] = op.wc; info[4] = (op.flags & FLAG_POOL) ? 1 : 0;
      info[5] = op.launch_tiles; info[6] = op.launch_wgs;
    }
    return SPVO_OK;
  }
  return fail(c, SPVO_ERR_INVALID, "no convolution of the loaded engine is timed under that stage name");
}

int spvo_profile_stage_fused(spvo_ctx *c, const char *stage, int info[8]) {
  if (!c || !stage || !info) return fail(c, SPVO_ERR_INVALID, "null argument");
  for (int q = 0; q < 8; ++q) info[q] = 0;
  if (!std::strcmp(stage, "heads")) {
    if (!c->weights) return fail(c, SPVO_ERR_STATE, "no engine is loaded");
    if (c->heads_fused && c->heads_kind) { info[0] = 1; info[1] = c->heads_kind; info[6] = c->heads_tiles; info[7] = c->heads_wgs; }
    return SPVO_OK;
  }
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const Op &op = c->ops[i];
    if (op.type != OP_CONV || op.stage < 0 || op.stage >= (int)c->stages.size() || c->stages[op.stage].name != stage) continue;
    if (op.fused_dw >= 0 && op.launch_block) {
      info[0] = 1; info[1] = op.launch_block / 1000; info[2] = op.launch_block / 100 % 10; info[3] = op.launch_block / 10 % 10; info[4] = op.launch_block % 10;
      info[5] = op.cout / 64; info[6] = op.launch_tiles; info[7] = op.launch_wgs;
    }
    return SPVO_OK;
  }
  return fail(c, SPVO_ERR_INVALID, "no convolution of the loaded engine is timed under that stage name");
}

}  // extern "C"
