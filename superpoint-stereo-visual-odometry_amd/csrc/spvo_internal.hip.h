// spvo_internal.hip.h -- what the translation units of libspvo.so share: the context (struct spvo_ctx), the execution plan's
// records, error / profiling helpers and the functions one unit offers the others.  Not installed, not part of the C ABI
// (include/spvo.h is); everything here has hidden visibility.
//
//   spvo_core.hip      context and submission-set (SubmitSet) life cycle, tuning switches, launch segments, profiling entry points
//   engine_file.h      an engine file's bytes -> records, with every check that needs the file alone (plain C++: no HIP)
//   dev_buf.h          the buffers that grow on demand: the owning pointer (Buf; here DevBuf / PinBuf) and the grow protocol (grow_list; here grow),
//                      plain C++ with the memory as a policy (no HIP)
//   spvo_plan.hip      the plan loader (spvo_load_weights) as a list of steps: records -> tensors and ops, storage classes, heads, activations,
//                      the part of preparing a layer that every engine kind shares, placement; choose_variant, free_plan
//   spvo_net_f32.hip   FP32 engines: what the loader prepares of a layer (Winograd choice, packers, the fused tail of FP32 / FP16 engines), direct +
//                      Winograd convolution launchers, the layer executor (run_ops)
//   spvo_net_f16.hip   FP16 engines                     spvo_net_s3.hip   FP32 engines in split (bf16x3) mode
//   spvo_net_i8.hip    INT8 engines (each: a layer's preparation beside its launcher -- the tiles choose_variant offers are the launcher's cases)
//   spvo_detect.hip    preprocess, heat map / NMS / sampling, the detector submissions, spvo_forward
//   spvo_classic.hip   the classic front end: ORB, Shi-Tomasi, FAST, the ORB extractor (on given keypoints, at their octaves, as a device link), the
//                      binary slots and spvo_classic_detect, preprocess without an engine
//   spvo_sift.hip      the classic front end: SIFT detector + descriptor, the extractor on given keypoints, the SIFT slots and the three pair calls that fill
//                      them (spvo_sift_detect_pair, spvo_classic_sift_pair, sift_link_pair behind the BRISK / AKAZE detectors)
//   spvo_brisk.hip     the classic front end: BRISK descriptor extractor on given keypoints and as a link of the pair calls' chains
//   spvo_brisk_detect.hip   the classic front end: BRISK keypoint detector, and its stereo-pair calls (BRISK / ORB rows into the binary slots, SIFT rows into the SIFT slots)
//   spvo_akaze.hip     the classic front end: AKAZE keypoint detector and MLDB descriptor, and its stereo-pair calls (MLDB / ORB / BRISK rows into the binary
//                      slots, SIFT rows into the SIFT slots)
//   pair_call.hip.h    the resident stereo-pair protocol all of those pair calls run through (PairCall: refusals, staging, temporal partner, prematch, the
//                      one wait, capacity rule, slot bookkeeping), with the binary slots' side of it; the SIFT slots' side is in spvo_sift.hip
//   list_steps.hip.h   the keypoint-list steps the detectors' and extractors' kernels share: append per wave / per workgroup, rank by counting, the
//                      one-workgroup order-preserving compaction (device functions that take lambdas; included by the kernel headers that use them)
//   spvo_match.hip     descriptor matching (L2, Hamming)
//   spvo_solve.hip     triangulation, PnP-RANSAC, gating, Levenberg-Marquardt, the fused solve
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <deque>
#include <functional>
#include <time.h>

#include "../../include/spvo.h"
#include "spvo_types.hip.h"
#include "engine_file.h"

#pragma GCC visibility push(hidden)
#include "dev_buf.h"   // (inside the hidden region: its types name no exported symbol)
namespace spvo { struct BriskLongPair; struct BriskShortPair; }   // brisk.hip.h
using namespace spvo;

#include "launch_segments.hip.h"

namespace spvo_int {

// where the owned buffers' memory comes from (dev_buf.h): the device's, pinned host memory
struct DevMem {
  static constexpr const char *alloc_call = "hipMalloc", *clear_call = "hipMemsetAsync";
  static int alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  static void release(void *p) { (void)hipFree(p); }
  static int clear(void *p, size_t bytes, void *stream) { return (int)hipMemsetAsync(p, 0, bytes, (hipStream_t)stream); }
};
struct PinnedMem {
  static constexpr const char *alloc_call = "hipHostMalloc";
  static int alloc(void **p, size_t bytes) { return (int)hipHostMalloc(p, bytes); }
  static void release(void *p) { (void)hipHostFree(p); }
};
template <class T> using DevBuf = Buf<T, DevMem>;
template <class T> using PinBuf = Buf<T, PinnedMem>;

constexpr int RING = 8;          // buffer sets a detector submission owns (network outputs, heat map, NMS state, counters, host mirrors)
constexpr int MAX_INFLIGHT = 6;  // detector submissions that may be queued at once (< RING - 1: the sets of the pairs just completed still serve their matches and mirrors)
constexpr int N_SLOTS = 16;      // feature slots: 8 stereo pairs (previous, current and up to six in flight)
constexpr int N_BIN_SLOTS = 10;  // binary feature slots of the classic front end (spvo_classic_detect): a ring of stereo pairs, numbered like the float slots
constexpr int N_SIFT_SLOTS = 10;   // SIFT feature slots (spvo_sift_detect_pair): a third ring of stereo pairs, numbered like the others
constexpr int SIFT_SLOT_MAX = 32768;   // rows a SIFT slot may be asked to hold
constexpr int BIN_COUNTER_INTS = 16;   // ints of an image's counter block in spvo_ctx::bin.d_cnt (= CLS_COUNTER_INTS, classic_detect.hip.h)
constexpr int HAM_KEY_SHIFT = 22;   // the tiled Hamming matcher orders (distance, row) as ONE 32-bit key: distance << 22 | row, so a slot holds at most 2^22 rows

struct Tensor {
  int ch = 0, level = 0, H = 0, W = 0, hp = 0, wp = 0;
  bool nhwc = false;  // dense [B][H][W][C] (descriptor map) instead of padded planes
  bool f16 = false;   // FP16 engines: C8 fp16 [C/8][Hp][Wp][8] instead of fp32 planes (per_image still counts floats = 4 bytes)
  bool i8 = false;    // INT8 engines: C16 int8 [C/16][Hp][Wp][16]
  bool s3 = false;    // FP32 engines in split mode: C8x3 bf16 pieces [C/8][3][Hp][Wp][8] (conv_bf16x3.hip.h)
  float scale = 0.f;  // INT8 engines: real value = q * scale (calibrated)
  float *d = nullptr;
  float *dr[RING] = {};  // network outputs only: one buffer per submission set (d == dr[0])
  size_t per_image = 0;  // floats
};

// (OP_*, FLAG_*: engine_file.h)
struct Op {
  int type = 0, in = 0, out = 0, out_c_off = 0, in_c_off = 0, cin = 0, cout = 0, ks = 0, flags = 0;
  int ck = 0, n_chunks = 0, co_tiles = 0, wr = 0, wc = 0;
  int residual = 0;  // tensor added before the last ReLU (FLAG_ADD)
  bool merged = false;     // FP32 engines: this op's output channels are computed by the previous op's launch (sibling layers
                           // that read the same tensor and write adjacent channel ranges of one tensor: convPa + convDa)
  bool wino = false;       // FP32 engines: this 3x3 layer runs a Winograd kernel: F(2x2,3x3) (conv_wino2.hip.h) unless wino4 is set
  bool wino_narrow = false;   // ... with 32 instead of 64 output channels per workgroup (layers whose 64-channel tiles would leave CUs idle)
  bool wino4 = false;      // ... the F(4x4,3x3) form (conv_wino4.hip.h: 9/16 of F(2x2)'s matrix work; pooled layers with even H and W, unpooled layers of any size)
  int wino4_item = 3;      // ... which item (conv_wino4.hip.h, ITEM; "wino4_item"): 3 = 2 with its scalar and no-result instructions cut, 2 counted operand waits + LDS-DMA from a scalar base, 1 counted operand waits only, 0 the compiler's waits (A/B runs)
  bool dominant = false;   // the op with the most FLOPs: launched under its own kernel name (TAG = 1)
  float *d_w = nullptr, *d_b = nullptr, *d_bn_scale = nullptr, *d_bn_shift = nullptr;
  int *d_sched = nullptr;      // Winograd layers (8-wave form): {8 band counters, workgroups done}, zero between launches (SPVO_WINO_DYNAMIC=0: none)
  _Float16 *d_w16 = nullptr;   // FP16 engines: pack_conv_weights_f16()
  int8_t *d_w8 = nullptr;      // INT8 engines: pack_conv_weights_i8()
  unsigned short *d_ws3 = nullptr;   // FP32 engines in split mode: pack_conv_weights_s3()
  int *d_wq32 = nullptr;       // INT8 engines, depthwise: quantised weights [C][9] as int32
  int *d_wsel = nullptr;       // INT8 engines, depthwise: the dot4 operands of the fused block kernel (conv_i8_fused.hip.h: pack_dw_wsel)
  int fused_dw = -1;           // INT8 engines, pointwise 1x1 op: index of the depthwise op in front of it that runs in the SAME launch (dwpw_i8_kernel), or -1
  bool fused_stem = false;     // ... and ops 0, 1 (the fp32 stem) as well
  bool fused_away = false;     // INT8 engines: this op's work is done by a later op's launch
  float *d_qm = nullptr;       // INT8 engines: weight scale * input scale per output channel
  float inv_s_out = 0.f, s_res = 0.f;
  float pool_m = 0.f;          // INT8 engines, stand-alone max-pool (int8_general): f32(s_in * (1 / s_out)), the kernel's one multiplier
  double flops_per_image = 0;
  int stage = -1;
  mutable int launch_tiles = 0, launch_wgs = 0;   // tiled kernels: tiles and workgroups of this op's most recent launch (spvo_profile_stage_variant)
  mutable int launch_block = 0;                   // INT8 fused block: the dwpw_i8_kernel instance of that launch, 1000 G + 100 STEM + 10 POOL + EPI (spvo_profile_stage_fused)
};

struct Stage {
  std::string name;
  double total_ms = 0;
  long long calls = 0;
  double flops = 0, bytes = 0;  // algorithmic, per call (last call's value)
  double flops_sum = 0, bytes_sum = 0;   // ... summed over the timed calls (launches of two and of four images mix under trunk pairing)
};

struct Pending { int stage; hipEvent_t e0, e1; double flops = 0, bytes = 0; };

// what every kind of feature slot keeps about its contents; the host's side of the resident-pair protocol
struct SlotState {
  int n = 0;
  bool filled = false;         // a submission / call has written (or is writing) this slot
  DevBuf<int> d_n;             // device copy of n (read by kernels enqueued before the host knows n)
  unsigned long long gen = 0;  // bumped whenever the slot is rewritten
};
// the slot is being rewritten: it holds nothing, and whatever was matched against its old contents is stale
inline void slot_rewrite(SlotState &s) { s.filled = false; s.n = 0; ++s.gen; }

struct FeatureSlot : SlotState {
  DevBuf<int> d_xy;         // [cap][2] int
  DevBuf<float> d_desc;     // [cap][256]
  DevBuf<float> d_sqn;      // [cap] squared norms of the descriptors (written by the sampler)
};

// a classic stereo image's features, resident on the device (spvo_classic_detect -> spvo_match_hamming_slots); the buffers of all
// binary slots have ONE capacity (spvo_ctx::bin.cap)
struct BinarySlot : SlotState {
  DevBuf<OrbKeypoint> d_kp;      // [cap] x, y, angle, response, octave
  DevBuf<uint32_t> d_desc;       // [cap][16] allocated for the widest row; the matcher's row format: 8 words back to back for 32-byte rows, 16 for wider ones
  int row_bytes = 32;            // width of the rows it holds: 32 (the ORB extractor), 64 (BRISK) or 61 (AKAZE: stored in 16 words, bytes 61 .. 63 zero);
                                 // two slots are matched only at one width
};

// a SIFT stereo image's features, resident on the device (spvo_sift_detect_pair -> spvo_match_l2_slots) in the L2 matcher's row format; the
// buffers of all SIFT slots have ONE capacity (spvo_ctx::sift.slot_cap)
struct SiftSlot : SlotState {
  DevBuf<float> d_desc;          // [cap][256] 128 integers as float, columns 128.. zero
  DevBuf<float> d_sqn;           // [cap] squared norms (exact integers)
  DevBuf<SiftSrc> d_src;         // [cap] candidate and angle every row came from (spvo_classic_sift_pair: its 24-byte record, a SiftKey, back to back)
};

// a match enqueued together with the detector (spvo_set_prematch); the result lives in pinned memory
struct MatchCache {
  bool valid = false;
  int slot_a = -1, slot_b = -1, selector = 0, cross = 0;
  float ratio = 0.f;
  unsigned long long gen_a = 0, gen_b = 0;
  int2 *h_out = nullptr;      // pinned [cap] packed {train_idx, distance bits}; meaningful while `valid`
  int norm = 0;               // binary slots: SPVO_NORM_HAMMING or SPVO_NORM_L2, the matcher that produced it (0 for the float owners)
};

// the two prematches of one owner (a submission set, the binary slots, the SIFT slots); slot numbers are the owner's kind of slot
struct PrematchCache {
  MatchCache e[2];            // [stereo, temporal]
  void invalidate() { for (MatchCache &m : e) m.valid = false; }
  // the stored result of exactly this match of exactly these slot contents, or NULL
  const MatchCache *find(int slot_a, int slot_b, unsigned long long gen_a, unsigned long long gen_b, int selector, int cross, float ratio, int norm = 0) const {
    for (const MatchCache &m : e)
      if (m.valid && m.slot_a == slot_a && m.slot_b == slot_b && m.gen_a == gen_a && m.gen_b == gen_b && m.selector == selector && m.cross == cross && m.ratio == ratio && m.norm == norm)
        return &m;
    return nullptr;
  }
  void record(int entry, int slot_a, int slot_b, unsigned long long gen_a, unsigned long long gen_b, int selector, int cross, float ratio, int2 *h_out, int norm = 0) {
    e[entry] = MatchCache{true, slot_a, slot_b, selector, cross, ratio, gen_a, gen_b, h_out, norm};
  }
};

// What a "stereo pair into two slots" entry point stages a call through: the pinned copy of both images, the events the host and the
// matcher wait for, the temporal partner and the call's prematches.  Works on the solver's stream.  One per family of slots (spvo_ctx::bin,
// spvo_ctx::sift); the protocol that drives it is PairCall (pair_call.hip.h), the only caller of stage and temporal_partner.
struct PairStage {
  PinBuf<uint8_t> h_img;               // pinned [2][px]: both images of a call, rows packed (px: the largest image so far)
  hipEvent_t ev_feat = nullptr, ev_match = nullptr;   // features of the last call final / its prematches landed
  int last_slot_l = -1;                // left slot of the previous call (temporal partner)
  PrematchCache mcache;
  int ensure(spvo_ctx *c, size_t px);  // the events on first use, h_img grown to images of `px` bytes
  // both images with packed rows (of a strided view only the rows' own bytes are the caller's); h_img must be the caller's to write
  void stage(const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride);
  // the previous call's left slot if it survives this call and `partner_ok` (it is filled, and whatever else its kind of slot asks), else -1
  int temporal_partner(int slot_l, int slot_r, bool partner_ok) const { return last_slot_l >= 0 && last_slot_l != slot_l && last_slot_l != slot_r && partner_ok ? last_slot_l : -1; }
  void release();
};
// one image's output struct of such an entry point (spvo_classic_features, spvo_brisk_features, spvo_akaze_features, spvo_sift_features,
// spvo_akaze_sift_features: one layout, records and rows that differ)
struct PairOut { int *n; void *kp; void *desc; int cap; };
template <class T> inline PairOut pair_out(T *o) { return PairOut{&o->n, o->kp, o->desc, o->cap}; }

struct MatchScratch {         // one set per concurrently enqueued match
  DevBuf<float> d_na, d_nb, d_best_d2;
  DevBuf<float> d_dt;         // [cap][match_ldt(cap)] approximate squared distances of every pair (K12a -> K12b; the fp8 shortlist mode)
  DevBuf<int2> d_cand;        // [cap][nt][MATCH_C] a tile's survivors per query row (fused K12a -> K12m), nt = ceil(cap / 128)
  DevBuf<int4> d_meta;        // [cap][nt] survivor count and the two smallest upper bounds per (row, tile)
  DevBuf<int> d_best_idx;
  DevBuf<unsigned long long> d_train_best;
  DevBuf<unsigned char> d_a8, d_b8;                 // fp8 copies of both sides (spvo_set_match_fp8)
  DevBuf<float2> d_qa8, d_qb8;                      // [cap] {|x - x8|, |x8|} per row of those copies: the certificate of the exact second pass
  int2 *d_out = nullptr;      // packed result, points into spvo_ctx::d_match_out
};

// One of the RING buffer sets a detector submission owns from spvo_detect*_submit until a later submission takes the set over: everything its
// tail writes, the mirrors the host reads its results from, and the events that say when.  Who may touch what:
//   the tail's kernels (behind ev_net)  nms, d_counters, d_heat, and through them h_counters, h_xy; the matches write h_match_out
//   the host                            h_counters, h_xy after ev_feat; mcache[].h_out after ev_tail; h_desc after ev_copy; h_resized after ev_res
//   the network stream                  d_img behind ev_up; d_resized (preprocess / first layer), read by the tail stream's copy behind ev_pre
// (the network outputs a tail reads are the tensors' own: Tensor::dr[set])
struct SubmitSet {
  NmsBuffers nms[2];             // per image (`counters` is filled in per use: nms_pair)
  int *d_counters = nullptr;     // [2 images][NMS_COUNTER_INTS], inside spvo_ctx::d_counters_all: zeroed by the last NMS kernel of the submission before
  float *d_heat = nullptr, *d_heat_base = nullptr;   // [2][H][W], inside d_heat_base with a 64-float guard on both sides
  int *h_counters = nullptr;     // pinned [2][NMS_COUNTER_INTS]
  float *h_xy = nullptr;         // pinned [2][cap][2]
  // host-image submissions (spvo_detect_submit): pinned staging + device copies of the two input images (ensure_host_sets: on first use, grown
  // with the image), a resized-image buffer of its own and pinned mirrors of the resized images and of the descriptors
  uint8_t *h_img = nullptr, *d_img = nullptr;   // [2][spvo_ctx::img_cap_r]
  uint8_t *d_resized = nullptr, *h_resized = nullptr;   // [2][H][W]
  float *h_desc = nullptr;       // pinned [2][cap][256]
  hipEvent_t ev_net = nullptr;   // the trunk (and the heads that went with it) of the submission's group is done: its tail may start
  // a submission's tail in two parts: ev_feat = keypoints, counts and descriptors are final (what spvo_detect_wait needs), ev_tail = the
  // matches enqueued behind them have landed too (what spvo_match_slots needs); ev_copy = the descriptors of a host-image submission have reached their pinned mirror (copy kernel behind the matches)
  hipEvent_t ev_feat = nullptr, ev_tail = nullptr, ev_copy = nullptr;
  hipEvent_t ev_pre = nullptr, ev_res = nullptr;   // first layer done (network stream) / resized images on the host (tail stream)
  hipEvent_t ev_up = nullptr;    // a queued host-image submission's upload, on the solver's stream, has landed (its preprocess kernel waits for it)
  hipEvent_t ev_heads = nullptr; // the group's heads are done (tail_streams == 2, heads on the tail stream: the second pair's stream waits for it)
  GraphEntry seg_T[2], seg_H[2], seg_A, seg_B;   // launch segments: trunk / heads per pairs in the group (the set is the group's network set); the two halves of the set's tail
  PrematchCache mcache;
  int2 *h_match_out = nullptr;   // pinned [2][cap] (ensure_match)
};

// what base.cpp:75-119 crops of an image before it resizes it to the network's size, and the resize's scale
struct CropGeom { int row_off = 0, col_off = 0, crop_rows = 0, crop_cols = 0; float scale = 1.f; };

}  // namespace spvo_int
using namespace spvo_int;

struct PendingDetect {           // one spvo_detect*_submit in flight
  CropGeom g;
  int rows = 0, cols = 0, slot_l = 0, slot_r = 0, prev_l = -1, ring = 0;
  bool rematch = false;          // the temporal partner's keypoints were redone after this submission matched against them
  int extras = 0;                // spvo_detect_submit: bit 0 resized images, bit 1 descriptors travel to the set's pinned mirrors
  bool early_res = false;        // the resized images leave for their pinned mirror behind the first layer (copy kernel on the tail stream, ev_res), under the network
  bool launched = false;         // its trunk and tail are enqueued (false: held for a partner, spvo_set_trunk_pairing)
  bool failed = false;           // its group's launch failed after the submission had been accepted: spvo_detect_wait / _collect takes it off the queue and reports that
  int img0 = 0;                  // its first image in the network's planes (0, or 2 as the second pair of a group)
  int tring = 0;                 // the set whose network outputs hold its detector / descriptor maps (its own, or its group's first)
  int ts = 0;                    // the tail stream its tail runs on (0: stream_t, 1: stream_tb)
  // preprocess fused into the first layer (conv_first_pre.hip.h): what the launch of its group needs of the submission's images
  bool pre_pending = false;
  const uint8_t *src[2] = {nullptr, nullptr};
  uint8_t *res_dst = nullptr;    // the submission's own buffer for its two resized images, or NULL (the context's)
  size_t stride = 0;
};


// tuning "trunk_timing" (diagnostic): timing events at both ends of every trunk and tail, and what is summed from them
struct TrunkDiag {
  static constexpr int TT = 16;
  hipEvent_t b[TT] = {}, e[TT] = {}, tb[TT] = {}, te[TT] = {};
  hipEvent_t base = nullptr;
  double base_host = 0, tail = 0, lag = 0, busy = 0, idle = 0, pairs = 0;
  int np[TT] = {};
  long n = 0;
  int late = 0;
  float max_idle = 0;
  std::string pat;
  // the four points of a group launch where it records (spvo_core.hip); every caller tests spvo_ctx::trunk_timing first
  void launch_begin(spvo_ctx *c, int npairs);   // the report lines, the sums from the events of the launch eight back, the trunk's begin event
  void trunk_end(hipStream_t net) { (void)hipEventRecord(e[n % TT], net); }
  void tail_begin(hipStream_t tail) { (void)hipEventRecord(tb[n % TT], tail); }
  void tail_end(hipStream_t tail) { (void)hipEventRecord(te[n % TT], tail); ++n; }
};

struct spvo_ctx {
  spvo_config cfg;
  int trunk_timing = 0, solve_timing = 0;   // diagnostic switches, read at spvo_create (spvo_set_tuning: "takes effect for contexts created afterwards")
  int inject_launch_failure = 0, launch_count = 0;   // tests of launch_group's error path: the n-th group launch of this context fails
  TrunkDiag tdiag;
  double solve_tacc[4] = {0, 0, 0, 0};
  long solve_tcalls = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // fused solve: overlaps with a detector submission in flight
  hipStream_t stream_t = nullptr;  // detector tail (heat map, NMS, sampling, matching): overlaps with the NEXT submission's network
  hipStream_t stream_tb = nullptr; // a second tail stream (tail_streams == 2): submissions alternate between the two by the parity of their set
  int tail_streams = 1;            // set by the plan loader from tuning "tail_streams" (1, or 2: opt-in for the small engines, needs GPU_MAX_HW_QUEUES >= 8)
  int ms_set = 0;                  // which set of matcher scratch enqueue_matches uses: the tail stream's index (0 for everything else)
  hipStream_t post = nullptr;      // where post-processing is enqueued right now: `stream`, or `stream_t` for a submission
  std::deque<PendingDetect> pendq;
  int held = 0;                  // submissions at the back of pendq whose trunk has not been launched yet (0 .. 2: trunk pairing)
  bool pair_trunks = false;      // spvo_set_trunk_pairing
  bool pair_always = true;       // ... the first pair of a group waits for its partner also when the network stream is idle (tuning "pair_always", read at spvo_create)
  int last_launch_ring = -1;     // the set whose ev_net belongs to the newest trunk launched
  int cur_ring = 0;                // set whose network outputs the running forward pass writes
  unsigned submit_count = 0;
  std::string error;
  bool weights = false;
  bool fp16 = false;               // the loaded engine's precision
  bool split_req = false;          // spvo_set_fp32_split / SPVO_FP32_SPLIT: FP32 engines loaded from now on run on the bf16x3 kernels
  bool s3 = false;                 // the loaded FP32 engine runs in split mode
  bool int8_general_req = false;   // spvo_set_int8_general / tuning "int8_general": INT8 engines loaded from now on accept a stand-alone max-pool and a cin of 16 more than a multiple of 32
  size_t head_start = 0;           // ops [head_start, end) = the 1x1 heads + L2 norm: a submission runs them on the tail stream
  int launch_tiles = 0, launch_wgs = 0;   // what the tiled kernels' launchers (launch_conv*_instance) last enqueued; launch_op copies them to its op
  int launch_block = 0;                   // ... and launch_dwpw8_instance: its instance (Op::launch_block)
  int heads_kind = 0, heads_tiles = 0, heads_wgs = 0;   // the fused tail's most recent launch (launch_heads, launch_heads8): 1 = heads_fused_kernel<false>, 2 = <true>, 3 = heads_i8_kernel
  // launch segments replayed from HIP graphs (launch_segments.hip.h; the entries are the sets': SubmitSet::seg_*): on for FP16 / INT8 engines (tuning "graphs": 0 off, 2 on for every engine)
  bool use_graphs = false;
  LaunchRecorder rec;
  bool heads_fused = false;        // ... as ONE launch (heads.hip.h): FP32 engines whose tail is convPb (256 -> 65), convDb (256 -> 256), L2 norm
  bool heads_keep_raw = false;     // the fused launch also stores the un-normalised descriptor planes (spvo_forward / spvo_debug_tensor)
  float *d_heads_w = nullptr;      // pack_heads_weights()
  int8_t *d_heads_w8 = nullptr;    // INT8 engines (heads_i8.hip.h): pack_heads_weights_i8(), ...
  float *d_heads_qm = nullptr, *d_heads_b = nullptr;   // ... and per output channel of the 21 units: weight scale x input scale of its branch, bias
  bool int8 = false;
  int H = 0, W = 0, Hc = 0, Wc = 0, B = 0;
  int num_cus = 256;

  std::vector<Tensor> tensors;
  std::vector<Op> ops;
  int t_input = 0, t_det = 0, t_desc = 0;
  int last_batch = 0;

  // post-processing buffers
  DevBuf<float> d_dense_in;      // [B][H][W] staging for spvo_forward
  DevBuf<float> d_det_dense;     // [B][65][Hc][Wc]
  int surv_cap = 0;
  int nms_first = 4;             // NMS launches enqueued with a submission: nms_first - 1 round launches (4 in-kernel rounds each) + the finishing kernel; what that leaves undecided is continued by the host (nms_settle)
  DevBuf<uint8_t> d_img[2];      // the stand-alone entry points' staging for two input images, grown with them
  DevBuf<uint8_t> d_resized;     // [2][H][W]
  DevBuf<int> d_tab;             // resize tables: xi,xa0,xa1 [W] ; yi,yb0,yb1 [H]
  int tab_rows = -1, tab_cols = -1;
  FeatureSlot slots[N_SLOTS];
  DevBuf<int> d_xy_tmp;          // [cap][2] for spvo_sample_descriptors
  DevBuf<float> d_desc_tmp;      // [cap][256]
  int last_slot_l = -1;          // left slot of the previous submission (temporal partner)

  // matching scratch
  int match_cap = 0;
  DevBuf<float> d_ma, d_mb;
  MatchScratch ms[2][2];         // [tail stream][stereo, temporal]
  DevBuf<int2> d_match_out;      // [2][cap]: both jobs' results leave in one copy
  PinBuf<int2> h_match_tmp;      // pinned [cap] for the synchronous entry points
  DevBuf<int> d_counters_all;    // [RING sets + 1 stand-alone block][2 images][NMS_COUNTER_INTS]: ONE zeroed allocation (a tail zeroes the block of the set behind it)
  int *d_counters_alone = nullptr;   // ... its last block: the stand-alone entry points' (standalone(), below)
  SubmitSet sets[RING];          // submission n works in sets[n % RING]
  size_t img_cap_r = 0;          // bytes per image in the sets' h_img / d_img
  bool host_sets_ready = false;  // d_resized / h_resized / h_desc of EVERY set are allocated
  hipEvent_t ev_post = nullptr, ev_post_b = nullptr;    // PostScope: orders a synchronous entry point behind what is left on the tail stream(s)
  bool match_fp8 = false;        // fp8 shortlist GEMM (approximate; spvo_set_match_fp8)
  int match_form[4] = {0, 0, 0, 0};   // {fp8, fused, NCH of the re-rank, jobs} of the most recent enqueue_matches (spvo_match_last_form); jobs = 0: none yet
  bool prematch = false;
  int pm_selector = SPVO_SELECT_KNN, pm_cross = 0;
  float pm_ratio = 0.8f;

  // odometry scratch
  int odo_cap = 0, ransac_cap = 0, obs_cap = 0;
  DevBuf<double> d_P;            // Pl[12], Pr[12], K[9], prior[6], start[7]
  DevBuf<float> d_pts_a, d_pts_b, d_xyz;
  struct RansacBufs {            // RansacWork's buffers, and the record the kernels take of them
    DevBuf<int> counts, inliers;
    DevBuf<double> poses, result;
    RansacWork work() const { return RansacWork{counts, poses, result, inliers}; }
  } rw;
  DevBuf<ObsDev> d_obs;
  DevBuf<RefineOut> d_refine;
  // ORB detector / extractor of the classic front end (orb.hip.h): buffers grow on demand
  struct OrbBufs {
    size_t pyr_cap = 0;       // bytes per pyramid buffer (all levels side by side), key / rank entries, resize-table ints the buffers hold:
    size_t key_cap = 0;       // each is compared with what an image NEEDS (they depend on rows and cols separately, not on rows x cols)
    size_t tab_cap = 0;
    int kp_cap = 0;
    DevBuf<uint8_t> im, score, blur, src;   // im: all pyramid levels back to back; src: the strided upload's staging, of its own size
    DevBuf<float> tmp, pattern, taps;
    DevBuf<unsigned long long> keys;
    DevBuf<int> rank, out_xy, counters, tab;
    DevBuf<signed char> disc;
    DevBuf<OrbKeypoint> kps;
    DevBuf<uint8_t> desc;
    int tab_rows = 0, tab_cols = 0;   // image size the resize tables in `tab` belong to
    // spvo_orb_brisk_pair / spvo_orb_sift_pair (orb_records_kernel, orb_link.hip.h): the detector's list as the BRISK extractor's chain and the
    // SIFT link read one -- 24-byte records, keep flags, a BRISK detector's counter block, the chain's compacted records -- `rec_cap` of each
    int rec_cap = 0;
    DevBuf<BriskDetKeypoint> rec, crec;
    DevBuf<int> rec_keep, rec_cnt;
  } orb;
  // Shi-Tomasi / FAST detectors and the ORB extractor for given keypoints (classic_detect.hip.h): one image resident at a time,
  // buffers grow with the image (per-pixel ones with rows x cols, the state map with its padded shape) and the keypoint list
  struct ClassicBufs {
    size_t px_cap = 0, state_cap = 0;
    int kp_cap = 0;
    int rows = 0, cols = 0;               // shape of the image in `im` (0: none resident)
    unsigned image_gen = 0;               // bumped whenever `im` is about to receive another image (cls_ensure): who caches results about `im` compares it
    int state_rows = 0, state_cols = 0;   // shape the state map's padding was cleared for
    DevBuf<uint8_t> im, score, blur, src, state, desc;
    DevBuf<float> tmp, lam, xy, resp;
    DevBuf<unsigned long long> keys;
    DevBuf<int> rank, cand, counters, kp_xy;
    DevBuf<OrbKeypoint> kps;
    int oct_cap = 0;                      // spvo_orb_describe_octaves: rows its three buffers hold -- records (cx, cy, level) in output order,
    DevBuf<int> oct_rec;                  // the directions and the 32-byte rows
    DevBuf<float> oct_angle;
    DevBuf<uint8_t> oct_desc;
    // the device link of orb_link.hip.h (spvo_brisk_orb_pair, spvo_akaze_orb_pair, spvo_orb_octaves_link_debug): `lnk_cap` rows of source
    // indices, (cx, cy, level) records and directions, the counts (ORB_LINK_*), and the test hook's own list and rows
    int lnk_cap = 0, lnk_src_cap = 0;
    DevBuf<int> lnk_kept, lnk_rec, lnk_cnt, lnk_src, lnk_keep;
    DevBuf<float> lnk_angle;
    DevBuf<uint8_t> lnk_desc;
    DevBuf<uint8_t> pre_out;              // spvo_preprocess of a context without an engine (the classic front end at a fixed input size): resized image,
    DevBuf<int> pre_tab;                  // resize tables of the crop pre_crop_rows x pre_crop_cols
    int pre_crop_rows = 0, pre_crop_cols = 0;
    int last_counters[16] = {0};          // the counter block of the last spvo_gftt_detect (rounds, undecided after each launch)
  } cls;
  // spvo_classic_detect / spvo_match_hamming_slots: the binary slots, the call's pinned staging and mirrors, the matcher's vote scratch and
  // the two matches enqueued with the detector (spvo_set_prematch).  Everything is sized by `cap` rows and lives on the solver's stream.
  struct BinaryBufs {
    int cap = 0;
    BinarySlot slots[N_BIN_SLOTS];
    PairStage pair;                      // (its prematches' slot numbers are BINARY slots)
    PinBuf<OrbKeypoint> h_kp;            // pinned [2][cap]      what the finishing kernel of an image writes for the host:
    PinBuf<uint8_t> h_desc;              // pinned [2][cap][64]  keypoint records, descriptors ([2][cap][32] in its front part for the 32-byte kinds),
    PinBuf<int> h_n;                     // pinned [2][4]        {rows found, overflow flag of the detector}; behind them [2][4] the contrast factors spvo_akaze_detect_pair reports
    PinBuf<BriskDetKeypoint> h_bkp;      // pinned [2][cap]      spvo_brisk_detect_pair's records (24 bytes: they carry a size), in the place of h_kp
    PinBuf<AkazeKp> h_akp;               // pinned [2][cap]      spvo_akaze_detect_pair's records (28 bytes: size and level), in the place of h_kp
    DevBuf<int> d_cnt;                   // [2][CLS_COUNTER_INTS] the extractor's counter block per image (0: kept in all, 2: kept and described)
    DevBuf<int> d_kxy;                   // [cap][2] the kept keypoints of a Shi-Tomasi / FAST image (cls_compact_kernel), ...
    DevBuf<float> d_kresp;               // [cap]    ... and the detector's responses of those (also brisk_compact_list_kernel's)
    DevBuf<unsigned long long> d_vote;   // [cap] cross-check votes
    PinBuf<int2> h_match;                // pinned [3][cap]: the two prematches, the synchronous call
  } bin;
  // BRISK extractor for given keypoints (brisk.hip.h) on the image resident in `cls`: the pattern tables (uploaded on the first call), the
  // integral image, the keypoint list with its results and their pinned mirrors; buffers grow on demand
  struct BriskBufs {
    DevBuf<float> points;                 // [64][1024][60][3] x, y, sigma
    DevBuf<BriskLongPair> long_pairs;
    DevBuf<BriskShortPair> short_pairs;
    bool tables_ready = false;            // set last: every table above is on the device, cnt and h_n exist
    DevBuf<int> cnt;                      // [4]: kept keypoints
    DevBuf<int> integ;                    // (rows + 1) x (cols + 1), or what a larger image before needed
    int kp_cap = 0, v0_cap = 0;           // rows the keypoint buffers / the values0 buffers (test hook: allocated on demand) hold
    DevBuf<float> xy, size, angle;
    DevBuf<int> kept, kscale, values0;
    DevBuf<uint8_t> desc;
    PinBuf<int> h_n, h_kept, h_values0;   // pinned: what brisk_finish_kernel writes for the host
    PinBuf<float> h_angle;
    PinBuf<uint8_t> h_desc;
  } brisk;
  // BRISK detector (brisk_detect.hip.h) on the image resident in `cls` (its layer 0): layers 1-5, the score maps of all six and the 5-8
  // map of layer 0 (what spvo_brisk_detect_debug_layer serves until the next call), the area taps of the shape, the candidate lists --
  // sized from the image (a candidate per interior pixel of every layer), grown on demand
  struct BriskDetBufs {
    int rows = 0, cols = 0;               // shape the layout, the tables and (after a call) the maps belong to (0: none)
    bool valid = false;                   // the maps of a completed spvo_brisk_detect are on the device ...
    unsigned image_gen = 0;               // ... and belong to the image spvo_ctx::cls held at this generation
    size_t px_cap = 0, tab_cap = 0;       // bytes of pyr / score each; entries of tabs
    int cand_cap = 0;                     // candidates the lists hold (>= what the shape can yield: an interior pixel each)
    DevBuf<uint8_t> pyr, score;
    DevBuf<BriskAreaTap> tabs;
    std::vector<BriskAreaTap> h_tabs;
    DevBuf<unsigned long long> keys;
    DevBuf<int> rank, keep, counters;
    DevBuf<BriskDetKeypoint> rec, out;
    BriskDetLayers lv{};
    BriskResizeJob jobs[BRISK_DET_LAYERS]{};   // jobs[i]: layer i from its source (i >= 1)
  } brisk_det;
  // AKAZE detector (akaze.hip.h) on the image resident in `cls`: the six planes of every level (the four spvo_akaze_debug_level serves until
  // the next call, and the scaled first derivatives Lx, Ly that spvo_akaze_describe samples), two scratch planes of the image's size (the
  // contrast factor's sigma 1 blur; the second buffer of the diffusion steps), the area taps of the octaves that are no exact halves, the
  // candidate lists -- sized from the image, grown on demand -- the tables, and the descriptor's keypoint, angle and row buffers
  struct AkazeBufs {
    int rows = 0, cols = 0;               // shape the layout and the tables belong to (0: none)
    bool valid = false;                   // the planes of a completed spvo_akaze_detect are on the device ...
    unsigned image_gen = 0;               // ... and belong to the image spvo_ctx::cls held at this generation
    size_t plane_cap = 0, scratch_cap = 0, tab_cap = 0;   // floats of planes / scratch; entries of tabs
    int cand_cap = 0;
    DevBuf<float> planes, scratch;
    DevBuf<BriskAreaTap> tabs;
    std::vector<BriskAreaTap> h_tabs;
    const BriskAreaTap *xtab[AKAZE_MAX_OCTAVES] = {nullptr}, *ytab[AKAZE_MAX_OCTAVES] = {nullptr};   // of octave o from o - 1 (NULL: the exact half)
    DevBuf<unsigned long long> keys;
    DevBuf<int> rank, stat;                 // stat: AKAZE_STAT_* (spvo_types.hip.h)
    DevBuf<AkazeCand> rec;
    std::vector<AkazeCand> h_cand;
    AkazeLevels lv{};
    int octaves = 0, nsteps[AKAZE_MAX_LEVELS] = {0};   // nsteps[i]: diffusion steps of the transition i - 1 -> i
    std::vector<float> h_tau;                          // their sizes, transition after transition
    AkazeTaps g0{}, g1{};                              // sigma 1.6 and sigma 1
    float k[AKAZE_MAX_OCTAVES] = {0};                  // the last call's contrast factor per octave
    DevBuf<AkazeKp> d_kp;                              // spvo_akaze_describe (akaze_mldb.hip.h): records in, angles and 61-byte rows out
    DevBuf<float> d_angle;
    DevBuf<uint8_t> d_desc;
    int kp_cap = 0;
    std::vector<float> h_angle;                        // host staging of a call's results
    std::vector<uint8_t> h_desc;
    // rule 11 on the device (akaze_suppress.hip.h; spvo_akaze_detect_pair, spvo_akaze_suppress_debug): the list of the first loop and the
    // candidate of every entry, the keep flags, the compacted records with their candidates' indices, and the counts
    int sup_cap = 0;
    DevBuf<float4> sup_list;
    DevBuf<int> sup_idx, sup_keep, sup_src, sup_cnt;   // sup_cnt: AKAZE_SUP_*
    DevBuf<AkazeKp> sup_kp;
    // spvo_akaze_brisk_pair: the kept records as the BRISK extractor's chain reads a detector's list (brisk_pair_chain_enqueue) -- records,
    // keep flags, the counter block, the compacted records -- `brk_cap` of each
    int brk_cap = 0;
    DevBuf<BriskDetKeypoint> brk_rec, brk_crec;
    DevBuf<int> brk_keep, brk_cnt;
  } akaze;
  // SIFT detector + descriptor of the classic front end (sift.hip.h): the image, its pyramid (all Gaussian and DoG levels: what
  // spvo_sift_debug_level serves until the next call), the candidate and output lists; device buffers grow on demand, the host staging keeps its capacity
  struct SiftBufs {
    int rows = 0, cols = 0;               // shape of the image whose pyramid is resident (0: none)
    SiftPyr plan{};
    bool gauss_only = false;              // the resident pyramid is spvo_sift_describe's: Gaussian levels only, octave index 0 = octave `first`
    int first = -1;
    DevBuf<SiftKey> given_kp;             // spvo_sift_describe: the caller's records and their rows, `given_cap` of each
    DevBuf<float> given_desc;
    int given_cap = 0;
    int cand_cap = 0;                     // candidates, and output rows, the lists hold
    DevBuf<uint8_t> img;
    DevBuf<float> pyr, desc;
    DevBuf<int4> cand_pos;                // {octave, layer (0: rejected), row, column}
    DevBuf<float4> cand_off;              // {xi, xr, xc, contrast}
    DevBuf<int2> kp;                      // {candidate, angle bits}
    DevBuf<int> counters;                 // [4]: candidates, output rows
    std::vector<int4> h_pos;
    std::vector<float4> h_off;
    std::vector<int2> h_kp;
    std::vector<float> h_desc;
    std::vector<spvo_sift_keypoint> h_rec;
    std::vector<int> h_order;
    // the ordering stage on the device (sift.hip.h: spvo_sift_detect_pair, spvo_sift_order_debug), `ord_cap` raw rows
    int ord_cap = 0;
    DevBuf<SiftKey> keys;
    DevBuf<int> sorted, order;                 // raw row at every sorted position / at every final position
    DevBuf<int> ord_n;                         // [2]: final rows; spvo_sift_order_debug's n
    // spvo_sift_detect_pair / spvo_match_l2_slots: the SIFT slots (`slot_cap` rows each), the call's pinned staging and mirrors and the two
    // matches enqueued with the detector (spvo_set_prematch).  Features on the solver's stream, matches where the L2 matcher runs (PostScope).
    int slot_cap = 0;
    SiftSlot slots[N_SIFT_SLOTS];
    PairStage pair;                      // (its prematches' slot numbers are SIFT slots)
    PinBuf<SiftSrc> h_src;               // pinned [2][slot_cap]      what sift_gather_kernel writes for the host: sources (spvo_classic_sift_pair: SiftKey records in each half's front),
    PinBuf<float> hm_desc;               // pinned [2][slot_cap][128] descriptors,
    PinBuf<int> h_n;                     // pinned [2][4]             {final rows, candidates counted, raw rows counted}; behind them [2][4] the contrast factors spvo_akaze_sift_pair reports
    PinBuf<int2> h_match;                // pinned [2][h_match_cap]: the two prematches (enqueue_matches spaces its jobs by spvo_ctx::match_cap)
    int h_match_cap = 0;
    bool match_pending = false;          // pair.ev_match has been recorded: a later call's kernels wait for it before they rewrite a slot
    // the link behind a detector that reports an octave (spvo_brisk_sift_pair, spvo_akaze_sift_pair, spvo_sift_link_debug): the indices
    // sift_link_compact_kernel keeps, `lnk_cap` of them, its counts {kept, the hook's list length}, and the hook's keep flags
    int lnk_cap = 0;
    DevBuf<int> lnk_kept, lnk_cnt, lnk_keep;
    // spvo_sift_brisk_pair (sift_records_kernel, sift.hip.h): the ordered list as the BRISK extractor's chain reads a detector's list --
    // 24-byte records, keep flags, the chain's compacted records, `brk_cap` of each; a counter block per image -- and the pinned mirrors
    // of every final row's source, [2][brk_cap], with their counts [2][4] {final rows, candidates counted, raw rows counted}
    int brk_cap = 0;
    DevBuf<BriskDetKeypoint> brk_rec, brk_crec;
    DevBuf<int> brk_keep, brk_cnt;
    PinBuf<SiftSrc> hb_src;
    PinBuf<int> hb_n;
    std::vector<BriskDetKeypoint> hb_rec;   // the host's records of an image whose device sizes it did not confirm (the second pass)
  } sift;
  // Hamming matcher (classic front end's binary descriptors): rows padded to 16 words
  int ham_cap = 0;
  DevBuf<uint32_t> d_ham_a, d_ham_b;
  DevBuf<int> d_ham_idx;
  DevBuf<float> d_ham_dist;
  DevBuf<unsigned long long> d_ham_vote;
  DevBuf<int2> d_ham_out;                 // spvo_match_l2_u8's packed result
  int bin_pm_norm = SPVO_NORM_HAMMING;    // spvo_set_binary_prematch_norm: the matcher a binary pair call enqueues behind its features
  // fused solve: one packed input, one packed result -- per buffer SET: up to three solves may be pending (spvo_solve_submit .. _wait), a frame's
  // chain enqueued before the previous frames' have been collected; the sets rotate, so the previous solve's points (prev_index) sit in the set before.
  // The TAIL kernel of a solve submitted with `late_prior` is held back (tail_deferred) and goes out in ONE launch with the hypotheses of the next
  // submission (solve_hyp_tail_kernel: the two overlap) -- or alone, when the solve is waited for first.
  static constexpr int SOLVE_SLOTS = 3;   // solves that may be pending
  static constexpr int SOLVE_BUFS = 4;    // buffer sets they rotate through (a pending solve's tail reads the set before its own)
  bool tail_deferred = false;             // the newest submission's tail kernel has not been launched yet ...
  int tail_slot = -1;                     // ... its set, and its arguments (SolveTailArgs, odometry.hip.h: plain data)
  alignas(16) char tail_args[320];
  int solve_fuse = 1;                     // tuning "solve_fuse" (read at spvo_create): 0 = every tail is launched with its own submission
  DevBuf<int> x_counts[SOLVE_BUFS];       // RANSAC scratch of sets 1 .. (set 0: rw): a solve's hypotheses are written while its predecessor's are read
  DevBuf<double> x_poses[SOLVE_BUFS];
  DevBuf<ObsDev> x_obs[SOLVE_BUFS];       // residual blocks of sets 1 .. (set 0: d_obs)
  struct SolvePending { int n = 0, refinement_degree = 0, slot = 0, frame_count = 0; bool late = false; double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0}; };
  std::deque<SolvePending> solve_q;     // oldest first, at most SOLVE_SLOTS
  int solve_next_slot = 0;
  int solve_last_slot = -1, solve_last_n = 0;   // the most recent submission: where its triangulated points are and how many
  hipEvent_t ev_solve[SOLVE_BUFS] = {};
  int solve_cap = 0;
  struct SolveSet {                       // one of the SOLVE_BUFS sets, device and pinned
    DevBuf<char> d_in, d_o;               // 64 doubles + 12*cap words / xyz [3n] floats, inliers [n] ints
    DevBuf<double> d_res;                 // ransac[8] gate[16] refine[12] + pad
    PinBuf<char> h_in, h_o;
    PinBuf<double> h_res;
  } solve_set[SOLVE_BUFS];
  DevBuf<int> d_ctl;                      // [SOLVE_BUFS][4]

  // profiling
  bool prof = false;
  int prof_only = -1;            // >= 0: only this stage is timed (spvo_profile_only)
  std::vector<Stage> stages;
  std::vector<Pending> pending;
  bool pre_fused = false;          // set by the plan loader: a submission's crop / resize / normalise runs inside its group's first layer (conv_first_pre.hip.h; tuning "preprocess_fused")
  bool heads_on_net = false;       // set by the plan loader: the heads of a submission stay on the network stream (VGG fp32) or go to the tail stream
  std::vector<hipEvent_t> free_events;
};

namespace spvo_int {

// SPVO_TRUNK_TIMING diagnostics: where the host spends its time between two submissions (maxima over the 200 submissions of a report)
struct HostDiag { double t_last_submit = 0, max_interval = 0, max_tail_wait = 0, max_solve_wait = 0; int match_miss = 0, late = 0, depth_sum = 0;
                  double iv_tail = 0, iv_match = 0, iv_solve = 0; int iv_printed = 0; long launches = 0; };   // iv_*: host time inside the three waits since the previous launch
extern HostDiag g_diag;
inline double diag_now_us() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }

int fail(spvo_ctx *c, int code, const char *fmt, ...);

#define HIP_TRY(c, expr)                                                                     \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return fail(c, SPVO_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                  __FILE__, __LINE__);                                                       \
  } while (0)

// raw device / pinned pointers, for what is not an owned buffer: the engine plan (Tensor::d / dr[], the Op weight pointers: free_plan),
// SubmitSet's members (set_alloc, set_release*).  Everything else that grows on demand or is allocated on first use is a DevBuf / PinBuf
// and goes through grow(), below.
template <typename T>
int dev_alloc(spvo_ctx *c, T **p, size_t count, bool zero = true) {
  HIP_TRY(c, hipMalloc((void **)p, std::max<size_t>(count, 1) * sizeof(T)));
  if (zero) HIP_TRY(c, hipMemsetAsync(*p, 0, std::max<size_t>(count, 1) * sizeof(T), c->stream));
  return SPVO_OK;
}

// a device buffer of its own for `count` values of the host's, copied synchronously (the plan loader's sources are temporaries)
template <typename T>
int upload(spvo_ctx *c, T **p, const T *src, size_t count) {
  const int rc = dev_alloc(c, p, count, false);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice));
  return SPVO_OK;
}
template <typename T>
int upload(spvo_ctx *c, T **p, const std::vector<T> &v) { return upload(c, p, v.data(), v.size()); }

// frees device buffers, where there is one, and forgets them
template <typename T, typename... Rest>
void dev_free(T *&p, Rest *&...rest) {
  if (p) { (void)hipFree(p); p = nullptr; }
  if constexpr (sizeof...(rest) > 0) dev_free(rest...);
}

// pinned host buffers, where there is one, freed and forgotten
template <typename T, typename... Rest>
void host_free(T *&p, Rest *&...rest) {
  if (p) { (void)hipHostFree(p); p = nullptr; }
  if constexpr (sizeof...(rest) > 0) host_free(rest...);
}

// ---- the grow protocol of the owned buffers (DevBuf / PinBuf), written once.  Every block that re-allocates a group says what to wait
// for first -- a stream, the whole device, nothing -- and lists its buffers, each zeroed() or plain(); grow() waits, frees every
// buffer of the list, allocates every one, and waits for the network stream if any was zeroed (the clearing runs there).  A failed
// allocation leaves every buffer of the list empty (dev_buf.h) and answers SPVO_ERR_DEVICE with the failing call's text -- a context
// that spvo_destroy and a later call can still handle, provided the caller set its capacity fields to 0 before the call.
// The order of a list is the order of allocation, and that decides where the buffers land: a list is not re-sorted.
struct GrowWait { hipStream_t stream = nullptr; };
inline GrowWait wait_for(hipStream_t s) { return GrowWait{s}; }
inline GrowWait wait_for_nothing() { return GrowWait{}; }
template <class T> GrowEntry zeroed(DevBuf<T> &b, size_t count) { return grow_entry<true>(b, count); }
template <class T, class P> GrowEntry plain(Buf<T, P> &b, size_t count) { return grow_entry<false>(b, count); }
inline int grow(spvo_ctx *c, GrowWait w, const std::vector<GrowEntry> &list) {
  if (w.stream) HIP_TRY(c, hipStreamSynchronize(w.stream));
  const GrowResult r = grow_list(list, c->stream);
  if (r.code) return fail(c, SPVO_ERR_DEVICE, "%s failed: %s (%s:%d)", r.call, hipGetErrorString((hipError_t)r.code), __FILE__, __LINE__);
  if (r.cleared) HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SPVO_OK;
}

inline int PairStage::ensure(spvo_ctx *c, size_t px) {
  if (!ev_feat) {
    HIP_TRY(c, hipEventCreateWithFlags(&ev_feat, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&ev_match, hipEventDisableTiming));
  }
  if (2 * px > h_img.count()) return grow(c, wait_for(c->stream2), {plain(h_img, 2 * px)});
  return SPVO_OK;
}
inline void PairStage::stage(const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride) {
  const uint8_t *imgs[2] = {img_l, img_r};
  const size_t px = (size_t)rows * cols;
  for (int k = 0; k < 2; ++k)
    for (int r = 0; r < rows; ++r) std::memcpy(h_img + k * px + (size_t)r * cols, imgs[k] + (size_t)r * stride, cols);
}
inline void PairStage::release() {
  for (hipEvent_t *e : {&ev_feat, &ev_match}) if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
}

// the synchronous entry points that work in the submissions' buffers refuse to run beside them; a failed wait / record: "`what` failed"
inline int require_idle(spvo_ctx *c) {
  return c->pendq.empty() ? SPVO_OK : fail(c, SPVO_ERR_STATE, "detector submissions are in flight: complete them with spvo_detect_wait first");
}
inline int dev_check(spvo_ctx *c, hipError_t e, const char *what) { return e == hipSuccess ? SPVO_OK : fail(c, SPVO_ERR_DEVICE, "%s failed", what); }

int stage_id(spvo_ctx *c, const std::string &name);
hipError_t wait_event(hipEvent_t ev);
// a diagnostic switch (spvo_set_tuning, include/spvo.h): the value set for `name`, or `dflt`.  Never the environment.
int tuning(const char *name, int dflt);
// trunk pairing: a pair held for a partner whose predecessor's trunk has meanwhile finished is launched alone (called from the entry
// points a host passes through while it waits: the network stream must not idle because the partner is late)
int release_held_if_idle(spvo_ctx *c);
hipEvent_t get_event(spvo_ctx *c);
void resolve_pending(spvo_ctx *c);
// launch segments (spvo_core.hip): seg_begin opens one on `stream` when graphs are on for this context (and the profiler is off) and returns
// whether it did; seg_end closes it -- replayed from the entry's graph when the recorded launches are identical to the ones it was built
// from, or plain launches + a graph for the next time; seg_free_all drops every graph
bool seg_begin(spvo_ctx *c, GraphEntry *e, hipStream_t stream);
int seg_end(spvo_ctx *c);
void seg_abort(spvo_ctx *c);      // drops an open segment without launching it (a failed group launch; a stale one found at the next begin)
void seg_free_all(spvo_ctx *c);

struct ScopedStage {
  spvo_ctx *c;
  int id = -1;
  hipEvent_t e0 = nullptr;
  hipStream_t st = nullptr;
  ScopedStage(spvo_ctx *ctx, int stage, double flops = 0, double bytes = 0, hipStream_t stream = nullptr) : c(ctx) {
    if (!c->prof || stage < 0 || (c->prof_only >= 0 && stage != c->prof_only)) return;
    id = stage;
    st = stream ? stream : (c->post ? c->post : c->stream);
    if (flops > 0) c->stages[id].flops = flops;
    if (bytes > 0) c->stages[id].bytes = bytes;
    e0 = get_event(c);
    (void)hipEventRecord(e0, st);
  }
  ~ScopedStage() {
    if (id < 0) return;
    hipEvent_t e1 = get_event(c);
    (void)hipEventRecord(e1, st);
    c->pending.push_back({id, e0, e1, c->stages[id].flops, c->stages[id].bytes});
    if (c->pending.size() > 8192) resolve_pending(c);
  }
};

// a tensor's buffer, from image `img0` on, for submission set `ring` (tensors a tail reads have one per set, the others one for all) / for the forward pass being enqueued
inline float *ring_ptr(const Tensor &t, int ring, int img0 = 0) { return (t.dr[ring] ? t.dr[ring] : t.d) + (size_t)img0 * t.per_image; }
inline float *ring_ptr(spvo_ctx *c, const Tensor &t, int img0 = 0) { return ring_ptr(t, c->cur_ring, img0); }
// The stand-alone entry points (spvo_heatmap, spvo_nms) have no set of their own: index 0 doubles as theirs -- they refuse to run beside
// submissions (require_idle) -- with the counter block spvo_ctx::d_counters_alone, so that the submissions' blocks stay zeroed.
inline SubmitSet &standalone(spvo_ctx *c) { return c->sets[0]; }

// post-processing issued by a synchronous entry point while submissions are queued goes behind them
struct PostScope {
  spvo_ctx *c;
  explicit PostScope(spvo_ctx *ctx) : c(ctx) {
    c->post = c->pendq.empty() ? c->stream : c->stream_t;
    c->ms_set = 0;
    // nothing queued, but the matches of the submission collected last may still run on the tail stream (spvo_detect_wait returns
    // when the FEATURES are final) and they share the matcher's scratch: the network stream waits for them, asynchronously
    if (c->pendq.empty() && c->ev_post && hipEventRecord(c->ev_post, c->stream_t) == hipSuccess) (void)hipStreamWaitEvent(c->stream, c->ev_post, 0);
    if (c->stream_tb && c->ev_post_b && hipEventRecord(c->ev_post_b, c->stream_tb) == hipSuccess) (void)hipStreamWaitEvent(c->post, c->ev_post_b, 0);
  }
  ~PostScope() { c->post = c->stream; }
};

// The launcher of one instance `k` of the tiled convolution kernels (conv_mfma / conv_f16 / conv_bf16x3 / conv_i8 .hip.h; T: its tile).
// Persistent grid: what the chip holds at once -- the instance's resident workgroups per CU, asked once per device -- and each workgroup
// walks tiles with that stride.  Leaves the tiles and workgroups of the launch in the context (launch_op copies them to its op).
template <class T, auto k, class Args>
int launch_persistent_tiles(spvo_ctx *c, Args args, hipStream_t stream) {
  static int per_cu[64] = {};   // resident workgroups per CU of this instance, per device
  const int dev = c->cfg.device & 63;
  if (!per_cu[dev]) {
    HIP_TRY(c, hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, T::LDS_BYTES));
    int n = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)k, 256, T::LDS_BYTES));
    per_cu[dev] = std::max(n, 1);
  }
  args.tiles_x = (args.W + T::TW - 1) / T::TW;
  args.tiles_y = (args.H + T::TH - 1) / T::TH;
  const int n_tiles = args.tiles_x * args.tiles_y * args.co_tiles * args.batch;
  c->launch_tiles = n_tiles; c->launch_wgs = std::min(n_tiles, c->num_cus * per_cu[dev]);
  hipLaunchKernelGGL(k, dim3(c->launch_wgs), dim3(256), T::LDS_BYTES, stream, args);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// ---- spvo_core.hip
// a submission set's life cycle: set_alloc creates what every set has from spvo_create on; set_release frees ALL a set holds and forgets it
// (the one list of its members), through the three helpers for what is allocated lazily and re-allocated when it grows
int set_alloc(spvo_ctx *c, int index);
void set_release(SubmitSet &s);
void set_release_images(SubmitSet &s);     // h_img, d_img (ensure_host_sets)
void set_release_match(SubmitSet &s);      // h_match_out and the cache entries that point into it (ensure_match)
void set_release_segments(SubmitSet &s);   // the graphs of its launch segments (seg_free_all)
// ---- spvo_plan.hip
void free_plan(spvo_ctx *c);
// a tiled layer's co_tiles and tile (wr, wc) -- it offers the tiles the launchers' tables have a case for (FP32: `switch (key)` in spvo_net_f32.hip; the others: with_tile_variant, conv_packed.hip.h); returns the channels
// per chunk of the FP32 direct kernel (the other kinds chunk by their own rule)
int choose_variant(const spvo_ctx *c, Op &op, const Tensor &ti, bool split = false);
int upload_stem(spvo_ctx *c, Op &op, const float *w, const float *b);   // d_w, d_b of a plain single-channel-input layer: OIHW weights and bias as they are
// ops head_start .. + 2 are convPb `cin` -> 65 into output_det, convDb `cin` -> 256 (both 1x1, plain, on 1/8-size tensors) and its L2 norm into output_desc
bool tail_is_plain(const spvo_ctx *c, int cin);
// ---- spvo_net_*.hip
// What the plan loader prepares of convolution `i` for its engine kind, beside the launcher that runs it, after the common part (spvo_plan.hip:
// prepare_conv): the kind's refusals, chunking, tile variant, repacked weights.  `w`, `b`: OIHW weights and bias (a merged sibling's appended)
int prepare_conv_f32(spvo_ctx *c, unsigned i, const float *w, const float *b);
int prepare_conv_f16(spvo_ctx *c, unsigned i, const float *w, const float *b);
int prepare_conv_s3(spvo_ctx *c, unsigned i, const float *w, const float *b);
int prepare_conv_i8(spvo_ctx *c, unsigned i, const float *w, const float *b);
int prepare_dwconv_i8(spvo_ctx *c, unsigned i, const float *w, const float *b);
int prepare_maxpool_i8(spvo_ctx *c, unsigned i);   // a stand-alone max-pool of an INT8 engine in the int8_general mode: its refusals, and Op::pool_m
// the tail as one launch where it is the plain one (tail_is_plain + the kind's own terms): FP32 and FP16 / INT8 engines.  rp, rd: convPb's, convDb's records
int fuse_tail_f32(spvo_ctx *c, const float *payload, const EngineOp &rp, const EngineOp &rd);
int fuse_tail_i8(spvo_ctx *c, const float *payload, const EngineOp &rp, const EngineOp &rd);
int launch_conv16(spvo_ctx *c, const Op &op, int img0, int batch, hipStream_t stream);
int launch_conv_s3(spvo_ctx *c, const Op &op, int img0, int batch, hipStream_t stream);
int launch_conv8(spvo_ctx *c, const Op &op, int img0, int batch, hipStream_t stream);
int launch_heads8(spvo_ctx *c, int batch, hipStream_t stream);   // spvo_net_i8.hip: the fused tail of an INT8 engine (heads_i8.hip.h)
void plan_int8_fusion(spvo_ctx *c);   // spvo_net_i8.hip: marks the MobileNet blocks (and the stem) of a loaded INT8 plan that run as one launch
int launch_maxpool_f16(spvo_ctx *c, const Tensor &ti, const Tensor &to, const float *tin, float *tout, int batch, hipStream_t stream);
int launch_maxpool_i8(spvo_ctx *c, const Op &op, const Tensor &ti, const Tensor &to, const float *tin, float *tout, int batch, hipStream_t stream);   // spvo_net_i8.hip: maxpool2_i8_kernel (conv_i8.hip.h)
void launch_unpad_c8(const Tensor &t, int batch, float *dst, hipStream_t stream);    // spvo_debug_tensor
void launch_unpad_s3(const Tensor &t, int batch, float *dst, hipStream_t stream);
void launch_unpad_c16(const Tensor &t, int batch, float *dst, hipStream_t stream);
int run_ops(spvo_ctx *c, int batch, size_t first, size_t last, hipStream_t stream);   // ops [first, last) on `stream`
int run_network(spvo_ctx *c, int batch);
// ---- spvo_detect.hip
// appends the six tables of a dst_w x dst_h <- src_w x src_h bilinear resize: xi, xa0, xa1 [dst_w]; yi, yb0, yb1 [dst_h]
void resize_tables(int dst_w, int src_w, int dst_h, int src_h, std::vector<int> &out);
// ---- spvo_classic.hip: spvo_preprocess of a context without an engine (d_img[0] -> cls.pre_out, enqueued on the network stream)
int classic_preprocess(spvo_ctx *c, const CropGeom &g, size_t stride);
void classic_release(spvo_ctx *c);   // what spvo_ctx::bin holds besides memory: its events (spvo_destroy)
void classic_release_slots(spvo_ctx *c);   // every binary slot emptied and back to 32-byte rows, the prematches forgotten
// a host image (strided view) becomes the resident image of spvo_ctx::cls, every buffer of it grown to the shape (enqueued on the solver's stream)
int classic_upload_image(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride);
// a staged image (pinned, rows packed: PairCall::image) becomes the resident image of spvo_ctx::cls, behind classic_image_ensure for its shape
// (enqueued on the solver's stream); the first link of every pair call's chain whose detector reads spvo_ctx::cls
int classic_image_from_staged(spvo_ctx *c, const uint8_t *h_img, int rows, int cols);
// spvo_classic_detect's own preparations, for another entry point that fills the binary slots (spvo_brisk_detect_pair).  classic_slots_ensure:
// the slots, the call's mirrors and the pinned staging for `cap` rows per slot and images of `px` bytes; a larger `cap` than any before
// empties every slot.  classic_image_ensure: every buffer of spvo_ctx::cls grown to a rows x cols image; none is resident afterwards.
int classic_slots_ensure(spvo_ctx *c, int cap, size_t px);
int classic_image_ensure(spvo_ctx *c, int rows, int cols);
// The Shi-Tomasi / FAST detector as the first link of another unit's chain (spvo_classic_sift_pair; the kinds whose detector is one of the
// two).  classic_detector_check: what spvo_gftt_detect / spvo_fast_detect refuse of these options and this shape.  classic_detector_enqueue,
// behind classic_image_ensure: the staged image `h_img` (pinned, rows packed) becomes the resident image and goes through the detector on
// the solver's stream; the list stays in spvo_ctx::cls (xy, resp, counters[2]; counters[3]: the key buffer overflowed).
int classic_detector_check(spvo_ctx *c, const char *who, const spvo_classic_opts *opts, int rows, int cols);
int classic_detector_enqueue(spvo_ctx *c, const spvo_classic_opts *opts, const uint8_t *h_img, int rows, int cols);
// cls_rank_kernel (classic_detect.hip.h) over a key list whose length lies in device memory, enqueued on the solver's stream: rank[i] += the
// number of keys smaller than keys[i] (rank is zero between uses)
void classic_rank_enqueue(spvo_ctx *c, const unsigned long long *keys, int *rank, const int *n_ptr, int cap);
// The octave-aware ORB extractor as a link behind a detector that left records with an octave on the device (orb_link.hip.h;
// spvo_brisk_orb_pair, spvo_akaze_orb_pair).  orb_link_check: refuses a shape whose level `max_octave` is smaller than the extractor
// accepts (`who` names the entry point).  orb_link_ensure: the pyramid, its tables and the link's buffers for `cap` rows.  orb_link_enqueue,
// on the solver's stream with the image resident in spvo_ctx::cls: border rule + stable grouping by octave, levels 1 .. max_octave, the
// smoothing of levels 0 .. max_octave, the 32-byte rows of min(rows found, cap) records into `desc`; kept / angle / counts stay in
// spvo_ctx::cls (lnk_*).  orb_link_finish_*: the finishing launch of an image -- slot count and records, the pinned mirrors (h_n = {rows
// found, overflow flag of the detector}; AKAZE: the contrast factors in h_k).
int orb_link_check(spvo_ctx *c, const char *who, int rows, int cols, int max_octave);
int orb_link_ensure(spvo_ctx *c, int rows, int cols, int cap);
int orb_link_enqueue(spvo_ctx *c, int rows, int cols, int max_octave, const OrbLinkSrc &src, int cap, uint8_t *desc);
void orb_link_finish_brisk(spvo_ctx *c, const BriskDetKeypoint *src, const int *det_counters, int cap, OrbKeypoint *d_kp, const uint32_t *d_desc, int *d_n, int *h_n,
                           BriskDetKeypoint *h_kp, uint8_t *h_desc);
void orb_link_finish_akaze(spvo_ctx *c, const AkazeKp *src, const int *stat, int cand_cap, int cap, OrbKeypoint *d_kp, const uint32_t *d_desc, int *d_n, int *h_n, int *h_k,
                           AkazeKp *h_kp, uint8_t *h_desc);
// ---- spvo_brisk.hip
// what spvo_brisk_describe refuses of an image, for every entry point that runs the extractor (`who` names it in the error text)
int brisk_check_image(spvo_ctx *c, const char *who, int rows, int cols);
// ---- spvo_brisk_detect.hip
// brisk_detect_ref.py choice 3: the taps of one axis of cv::resize(INTER_AREA)'s general path; false if a run is longer than BRISK_DET_TAPS
// or not contiguous (cannot happen for ratios below 3)
bool brisk_area_tab(int ssize, int dsize, BriskAreaTap *out);
// ---- spvo_akaze.hip
// The extractor as a link of spvo_classic_detect's chain (kinds SPVO_CLASSIC_*_BRISK).  brisk_chain_ensure: the tables, the integral image
// of a rows x cols image and the keypoint buffers for `cap` rows.  brisk_chain_enqueue, on the solver's stream behind a detector that left
// its list in spvo_ctx::cls (xy, resp, counters[2]): integral image, border rule of keypoints of ONE `size` as a compaction that keeps at
// most `cap` rows and counts all, descriptors of at most `most` <= cap rows into the slot, and the finish launch -- records, rows and
// count of the slot, and their pinned mirrors (h_n = {rows that passed the border rule, overflow flag of the detector}).
int brisk_chain_ensure(spvo_ctx *c, int rows, int cols, int cap);
struct ChainOut {         // where image k of a spvo_classic_detect call leaves its rows (every chain's, the ORB kinds' included)
  int *cnt;               // [CLS_COUNTER_INTS] the extractor's counter block: 0: kept in all, 2: kept and described
  float *kresp;           // [cap] the detector's responses of the kept
  OrbKeypoint *d_kp; uint32_t *d_desc; int *d_n;          // the slot
  int *h_n; OrbKeypoint *h_kp; uint8_t *h_desc;           // its pinned mirrors
};
int brisk_chain_enqueue(spvo_ctx *c, int rows, int cols, float size, int cap, int most, const ChainOut &o);
// The extractor behind the BRISK detector (spvo_brisk_detect_pair), on the solver's stream behind brisk_refine_kernel: rec / keep of the
// min(det_counters[1], det_cap) candidates -> integral image, keep flag + border rule of every record's own size as ONE compaction (at most
// `cap` rows kept, all counted; compacted records in `crec`), descriptors with the count read on the device, and the finish launch: the
// slot's count, 20-byte records and rows, the pinned mirrors o.h_n, o.h_desc and the 24-byte records in h_kp (o.h_kp, o.kresp: unused).
int brisk_pair_chain_enqueue(spvo_ctx *c, int rows, int cols, int cap, const BriskDetKeypoint *rec, const int *keep, const int *det_counters, int det_cap, BriskDetKeypoint *crec,
                             const ChainOut &o, BriskDetKeypoint *h_kp);
// ---- spvo_sift.hip
void sift_release(spvo_ctx *c);      // what spvo_ctx::sift holds besides memory: its events (spvo_destroy)
// The SIFT extractor as a link behind a detector that left records with an octave on the device (sift.hip.h: SiftLinkIO;
// spvo_brisk_sift_pair, spvo_akaze_sift_pair, spvo_orb_sift_pair).  sift_link_pair is the whole call around the detector -- a PairCall on the SIFT slots
// (pair_call.hip.h) with the link's allocations and chains -- so that neither detector object needs the SIFT unit's internals; the detector
// is three functions.  Every refusal comes before anything is touched, every allocation (`prepare` included) before the first launch.
struct SiftLinkDetector {
  const char *who;                                   // the entry point, for the error text
  int max_octave;                                    // the pyramid is built for octaves 0 .. max_octave, whichever the records name
  std::function<int()> check;                        // what the detector's sibling refuses of its parameters and the shape
  std::function<int(SiftLinkSrc &)> prepare;         // behind classic_image_ensure: the detector's buffers for the shape; where its list will lie
  std::function<int(const uint8_t *)> enqueue;       // the staged image (pinned, rows packed) becomes the resident one and goes through the detector's chain
  bool overflow_is_capacity = false;                 // a set overflow flag is an input's doing (ORB's corner buffers): SPVO_ERR_CAPACITY, not the defect the others report
};
// (SPVO_OK and SPVO_ERR_CAPACITY are answered behind the call's one wait: the chains of both images have run, and an AKAZE sink has left
// image k's contrast factors in spvo_ctx::sift.h_n + 8 + 4 k)
int sift_link_pair(spvo_ctx *c, const SiftLinkDetector &det, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int slot_l, int slot_r, int slot_capacity,
                   const PairOut &out_l, const PairOut &out_r);
// ---- spvo_match.hip
int ensure_match(spvo_ctx *c, int na, int nb);
struct MatchReq {
  const float *dA, *dB;
  int na, nb;                     // counts, or upper bounds when the pointers are set
  const int *na_ptr, *nb_ptr;
  const float *sqA, *sqB;         // squared norms if already known (feature slots), else NULL
};
int enqueue_matches(spvo_ctx *c, const MatchReq *req_in, int njobs, int selector, int cross_check, float ratio, int2 *host_out);
// one Hamming match between two binary slots, enqueued on the solver's stream with the counts read on the device; packed result -> host_out (pinned)
int enqueue_hamming_slots(spvo_ctx *c, int slot_a, int slot_b, int selector, int cross_check, float ratio, int2 *host_out);
int enqueue_l2u8_slots(spvo_ctx *c, int slot_a, int slot_b, int selector, int cross_check, float ratio, int2 *host_out);   // the same under the byte-L2 norm (K12u)
int enqueue_binary_prematch(spvo_ctx *c, int slot_a, int slot_b, int2 *host_out);   // spvo_set_prematch's match under spvo_set_binary_prematch_norm's norm

}  // namespace spvo_int
#pragma GCC visibility pop
