// spvo_brisk_detect.hip -- the classic front end's BRISK keypoint detector (brisk_detect.hip.h): the layout of the six layers and the area
// taps of a shape (built on the host in double, by the formulas tests/brisk_detect_ref.py lists), spvo_brisk_detect,
// spvo_brisk_detect_debug_layer and spvo_brisk_detect_pair (detector + extractor of a stereo pair in one submission into two binary slots,
// by the resident-pair protocol of pair_call.hip.h; spvo_brisk_orb_pair: the same call with the octave-aware ORB extractor behind the detector;
// spvo_brisk_sift_pair: the detector as the first link of spvo_sift.hip's sift_link_pair, into two SIFT slots).  Runs on the solver's stream (stream2) with the image resident in spvo_ctx::cls as
// layer 0 -- it stays there for a spvo_brisk_describe(img = NULL) that follows -- and owns everything else it needs (spvo_ctx::brisk_det).
#include "spvo_internal.hip.h"
#include "pair_call.hip.h"
#include "brisk_detect.hip.h"

// brisk_detect_ref.py choice 3: the taps of one axis; false if a run is longer than BRISK_DET_TAPS or not contiguous (cannot happen for the
// two ratios of the scale space, both below 3).  The AKAZE detector's octaves take the same path (spvo_akaze.hip).
bool spvo_int::brisk_area_tab(int ssize, int dsize, BriskAreaTap *out) {
  const double scale = (double)ssize / (double)dsize;
  for (int d = 0; d < dsize; ++d) {
    const double fsx1 = (double)d * scale, fsx2 = fsx1 + scale, cell = std::min(scale, (double)ssize - fsx1);
    int sx1 = (int)std::ceil(fsx1), sx2 = std::min((int)std::floor(fsx2), ssize - 1);
    sx1 = std::min(sx1, sx2);
    BriskAreaTap t{};
    bool ok = true;
    auto push = [&](int s, float a) {
      if (t.n == 0) t.start = s;
      if (t.n >= BRISK_DET_TAPS || s != t.start + t.n || s < 0 || s >= ssize) { ok = false; return; }
      t.a[t.n++] = a;
    };
    if (sx1 - fsx1 > 1e-3) push(sx1 - 1, (float)((sx1 - fsx1) / cell));
    for (int sx = sx1; sx < sx2; ++sx) push(sx, (float)(1.0 / cell));
    if (fsx2 - sx2 > 1e-3) push(sx2, (float)(std::min(std::min(fsx2 - sx2, 1.0), cell) / cell));
    if (!ok || t.n == 0) return false;
    out[d] = t;
  }
  return true;
}

namespace {
constexpr int BD_COUNTER_INTS = 4;   // 1 candidates, 2 keypoints, 3 overflow

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// layout, tables and buffers for a rows x cols image whose layer 0 is resident in spvo_ctx::cls
int bd_ensure(spvo_ctx *c, int rows, int cols) {
  auto &d = c->brisk_det;
  hipStream_t st = c->stream2;
  d.valid = false;
  if (!d.counters)
    if (int rc = grow(c, wait_for_nothing(), {zeroed(d.counters, BD_COUNTER_INTS)})) return rc;
  int h[BRISK_DET_LAYERS], w[BRISK_DET_LAYERS];
  h[0] = rows; w[0] = cols;
  h[1] = 2 * (rows / 3); w[1] = 2 * (cols / 3);
  for (int i = 2; i < BRISK_DET_LAYERS; ++i) { h[i] = h[i - 2] / 2; w[i] = w[i - 2] / 2; }
  if (d.rows != rows || d.cols != cols) {
    d.rows = d.cols = 0;
    size_t pyr = 0, score = 0, tabs = 0;
    size_t pyr_off[BRISK_DET_LAYERS] = {0}, score_off[BRISK_DET_LAYERS + 1], tab_off[BRISK_DET_LAYERS] = {0};
    long long cand = 0;
    for (int i = 0; i < BRISK_DET_LAYERS; ++i) {
      const size_t px = (size_t)h[i] * w[i];
      score_off[i] = score; score = align256(score + px);
      if (i > 0) { pyr_off[i] = pyr; pyr = align256(pyr + px); }
      cand += (long long)std::max(h[i] - 6, 0) * std::max(w[i] - 6, 0);
    }
    score_off[BRISK_DET_LAYERS] = score; score = align256(score + (size_t)rows * cols);
    // which samplings are exact halves (choice 2), and the taps of the others
    bool exact[BRISK_DET_LAYERS] = {false};
    for (int i = 1; i < BRISK_DET_LAYERS; ++i) {
      const int s = i == 1 ? 0 : i - 2;
      exact[i] = h[s] == 2 * h[i] && w[s] == 2 * w[i];
      if (!exact[i]) { tab_off[i] = tabs; tabs += (size_t)w[i] + h[i]; }
    }
    d.h_tabs.assign(std::max<size_t>(tabs, 1), BriskAreaTap{});
    for (int i = 1; i < BRISK_DET_LAYERS; ++i) {
      const int s = i == 1 ? 0 : i - 2;
      if (!exact[i] && !(brisk_area_tab(w[s], w[i], d.h_tabs.data() + tab_off[i]) && brisk_area_tab(h[s], h[i], d.h_tabs.data() + tab_off[i] + w[i])))
        return fail(c, SPVO_ERR_STATE, "BRISK detector: the area taps of layer %d (%d x %d from %d x %d) failed their own checks", i, h[i], w[i], h[s], w[s]);
    }
    if (pyr > d.px_cap || score > d.px_cap || tabs > d.tab_cap || cand > d.cand_cap) {
      const size_t npx = std::max(std::max(pyr, score), d.px_cap), ntab = std::max(std::max<size_t>(tabs, 1), d.tab_cap);
      const int ncand = (int)std::min<long long>(std::max<long long>(std::max<long long>(cand, 1), d.cand_cap), 0x7FFFFFFF);
      d.px_cap = d.tab_cap = 0; d.cand_cap = 0;   // a failed allocation below leaves a context that spvo_destroy and a later call can still handle
      if (int rc = grow(c, wait_for(st), {plain(d.pyr, npx), plain(d.score, npx), plain(d.tabs, ntab), plain(d.keys, ncand), zeroed(d.rank, ncand), plain(d.keep, ncand), plain(d.rec, ncand),
                                          plain(d.out, ncand)}))
        return rc;
      d.px_cap = npx; d.tab_cap = ntab; d.cand_cap = ncand;
    }
    HIP_TRY(c, hipMemcpyAsync(d.tabs, d.h_tabs.data(), d.h_tabs.size() * sizeof(BriskAreaTap), hipMemcpyHostToDevice, st));
    float scale[BRISK_DET_LAYERS] = {1.f, 1.5f};
    for (int i = 2; i < BRISK_DET_LAYERS; ++i) scale[i] = scale[i - 2] * 2.f;
    for (int i = 0; i < BRISK_DET_LAYERS; ++i) {
      BriskDetLayer &L = d.lv.l[i];
      L.im = i == 0 ? nullptr : d.pyr + pyr_off[i];
      L.score = d.score + score_off[i];
      L.h = h[i]; L.w = w[i];
      L.scale = scale[i];
      L.offset = 0.5f * scale[i] - 0.5f;   // (exact: the scales are 1, 1.5, 2, 3, 4, 6)
    }
    d.lv.score58 = d.score + score_off[BRISK_DET_LAYERS];
    for (int i = 1; i < BRISK_DET_LAYERS; ++i) {
      const int s = i == 1 ? 0 : i - 2;
      BriskResizeJob &J = d.jobs[i];
      J.src = nullptr; J.dst = d.lv.l[i].im;   // (the sources are filled in per call: layer 0 is spvo_ctx::cls's image)
      J.sh = h[s]; J.sw = w[s]; J.dh = h[i]; J.dw = w[i];
      J.xtab = exact[i] ? nullptr : d.tabs + tab_off[i];
      J.ytab = exact[i] ? nullptr : d.tabs + tab_off[i] + w[i];
    }
    d.rows = rows; d.cols = cols;
  }
  d.lv.l[0].im = c->cls.im;   // (may have been re-allocated by the upload)
  for (int i = 1; i < BRISK_DET_LAYERS; ++i) d.jobs[i].src = d.lv.l[i == 1 ? 0 : i - 2].im;
  return SPVO_OK;
}

// one group of the pyramid: layers first .. first + count - 1, each kernel launched only if the group has a job of its kind
void bd_resize_group(spvo_ctx *c, int first, int count) {
  auto &d = c->brisk_det;
  BriskResizeJobs jobs{};
  bool any_exact = false, any_area = false;
  int gw = 1, gh = 1;
  for (int k = 0; k < count; ++k) {
    jobs.j[k] = d.jobs[first + k];
    (jobs.j[k].xtab ? any_area : any_exact) = true;
    gw = std::max(gw, jobs.j[k].dw); gh = std::max(gh, jobs.j[k].dh);
  }
  const dim3 grid((gw + 63) / 64, (gh + 3) / 4, count);
  if (any_exact) hipLaunchKernelGGL(brisk_half_kernel, grid, dim3(256), 0, c->stream2, jobs);
  if (any_area) hipLaunchKernelGGL(brisk_area_kernel, grid, dim3(256), 0, c->stream2, jobs);
}

// the image resident in spvo_ctx::cls -> rec / keep of its candidates in output order, their number in counters[1] (bd_ensure has run)
int bd_enqueue(spvo_ctx *c, int rows, int cols, int threshold) {
  auto &d = c->brisk_det;
  hipStream_t st = c->stream2;
  HIP_TRY(c, hipMemsetAsync(d.counters, 0, BD_COUNTER_INTS * sizeof(int), st));
  bd_resize_group(c, 1, 1);
  bd_resize_group(c, 2, 2);
  bd_resize_group(c, 4, 2);
  const dim3 grid((cols + 63) / 64, (rows + 3) / 4, BRISK_DET_LAYERS), grid0(grid.x, grid.y, 1);
  hipLaunchKernelGGL(brisk_score916_kernel, grid, dim3(256), 0, st, d.lv);
  hipLaunchKernelGGL(brisk_score58_kernel, grid0, dim3(256), 0, st, d.lv);
  hipLaunchKernelGGL(brisk_collect_kernel, grid, dim3(256), 0, st, d.lv, threshold, d.keys, d.cand_cap, d.counters);
  classic_rank_enqueue(c, d.keys, d.rank, d.counters + 1, d.cand_cap);
  hipLaunchKernelGGL(brisk_refine_kernel, dim3(64), dim3(256), 0, st, d.lv, threshold, d.keys, d.rank, d.cand_cap, d.counters, d.rec, d.keep);
  return SPVO_OK;
}
// a pair call's first link (spvo_brisk_detect_pair, spvo_brisk_orb_pair, spvo_brisk_sift_pair): a staged image becomes the resident one and goes through that chain
int bd_staged_enqueue(spvo_ctx *c, const uint8_t *h_img, int rows, int cols, int threshold) {
  if (int rc = classic_image_from_staged(c, h_img, rows, cols)) return rc;
  return bd_enqueue(c, rows, cols, threshold);
}

// what spvo_brisk_detect refuses of its parameters and of the image shape (`who` names the entry point in the error text)
int bd_check(spvo_ctx *c, const char *who, int rows, int cols, int threshold, int octaves) {
  if (threshold < 1 || threshold > 255) return fail(c, SPVO_ERR_INVALID, "%s: threshold must be 1 .. 255", who);
  if (octaves != 3) return fail(c, SPVO_ERR_INVALID, "%s: only octaves = 3 (six layers) is built", who);
  if (rows < 8 || cols < 8) return fail(c, SPVO_ERR_INVALID, "%s: images of at least 8 x 8 only", who);
  return brisk_check_image(c, who, rows, cols);
}
}  // namespace

extern "C" {

int spvo_brisk_detect(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, int threshold, int octaves, spvo_brisk_keypoint *kp, int cap, int *n_out) {
  if (!c || !img || !n_out || rows <= 0 || cols <= 0 || stride < (size_t)cols || cap < 0 || (cap > 0 && !kp)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  *n_out = 0;
  if (int rc = bd_check(c, "spvo_brisk_detect", rows, cols, threshold, octaves)) return rc;
  if (int rc = require_idle(c)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream2;
  if (int rc = classic_upload_image(c, img, rows, cols, stride)) return rc;
  if (int rc = bd_ensure(c, rows, cols)) return rc;
  auto &d = c->brisk_det;
  if (int rc = bd_enqueue(c, rows, cols, threshold)) return rc;
  hipLaunchKernelGGL(brisk_det_compact_kernel, dim3(1), dim3(1024), 0, st, d.rec, d.keep, d.cand_cap, d.counters, d.out);
  HIP_TRY(c, hipGetLastError());
  int cnt[BD_COUNTER_INTS];
  HIP_TRY(c, hipMemcpyAsync(cnt, d.counters, sizeof cnt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  // (the lists hold a candidate per interior pixel of every layer, so the overflow flag cannot be set; were it, the count would be wrong)
  if (cnt[3]) return fail(c, SPVO_ERR_STATE, "spvo_brisk_detect: the candidate list overflowed although it is sized from the image");
  d.valid = true;
  d.image_gen = c->cls.image_gen;
  *n_out = cnt[2];
  const int ncopy = std::min(cnt[2], cap);
  if (ncopy > 0) {
    static_assert(sizeof(spvo_brisk_keypoint) == sizeof(BriskDetKeypoint), "record layout");
    HIP_TRY(c, hipMemcpyAsync(kp, d.out, (size_t)ncopy * sizeof(BriskDetKeypoint), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  return SPVO_OK;
}

// One submission per stereo pair: the resident-pair protocol (PairCall on the binary slots, pair_call.hip.h) around the detector's chain
// up to brisk_refine_kernel and the extractor behind it (brisk_pair_chain_enqueue), image by image in stream order.  The scale space, the
// candidate lists, the integral image, the extractor's lists and the detector's counter block are the left image's first and the right
// image's afterwards: an image's finishing kernel has put its counts into the pinned h_n before the next image's clear.
// orb = true (spvo_brisk_orb_pair): the extractor behind the detector is the octave-aware ORB one (orb_link.hip.h through spvo_classic.hip)
// on the records where brisk_refine_kernel left them, rows of 32 bytes; everything else is the same call.
}  // extern "C"
namespace {
constexpr int BRISK_ORB_MAX_OCTAVE = BRISK_DET_LAYERS - 1;   // a BRISK keypoint's octave is its layer, 0 .. 5
int brisk_pair(spvo_ctx *c, const char *who, bool orb, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int threshold, int octaves, int slot_l, int slot_r,
               int slot_capacity, spvo_brisk_features *out_l, spvo_brisk_features *out_r) {
  if (!c || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  const int cap = slot_capacity, row_bytes = orb ? 32 : 64;
  PairCall<BinPairFamily> pc(c, who, BinPairFamily{row_bytes}, pair_out(out_l), pair_out(out_r));
  int rc;
  if ((rc = pc.check(slot_l, slot_r)) || (rc = pc.check_capacity(cap)) || (rc = bd_check(c, who, rows, cols, threshold, octaves))) return rc;
  if (orb)
    if ((rc = orb_link_check(c, who, rows, cols, BRISK_ORB_MAX_OCTAVE))) return rc;
  if ((rc = pc.open())) return rc;
  auto &bb = c->bin;
  auto &d = c->brisk_det;
  // every allocation and the 47 MB point table before the first launch of the chain; the image buffer before the layout that points into it
  if ((rc = classic_slots_ensure(c, cap, (size_t)rows * cols)) || (rc = classic_image_ensure(c, rows, cols)) ||
      (rc = orb ? orb_link_ensure(c, rows, cols, cap) : brisk_chain_ensure(c, rows, cols, cap)) || (rc = bd_ensure(c, rows, cols)))
    return rc;
  if ((rc = pc.load(img_l, img_r, rows, cols, stride))) return rc;
  for (int k = 0; k < 2; ++k) {
    const BinarySlot &s = bb.slots[pc.slots[k]];
    if ((rc = bd_staged_enqueue(c, pc.image(k), rows, cols, threshold))) return rc;
    const ChainOut out{bb.d_cnt + k * BIN_COUNTER_INTS, bb.d_kresp, s.d_kp, s.d_desc, s.d_n, bb.h_n + 4 * k, nullptr, bb.h_desc + (size_t)k * cap * row_bytes};
    if (!orb) {
      if ((rc = brisk_pair_chain_enqueue(c, rows, cols, cap, d.rec, d.keep, d.counters, d.cand_cap, d.out, out, bb.h_bkp + (size_t)k * cap))) return rc;
      continue;
    }
    static_assert(offsetof(BriskDetKeypoint, x) == 0 && offsetof(BriskDetKeypoint, y) == 4 && offsetof(BriskDetKeypoint, octave) == 20, "record layout");
    const OrbLinkSrc src{reinterpret_cast<const char *>(d.rec.get()), (int)sizeof(BriskDetKeypoint), 0, 4, 20, d.keep, d.counters + 1, d.cand_cap};
    if ((rc = orb_link_enqueue(c, rows, cols, BRISK_ORB_MAX_OCTAVE, src, cap, reinterpret_cast<uint8_t *>(s.d_desc.get())))) return rc;
    orb_link_finish_brisk(c, d.rec, d.counters, cap, s.d_kp, s.d_desc, s.d_n, out.h_n, bb.h_bkp + (size_t)k * cap, out.h_desc);
    HIP_TRY(c, hipGetLastError());
  }
  if ((rc = pc.submit())) return rc;
  pc.count(0); pc.count(1);
  // (kept: the BRISK callers answer a detector overflow with SPVO_ERR_STATE -- the lists hold a candidate per interior pixel of every layer,
  // so the flag cannot be set; were it, the counts would be wrong)
  if (bb.h_n[1] || bb.h_n[5]) return fail(c, SPVO_ERR_STATE, "%s: the candidate list overflowed although it is sized from the image", who);
  static_assert(sizeof(spvo_brisk_keypoint) == sizeof(BriskDetKeypoint), "record layout");
  const PairMirror mirrors[2] = {{bb.h_bkp, sizeof(BriskDetKeypoint), bb.h_desc, (size_t)row_bytes},
                                 {bb.h_bkp + cap, sizeof(BriskDetKeypoint), bb.h_desc + (size_t)cap * row_bytes, (size_t)row_bytes}};
  return pc.commit(mirrors);
}
}  // namespace
extern "C" {

int spvo_brisk_detect_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int threshold, int octaves, int slot_l, int slot_r,
                           int slot_capacity, spvo_brisk_features *out_l, spvo_brisk_features *out_r) {
  return brisk_pair(c, "spvo_brisk_detect_pair", false, img_l, img_r, rows, cols, stride, threshold, octaves, slot_l, slot_r, slot_capacity, out_l, out_r);
}

// The BRISK detector with the ORB extractor at the keypoints' octaves, pair-resident: per image what spvo_brisk_detect followed by
// spvo_orb_describe_octaves(img = NULL) hands out, byte for byte, in slots of 32-byte rows
int spvo_brisk_orb_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int threshold, int octaves, int slot_l, int slot_r,
                        int slot_capacity, spvo_brisk_features *out_l, spvo_brisk_features *out_r) {
  return brisk_pair(c, "spvo_brisk_orb_pair", true, img_l, img_r, rows, cols, stride, threshold, octaves, slot_l, slot_r, slot_capacity, out_l, out_r);
}

// The BRISK detector with the SIFT extractor, pair-resident in the SIFT slots: per image what spvo_brisk_detect followed by
// spvo_sift_describe(img = NULL) on its records hands out, byte for byte.  The call is sift_link_pair's (spvo_sift.hip); the detector's
// part is bd_check, bd_ensure and, per image, bd_staged_enqueue -- the chain up to the refined records with their keep flags, which
// the link compacts in the detector's order.  A keypoint's octave is its layer, 0 .. 5, so the pyramid is built for octaves 0 .. 5.
int spvo_brisk_sift_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int threshold, int octaves, int slot_l, int slot_r,
                         int slot_capacity, spvo_sift_features *out_l, spvo_sift_features *out_r) {
  if (!c || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  static_assert(sizeof(spvo_sift_keypoint) == sizeof(BriskDetKeypoint), "record layout");
  const char *who = "spvo_brisk_sift_pair";
  auto &d = c->brisk_det;
  SiftLinkDetector det;
  det.who = who;
  det.max_octave = BRISK_DET_LAYERS - 1;
  det.check = [&]() -> int { return bd_check(c, who, rows, cols, threshold, octaves); };
  det.prepare = [&](SiftLinkSrc &src) -> int {
    if (int rc = bd_ensure(c, rows, cols)) return rc;
    src = SiftLinkSrc{reinterpret_cast<const char *>(d.rec.get()), (int)sizeof(BriskDetKeypoint), (int)offsetof(BriskDetKeypoint, x), (int)offsetof(BriskDetKeypoint, y),
                      (int)offsetof(BriskDetKeypoint, size), (int)offsetof(BriskDetKeypoint, angle), (int)offsetof(BriskDetKeypoint, response), (int)offsetof(BriskDetKeypoint, octave),
                      d.keep, d.counters + 1, d.cand_cap, d.counters, nullptr, 0};
    return SPVO_OK;
  };
  det.enqueue = [&](const uint8_t *h_img) -> int { return bd_staged_enqueue(c, h_img, rows, cols, threshold); };
  return sift_link_pair(c, det, img_l, img_r, rows, cols, stride, slot_l, slot_r, slot_capacity, pair_out(out_l), pair_out(out_r));
}

int spvo_brisk_detect_debug_layer(spvo_ctx *c, int layer, int what, uint8_t *out, int *rows, int *cols) {
  if (!c || !rows || !cols || layer < 0 || layer >= BRISK_DET_LAYERS || what < 0 || what > 2 || (what == 2 && layer != 0)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  auto &d = c->brisk_det;
  if (!d.valid || d.image_gen != c->cls.image_gen || c->cls.rows != d.rows || c->cls.cols != d.cols) return fail(c, SPVO_ERR_STATE, "spvo_brisk_detect_debug_layer: no spvo_brisk_detect result is resident");
  if (int rc = require_idle(c)) return rc;
  const BriskDetLayer &L = d.lv.l[layer];
  *rows = L.h; *cols = L.w;
  if (!out || L.h == 0 || L.w == 0) return SPVO_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const uint8_t *src = what == 0 ? (layer == 0 ? c->cls.im : L.im) : (what == 1 ? L.score : d.lv.score58);
  HIP_TRY(c, hipMemcpyAsync(out, src, (size_t)L.h * L.w, hipMemcpyDeviceToHost, c->stream2));
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  return SPVO_OK;
}

}  // extern "C"
