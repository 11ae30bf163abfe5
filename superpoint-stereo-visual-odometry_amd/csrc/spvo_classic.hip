// spvo_classic.hip -- the classic front end (ClassicFeatureFrontEnd, feature_detection_classic.cpp): the ORB detector / extractor (orb.hip.h),
// the Shi-Tomasi and FAST detectors and the ORB extractor for given keypoints (classic_detect.hip.h; at the keypoints' octaves: spvo_orb_describe_octaves), one submission per stereo pair into the
// binary feature slots (spvo_classic_detect; its BRISK kinds hand the detector's list to spvo_brisk.hip, and spvo_sift.hip takes the same
// detector link for spvo_classic_sift_pair), the ORB extractor as a device link behind a detector that reports octaves (orb_link.hip.h: orb_link_* for
// spvo_brisk_orb_pair / spvo_akaze_orb_pair, and the test hook spvo_orb_octaves_link_debug), the ORB detector in front of the BRISK extractor's chain and of the SIFT link
// (spvo_orb_brisk_pair, spvo_orb_sift_pair: orb_records_kernel), and spvo_preprocess for a context without an engine.  Everything here runs on the solver's stream (stream2) and owns its buffers (spvo_ctx::orb, spvo_ctx::cls).
#include "spvo_internal.hip.h"
#include "pair_call.hip.h"
#include "orb.hip.h"
#include "orb_link.hip.h"
#include "classic_detect.hip.h"

namespace {
// a host image of a strided view into the packed rows of `dst`, through the staging buffer `src` (grown on demand).  Of a strided view
// (a cv::Mat ROI) only (rows - 1) * stride + cols bytes are the caller's: the last row's padding may lie beyond the end of the parent allocation
int upload_strided(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, DevBuf<uint8_t> &src, uint8_t *dst, hipStream_t st) {
  const size_t src_bytes = (size_t)(rows - 1) * stride + cols;
  if (src_bytes > src.count())
    if (int rc = grow(c, wait_for(st), {plain(src, src_bytes)})) return rc;
  HIP_TRY(c, hipMemcpyAsync(src, img, src_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpy2DAsync(dst, cols, src, stride, cols, rows, hipMemcpyDeviceToDevice, st));
  return SPVO_OK;
}
}  // namespace

// A context without an engine (the classic front end with a fixed input size, classic.cpp:96-100): there is no network input
// plane to fill, only the crop + cv::resize(INTER_LINEAR) of the u8 image -- orb_resize_kernel is preprocess_kernel's arithmetic.
int spvo_int::classic_preprocess(spvo_ctx *c, const CropGeom &g, size_t stride) {
  auto &b = c->cls;
  const int H = c->H, W = c->W;
  if (!b.pre_out) {
    if (int rc = grow(c, wait_for_nothing(), {zeroed(b.pre_out, (size_t)H * W), zeroed(b.pre_tab, (size_t)3 * (H + W))})) return rc;
    b.pre_crop_rows = b.pre_crop_cols = 0;
  }
  const uint8_t *src = c->d_img[0] + (size_t)g.row_off * stride + g.col_off;
  if (g.crop_rows == H && g.crop_cols == W) {   // cv::resize copies when the sizes already match
    HIP_TRY(c, hipMemcpy2DAsync(b.pre_out, W, src, stride, W, H, hipMemcpyDeviceToDevice, c->stream));
    return SPVO_OK;
  }
  if (b.pre_crop_rows != g.crop_rows || b.pre_crop_cols != g.crop_cols) {
    std::vector<int> all;
    resize_tables(W, g.crop_cols, H, g.crop_rows, all);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(b.pre_tab, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice));
    b.pre_crop_rows = g.crop_rows; b.pre_crop_cols = g.crop_cols;
  }
  hipLaunchKernelGGL(orb_resize_kernel, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, c->stream, src, g.crop_rows, g.crop_cols, (int)stride, b.pre_out, H, W, b.pre_tab);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

extern "C" {

// ---------------------------------------------------------------- ORB (orb.hip.h)
namespace {
uint32_t host_hash32(uint32_t x) { x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16; return x; }
// the 256 test pairs: isotropic Gaussian of the original BRIEF (sigma = patch / 5), fixed seed, rounded, kept inside the patch
// (the same construction as oracle/cpu/orb_cpu.inc; tests/test_gpu_orb.py compares the two tables)
void orb_host_tables(std::vector<float> &pattern, float taps[7], std::vector<signed char> &disc) {
  constexpr int PATCH = 31, HALF = ORB_HALF;
  pattern.resize(1024);
  uint32_t state = 0x9E3779B9u;
  auto uni = [&]() { state = host_hash32(state + 0x6D2B79F5u); return ((state >> 8) + 0.5f) / 16777216.0f; };
  auto gauss = [&]() { const float u1 = uni(), u2 = uni(); return std::sqrt(-2.0f * std::log(u1)) * std::cos(6.2831853f * u2); };
  for (int i = 0; i < 1024; ++i) {
    float v = gauss() * (PATCH / 5.0f);
    v = std::min(std::max(v, -(float)(HALF - 2)), (float)(HALF - 2));
    pattern[i] = std::round(v);
  }
  float sum = 0;
  for (int i = 0; i < 7; ++i) { taps[i] = std::exp(-0.5f * (i - 3) * (i - 3) / 4.0f); sum += taps[i]; }
  for (int i = 0; i < 7; ++i) taps[i] /= sum;
  disc.clear();
  for (int dy = -HALF; dy <= HALF; ++dy) {
    const int lim = (int)std::floor(std::sqrt((double)HALF * HALF - dy * dy));
    for (int dx = -lim; dx <= lim; ++dx) { disc.push_back((signed char)dx); disc.push_back((signed char)dy); }
  }
}
// the descriptor's tables on the device (pattern, taps, disc), uploaded once per context
int orb_ensure_tables(spvo_ctx *c) {
  auto &o = c->orb;
  if (o.pattern) return SPVO_OK;
  std::vector<float> pat;
  std::vector<signed char> disc;
  float taps[7];
  orb_host_tables(pat, taps, disc);
  if (int rc = grow(c, wait_for_nothing(), {zeroed(o.pattern, 1024), zeroed(o.taps, 8), zeroed(o.disc, disc.size())})) return rc;
  HIP_TRY(c, hipMemcpy(o.pattern, pat.data(), 1024 * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(o.taps, taps, 7 * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(o.disc, disc.data(), disc.size(), hipMemcpyHostToDevice));
  return SPVO_OK;
}
}  // namespace

int spvo_orb_tables(float *pattern, float *taps) {
  std::vector<float> p;
  std::vector<signed char> d;
  float t[7];
  orb_host_tables(p, t, d);
  if (pattern) std::memcpy(pattern, p.data(), 1024 * sizeof(float));
  if (taps) std::memcpy(taps, t, sizeof t);
  return SPVO_OK;
}

namespace {
// level geometry and per-level quota of an image (the reference's parameters: 8 levels, scale 1.2), and where a level lies in the buffers
struct OrbPlan {
  int ph[ORB_LEVELS], pw[ORB_LEVELS], want[ORB_LEVELS];
  float lscale[ORB_LEVELS];
  size_t off[ORB_LEVELS + 1], toff[ORB_LEVELS];
  int surv_cap;
};

// the plan of a rows x cols image, every buffer grown to what it needs, the resize tables and the descriptor's tables on the device
int orb_prepare(spvo_ctx *c, int rows, int cols, int nfeatures, OrbPlan &p) {
  hipStream_t st = c->stream2;
  auto &o = c->orb;
  constexpr float SCALE = 1.2f;
  int *ph = p.ph, *pw = p.pw, *want = p.want;
  float *lscale = p.lscale;
  size_t *off = p.off;
  {
    float scale = 1.f;
    const float f = 1.0f / SCALE;
    float n_level = nfeatures * (1 - f) / (1 - std::pow(f, (float)ORB_LEVELS));
    int assigned = 0;
    off[0] = 0;
    for (int l = 0; l < ORB_LEVELS; ++l, scale *= SCALE) {
      ph[l] = (int)std::lround(rows / scale); pw[l] = (int)std::lround(cols / scale);
      lscale[l] = scale;
      want[l] = l == ORB_LEVELS - 1 ? std::max(nfeatures - assigned, 0) : (int)std::lround(n_level);
      assigned += want[l];
      n_level *= f;
      off[l + 1] = off[l] + (((size_t)ph[l] * pw[l] + 255) & ~(size_t)255);
    }
  }
  const int surv_cap = p.surv_cap = (rows / 2 + 1) * (cols / 2 + 1);   // 3x3 suppression: at most one survivor per 2x2 block
  const int kp_cap = nfeatures;
  // what THIS image needs: the pyramid (all levels side by side), one key / rank entry per possible survivor of every level, the
  // resize tables of levels 1..7.  All three depend on rows and cols separately (a 100 x 1500 image needs longer tables than a
  // 400 x 400 one although it has fewer pixels), so each is compared with what is allocated.
  size_t need_keys = 0, need_tab = 0;
  for (int l = 0; l < ORB_LEVELS; ++l) {
    need_keys += (size_t)std::min(surv_cap, (ph[l] / 2 + 1) * (pw[l] / 2 + 1));
    if (l > 0) need_tab += (size_t)3 * (pw[l] + ph[l]);
  }
  const size_t need_pyr = off[ORB_LEVELS] + 256;
  if (need_pyr > o.pyr_cap || need_keys > o.key_cap || need_tab > o.tab_cap || kp_cap > o.kp_cap) {
    const size_t pyr = std::max(need_pyr, o.pyr_cap), kall = std::max(need_keys, o.key_cap), tabn = std::max(need_tab, o.tab_cap);
    const int kpn = std::max(kp_cap, o.kp_cap);
    o.pyr_cap = o.key_cap = o.tab_cap = 0; o.kp_cap = 0;   // a failed allocation below leaves a context that spvo_destroy and a later call can still handle
    if (int rc = grow(c, wait_for(st), {zeroed(o.im, pyr), zeroed(o.score, pyr), zeroed(o.blur, pyr), zeroed(o.tmp, pyr), zeroed(o.keys, kall), zeroed(o.rank, kall),
                                        zeroed(o.out_xy, 2 * kall), zeroed(o.counters, (size_t)ORB_LEVELS * NMS_COUNTER_INTS), zeroed(o.tab, tabn), zeroed(o.kps, kpn),
                                        zeroed(o.desc, (size_t)kpn * 32)}))
      return rc;
    o.pyr_cap = pyr; o.key_cap = kall; o.tab_cap = tabn; o.kp_cap = kpn;
    o.tab_rows = o.tab_cols = 0;
  }
  // resize tables of all levels, one upload per image size
  {
    size_t t = 0;
    p.toff[0] = 0;
    for (int l = 1; l < ORB_LEVELS; ++l) { p.toff[l] = t; t += (size_t)3 * (pw[l] + ph[l]); }
    if (o.tab_rows != rows || o.tab_cols != cols) {
      std::vector<int> all;
      for (int l = 1; l < ORB_LEVELS; ++l) resize_tables(pw[l], pw[l - 1], ph[l], ph[l - 1], all);
      HIP_TRY(c, hipStreamSynchronize(st));
      HIP_TRY(c, hipMemcpy(o.tab, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice));
      o.tab_rows = rows; o.tab_cols = cols;
    }
  }
  return orb_ensure_tables(c);
}

// The image in level 0 (`im0`: o.im, or the resident image of spvo_ctx::cls for the pair calls whose extractor looks there -- levels 1 .. 7
// and level 0's score / blur / tmp are ORB's own either way) -> keypoint records and descriptors in `kps` / `desc` (kp_cap rows), enqueued
// without a host round trip: the pyramid level by level, then every stage once for all levels; one counter block per level, a level's
// keypoints land behind those of the levels below (orb_describe_kernel sums their counts)
int orb_enqueue(spvo_ctx *c, const OrbPlan &p, int rows, int cols, uint8_t *im0, OrbKeypoint *kps, uint8_t *desc, int kp_cap) {
  hipStream_t st = c->stream2;
  auto &o = c->orb;
  const int *ph = p.ph, *pw = p.pw;
  HIP_TRY(c, hipMemsetAsync(o.counters, 0, (size_t)ORB_LEVELS * NMS_COUNTER_INTS * sizeof(int), st));
  OrbLevels lv;
  size_t koff = 0;
  int want_max = 0;
  for (int l = 0; l < ORB_LEVELS; ++l) {
    OrbLevel &L = lv.l[l];
    const int lcap = std::min(p.surv_cap, (ph[l] / 2 + 1) * (pw[l] / 2 + 1));
    L.im = l == 0 ? im0 : o.im + p.off[l]; L.score = o.score + p.off[l]; L.blur = o.blur + p.off[l]; L.tmp = o.tmp + p.off[l];
    L.keys = o.keys + koff; L.rank = o.rank + koff; L.out_xy = o.out_xy + 2 * koff; L.counters = o.counters + l * NMS_COUNTER_INTS;
    L.h = ph[l]; L.w = pw[l]; L.cap = lcap; L.scale = p.lscale[l];
    L.want = (ph[l] <= 2 * ORB_EDGE + 2 || pw[l] <= 2 * ORB_EDGE + 2) ? 0 : p.want[l];
    want_max = std::max(want_max, L.want);
    koff += lcap;
    if (l > 0) hipLaunchKernelGGL(orb_resize_kernel, dim3((pw[l] + 63) / 64, (ph[l] + 3) / 4), dim3(256), 0, st, lv.l[l - 1].im, ph[l - 1], pw[l - 1], pw[l - 1], L.im, ph[l], pw[l],
                                  o.tab + p.toff[l]);
  }
  if (want_max > 0) {
    const dim3 grid((cols + 63) / 64, (rows + 3) / 4, ORB_LEVELS);
    hipLaunchKernelGGL(orb_fast_kernel, grid, dim3(256), 0, st, lv, ORB_FAST_T, ORB_EDGE);
    hipLaunchKernelGGL(orb_collect_kernel, grid, dim3(256), 0, st, lv);
    hipLaunchKernelGGL(orb_rank_kernel, dim3(128, ORB_LEVELS), dim3(256), 0, st, lv);
    hipLaunchKernelGGL(orb_write_kernel, dim3(32, ORB_LEVELS), dim3(256), 0, st, lv);
    hipLaunchKernelGGL(orb_blur_h_kernel, grid, dim3(256), 0, st, lv, o.taps);
    hipLaunchKernelGGL(orb_blur_v_kernel, grid, dim3(256), 0, st, lv, o.taps);
    hipLaunchKernelGGL(orb_describe_kernel, dim3((want_max + 3) / 4, ORB_LEVELS), dim3(256), 0, st, lv, o.disc, o.pattern, kps, desc, kp_cap);
  }
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// The extractor's levels 0 .. top of the image resident in spvo_ctx::cls (spvo_orb_describe_octaves, orb_link_enqueue): level 0 is that image
// itself (its image, smoothed image and scratch), levels 1 .. top live in spvo_ctx::orb's pyramid buffers with orb_prepare's geometry and
// resize tables.  At most 7 resize launches, then the two smoothing launches over all of them; want[l] = 0 skips the smoothing of level l
// (a level's bytes do not depend on who reads them).  -> the levels, for the describe launch that follows
// (static: this namespace lies inside extern "C", where the library would export the name; its exported symbols stay as they are)
static OrbLevels orb_levels_enqueue(spvo_ctx *c, const OrbPlan &plan, int rows, int cols, int top, const int *want) {
  auto &b = c->cls;
  auto &o = c->orb;
  hipStream_t st = c->stream2;
  OrbLevels lv{};
  for (int l = 0; l <= top; ++l) {
    OrbLevel &L = lv.l[l];
    if (l == 0) { L.im = b.im; L.blur = b.blur; L.tmp = b.tmp; }
    else { L.im = o.im + plan.off[l]; L.blur = o.blur + plan.off[l]; L.tmp = o.tmp + plan.off[l]; }
    L.h = plan.ph[l]; L.w = plan.pw[l]; L.scale = plan.lscale[l];
    L.want = L.cap = want[l];
    if (l > 0)
      hipLaunchKernelGGL(orb_resize_kernel, dim3((L.w + 63) / 64, (L.h + 3) / 4), dim3(256), 0, st, lv.l[l - 1].im, plan.ph[l - 1], plan.pw[l - 1], plan.pw[l - 1], L.im, L.h, L.w,
                         o.tab + plan.toff[l]);
  }
  const dim3 grid((cols + 63) / 64, (rows + 3) / 4, top + 1);
  hipLaunchKernelGGL(orb_blur_h_kernel, grid, dim3(256), 0, st, lv, o.taps);
  hipLaunchKernelGGL(orb_blur_v_kernel, grid, dim3(256), 0, st, lv, o.taps);
  return lv;
}
}  // namespace

int spvo_orb_detect(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, int nfeatures, spvo_orb_keypoint *kps, uint8_t *desc, int cap, int *n_out) {
  if (!c || !img || !n_out || rows <= 0 || cols <= 0 || stride < (size_t)cols || nfeatures <= 0 || cap < 0 || (cap > 0 && (!kps || !desc)))
    return fail(c, SPVO_ERR_INVALID, "bad argument");
  static_assert(sizeof(spvo_orb_keypoint) == sizeof(OrbKeypoint), "keypoint records differ");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  *n_out = 0;
  hipStream_t st = c->stream2;
  auto &o = c->orb;
  const int kp_cap = nfeatures;
  OrbPlan plan;
  if (int rc = orb_prepare(c, rows, cols, nfeatures, plan)) return rc;
  if (int rc = upload_strided(c, img, rows, cols, stride, o.src, o.im, st)) return rc;   // level 0: the image, rows packed
  if (int rc = orb_enqueue(c, plan, rows, cols, o.im, o.kps, o.desc, kp_cap)) return rc;
  int cnt[ORB_LEVELS * NMS_COUNTER_INTS];
  HIP_TRY(c, hipMemcpyAsync(cnt, o.counters, sizeof cnt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  int base = 0;
  for (int l = 0; l < ORB_LEVELS; ++l) {
    if (cnt[l * NMS_COUNTER_INTS + 3]) return fail(c, SPVO_ERR_CAPACITY, "ORB: corner buffer overflow at level %d", l);
    base += cnt[l * NMS_COUNTER_INTS + 2];
  }
  base = std::min(base, kp_cap);
  *n_out = base;
  const int ncopy = std::min(base, cap);
  if (ncopy > 0) {
    HIP_TRY(c, hipMemcpyAsync(kps, o.kps, (size_t)ncopy * sizeof(OrbKeypoint), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(desc, o.desc, (size_t)ncopy * 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  return SPVO_OK;
}

// ---------------------------------------------------------------- Shi-Tomasi, FAST, ORB extractor (classic_detect.hip.h)
namespace {
// every buffer of the Shi-Tomasi / FAST detectors grown to what a rows x cols image needs; no image is resident afterwards
int cls_ensure(spvo_ctx *c, int rows, int cols) {
  auto &b = c->cls;
  hipStream_t st = c->stream2;
  const size_t px = (size_t)rows * cols, state_bytes = (size_t)(rows + 2 * CLS_PAD) * cls_state_pitch(cols);
  b.rows = b.cols = 0;   // nothing resident until the upload below is enqueued
  ++b.image_gen;
  if (px > b.px_cap || state_bytes > b.state_cap) {
    const size_t npx = std::max(px, b.px_cap), nst = std::max(state_bytes, b.state_cap);
    b.px_cap = b.state_cap = 0;   // a failed allocation below leaves a context that spvo_destroy and a later call can still handle
    b.state_rows = b.state_cols = 0;
    if (int rc = grow(c, wait_for(st), {zeroed(b.im, npx + 256), zeroed(b.score, npx + 256), zeroed(b.blur, npx + 256), zeroed(b.state, nst), zeroed(b.tmp, npx), zeroed(b.lam, npx),
                                        zeroed(b.xy, 2 * npx), zeroed(b.resp, npx), zeroed(b.keys, npx), zeroed(b.rank, npx), zeroed(b.cand, npx)}))
      return rc;
    b.px_cap = npx; b.state_cap = nst;
  }
  if (!b.counters) return grow(c, wait_for_nothing(), {zeroed(b.counters, CLS_COUNTER_INTS)});
  return SPVO_OK;
}

// the image into the context's level-0 buffer (rows packed), every buffer grown to what this image needs
int cls_prepare(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride) {
  auto &b = c->cls;
  if (int rc = cls_ensure(c, rows, cols)) return rc;
  if (int rc = upload_strided(c, img, rows, cols, stride, b.src, b.im, c->stream2)) return rc;
  b.rows = rows; b.cols = cols;
  return SPVO_OK;
}

// the resident image -> Shi-Tomasi corners in b.xy / b.resp, their number in b.counters[2]
int gftt_enqueue(spvo_ctx *c, int rows, int cols, int max_corners, double quality_level, double min_distance) {
  auto &b = c->cls;
  hipStream_t st = c->stream2;
  // dx^2 + dy^2 < min_distance^2 on integer coordinates: <= lim (OpenCV compares in float: min_distance as float, squared in float)
  const float mdf = (float)min_distance;
  const int lim = (int)std::ceil((double)mdf * (double)mdf) - 1;
  const int radius = lim > 0 ? (int)std::floor(std::sqrt((double)lim)) : 0;
  const int want = max_corners > 0 ? max_corners : 0x7FFFFFFF;   // (cv::goodFeaturesToTrack: max_corners <= 0 is "no limit")
  const int key_cap = (int)std::min<size_t>((size_t)rows * cols, 0x7FFFFFFF);
  HIP_TRY(c, hipMemsetAsync(b.counters, 0, CLS_COUNTER_INTS * sizeof(int), st));
  if (b.state_rows != rows || b.state_cols != cols) {   // the padding of the state map: cleared once per shape (the kernels write the image's own bytes only)
    HIP_TRY(c, hipMemsetAsync(b.state, 0, (size_t)(rows + 2 * CLS_PAD) * cls_state_pitch(cols), st));
    b.state_rows = rows; b.state_cols = cols;
  }
  const dim3 grid((cols + 63) / 64, (rows + 3) / 4);
  hipLaunchKernelGGL(gftt_response_kernel, grid, dim3(256), 0, st, b.im, rows, cols, b.lam, b.counters);
  hipLaunchKernelGGL(gftt_collect_kernel, grid, dim3(256), 0, st, b.lam, rows, cols, quality_level, b.state, b.cand, b.counters);
  for (int l = 0; l < CLS_ROUND_LAUNCHES; ++l)
    hipLaunchKernelGGL(gftt_round_kernel<4>, dim3(64), dim3(256), 0, st, b.lam, cols, radius, lim, b.state, b.cand, b.keys, key_cap, b.counters, l);
  hipLaunchKernelGGL(gftt_finish_kernel, dim3(1), dim3(1024), 0, st, b.lam, cols, radius, lim, b.state, b.cand, b.keys, key_cap, b.counters, CLS_ROUND_LAUNCHES);
  hipLaunchKernelGGL(cls_rank_kernel, dim3(128), dim3(256), 0, st, b.keys, b.rank, b.counters + 1, key_cap);
  hipLaunchKernelGGL(gftt_write_kernel, dim3(32), dim3(256), 0, st, b.lam, cols, b.keys, b.rank, key_cap, want, (float)(0.5 / (5100.0 * 5100.0)), b.xy, b.resp, b.counters);
  return SPVO_OK;
}

// the resident image -> FAST corners in b.xy / b.resp (raster order), their number in b.counters[2]
int fast_enqueue(spvo_ctx *c, int rows, int cols, int threshold, int nonmax_suppression) {
  auto &b = c->cls;
  hipStream_t st = c->stream2;
  const int key_cap = (int)std::min<size_t>((size_t)rows * cols, 0x7FFFFFFF);   // no cap in the reference: with suppression off every pixel can be a corner
  HIP_TRY(c, hipMemsetAsync(b.counters, 0, CLS_COUNTER_INTS * sizeof(int), st));
  OrbLevels lv{};
  lv.l[0].im = b.im; lv.l[0].score = b.score; lv.l[0].h = rows; lv.l[0].w = cols; lv.l[0].want = 1; lv.l[0].scale = 1.f;
  const dim3 grid((cols + 63) / 64, (rows + 3) / 4, 1);
  hipLaunchKernelGGL(orb_fast_kernel, grid, dim3(256), 0, st, lv, threshold, 3);
  hipLaunchKernelGGL(fast_collect_kernel, grid, dim3(256), 0, st, b.score, rows, cols, nonmax_suppression ? 1 : 0, b.keys, key_cap, b.counters);
  hipLaunchKernelGGL(cls_rank_kernel, dim3(128), dim3(256), 0, st, b.keys, b.rank, b.counters + 1, key_cap);
  hipLaunchKernelGGL(fast_write_kernel, dim3(32), dim3(256), 0, st, cols, b.keys, b.rank, key_cap, b.xy, b.resp, b.counters);
  return SPVO_OK;
}

// What the per-image entry points refuse, for every entry point that runs the same detector (`who` names it in the error text)
int gftt_check(spvo_ctx *c, const char *who, int rows, int cols, double quality_level, double min_distance, int block_size) {
  if (rows < 8 || cols < 8 || !(quality_level > 0)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (block_size != 5 || !(min_distance >= 0 && min_distance <= 15)) return fail(c, SPVO_ERR_INVALID, "%s: block_size 5 and min_distance <= 15 only", who);
  return SPVO_OK;
}
int fast_check(spvo_ctx *c, int threshold) { return threshold < 0 || threshold > 255 ? fail(c, SPVO_ERR_INVALID, "bad argument") : SPVO_OK; }

// orb.hip.h's extractor on a one-level OrbLevels over the resident image (spvo_ctx::cls) whose keypoint list is `out_xy` and whose count is
// counters[2]: 7x7 blur of level 0, then direction + steered tests of the first `rows_covered` keypoints into d_kp / d_desc (kp_cap rows)
void orb_extract_one_level(spvo_ctx *c, int rows, int cols, int *out_xy, int *counters, int rows_covered, OrbKeypoint *d_kp, uint8_t *d_desc, int kp_cap) {
  auto &b = c->cls;
  auto &o = c->orb;
  hipStream_t st = c->stream2;
  OrbLevels lv{};
  OrbLevel &L = lv.l[0];
  L.im = b.im; L.score = b.score; L.blur = b.blur; L.tmp = b.tmp; L.out_xy = out_xy; L.counters = counters;
  L.h = rows; L.w = cols; L.want = rows_covered; L.cap = rows_covered; L.scale = 1.f;
  const dim3 grid((cols + 63) / 64, (rows + 3) / 4, 1);
  hipLaunchKernelGGL(orb_blur_h_kernel, grid, dim3(256), 0, st, lv, o.taps);
  hipLaunchKernelGGL(orb_blur_v_kernel, grid, dim3(256), 0, st, lv, o.taps);
  hipLaunchKernelGGL(orb_describe_kernel, dim3((rows_covered + 3) / 4, 1), dim3(256), 0, st, lv, o.disc, o.pattern, d_kp, d_desc, kp_cap);
}

// counters -> host, then min(n, cap) keypoints
int cls_read_out(spvo_ctx *c, float *xy, float *response, int cap, int *n_out, const char *what) {
  auto &b = c->cls;
  hipStream_t st = c->stream2;
  HIP_TRY(c, hipGetLastError());
  int cnt[CLS_COUNTER_INTS];
  HIP_TRY(c, hipMemcpyAsync(cnt, b.counters, sizeof cnt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  std::memcpy(b.last_counters, cnt, sizeof cnt);
  if (cnt[3]) return fail(c, SPVO_ERR_CAPACITY, "%s: key buffer overflow", what);
  *n_out = cnt[2];
  const int ncopy = std::min(cnt[2], cap);
  if (ncopy > 0) {
    HIP_TRY(c, hipMemcpyAsync(xy, b.xy, (size_t)ncopy * 2 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (response) HIP_TRY(c, hipMemcpyAsync(response, b.resp, (size_t)ncopy * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  return SPVO_OK;
}
}  // namespace

int spvo_gftt_detect(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, int max_corners, double quality_level, double min_distance, int block_size,
                     float *xy, float *response, int cap, int *n_out) {
  if (!c || !img || !n_out || stride < (size_t)cols || cap < 0 || (cap > 0 && !xy)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (int rc = gftt_check(c, "spvo_gftt_detect", rows, cols, quality_level, min_distance, block_size)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  *n_out = 0;
  if (int rc = cls_prepare(c, img, rows, cols, stride)) return rc;
  if (int rc = gftt_enqueue(c, rows, cols, max_corners, quality_level, min_distance)) return rc;
  return cls_read_out(c, xy, response, cap, n_out, "spvo_gftt_detect");
}

int spvo_gftt_last_rounds(spvo_ctx *c, int *undecided_after_launch /* [3] */, int *finish_rounds) {
  if (!c) return fail(c, SPVO_ERR_INVALID, "null context");
  for (int l = 0; l < CLS_ROUND_LAUNCHES; ++l) if (undecided_after_launch) undecided_after_launch[l] = c->cls.last_counters[8 + l];
  if (finish_rounds) *finish_rounds = c->cls.last_counters[5];
  return SPVO_OK;
}

int spvo_fast_detect(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, int threshold, int nonmax_suppression, float *xy, float *response, int cap,
                     int *n_out) {
  if (!c || !img || !n_out || rows <= 0 || cols <= 0 || stride < (size_t)cols || cap < 0 || (cap > 0 && !xy)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (int rc = fast_check(c, threshold)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  *n_out = 0;
  if (int rc = cls_prepare(c, img, rows, cols, stride)) return rc;
  if (int rc = fast_enqueue(c, rows, cols, threshold, nonmax_suppression)) return rc;
  return cls_read_out(c, xy, response, cap, n_out, "spvo_fast_detect");
}

int spvo_orb_describe(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, const float *xy, int n, int32_t *kept, float *angle, uint8_t *desc, int *n_kept) {
  if (!c || !n_kept || rows <= 0 || cols <= 0 || n < 0 || (n > 0 && (!xy || !kept || !desc)) || (img && stride < (size_t)cols)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  *n_kept = 0;
  auto &b = c->cls;
  if (!img && (b.rows != rows || b.cols != cols))
    return fail(c, SPVO_ERR_STATE, "spvo_orb_describe: no image of %d x %d is resident (call spvo_gftt_detect / spvo_fast_detect first, or pass the image)", rows, cols);
  // cv::ORB::compute drops, order-preserving, what is closer than 31 pixels to a border; coordinates must be integers (no rounding rule is invented)
  std::vector<int> kxy;
  kxy.reserve((size_t)n * 2);
  int nk = 0;
  for (int i = 0; i < n; ++i) {
    const float x = xy[2 * i], y = xy[2 * i + 1];
    if (!(x == std::floor(x)) || !(y == std::floor(y)) || std::fabs(x) > 1e9f || std::fabs(y) > 1e9f)
      return fail(c, SPVO_ERR_INVALID, "spvo_orb_describe: keypoint %d (%g, %g) is not at integer coordinates", i, (double)x, (double)y);
    const int xi = (int)x, yi = (int)y;
    if (xi < ORB_EDGE || xi >= cols - ORB_EDGE || yi < ORB_EDGE || yi >= rows - ORB_EDGE) continue;
    kept[nk++] = i;
    kxy.push_back(xi); kxy.push_back(yi);
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream2;
  if (img) {
    if (int rc = cls_prepare(c, img, rows, cols, stride)) return rc;
  }
  *n_kept = nk;
  if (nk == 0) {
    HIP_TRY(c, hipStreamSynchronize(st));   // (the caller's image may be in flight)
    return SPVO_OK;
  }
  if (int rc = orb_ensure_tables(c)) return rc;
  if (nk > b.kp_cap) {
    b.kp_cap = 0;
    if (int rc = grow(c, wait_for(st), {zeroed(b.kp_xy, (size_t)2 * nk), zeroed(b.kps, (size_t)nk), zeroed(b.desc, (size_t)nk * 32)})) return rc;
    b.kp_cap = nk;
  }
  int cnt[CLS_COUNTER_INTS] = {0};
  cnt[2] = nk;
  HIP_TRY(c, hipMemcpyAsync(b.counters, cnt, sizeof cnt, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(b.kp_xy, kxy.data(), (size_t)2 * nk * sizeof(int), hipMemcpyHostToDevice, st));
  orb_extract_one_level(c, rows, cols, b.kp_xy, b.counters, nk, b.kps, b.desc, nk);   // the keypoint list is the caller's
  HIP_TRY(c, hipGetLastError());
  std::vector<OrbKeypoint> kp((size_t)nk);
  HIP_TRY(c, hipMemcpyAsync(kp.data(), b.kps, (size_t)nk * sizeof(OrbKeypoint), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(desc, b.desc, (size_t)nk * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (angle) for (int i = 0; i < nk; ++i) angle[i] = kp[i].angle;
  return SPVO_OK;
}

// The extractor on keypoints that carry an octave (tests/orb_octaves_ref.py is the definition).  Level 0 is the resident image itself
// (spvo_ctx::cls: its image, smoothed image and scratch), levels 1 .. top live in spvo_ctx::orb's pyramid buffers, whose geometry and
// resize tables are orb_prepare's -- the levels are spvo_orb_detect's by construction.  At most 7 resize launches, the two smoothing
// launches (a level without a kept keypoint has want = 0 and is skipped) and one describe launch, one wait at the end.
int spvo_orb_describe_octaves(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, const float *xy, const int32_t *octave, int n, int32_t *kept, float *angle,
                              uint8_t *desc, int *n_kept) {
  if (!c || !n_kept || rows <= 0 || cols <= 0 || n < 0 || (n > 0 && (!xy || !octave || !kept || !desc)) || (img && stride < (size_t)cols)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  // every refusal first: nothing on the device and nothing in the outputs is touched by a call that fails here
  float lscale[ORB_LEVELS];
  int ph[ORB_LEVELS], pw[ORB_LEVELS], per_level[ORB_LEVELS] = {0};
  {
    float scale = 1.f;
    for (int l = 0; l < ORB_LEVELS; ++l, scale *= 1.2f) {   // (orb_prepare's geometry; spvo_orb_detect's)
      lscale[l] = scale;
      ph[l] = (int)std::lround(rows / scale); pw[l] = (int)std::lround(cols / scale);
    }
  }
  for (int i = 0; i < n; ++i) {
    const int o = octave[i];
    if (o < 0 || o >= ORB_LEVELS) return fail(c, SPVO_ERR_INVALID, "spvo_orb_describe_octaves: keypoint %d has octave %d; the pyramid has levels 0 .. %d", i, o, ORB_LEVELS - 1);
    if (!std::isfinite(xy[2 * i]) || !std::isfinite(xy[2 * i + 1]))
      return fail(c, SPVO_ERR_INVALID, "spvo_orb_describe_octaves: keypoint %d is (%g, %g)", i, (double)xy[2 * i], (double)xy[2 * i + 1]);
    if (ph[o] < ORB_MIN_LEVEL || pw[o] < ORB_MIN_LEVEL)
      return fail(c, SPVO_ERR_INVALID, "spvo_orb_describe_octaves: keypoint %d names octave %d, whose level is %d x %d: levels of at least %d x %d only", i, o, ph[o], pw[o], ORB_MIN_LEVEL,
                  ORB_MIN_LEVEL);
  }
  if (int rc = require_idle(c)) return rc;
  auto &b = c->cls;
  if (!img && (b.rows != rows || b.cols != cols))
    return fail(c, SPVO_ERR_STATE, "spvo_orb_describe_octaves: no image of %d x %d is resident (call a detector first, or pass the image)", rows, cols);
  // cv::ORB::compute: the border rule at level 0 (coordinates rounded half to even), then the survivors grouped by level, stable
  std::vector<int> pass;
  pass.reserve((size_t)n);
  for (int i = 0; i < n; ++i) {
    const float xi = std::rint(xy[2 * i]), yi = std::rint(xy[2 * i + 1]);
    if (xi < (float)ORB_EDGE || xi >= (float)(cols - ORB_EDGE) || yi < (float)ORB_EDGE || yi >= (float)(rows - ORB_EDGE)) continue;
    pass.push_back(i);
    ++per_level[octave[i]];
  }
  const int nk = (int)pass.size();
  int first[ORB_LEVELS], top = 0;
  for (int l = 0, at = 0; l < ORB_LEVELS; ++l) {
    first[l] = at;
    at += per_level[l];
    if (per_level[l]) top = l;
  }
  std::vector<int> rec((size_t)3 * nk);
  for (int i : pass) {   // (a kept keypoint lies within the level-0 image, so x / scale fits an int)
    const int l = octave[i], r = first[l]++;
    kept[r] = i;
    rec[3 * r] = std::min(std::max((int)std::rint(xy[2 * i] / lscale[l]), 0), pw[l] - 1);
    rec[3 * r + 1] = std::min(std::max((int)std::rint(xy[2 * i + 1] / lscale[l]), 0), ph[l] - 1);
    rec[3 * r + 2] = l;
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream2;
  if (img) {
    if (int rc = cls_prepare(c, img, rows, cols, stride)) return rc;
  }
  *n_kept = nk;
  if (nk == 0) {
    HIP_TRY(c, hipStreamSynchronize(st));   // (the caller's image may be in flight)
    return SPVO_OK;
  }
  auto &o = c->orb;
  OrbPlan plan;
  if (int rc = orb_prepare(c, rows, cols, 1, plan)) return rc;   // (no keypoint buffer of spvo_orb_detect's is used: nfeatures 1 grows none)
  if (nk > b.oct_cap) {
    b.oct_cap = 0;
    if (int rc = grow(c, wait_for(st), {zeroed(b.oct_rec, (size_t)3 * nk), zeroed(b.oct_angle, (size_t)nk), zeroed(b.oct_desc, (size_t)nk * 32)})) return rc;
    b.oct_cap = nk;
  }
  HIP_TRY(c, hipMemcpyAsync(b.oct_rec, rec.data(), rec.size() * sizeof(int), hipMemcpyHostToDevice, st));
  const OrbLevels lv = orb_levels_enqueue(c, plan, rows, cols, top, per_level);   // (a level without a kept keypoint is not smoothed)
  hipLaunchKernelGGL(orb_describe_given_kernel, dim3((nk + 3) / 4), dim3(256), 0, st, lv, b.oct_rec, nk, o.disc, o.pattern, b.oct_angle, b.oct_desc);
  HIP_TRY(c, hipGetLastError());
  if (angle) HIP_TRY(c, hipMemcpyAsync(angle, b.oct_angle, (size_t)nk * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(desc, b.oct_desc, (size_t)nk * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));   // the one wait of the call
  return SPVO_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the same extractor behind a detector's list on the device (orb_link.hip.h)
namespace {
// the link's buffers for `cap` rows (and, for the test hook, a list of `n_src` records with its keep flags)
int orb_link_buffers(spvo_ctx *c, int cap, int n_src) {
  auto &b = c->cls;
  if (!b.lnk_cnt)
    if (int rc = grow(c, wait_for_nothing(), {zeroed(b.lnk_cnt, ORB_LINK_INTS)})) return rc;
  if (cap > b.lnk_cap) {
    b.lnk_cap = 0;
    if (int rc = grow(c, wait_for(c->stream2), {plain(b.lnk_kept, (size_t)cap), plain(b.lnk_rec, (size_t)3 * cap), plain(b.lnk_angle, (size_t)cap), plain(b.lnk_desc, (size_t)cap * 32)})) return rc;
    b.lnk_cap = cap;
  }
  if (n_src > b.lnk_src_cap) {
    b.lnk_src_cap = 0;
    if (int rc = grow(c, wait_for(c->stream2), {plain(b.lnk_src, (size_t)3 * n_src), plain(b.lnk_keep, (size_t)n_src)})) return rc;
    b.lnk_src_cap = n_src;
  }
  return SPVO_OK;
}
}  // namespace

int spvo_int::orb_link_check(spvo_ctx *c, const char *who, int rows, int cols, int max_octave) {
  if (max_octave < 0 || max_octave >= ORB_LEVELS) return fail(c, SPVO_ERR_INVALID, "%s: max_octave %d; the pyramid has levels 0 .. %d", who, max_octave, ORB_LEVELS - 1);
  float scale = 1.f;
  for (int l = 0; l < max_octave; ++l) scale *= 1.2f;   // (orb_prepare's geometry)
  const int h = (int)std::lround(rows / scale), w = (int)std::lround(cols / scale);
  if (h < ORB_MIN_LEVEL || w < ORB_MIN_LEVEL)
    return fail(c, SPVO_ERR_INVALID, "%s: level %d of a %d x %d image is %d x %d: levels of at least %d x %d only", who, max_octave, rows, cols, h, w, ORB_MIN_LEVEL, ORB_MIN_LEVEL);
  return SPVO_OK;
}

int spvo_int::orb_link_ensure(spvo_ctx *c, int rows, int cols, int cap) {
  OrbPlan plan;
  if (int rc = orb_prepare(c, rows, cols, 1, plan)) return rc;   // (no keypoint buffer of spvo_orb_detect's is used: nfeatures 1 grows none)
  return orb_link_buffers(c, cap, 0);
}

// Smoothing: EVERY level 0 .. max_octave is built and smoothed, whether a record names it or not -- the host cannot know the counts, and a
// level's bytes do not depend on who reads them, so the rows equal spvo_orb_describe_octaves', which skips what lies above its `top`.
int spvo_int::orb_link_enqueue(spvo_ctx *c, int rows, int cols, int max_octave, const OrbLinkSrc &src, int cap, uint8_t *desc) {
  auto &b = c->cls;
  auto &o = c->orb;
  hipStream_t st = c->stream2;
  OrbPlan plan;
  if (int rc = orb_prepare(c, rows, cols, 1, plan)) return rc;   // (sized by orb_link_ensure: the plan only)
  OrbLinkGeom g{};
  for (int l = 0; l < ORB_LEVELS; ++l) { g.h[l] = plan.ph[l]; g.w[l] = plan.pw[l]; g.lscale[l] = plan.lscale[l]; }
  hipLaunchKernelGGL(orb_link_group_kernel, dim3(1), dim3(1024), 0, st, src, rows, cols, std::min(max_octave, ORB_LEVELS - 1), g, cap, b.lnk_kept, b.lnk_rec, b.lnk_cnt);
  int smoothed[ORB_LEVELS];
  std::fill(smoothed, smoothed + ORB_LEVELS, 1);
  const OrbLevels lv = orb_levels_enqueue(c, plan, rows, cols, max_octave, smoothed);
  hipLaunchKernelGGL(orb_link_describe_kernel, dim3(std::min((cap + 3) / 4, 1024)), dim3(256), 0, st, lv, b.lnk_rec, b.lnk_cnt, cap, o.disc, o.pattern, b.lnk_angle, desc);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

void spvo_int::orb_link_finish_brisk(spvo_ctx *c, const BriskDetKeypoint *src, const int *det_counters, int cap, OrbKeypoint *d_kp, const uint32_t *d_desc, int *d_n, int *h_n,
                                     BriskDetKeypoint *h_kp, uint8_t *h_desc) {
  auto &b = c->cls;
  hipLaunchKernelGGL(orb_link_finish_kernel<BriskDetKeypoint>, dim3(32), dim3(256), 0, c->stream2, src, b.lnk_kept, b.lnk_cnt, b.lnk_angle, reinterpret_cast<const uint4 *>(d_desc), cap,
                     det_counters, (const int *)nullptr, 0, d_kp, d_n, h_n, (int *)nullptr, h_kp, reinterpret_cast<uint4 *>(h_desc));
}
void spvo_int::orb_link_finish_akaze(spvo_ctx *c, const AkazeKp *src, const int *stat, int cand_cap, int cap, OrbKeypoint *d_kp, const uint32_t *d_desc, int *d_n, int *h_n, int *h_k,
                                     AkazeKp *h_kp, uint8_t *h_desc) {
  auto &b = c->cls;
  hipLaunchKernelGGL(orb_link_finish_kernel<AkazeKp>, dim3(32), dim3(256), 0, c->stream2, src, b.lnk_kept, b.lnk_cnt, b.lnk_angle, reinterpret_cast<const uint4 *>(d_desc), cap,
                     (const int *)nullptr, stat, cand_cap, d_kp, d_n, h_n, h_k, h_kp, reinterpret_cast<uint4 *>(h_desc));
}

extern "C" {

// Test hook: exactly the link's kernels and the describe kernel on a caller's list against the image already resident -- no detector runs,
// no slot is touched, the image stays.  The list goes up as 12-byte records (x, y, octave) with its keep flags as integers; its length lies
// in the link's counter block.
int spvo_orb_octaves_link_debug(spvo_ctx *c, int rows, int cols, const float *xy, const int32_t *octave, const uint8_t *keep, int n, int max_octave, int32_t *kept, float *angle,
                                uint8_t *desc, int *n_kept) {
  if (!c || !n_kept || rows <= 0 || cols <= 0 || n < 0 || (n > 0 && (!xy || !octave || !kept || !desc))) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (int rc = orb_link_check(c, "spvo_orb_octaves_link_debug", rows, cols, max_octave)) return rc;
  for (int i = 0; i < n; ++i) {
    if (octave[i] < 0 || octave[i] > max_octave)
      return fail(c, SPVO_ERR_INVALID, "spvo_orb_octaves_link_debug: keypoint %d has octave %d; max_octave is %d", i, octave[i], max_octave);
    if (!std::isfinite(xy[2 * i]) || !std::isfinite(xy[2 * i + 1]))
      return fail(c, SPVO_ERR_INVALID, "spvo_orb_octaves_link_debug: keypoint %d is (%g, %g)", i, (double)xy[2 * i], (double)xy[2 * i + 1]);
  }
  if (int rc = require_idle(c)) return rc;
  auto &b = c->cls;
  if (b.rows != rows || b.cols != cols) return fail(c, SPVO_ERR_STATE, "spvo_orb_octaves_link_debug: no image of %d x %d is resident (call a detector first)", rows, cols);
  *n_kept = 0;
  if (n == 0) return SPVO_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream2;
  OrbPlan plan;
  if (int rc = orb_prepare(c, rows, cols, 1, plan)) return rc;
  if (int rc = orb_link_buffers(c, n, n)) return rc;
  std::vector<int> rec((size_t)3 * n), flags(keep ? (size_t)n : 0);
  for (int i = 0; i < n; ++i) {
    std::memcpy(&rec[3 * i], &xy[2 * i], 2 * sizeof(float));
    rec[3 * i + 2] = octave[i];
    if (keep) flags[i] = keep[i] ? 1 : 0;
  }
  HIP_TRY(c, hipMemcpyAsync(b.lnk_src, rec.data(), rec.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (keep) HIP_TRY(c, hipMemcpyAsync(b.lnk_keep, flags.data(), flags.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(b.lnk_cnt + ORB_LINK_N, &n, sizeof n, hipMemcpyHostToDevice, st));
  const OrbLinkSrc src{reinterpret_cast<const char *>(b.lnk_src.get()), 12, 0, 4, 8, keep ? b.lnk_keep.get() : nullptr, b.lnk_cnt + ORB_LINK_N, n};
  if (int rc = orb_link_enqueue(c, rows, cols, max_octave, src, n, b.lnk_desc)) return rc;
  int cnt[ORB_LINK_INTS];
  HIP_TRY(c, hipMemcpyAsync(cnt, b.lnk_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const int m = std::min(std::max(cnt[ORB_LINK_TOTAL], 0), n);
  if (m > 0) {
    HIP_TRY(c, hipMemcpyAsync(kept, b.lnk_kept, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
    if (angle) HIP_TRY(c, hipMemcpyAsync(angle, b.lnk_angle, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(desc, b.lnk_desc, (size_t)m * 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  *n_kept = m;
  return SPVO_OK;
}

}  // extern "C"

int spvo_int::classic_upload_image(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride) { return cls_prepare(c, img, rows, cols, stride); }
int spvo_int::classic_image_ensure(spvo_ctx *c, int rows, int cols) { return cls_ensure(c, rows, cols); }
int spvo_int::classic_image_from_staged(spvo_ctx *c, const uint8_t *h_img, int rows, int cols) {
  auto &b = c->cls;
  b.rows = b.cols = 0;   // nothing resident until the upload is enqueued
  HIP_TRY(c, hipMemcpyAsync(b.im, h_img, (size_t)rows * cols, hipMemcpyHostToDevice, c->stream2));
  b.rows = rows; b.cols = cols;
  return SPVO_OK;
}
void spvo_int::classic_rank_enqueue(spvo_ctx *c, const unsigned long long *keys, int *rank, const int *n_ptr, int cap) {
  hipLaunchKernelGGL(cls_rank_kernel, dim3(128), dim3(256), 0, c->stream2, keys, rank, n_ptr, cap);
}

// ---------------------------------------------------------------- one submission per stereo pair, features stay on the device
// what bin_ensure forgets when it re-allocates everything the slot capacity sizes: the slots are empty afterwards
void spvo_int::classic_release_slots(spvo_ctx *c) {
  auto &bb = c->bin;
  for (BinarySlot &s : bb.slots) {
    slot_rewrite(s);
    s.row_bytes = 32;
  }
  bb.pair.mcache.invalidate();
  bb.cap = 0; bb.pair.last_slot_l = -1;
}

void spvo_int::classic_release(spvo_ctx *c) {
  classic_release_slots(c);
  c->bin.pair.release();
}

extern "C" {

namespace {
static_assert(BIN_COUNTER_INTS == CLS_COUNTER_INTS, "an image's counter block in spvo_ctx::bin.d_cnt");
constexpr int BIN_ROW_BYTES_MAX = 64;   // the widest row a binary slot holds (BRISK; AKAZE's 61 bytes are stored in 64); the ORB extractor's rows are 32 bytes
inline bool kind_is_brisk(int kind) { return kind == SPVO_CLASSIC_GFTT_BRISK || kind == SPVO_CLASSIC_FAST_BRISK; }
inline bool kind_is_gftt(int kind) { return kind == SPVO_CLASSIC_GFTT_ORB || kind == SPVO_CLASSIC_GFTT_BRISK || kind == SPVO_CLASSIC_GFTT_SIFT; }
inline bool kind_is_sift(int kind) { return kind == SPVO_CLASSIC_GFTT_SIFT || kind == SPVO_CLASSIC_FAST_SIFT; }   // float rows into the SIFT slots: spvo_classic_sift_pair's
// the binary slots and the call's own buffers for `cap` rows per slot and images of `px` bytes; growing un-fills every slot.  Every slot and
// both mirrors are sized for 64-byte rows whatever kind asks first: a BRISK kind's first call must not empty the slots the ORB kinds filled
int bin_ensure(spvo_ctx *c, int cap, size_t px) {
  auto &bb = c->bin;
  if (int rc = bb.pair.ensure(c, px)) return rc;
  if (cap <= bb.cap) return SPVO_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  classic_release_slots(c);
  std::vector<GrowEntry> list;
  for (BinarySlot &s : bb.slots) list.insert(list.end(), {zeroed(s.d_kp, cap), zeroed(s.d_desc, (size_t)cap * (BIN_ROW_BYTES_MAX / 4)), zeroed(s.d_n, 1)});
  list.insert(list.end(), {zeroed(bb.d_cnt, 2 * CLS_COUNTER_INTS), zeroed(bb.d_kxy, (size_t)2 * cap), zeroed(bb.d_kresp, cap), zeroed(bb.d_vote, cap), plain(bb.h_kp, (size_t)2 * cap),
                           plain(bb.h_bkp, (size_t)2 * cap), plain(bb.h_desc, (size_t)2 * cap * BIN_ROW_BYTES_MAX), plain(bb.h_akp, (size_t)2 * cap), plain(bb.h_n, 4 * 4),
                           plain(bb.h_match, (size_t)3 * cap)});
  if (int rc = grow(c, wait_for_nothing(), list)) return rc;
  bb.cap = cap;
  return SPVO_OK;
}
}  // namespace

void spvo_default_classic_opts(spvo_classic_opts *o, int kind) {
  if (!o) return;
  o->kind = kind;
  o->nfeatures = 2000;                                                                  // cv::ORB::create(2000, ...), classic.cpp:12-25
  o->max_corners = 1000; o->quality_level = 0.03; o->min_distance = 7.5; o->block_size = 5;   // cv::GFTTDetector::create(1000, 0.03, 7.5, 5, ..), classic.cpp:37-47
  o->fast_threshold = 10; o->fast_nonmax = 1;                                           // cv::FastFeatureDetector::create(10, true), classic.cpp:32-36
  o->slot_capacity = 8192;
}

int spvo_classic_slot_rows(spvo_ctx *c, int slot, int *n) {
  if (!c || !n || slot < 0 || slot >= N_BIN_SLOTS) return fail(c, SPVO_ERR_INVALID, "bad argument");
  const BinarySlot &s = c->bin.slots[slot];
  if (!s.filled) return fail(c, SPVO_ERR_STATE, "binary slot %d holds no features (spvo_classic_detect fills it)", slot);
  *n = s.n;
  return SPVO_OK;
}

// test hook: caller-supplied rows into a binary slot, as if a spvo_classic_detect call of that row width had left them there
int spvo_classic_slot_fill_debug(spvo_ctx *c, int slot, const uint8_t *desc, int n, int desc_bytes) {
  if (!c || slot < 0 || slot >= N_BIN_SLOTS || n < 0 || (n > 0 && !desc)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (desc_bytes != 32 && desc_bytes != 64) return fail(c, SPVO_ERR_INVALID, "spvo_classic_slot_fill_debug: rows of 32 or 64 bytes (got %d)", desc_bytes);
  if (int rc = require_idle(c)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  auto &bb = c->bin;
  if (bb.cap == 0) {
    spvo_classic_opts dflt;
    spvo_default_classic_opts(&dflt, SPVO_CLASSIC_ORB);
    if (int rc = bin_ensure(c, dflt.slot_capacity, 0)) return rc;
  }
  if (n > bb.cap) return fail(c, SPVO_ERR_INVALID, "spvo_classic_slot_fill_debug: %d rows do not fit slots of %d", n, bb.cap);
  HIP_TRY(c, hipStreamSynchronize(c->stream2));   // (a prematch of the slot's old rows may still run)
  BinarySlot &s = bb.slots[slot];
  slot_rewrite(s);
  bb.pair.mcache.invalidate();
  hipStream_t st = c->stream2;
  if (n > 0) {
    HIP_TRY(c, hipMemsetAsync(s.d_kp, 0, (size_t)n * sizeof(OrbKeypoint), st));
    HIP_TRY(c, hipMemcpyAsync(s.d_desc, desc, (size_t)n * desc_bytes, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(c, hipMemcpyAsync(s.d_n, &n, sizeof n, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  s.n = n; s.row_bytes = desc_bytes; s.filled = true;
  return SPVO_OK;
}

namespace {
// what spvo_classic_detect refuses of its options and of the image shape behind the slot capacity: what the kind's per-image entry points refuse
int classic_check_opts(spvo_ctx *c, const spvo_classic_opts *opts, int rows, int cols) {
  const int kind = opts->kind;
  if (kind == SPVO_CLASSIC_ORB) {
    if (opts->nfeatures <= 0) return fail(c, SPVO_ERR_INVALID, "bad argument");
  } else if (kind_is_gftt(kind)) {
    if (int rc = gftt_check(c, "spvo_classic_detect", rows, cols, opts->quality_level, opts->min_distance, opts->block_size)) return rc;
  } else if (kind == SPVO_CLASSIC_FAST_ORB || kind == SPVO_CLASSIC_FAST_BRISK) {
    if (int rc = fast_check(c, opts->fast_threshold)) return rc;
  } else {
    return fail(c, SPVO_ERR_INVALID, "unknown kind %d", kind);
  }
  return kind_is_brisk(kind) ? brisk_check_image(c, "spvo_classic_detect", rows, cols) : SPVO_OK;
}

// every buffer a call of these options needs for a rows x cols pair (`plan`: the ORB kind's)
int classic_pair_ensure(spvo_ctx *c, const spvo_classic_opts *opts, int rows, int cols, OrbPlan &plan) {
  const int cap = opts->slot_capacity;
  if (int rc = bin_ensure(c, cap, (size_t)rows * cols)) return rc;
  if (opts->kind == SPVO_CLASSIC_ORB) return orb_prepare(c, rows, cols, opts->nfeatures, plan);
  if (int rc = cls_ensure(c, rows, cols)) return rc;
  return kind_is_brisk(opts->kind) ? brisk_chain_ensure(c, rows, cols, cap) : orb_ensure_tables(c);   // (the BRISK tables: a one-off 47 MB upload, before the chain)
}

// image k of the staged pair through the ORB detector + extractor into its slot
int orb_pair_chain(spvo_ctx *c, const spvo_classic_opts *opts, const OrbPlan &plan, int rows, int cols, int k, const ChainOut &out) {
  auto &o = c->orb;
  hipStream_t st = c->stream2;
  const size_t px = (size_t)rows * cols;
  const int cap = opts->slot_capacity;
  HIP_TRY(c, hipMemcpyAsync(o.im, c->bin.pair.h_img + k * px, px, hipMemcpyHostToDevice, st));
  const int kp_cap = std::min(opts->nfeatures, cap);   // (more than `cap` rows are an error of the call: the slot need not hold them)
  if (int rc = orb_enqueue(c, plan, rows, cols, o.im, out.d_kp, reinterpret_cast<uint8_t *>(out.d_desc), kp_cap)) return rc;
  hipLaunchKernelGGL(classic_finish_kernel, dim3(32), dim3(256), 0, st, o.counters, ORB_LEVELS, NMS_COUNTER_INTS, opts->nfeatures, nullptr, nullptr, nullptr, out.d_kp,
                     reinterpret_cast<const uint4 *>(out.d_desc), cap, out.d_n, out.h_n, out.h_kp, reinterpret_cast<uint4 *>(out.h_desc));
  return SPVO_OK;
}

// a staged image (pinned, rows packed) becomes the resident image of spvo_ctx::cls and goes through the Shi-Tomasi or FAST detector, which leaves its list there
int detector_enqueue(spvo_ctx *c, const spvo_classic_opts *opts, const uint8_t *h_img, int rows, int cols) {
  if (int rc = classic_image_from_staged(c, h_img, rows, cols)) return rc;
  return kind_is_gftt(opts->kind) ? gftt_enqueue(c, rows, cols, opts->max_corners, opts->quality_level, opts->min_distance)
                                  : fast_enqueue(c, rows, cols, opts->fast_threshold, opts->fast_nonmax);
}
// rows the extractor's grid covers behind that detector
int detector_most(const spvo_classic_opts *opts) {
  return kind_is_gftt(opts->kind) && opts->max_corners > 0 ? std::min(opts->slot_capacity, opts->max_corners) : opts->slot_capacity;
}

// detector -> ORB extractor on the device: the border rule as an order-preserving compaction, then the one-level extractor whose keypoint
// list is the compacted one and whose count is the compaction's (spvo_orb_describe, without the host)
int detector_orb_chain(spvo_ctx *c, const spvo_classic_opts *opts, int rows, int cols, int k, const ChainOut &out) {
  if (int rc = detector_enqueue(c, opts, c->bin.pair.h_img + k * ((size_t)rows * cols), rows, cols)) return rc;
  auto &b = c->cls;
  hipStream_t st = c->stream2;
  const int cap = opts->slot_capacity;
  hipLaunchKernelGGL(cls_compact_kernel, dim3(1), dim3(1024), 0, st, b.xy, b.resp, b.counters, rows, cols, ORB_EDGE, c->bin.d_kxy, out.kresp, cap, out.cnt);
  orb_extract_one_level(c, rows, cols, c->bin.d_kxy, out.cnt, detector_most(opts), out.d_kp, reinterpret_cast<uint8_t *>(out.d_desc), cap);
  hipLaunchKernelGGL(classic_finish_kernel, dim3(32), dim3(256), 0, st, nullptr, 0, 0, 0, b.counters, out.cnt, out.kresp, out.d_kp, reinterpret_cast<const uint4 *>(out.d_desc), cap,
                     out.d_n, out.h_n, out.h_kp, reinterpret_cast<uint4 *>(out.h_desc));
  return SPVO_OK;
}

// the same hand-over to the BRISK extractor: its border rule (keypoint size 5 / 7, what detectKeypoints assigns) and the rest of
// spvo_brisk_describe's launches, 64-byte rows
int detector_brisk_chain(spvo_ctx *c, const spvo_classic_opts *opts, int rows, int cols, int k, const ChainOut &out) {
  if (int rc = detector_enqueue(c, opts, c->bin.pair.h_img + k * ((size_t)rows * cols), rows, cols)) return rc;
  return brisk_chain_enqueue(c, rows, cols, kind_is_gftt(opts->kind) ? 5.0f : 7.0f, opts->slot_capacity, detector_most(opts), out);
}

// the counts of both images from their mirrors, image by image (kept: this entry point answers a detector overflow with SPVO_ERR_CAPACITY;
// whether the pair fits its slots is the protocol's rule, PairCall::commit)
int classic_check_capacity(spvo_ctx *c, PairCall<BinPairFamily> &pc) {
  for (int k = 0; k < 2; ++k) {
    pc.count(k);
    if (c->bin.h_n[4 * k + 1]) return fail(c, SPVO_ERR_CAPACITY, "spvo_classic_detect: corner buffer overflow in the %s image", k ? "right" : "left");
  }
  return SPVO_OK;
}
}  // namespace

int spvo_classic_detect(spvo_ctx *c, const spvo_classic_opts *opts, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int slot_l, int slot_r,
                        spvo_classic_features *out_l, spvo_classic_features *out_r) {
  if (!c || !opts || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  const int kind = opts->kind, cap = opts->slot_capacity, row_bytes = kind_is_brisk(kind) ? 64 : 32;
  PairCall<BinPairFamily> pc(c, "spvo_classic_detect", BinPairFamily{row_bytes}, pair_out(out_l), pair_out(out_r));
  if (int rc = pc.check(slot_l, slot_r)) return rc;
  // (kept: a SIFT kind is refused before the capacity is looked at; then what the kind's per-image entry points refuse)
  if (kind_is_sift(kind)) return fail(c, SPVO_ERR_INVALID, "spvo_classic_detect: kind %d leaves rows of 128 floats, which no binary slot holds: call spvo_classic_sift_pair", kind);
  if (int rc = pc.check_capacity(cap)) return rc;
  if (int rc = classic_check_opts(c, opts, rows, cols)) return rc;
  if (int rc = pc.open()) return rc;
  auto &bb = c->bin;
  OrbPlan plan;
  if (int rc = classic_pair_ensure(c, opts, rows, cols, plan)) return rc;
  if (int rc = pc.load(img_l, img_r, rows, cols, stride)) return rc;
  for (int k = 0; k < 2; ++k) {
    const BinarySlot &s = bb.slots[pc.slots[k]];
    const ChainOut out{bb.d_cnt + k * CLS_COUNTER_INTS, bb.d_kresp, s.d_kp, s.d_desc, s.d_n, bb.h_n + 4 * k, bb.h_kp + (size_t)k * cap, bb.h_desc + (size_t)k * cap * row_bytes};
    if (int rc = kind == SPVO_CLASSIC_ORB ? orb_pair_chain(c, opts, plan, rows, cols, k, out)
                 : row_bytes == 64        ? detector_brisk_chain(c, opts, rows, cols, k, out)
                                          : detector_orb_chain(c, opts, rows, cols, k, out))
      return rc;
    HIP_TRY(c, hipGetLastError());
  }
  if (int rc = pc.submit()) return rc;
  if (int rc = classic_check_capacity(c, pc)) return rc;
  const PairMirror mirrors[2] = {{bb.h_kp, sizeof(OrbKeypoint), bb.h_desc, (size_t)row_bytes},
                                 {bb.h_kp + cap, sizeof(OrbKeypoint), bb.h_desc + (size_t)cap * row_bytes, (size_t)row_bytes}};
  return pc.commit(mirrors);
}

// ---------------------------------------------------------------- the ORB detector in front of another algorithm's extractor, pair-resident
namespace {
// the highest level of a rows x cols image that can hold a keypoint (orb_enqueue's rule for L.want, orb_prepare's geometry), or 0 if none can
int orb_top_level(int rows, int cols) {
  int top = 0;
  float scale = 1.f;
  for (int l = 0; l < ORB_LEVELS; ++l, scale *= 1.2f) {
    const int h = (int)std::lround(rows / scale), w = (int)std::lround(cols / scale);
    if (h > 2 * ORB_EDGE + 2 && w > 2 * ORB_EDGE + 2) top = l;
  }
  return top;
}

// the record buffers of orb_records_kernel for `n` records
int orb_records_ensure(spvo_ctx *c, int n) {
  auto &o = c->orb;
  if (n <= o.rec_cap) return SPVO_OK;
  o.rec_cap = 0;
  if (int rc = grow(c, wait_for(c->stream2), {plain(o.rec, (size_t)n), plain(o.crec, (size_t)n), plain(o.rec_keep, (size_t)n), zeroed(o.rec_cnt, 4)})) return rc;
  o.rec_cap = n;
  return SPVO_OK;
}

// A pair call's first link: the staged image becomes the resident image of spvo_ctx::cls, goes through spvo_orb_detect's launches with that
// image as level 0 (ORB's own rows go to o.desc and are not read), and orb_records_kernel leaves the list in o.rec / o.rec_keep / o.rec_cnt
int orb_staged_enqueue(spvo_ctx *c, const OrbPlan &plan, const uint8_t *h_img, int rows, int cols, int nfeatures) {
  auto &o = c->orb;
  if (int rc = classic_image_from_staged(c, h_img, rows, cols)) return rc;
  if (int rc = orb_enqueue(c, plan, rows, cols, c->cls.im, o.kps, o.desc, nfeatures)) return rc;
  OrbLevelScale ls;
  for (int l = 0; l < ORB_LEVELS; ++l) ls.s[l] = l == 0 ? 1.f : ls.s[l - 1] * 1.2f;   // (the host's to_keypoint: repeated * 1.2f)
  hipLaunchKernelGGL(orb_records_kernel, dim3(8), dim3(256), 0, c->stream2, o.kps, o.counters, nfeatures, ls, o.rec, o.rec_keep, o.rec_cnt);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}
}  // namespace

// ORB keypoints with BRISK descriptors, pair-resident in the binary slots (64-byte rows): per image what spvo_orb_detect(img, nfeatures)
// followed by spvo_brisk_describe on its x, y and 31 * 1.2^octave hands out, byte for byte.  spvo_brisk_detect_pair's protocol; the chain of
// an image is staged image -> resident image -> orb_enqueue -> orb_records_kernel -> brisk_pair_chain_enqueue.
int spvo_orb_brisk_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int nfeatures, int slot_l, int slot_r, int slot_capacity,
                        spvo_brisk_features *out_l, spvo_brisk_features *out_r) {
  if (!c || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  const char *who = "spvo_orb_brisk_pair";
  const int cap = slot_capacity, row_bytes = 64;
  PairCall<BinPairFamily> pc(c, who, BinPairFamily{row_bytes}, pair_out(out_l), pair_out(out_r));
  int rc;
  if ((rc = pc.check(slot_l, slot_r)) || (rc = pc.check_capacity(cap))) return rc;
  if (cap > 32768) return fail(c, SPVO_ERR_INVALID, "%s: slot_capacity must be 1 .. 32768", who);
  if (nfeatures <= 0) return fail(c, SPVO_ERR_INVALID, "%s: nfeatures must be positive", who);
  if ((rc = brisk_check_image(c, who, rows, cols)) || (rc = pc.open())) return rc;
  auto &bb = c->bin;
  auto &o = c->orb;
  OrbPlan plan;
  // every allocation and the BRISK point table before the first launch of the chain
  if ((rc = bin_ensure(c, cap, (size_t)rows * cols)) || (rc = cls_ensure(c, rows, cols)) || (rc = brisk_chain_ensure(c, rows, cols, cap)) ||
      (rc = orb_prepare(c, rows, cols, nfeatures, plan)) || (rc = orb_records_ensure(c, nfeatures)))
    return rc;
  if ((rc = pc.load(img_l, img_r, rows, cols, stride))) return rc;
  for (int k = 0; k < 2; ++k) {
    const BinarySlot &s = bb.slots[pc.slots[k]];
    if ((rc = orb_staged_enqueue(c, plan, pc.image(k), rows, cols, nfeatures))) return rc;
    const ChainOut out{bb.d_cnt + k * BIN_COUNTER_INTS, bb.d_kresp, s.d_kp, s.d_desc, s.d_n, bb.h_n + 4 * k, nullptr, bb.h_desc + (size_t)k * cap * row_bytes};
    if ((rc = brisk_pair_chain_enqueue(c, rows, cols, cap, o.rec, o.rec_keep, o.rec_cnt, nfeatures, o.crec, out, bb.h_bkp + (size_t)k * cap))) return rc;
  }
  if ((rc = pc.submit())) return rc;
  pc.count(0); pc.count(1);
  // (spvo_orb_detect's answer: a level found more corners than its buffer holds -- an input's doing, not a defect)
  if (bb.h_n[1] || bb.h_n[5]) return fail(c, SPVO_ERR_CAPACITY, "%s: corner buffer overflow in the %s image", who, bb.h_n[1] ? "left" : "right");
  static_assert(sizeof(spvo_brisk_keypoint) == sizeof(BriskDetKeypoint), "record layout");
  const PairMirror mirrors[2] = {{bb.h_bkp, sizeof(BriskDetKeypoint), bb.h_desc, (size_t)row_bytes},
                                 {bb.h_bkp + cap, sizeof(BriskDetKeypoint), bb.h_desc + (size_t)cap * row_bytes, (size_t)row_bytes}};
  return pc.commit(mirrors);
}

// ORB keypoints with SIFT descriptors, pair-resident in the SIFT slots: per image what spvo_orb_detect(img, nfeatures) followed by
// spvo_sift_describe on its records {x, y, 31 * 1.2^octave, degrees, response, octave} hands out, byte for byte.  The call is
// sift_link_pair's (spvo_sift.hip); the pyramid is built for octaves 0 .. the highest level of the shape that can hold a keypoint.
int spvo_orb_sift_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int nfeatures, int slot_l, int slot_r, int slot_capacity,
                       spvo_sift_features *out_l, spvo_sift_features *out_r) {
  if (!c || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  static_assert(sizeof(spvo_sift_keypoint) == sizeof(BriskDetKeypoint), "record layout");
  const char *who = "spvo_orb_sift_pair";
  auto &o = c->orb;
  OrbPlan plan;
  SiftLinkDetector det;
  det.who = who;
  det.max_octave = orb_top_level(rows, cols);
  det.overflow_is_capacity = true;
  det.check = [&]() -> int { return nfeatures <= 0 ? fail(c, SPVO_ERR_INVALID, "%s: nfeatures must be positive", who) : SPVO_OK; };
  det.prepare = [&](SiftLinkSrc &src) -> int {
    if (int rc = orb_prepare(c, rows, cols, nfeatures, plan)) return rc;
    if (int rc = orb_records_ensure(c, nfeatures)) return rc;
    src = SiftLinkSrc{reinterpret_cast<const char *>(o.rec.get()), (int)sizeof(BriskDetKeypoint), (int)offsetof(BriskDetKeypoint, x), (int)offsetof(BriskDetKeypoint, y),
                      (int)offsetof(BriskDetKeypoint, size), (int)offsetof(BriskDetKeypoint, angle), (int)offsetof(BriskDetKeypoint, response), (int)offsetof(BriskDetKeypoint, octave),
                      nullptr, o.rec_cnt + 1, nfeatures, o.rec_cnt, nullptr, 0};   // (every record is kept: no flags, no compaction)
    return SPVO_OK;
  };
  det.enqueue = [&](const uint8_t *h_img) -> int { return orb_staged_enqueue(c, plan, h_img, rows, cols, nfeatures); };
  return sift_link_pair(c, det, img_l, img_r, rows, cols, stride, slot_l, slot_r, slot_capacity, pair_out(out_l), pair_out(out_r));
}

}  // extern "C"

int spvo_int::classic_slots_ensure(spvo_ctx *c, int cap, size_t px) { return bin_ensure(c, cap, px); }
int spvo_int::classic_detector_check(spvo_ctx *c, const char *who, const spvo_classic_opts *opts, int rows, int cols) {
  return kind_is_gftt(opts->kind) ? gftt_check(c, who, rows, cols, opts->quality_level, opts->min_distance, opts->block_size) : fast_check(c, opts->fast_threshold);
}
int spvo_int::classic_detector_enqueue(spvo_ctx *c, const spvo_classic_opts *opts, const uint8_t *h_img, int rows, int cols) {
  if (int rc = detector_enqueue(c, opts, h_img, rows, cols)) return rc;
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}
