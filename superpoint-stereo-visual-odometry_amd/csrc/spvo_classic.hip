// spvo_classic.hip -- the classic front end (ClassicFeatureFrontEnd, feature_detection_classic.cpp): the ORB detector / extractor (orb.hip.h),
// the Shi-Tomasi and FAST detectors and the ORB extractor for given keypoints (classic_detect.hip.h), one submission per stereo pair into the
// binary feature slots (spvo_classic_detect; its BRISK kinds hand the detector's list to spvo_brisk.hip), and spvo_preprocess for a context
// without an engine.  Everything here runs on the solver's stream (stream2) and owns its buffers (spvo_ctx::orb, spvo_ctx::cls).
#include "spvo_internal.hip.h"
#include "orb.hip.h"
#include "classic_detect.hip.h"

namespace {
// a host image of a strided view into the packed rows of `dst`, through the staging buffer `src` (grown on demand).  Of a strided view
// (a cv::Mat ROI) only (rows - 1) * stride + cols bytes are the caller's: the last row's padding may lie beyond the end of the parent allocation
int upload_strided(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, uint8_t *&src, size_t &src_cap, uint8_t *dst, hipStream_t st) {
  const size_t src_bytes = (size_t)(rows - 1) * stride + cols;
  if (src_bytes > src_cap) {
    HIP_TRY(c, hipStreamSynchronize(st));
    dev_free(src);
    src_cap = 0;
    if (int rc = dev_alloc(c, &src, src_bytes, false)) return rc;
    src_cap = src_bytes;
  }
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
    int rc;
    if ((rc = dev_alloc(c, &b.pre_out, (size_t)H * W)) || (rc = dev_alloc(c, &b.pre_tab, (size_t)3 * (H + W)))) return rc;
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
  int rc;
  if ((rc = dev_alloc(c, &o.pattern, 1024)) || (rc = dev_alloc(c, &o.taps, 8)) || (rc = dev_alloc(c, &o.disc, disc.size()))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
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
    HIP_TRY(c, hipStreamSynchronize(st));
    dev_free(o.im, o.score, o.blur, o.tmp, o.keys, o.rank, o.out_xy, o.counters, o.tab, o.kps, o.desc);
    const size_t pyr = std::max(need_pyr, o.pyr_cap), kall = std::max(need_keys, o.key_cap), tabn = std::max(need_tab, o.tab_cap);
    const int kpn = std::max(kp_cap, o.kp_cap);
    o.pyr_cap = o.key_cap = o.tab_cap = 0; o.kp_cap = 0;   // a failed allocation below leaves a context that spvo_destroy and a later call can still handle
    int rc;
    if ((rc = dev_alloc(c, &o.im, pyr)) || (rc = dev_alloc(c, &o.score, pyr)) || (rc = dev_alloc(c, &o.blur, pyr)) || (rc = dev_alloc(c, &o.tmp, pyr)) ||
        (rc = dev_alloc(c, &o.keys, kall)) || (rc = dev_alloc(c, &o.rank, kall)) || (rc = dev_alloc(c, &o.out_xy, 2 * kall)) ||
        (rc = dev_alloc(c, &o.counters, (size_t)ORB_LEVELS * NMS_COUNTER_INTS)) || (rc = dev_alloc(c, &o.tab, tabn)) || (rc = dev_alloc(c, &o.kps, kpn)) ||
        (rc = dev_alloc(c, &o.desc, (size_t)kpn * 32)))
      return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (dev_alloc clears on the network stream)
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

// The image in level 0 (o.im) -> keypoint records and descriptors in `kps` / `desc` (kp_cap rows), enqueued without a host round trip:
// the pyramid level by level, then every stage once for all levels; one counter block per level, a level's keypoints land behind
// those of the levels below (orb_describe_kernel sums their counts)
int orb_enqueue(spvo_ctx *c, const OrbPlan &p, int rows, int cols, OrbKeypoint *kps, uint8_t *desc, int kp_cap) {
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
    L.im = o.im + p.off[l]; L.score = o.score + p.off[l]; L.blur = o.blur + p.off[l]; L.tmp = o.tmp + p.off[l];
    L.keys = o.keys + koff; L.rank = o.rank + koff; L.out_xy = o.out_xy + 2 * koff; L.counters = o.counters + l * NMS_COUNTER_INTS;
    L.h = ph[l]; L.w = pw[l]; L.cap = lcap; L.scale = p.lscale[l];
    L.want = (ph[l] <= 2 * ORB_EDGE + 2 || pw[l] <= 2 * ORB_EDGE + 2) ? 0 : p.want[l];
    want_max = std::max(want_max, L.want);
    koff += lcap;
    if (l > 0) hipLaunchKernelGGL(orb_resize_kernel, dim3((pw[l] + 63) / 64, (ph[l] + 3) / 4), dim3(256), 0, st, o.im + p.off[l - 1], ph[l - 1], pw[l - 1], pw[l - 1], L.im, ph[l], pw[l],
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
  if (int rc = upload_strided(c, img, rows, cols, stride, o.src, o.src_cap, o.im, st)) return rc;   // level 0: the image, rows packed
  if (int rc = orb_enqueue(c, plan, rows, cols, o.kps, o.desc, kp_cap)) return rc;
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
  if (px > b.px_cap || state_bytes > b.state_cap) {
    HIP_TRY(c, hipStreamSynchronize(st));
    dev_free(b.im, b.score, b.blur, b.state, b.tmp, b.lam, b.xy, b.resp, b.keys, b.rank, b.cand);
    const size_t npx = std::max(px, b.px_cap), nst = std::max(state_bytes, b.state_cap);
    b.px_cap = b.state_cap = 0;   // a failed allocation below leaves a context that spvo_destroy and a later call can still handle
    b.state_rows = b.state_cols = 0;
    int rc;
    if ((rc = dev_alloc(c, &b.im, npx + 256)) || (rc = dev_alloc(c, &b.score, npx + 256)) || (rc = dev_alloc(c, &b.blur, npx + 256)) || (rc = dev_alloc(c, &b.state, nst)) ||
        (rc = dev_alloc(c, &b.tmp, npx)) || (rc = dev_alloc(c, &b.lam, npx)) || (rc = dev_alloc(c, &b.xy, 2 * npx)) || (rc = dev_alloc(c, &b.resp, npx)) ||
        (rc = dev_alloc(c, &b.keys, npx)) || (rc = dev_alloc(c, &b.rank, npx)) || (rc = dev_alloc(c, &b.cand, npx)))
      return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (dev_alloc clears on the network stream)
    b.px_cap = npx; b.state_cap = nst;
  }
  if (!b.counters) {
    int rc = dev_alloc(c, &b.counters, CLS_COUNTER_INTS);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return SPVO_OK;
}

// the image into the context's level-0 buffer (rows packed), every buffer grown to what this image needs
int cls_prepare(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride) {
  auto &b = c->cls;
  if (int rc = cls_ensure(c, rows, cols)) return rc;
  if (int rc = upload_strided(c, img, rows, cols, stride, b.src, b.src_cap, b.im, c->stream2)) return rc;
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
  if (!c || !img || !n_out || rows < 8 || cols < 8 || stride < (size_t)cols || cap < 0 || (cap > 0 && !xy) || !(quality_level > 0))
    return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (block_size != 5 || !(min_distance >= 0 && min_distance <= 15)) return fail(c, SPVO_ERR_INVALID, "spvo_gftt_detect: block_size 5 and min_distance <= 15 only");
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
  if (!c || !img || !n_out || rows <= 0 || cols <= 0 || stride < (size_t)cols || cap < 0 || (cap > 0 && !xy) || threshold < 0 || threshold > 255)
    return fail(c, SPVO_ERR_INVALID, "bad argument");
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
    HIP_TRY(c, hipStreamSynchronize(st));
    dev_free(b.kp_xy, b.kps, b.desc);
    b.kp_cap = 0;
    int rc;
    if ((rc = dev_alloc(c, &b.kp_xy, (size_t)2 * nk)) || (rc = dev_alloc(c, &b.kps, (size_t)nk)) || (rc = dev_alloc(c, &b.desc, (size_t)nk * 32))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    b.kp_cap = nk;
  }
  int cnt[CLS_COUNTER_INTS] = {0};
  cnt[2] = nk;
  HIP_TRY(c, hipMemcpyAsync(b.counters, cnt, sizeof cnt, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(b.kp_xy, kxy.data(), (size_t)2 * nk * sizeof(int), hipMemcpyHostToDevice, st));
  // orb.hip.h's extractor on a one-level OrbLevels whose keypoint list is the caller's: 7x7 blur of level 0, then direction + steered tests
  OrbLevels lv{};
  OrbLevel &L = lv.l[0];
  L.im = b.im; L.score = b.score; L.blur = b.blur; L.tmp = b.tmp; L.out_xy = b.kp_xy; L.counters = b.counters;
  L.h = rows; L.w = cols; L.want = nk; L.cap = nk; L.scale = 1.f;
  const dim3 grid((cols + 63) / 64, (rows + 3) / 4, 1);
  hipLaunchKernelGGL(orb_blur_h_kernel, grid, dim3(256), 0, st, lv, c->orb.taps);
  hipLaunchKernelGGL(orb_blur_v_kernel, grid, dim3(256), 0, st, lv, c->orb.taps);
  hipLaunchKernelGGL(orb_describe_kernel, dim3((nk + 3) / 4, 1), dim3(256), 0, st, lv, c->orb.disc, c->orb.pattern, b.kps, b.desc, nk);
  HIP_TRY(c, hipGetLastError());
  std::vector<OrbKeypoint> kp((size_t)nk);
  HIP_TRY(c, hipMemcpyAsync(kp.data(), b.kps, (size_t)nk * sizeof(OrbKeypoint), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(desc, b.desc, (size_t)nk * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (angle) for (int i = 0; i < nk; ++i) angle[i] = kp[i].angle;
  return SPVO_OK;
}

}  // extern "C"

int spvo_int::classic_upload_image(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride) { return cls_prepare(c, img, rows, cols, stride); }

// ---------------------------------------------------------------- one submission per stereo pair, features stay on the device
// everything bin_ensure sizes by the slot capacity; the slots are empty afterwards
void spvo_int::classic_release_slots(spvo_ctx *c) {
  auto &bb = c->bin;
  for (BinarySlot &s : bb.slots) {
    dev_free(s.d_kp, s.d_desc, s.d_n);
    s.filled = false; s.n = 0; s.row_bytes = 32; ++s.gen;
  }
  dev_free(bb.d_cnt, bb.d_kxy, bb.d_kresp, bb.d_vote);
  for (void *p : {(void *)bb.h_kp, (void *)bb.h_desc, (void *)bb.h_n, (void *)bb.h_match}) if (p) (void)hipHostFree(p);
  bb.h_kp = nullptr; bb.h_desc = nullptr; bb.h_n = nullptr; bb.h_match = nullptr;
  for (auto &mc : bb.mcache) { mc.valid = false; mc.h_out = nullptr; }
  bb.cap = 0; bb.last_slot_l = -1;
}

void spvo_int::classic_release(spvo_ctx *c) {
  auto &bb = c->bin;
  classic_release_slots(c);
  if (bb.h_img) (void)hipHostFree(bb.h_img);
  bb.h_img = nullptr; bb.img_cap = 0;
  if (bb.ev_feat) (void)hipEventDestroy(bb.ev_feat);
  if (bb.ev_match) (void)hipEventDestroy(bb.ev_match);
  bb.ev_feat = bb.ev_match = nullptr;
}

extern "C" {

namespace {
constexpr int BIN_ROW_BYTES_MAX = 64;   // the widest row a binary slot holds (BRISK); the ORB extractor's rows are 32 bytes
inline bool kind_is_brisk(int kind) { return kind == SPVO_CLASSIC_GFTT_BRISK || kind == SPVO_CLASSIC_FAST_BRISK; }
inline bool kind_is_gftt(int kind) { return kind == SPVO_CLASSIC_GFTT_ORB || kind == SPVO_CLASSIC_GFTT_BRISK; }
// the binary slots and the call's own buffers for `cap` rows per slot and images of `px` bytes; growing un-fills every slot.  Every slot and
// both mirrors are sized for 64-byte rows whatever kind asks first: a BRISK kind's first call must not empty the slots the ORB kinds filled
int bin_ensure(spvo_ctx *c, int cap, size_t px) {
  auto &bb = c->bin;
  if (!bb.ev_feat) {
    HIP_TRY(c, hipEventCreateWithFlags(&bb.ev_feat, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&bb.ev_match, hipEventDisableTiming));
  }
  if (px > bb.img_cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream2));
    if (bb.h_img) (void)hipHostFree(bb.h_img);
    bb.h_img = nullptr; bb.img_cap = 0;
    HIP_TRY(c, hipHostMalloc((void **)&bb.h_img, 2 * px));
    bb.img_cap = px;
  }
  if (cap <= bb.cap) return SPVO_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  classic_release_slots(c);
  int rc;
  for (BinarySlot &s : bb.slots)
    if ((rc = dev_alloc(c, &s.d_kp, cap)) || (rc = dev_alloc(c, &s.d_desc, (size_t)cap * (BIN_ROW_BYTES_MAX / 4))) || (rc = dev_alloc(c, &s.d_n, 1))) return rc;
  if ((rc = dev_alloc(c, &bb.d_cnt, 2 * CLS_COUNTER_INTS)) || (rc = dev_alloc(c, &bb.d_kxy, (size_t)2 * cap)) || (rc = dev_alloc(c, &bb.d_kresp, cap)) ||
      (rc = dev_alloc(c, &bb.d_vote, cap)))
    return rc;
  HIP_TRY(c, hipHostMalloc((void **)&bb.h_kp, (size_t)2 * cap * sizeof(OrbKeypoint)));
  HIP_TRY(c, hipHostMalloc((void **)&bb.h_desc, (size_t)2 * cap * BIN_ROW_BYTES_MAX));
  HIP_TRY(c, hipHostMalloc((void **)&bb.h_n, 2 * 4 * sizeof(int)));
  HIP_TRY(c, hipHostMalloc((void **)&bb.h_match, (size_t)3 * cap * sizeof(int2)));
  for (int k = 0; k < 2; ++k) bb.mcache[k].h_out = bb.h_match + (size_t)k * cap;
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (dev_alloc clears on the network stream)
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
  s.filled = false; s.n = 0; ++s.gen;
  for (auto &mc : bb.mcache) mc.valid = false;
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

int spvo_classic_detect(spvo_ctx *c, const spvo_classic_opts *opts, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int slot_l, int slot_r,
                        spvo_classic_features *out_l, spvo_classic_features *out_r) {
  if (!c || !opts || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (slot_l < 0 || slot_l >= N_BIN_SLOTS || slot_r < 0 || slot_r >= N_BIN_SLOTS || slot_l == slot_r) return fail(c, SPVO_ERR_INVALID, "bad slot");
  spvo_classic_features *outs[2] = {out_l, out_r};
  for (auto *o : outs)
    if (o->cap < 0) return fail(c, SPVO_ERR_INVALID, "bad output buffer");
  const int kind = opts->kind, cap = opts->slot_capacity;
  if (cap <= 0 || cap > (1 << HAM_KEY_SHIFT)) return fail(c, SPVO_ERR_INVALID, "slot_capacity must be 1 .. %d", 1 << HAM_KEY_SHIFT);
  // what the per-image entry points refuse
  if (kind == SPVO_CLASSIC_ORB) {
    if (opts->nfeatures <= 0) return fail(c, SPVO_ERR_INVALID, "bad argument");
  } else if (kind_is_gftt(kind)) {
    if (rows < 8 || cols < 8 || !(opts->quality_level > 0)) return fail(c, SPVO_ERR_INVALID, "bad argument");
    if (opts->block_size != 5 || !(opts->min_distance >= 0 && opts->min_distance <= 15)) return fail(c, SPVO_ERR_INVALID, "spvo_classic_detect: block_size 5 and min_distance <= 15 only");
  } else if (kind == SPVO_CLASSIC_FAST_ORB || kind == SPVO_CLASSIC_FAST_BRISK) {
    if (opts->fast_threshold < 0 || opts->fast_threshold > 255) return fail(c, SPVO_ERR_INVALID, "bad argument");
  } else {
    return fail(c, SPVO_ERR_INVALID, "unknown kind %d", kind);
  }
  const bool brisk = kind_is_brisk(kind);
  if (brisk && (long long)rows * cols * 255 >= (1ll << 31)) return fail(c, SPVO_ERR_INVALID, "spvo_classic_detect: %d x %d pixels do not fit the int32 integral image", rows, cols);
  const int row_bytes = brisk ? 64 : 32;
  if (!c->pendq.empty()) return fail(c, SPVO_ERR_STATE, "detector submissions are in flight: complete them with spvo_detect_wait first");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  out_l->n = out_r->n = 0;
  hipStream_t st = c->stream2;
  auto &bb = c->bin;
  auto &o = c->orb;
  auto &b = c->cls;
  const size_t px = (size_t)rows * cols;
  if (int rc = bin_ensure(c, cap, px)) return rc;
  OrbPlan plan;
  if (kind == SPVO_CLASSIC_ORB) {
    if (int rc = orb_prepare(c, rows, cols, opts->nfeatures, plan)) return rc;
  } else {
    if (int rc = cls_ensure(c, rows, cols)) return rc;
    if (int rc = brisk ? brisk_chain_ensure(c, rows, cols, cap) : orb_ensure_tables(c)) return rc;   // (the BRISK tables: a one-off 47 MB upload, before the chain)
  }
  // both slots are being rewritten: whatever was matched against their old contents is stale
  const int slots[2] = {slot_l, slot_r};
  for (int sl : slots) { BinarySlot &s = bb.slots[sl]; s.filled = false; s.n = 0; s.row_bytes = row_bytes; ++s.gen; }
  for (auto &mc : bb.mcache) mc.valid = false;
  // pinned staging: both images with packed rows (of a strided view only the rows' own bytes are the caller's), one upload each
  HIP_TRY(c, hipStreamSynchronize(st));   // (the staging buffer and the mirrors are the previous call's until its work is done)
  const uint8_t *imgs[2] = {img_l, img_r};
  for (int k = 0; k < 2; ++k)
    for (int r = 0; r < rows; ++r) std::memcpy(bb.h_img + k * px + (size_t)r * cols, imgs[k] + (size_t)r * stride, cols);
  for (int k = 0; k < 2; ++k) {
    BinarySlot &s = bb.slots[slots[k]];
    int *h_n = bb.h_n + 4 * k;
    OrbKeypoint *h_kp = bb.h_kp + (size_t)k * cap;
    uint4 *h_desc = reinterpret_cast<uint4 *>(bb.h_desc + (size_t)k * cap * row_bytes);
    if (kind == SPVO_CLASSIC_ORB) {
      HIP_TRY(c, hipMemcpyAsync(o.im, bb.h_img + k * px, px, hipMemcpyHostToDevice, st));
      const int kp_cap = std::min(opts->nfeatures, cap);   // (more than `cap` rows are an error below: the slot need not hold them)
      if (int rc = orb_enqueue(c, plan, rows, cols, s.d_kp, reinterpret_cast<uint8_t *>(s.d_desc), kp_cap)) return rc;
      hipLaunchKernelGGL(classic_finish_kernel, dim3(32), dim3(256), 0, st, o.counters, ORB_LEVELS, NMS_COUNTER_INTS, opts->nfeatures, nullptr, nullptr, nullptr, s.d_kp,
                         reinterpret_cast<const uint4 *>(s.d_desc), cap, s.d_n, h_n, h_kp, h_desc);
    } else {
      b.rows = b.cols = 0;
      HIP_TRY(c, hipMemcpyAsync(b.im, bb.h_img + k * px, px, hipMemcpyHostToDevice, st));
      b.rows = rows; b.cols = cols;
      if (int rc = kind_is_gftt(kind) ? gftt_enqueue(c, rows, cols, opts->max_corners, opts->quality_level, opts->min_distance)
                                                 : fast_enqueue(c, rows, cols, opts->fast_threshold, opts->fast_nonmax))
        return rc;
      // detector -> extractor on the device: the border rule as an order-preserving compaction, then orb.hip.h's extractor on a one-level
      // OrbLevels whose keypoint list is the compacted one and whose count is the compaction's (spvo_orb_describe, without the host)
      int *cnt = bb.d_cnt + k * CLS_COUNTER_INTS;
      const int most = kind_is_gftt(kind) && opts->max_corners > 0 ? std::min(cap, opts->max_corners) : cap;   // rows the extractor's grid covers
      if (brisk) {
        // the same hand-over to the BRISK extractor: its border rule (keypoint size 5 / 7, what detectKeypoints assigns) and the rest of
        // spvo_brisk_describe's launches, 64-byte rows
        const BriskChainOut bo{cnt, bb.d_kresp, s.d_kp, s.d_desc, s.d_n, h_n, h_kp, reinterpret_cast<uint8_t *>(h_desc)};
        if (int rc = brisk_chain_enqueue(c, rows, cols, kind_is_gftt(kind) ? 5.0f : 7.0f, cap, most, bo)) return rc;
        continue;
      }
      hipLaunchKernelGGL(cls_compact_kernel, dim3(1), dim3(1024), 0, st, b.xy, b.resp, b.counters, rows, cols, ORB_EDGE, bb.d_kxy, bb.d_kresp, cap, cnt);
      OrbLevels lv{};
      OrbLevel &L = lv.l[0];
      L.im = b.im; L.score = b.score; L.blur = b.blur; L.tmp = b.tmp; L.out_xy = bb.d_kxy; L.counters = cnt;
      L.h = rows; L.w = cols; L.want = most; L.cap = most; L.scale = 1.f;
      const dim3 grid((cols + 63) / 64, (rows + 3) / 4, 1);
      hipLaunchKernelGGL(orb_blur_h_kernel, grid, dim3(256), 0, st, lv, o.taps);
      hipLaunchKernelGGL(orb_blur_v_kernel, grid, dim3(256), 0, st, lv, o.taps);
      hipLaunchKernelGGL(orb_describe_kernel, dim3((most + 3) / 4, 1), dim3(256), 0, st, lv, o.disc, o.pattern, s.d_kp, reinterpret_cast<uint8_t *>(s.d_desc), cap);
      hipLaunchKernelGGL(classic_finish_kernel, dim3(32), dim3(256), 0, st, nullptr, 0, 0, 0, b.counters, cnt, bb.d_kresp, s.d_kp, reinterpret_cast<const uint4 *>(s.d_desc), cap,
                         s.d_n, h_n, h_kp, h_desc);
    }
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(bb.ev_feat, st));
  // spvo_set_prematch: the two standard matches behind the features, counts read on the device (a pair that turns out not to fit its
  // slots is matched on whatever rows the slots hold; that result is dropped below)
  const int prev_l = bb.last_slot_l;
  // (a previous left slot of the other row width has no temporal match: skipped, the synchronous call reports the widths when asked)
  const bool temporal = prev_l >= 0 && prev_l != slot_l && prev_l != slot_r && bb.slots[prev_l].filled && bb.slots[prev_l].row_bytes == row_bytes;
  if (c->prematch) {
    if (int rc = enqueue_hamming_slots(c, slot_l, slot_r, c->pm_selector, c->pm_cross, c->pm_ratio, bb.mcache[0].h_out)) return rc;
    if (temporal)
      if (int rc = enqueue_hamming_slots(c, slot_l, prev_l, c->pm_selector, c->pm_cross, c->pm_ratio, bb.mcache[1].h_out)) return rc;
    HIP_TRY(c, hipEventRecord(bb.ev_match, st));
  }
  HIP_TRY(c, wait_event(bb.ev_feat));   // the one wait of the call: the matches go on behind it
  bb.last_slot_l = -1;
  int worst = SPVO_OK;
  for (int k = 0; k < 2; ++k) {
    const int *h_n = bb.h_n + 4 * k;
    outs[k]->n = h_n[0];
    if (h_n[1]) return fail(c, SPVO_ERR_CAPACITY, "spvo_classic_detect: corner buffer overflow in the %s image", k ? "right" : "left");
    if (h_n[0] > cap) worst = SPVO_ERR_CAPACITY;
  }
  if (worst) return fail(c, worst, "spvo_classic_detect: %d / %d rows do not fit slots of %d (slot_capacity)", out_l->n, out_r->n, cap);
  for (int k = 0; k < 2; ++k) {
    BinarySlot &s = bb.slots[slots[k]];
    s.n = outs[k]->n; s.filled = true;
    const int ncopy = std::min(s.n, outs[k]->cap);
    if (ncopy > 0 && outs[k]->kp) std::memcpy(outs[k]->kp, bb.h_kp + (size_t)k * cap, (size_t)ncopy * sizeof(OrbKeypoint));
    if (ncopy > 0 && outs[k]->desc) std::memcpy(outs[k]->desc, bb.h_desc + (size_t)k * cap * row_bytes, (size_t)ncopy * row_bytes);
  }
  if (c->prematch) {
    const BinarySlot &l = bb.slots[slot_l];
    const int partner[2] = {slot_r, temporal ? prev_l : -1};
    for (int k = 0; k < 2; ++k) {
      MatchCache &mc = bb.mcache[k];
      if (partner[k] < 0) continue;
      mc.valid = true;
      mc.slot_a = slot_l; mc.slot_b = partner[k]; mc.selector = c->pm_selector; mc.cross = c->pm_cross; mc.ratio = c->pm_ratio;
      mc.gen_a = l.gen; mc.gen_b = bb.slots[partner[k]].gen;
    }
  }
  bb.last_slot_l = slot_l;
  return SPVO_OK;
}

}  // extern "C"
