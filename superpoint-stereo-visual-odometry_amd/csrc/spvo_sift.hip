// spvo_sift.hip -- the classic front end's SIFT detector + descriptor (sift.hip.h): plan of the pyramid, scratch in the context (grown on
// shape change, nothing allocated per call in steady state), the launch chain, and the final ordering.  The final sort and the removal of
// duplicates run on the HOST after one copy of the records (a few thousand rows): OpenCV's total order (x, y, size, angle, response,
// octave) makes the output independent of the order in which the kernels appended candidates.  Runs on the solver's stream (stream2),
// like the rest of the classic front end.
#include "spvo_internal.hip.h"
#include "sift.hip.h"

#include <numeric>

namespace {
constexpr int SIFT_MIN_SIDE = 6;   // 2 x 6 = 12 > 2 x border: the first octave has an interior; the octave rule then gives >= 2 octaves

// tests/sift_ref.py: blur_taps -- double on the host, rounded to float once
bool sift_taps(double sigma, SiftTaps &tp) {
  const int r = (((int)std::nearbyint(sigma * 8 + 1) | 1) - 1) / 2;
  if (r > SIFT_MAX_R) return false;
  double t[2 * SIFT_MAX_R + 1], s = 0.0;
  for (int j = -r; j <= r; ++j) { t[j + r] = std::exp(-(double)(j * j) / (2.0 * sigma * sigma)); }
  for (int j = 0; j <= 2 * r; ++j) s += t[j];
  for (int j = 0; j <= SIFT_MAX_R; ++j) tp.t[j] = j <= r ? (float)(t[r + j] / s) : 0.f;
  tp.r = r;
  return true;
}

int sift_octaves(int rows, int cols) { return (int)std::nearbyint(std::log2((double)(2 * std::min(rows, cols))) - 2.0) + 1; }

// level geometry of a rows x cols image and where each level lies in the pyramid buffer
size_t sift_plan(int rows, int cols, SiftPyr &P) {
  P.n_oct = std::min(sift_octaves(rows, cols), SIFT_MAX_OCT);
  size_t off = 0;
  int h = 2 * rows, w = 2 * cols;
  for (int o = 0; o < P.n_oct; ++o, h /= 2, w /= 2) {
    const size_t lvl = (size_t)h * w;
    P.h[o] = h; P.w[o] = w;
    P.g_off[o] = (long long)off; off += SIFT_GAUSS * lvl;
    P.d_off[o] = (long long)off; off += SIFT_DOG * lvl;
  }
  return off;
}

// scratch for a rows x cols image with room for `cand_cap` candidates and as many output rows
int sift_ensure(spvo_ctx *c, int rows, int cols, size_t pyr_floats, int cand_cap) {
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  const size_t px = (size_t)rows * cols;
  if (px > s.img_cap || pyr_floats > s.pyr_cap) {
    HIP_TRY(c, hipStreamSynchronize(st));
    dev_free(s.img, s.pyr);
    const size_t npx = std::max(px, s.img_cap), npyr = std::max(pyr_floats, s.pyr_cap);
    s.img_cap = s.pyr_cap = 0;   // a failed allocation below leaves a context that spvo_destroy and a later call can still handle
    int rc;
    if ((rc = dev_alloc(c, &s.img, npx, false)) || (rc = dev_alloc(c, &s.pyr, npyr, false))) return rc;
    s.img_cap = npx; s.pyr_cap = npyr;
  }
  if (cand_cap > s.cand_cap) {
    HIP_TRY(c, hipStreamSynchronize(st));
    dev_free(s.cand_pos, s.cand_off, s.kp, s.desc);
    s.cand_cap = 0;
    int rc;
    if ((rc = dev_alloc(c, &s.cand_pos, cand_cap, false)) || (rc = dev_alloc(c, &s.cand_off, cand_cap, false)) || (rc = dev_alloc(c, &s.kp, cand_cap, false)) ||
        (rc = dev_alloc(c, &s.desc, (size_t)cand_cap * 128, false)))
      return rc;
    s.cand_cap = cand_cap;
  }
  if (!s.counters) {
    if (int rc = dev_alloc(c, &s.counters, 4, false)) return rc;
  }
  return SPVO_OK;
}

// the pyramid of the resident image: 1 + 5 launches per octave, every difference of Gaussians written by the blur that completes it
int sift_enqueue_pyramid(spvo_ctx *c, int rows, int cols, const SiftPyr &P) {
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  const double k = std::pow(2.0, 1.0 / 3.0), sigma = 1.6;
  SiftTaps tp[SIFT_GAUSS];
  if (!sift_taps(std::sqrt(std::max(sigma * sigma - 4 * 0.5 * 0.5, 0.01)), tp[0])) return fail(c, SPVO_ERR_INVALID, "spvo_sift_detect: blur radius above %d", SIFT_MAX_R);
  for (int i = 1; i < SIFT_GAUSS; ++i) {
    const double prev = std::pow(k, (double)(i - 1)) * sigma, total = prev * k;
    if (!sift_taps(std::sqrt(total * total - prev * prev), tp[i])) return fail(c, SPVO_ERR_INVALID, "spvo_sift_detect: blur radius above %d", SIFT_MAX_R);
  }
  for (int o = 0; o < P.n_oct; ++o) {
    const int h = P.h[o], w = P.w[o];
    const size_t lvl = (size_t)h * w;
    float *G = P.pyr + P.g_off[o], *D = P.pyr + P.d_off[o];
    const dim3 grid((w + SIFT_TW - 1) / SIFT_TW, (h + SIFT_TH - 1) / SIFT_TH);
    if (o == 0) {
      hipLaunchKernelGGL(sift_blur_kernel<2>, grid, dim3(256), 0, st, (const void *)s.img, rows, cols, G, (float *)nullptr, (float *)nullptr, h, w, tp[0]);
      hipLaunchKernelGGL(sift_blur_kernel<0>, grid, dim3(256), 0, st, (const void *)G, h, w, G + lvl, D, (float *)nullptr, h, w, tp[1]);
    } else {
      const float *below = P.pyr + P.g_off[o - 1] + (size_t)SIFT_LAYERS * P.h[o - 1] * P.w[o - 1];
      hipLaunchKernelGGL(sift_blur_kernel<1>, grid, dim3(256), 0, st, (const void *)below, P.h[o - 1], P.w[o - 1], G + lvl, D, G, h, w, tp[1]);
    }
    for (int i = 2; i < SIFT_GAUSS; ++i)
      hipLaunchKernelGGL(sift_blur_kernel<0>, grid, dim3(256), 0, st, (const void *)(G + (size_t)(i - 1) * lvl), h, w, G + (size_t)i * lvl, D + (size_t)(i - 1) * lvl, (float *)nullptr, h, w,
                         tp[i]);
  }
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// extrema -> refinement -> orientation + descriptor, behind the pyramid
int sift_enqueue_features(spvo_ctx *c, const SiftPyr &P) {
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  HIP_TRY(c, hipMemsetAsync(s.counters, 0, 4 * sizeof(int), st));
  for (int o = 0; o < P.n_oct; ++o) {
    const int h = P.h[o], w = P.w[o];
    if (h <= 2 * SIFT_BORDER || w <= 2 * SIFT_BORDER) continue;
    const dim3 grid((w - 2 * SIFT_BORDER + 63) / 64, (h - 2 * SIFT_BORDER + 15) / 16, SIFT_LAYERS);
    hipLaunchKernelGGL(sift_extrema_kernel, grid, dim3(256), 0, st, (const float *)(P.pyr + P.d_off[o]), h, w, o, s.cand_pos, s.cand_cap, s.counters);
  }
  hipLaunchKernelGGL(sift_refine_kernel, dim3(std::min((s.cand_cap + 255) / 256, 1024)), dim3(256), 0, st, P, s.cand_pos, s.cand_off, (const int *)s.counters, s.cand_cap);
  hipLaunchKernelGGL(sift_describe_kernel, dim3(std::min(s.cand_cap, 8192)), dim3(64), 0, st, P, (const int4 *)s.cand_pos, (const float4 *)s.cand_off, s.counters, s.cand_cap, s.kp,
                     s.desc, s.cand_cap);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}
}  // namespace

extern "C" {

int spvo_sift_detect(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, spvo_sift_keypoint *kp_out, float *desc_out, int cap, int *n_out) {
  if (!c || !img || !n_out || rows <= 0 || cols <= 0 || stride < (size_t)cols || cap < 0 || (cap > 0 && (!kp_out || !desc_out))) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (rows < SIFT_MIN_SIDE || cols < SIFT_MIN_SIDE) return fail(c, SPVO_ERR_INVALID, "spvo_sift_detect: images of at least %d x %d (the first octave needs an interior)", SIFT_MIN_SIDE, SIFT_MIN_SIDE);
  if ((size_t)rows * cols > ((size_t)1 << 26)) return fail(c, SPVO_ERR_INVALID, "spvo_sift_detect: image too large");
  if (!c->pendq.empty()) return fail(c, SPVO_ERR_STATE, "detector submissions are in flight: complete them with spvo_detect_wait first");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  *n_out = 0;
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  SiftPyr P{};
  const size_t pyr_floats = sift_plan(rows, cols, P);
  s.rows = s.cols = 0;   // nothing resident until the pyramid is enqueued
  int cand_cap = std::max(s.cand_cap, std::max(8192, (int)((size_t)4 * rows * cols / 16)));
  if (int rc = sift_ensure(c, rows, cols, pyr_floats, cand_cap)) return rc;
  P.pyr = s.pyr;
  HIP_TRY(c, hipMemcpy2DAsync(s.img, cols, img, stride, cols, rows, hipMemcpyHostToDevice, st));
  if (int rc = sift_enqueue_pyramid(c, rows, cols, P)) return rc;
  s.plan = P; s.rows = rows; s.cols = cols;
  int cnt[4] = {0, 0, 0, 0};
  for (int attempt = 0;; ++attempt) {
    if (int rc = sift_enqueue_features(c, P)) return rc;
    HIP_TRY(c, hipMemcpyAsync(cnt, s.counters, sizeof cnt, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (cnt[0] <= s.cand_cap && cnt[1] <= s.cand_cap) break;
    // more candidates (or output rows) than the lists hold: grow them to what was counted and run the stages behind the pyramid again
    if (attempt >= 2) return fail(c, SPVO_ERR_CAPACITY, "spvo_sift_detect: %d candidates / %d keypoints do not fit", cnt[0], cnt[1]);
    if (int rc = sift_ensure(c, rows, cols, pyr_floats, std::max(cnt[0], cnt[1]) + 1024)) return rc;
  }
  const int n_cand = cnt[0], n_kp = cnt[1];
  if (n_kp == 0) return SPVO_OK;
  s.h_pos.resize(n_cand); s.h_off.resize(n_cand); s.h_kp.resize(n_kp); s.h_desc.resize((size_t)n_kp * 128);
  HIP_TRY(c, hipMemcpyAsync(s.h_pos.data(), s.cand_pos, (size_t)n_cand * sizeof(int4), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(s.h_off.data(), s.cand_off, (size_t)n_cand * sizeof(float4), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(s.h_kp.data(), s.kp, (size_t)n_kp * sizeof(int2), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(s.h_desc.data(), s.desc, (size_t)n_kp * 128 * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  // keypoint records (tests/sift_ref.py: candidate_record), the first octave being -1: coordinates and size are halved
  s.h_rec.resize(n_kp);
  s.h_order.resize(n_kp);
  for (int i = 0; i < n_kp; ++i) {
    const int4 p = s.h_pos[s.h_kp[i].x];
    const float4 f = s.h_off[s.h_kp[i].x];
    const int o = p.x, layer = p.y;
    const float scale = std::ldexp(1.f, o);
    spvo_sift_keypoint &k = s.h_rec[i];
    k.x = (((float)p.w + f.z) * scale) * 0.5f;
    k.y = (((float)p.z + f.y) * scale) * 0.5f;
    k.size = (float)(1.6 * std::pow(2.0, ((double)layer + (double)f.x) / 3.0) * std::ldexp(1.0, o));
    std::memcpy(&k.angle, &s.h_kp[i].y, sizeof(float));
    k.response = std::fabs(f.w);
    const int packed = o + (layer << 8) + ((int)std::nearbyint((f.x + 0.5f) * 255.f) << 16);
    k.octave = (packed & ~255) | ((packed - 1) & 255);
    s.h_order[i] = i;
  }
  const auto &rec = s.h_rec;
  std::sort(s.h_order.begin(), s.h_order.end(), [&rec](int a, int b) {
    const spvo_sift_keypoint &p = rec[a], &q = rec[b];
    if (p.x != q.x) return p.x < q.x;
    if (p.y != q.y) return p.y < q.y;
    if (p.size != q.size) return p.size < q.size;
    if (p.angle != q.angle) return p.angle < q.angle;
    if (p.response != q.response) return p.response < q.response;
    return p.octave < q.octave;
  });
  int n = 0;
  const spvo_sift_keypoint *last = nullptr;
  for (int i : s.h_order) {
    const spvo_sift_keypoint &k = rec[i];
    if (last && last->x == k.x && last->y == k.y && last->size == k.size && last->angle == k.angle) continue;   // cv::KeyPointsFilter::removeDuplicatedSorted
    last = &k;
    if (n < cap) {
      kp_out[n] = k;
      std::memcpy(desc_out + (size_t)n * 128, s.h_desc.data() + (size_t)i * 128, 128 * sizeof(float));
    }
    ++n;
  }
  *n_out = n;
  return SPVO_OK;
}

int spvo_sift_debug_level(spvo_ctx *c, int octave, int layer, int dog, float *out, int *rows, int *cols) {
  if (!c) return fail(c, SPVO_ERR_INVALID, "null context");
  auto &s = c->sift;
  if (s.rows == 0) return fail(c, SPVO_ERR_STATE, "spvo_sift_debug_level: no pyramid is resident (call spvo_sift_detect first)");
  if (octave < 0 || octave >= s.plan.n_oct || layer < 0 || layer >= (dog ? SIFT_DOG : SIFT_GAUSS)) return fail(c, SPVO_ERR_INVALID, "spvo_sift_debug_level: no such level");
  const int h = s.plan.h[octave], w = s.plan.w[octave];
  if (rows) *rows = h;
  if (cols) *cols = w;
  if (out) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const float *src = s.pyr + (dog ? s.plan.d_off[octave] : s.plan.g_off[octave]) + (size_t)layer * h * w;
    HIP_TRY(c, hipMemcpyAsync(out, src, (size_t)h * w * sizeof(float), hipMemcpyDeviceToHost, c->stream2));
    HIP_TRY(c, hipStreamSynchronize(c->stream2));
  }
  return SPVO_OK;
}

}  // extern "C"
