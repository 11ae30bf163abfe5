// spvo_brisk.hip -- the classic front end's BRISK descriptor extractor on given keypoints (brisk.hip.h): the pattern tables (built once
// per process on the host, in double, by the formulas tests/brisk_ref.py lists), spvo_brisk_tables, spvo_brisk_describe and the extractor
// as a link of spvo_classic_detect's chain (brisk_chain_ensure / brisk_chain_enqueue) and of spvo_brisk_detect_pair's
// (brisk_pair_chain_enqueue).  Runs on the
// solver's stream (stream2) on the image the Shi-Tomasi / FAST detectors and the ORB extractor keep resident (spvo_ctx::cls) and owns
// everything else it needs (spvo_ctx::brisk).
#include "spvo_internal.hip.h"
#include "brisk.hip.h"

#include <mutex>

namespace {
struct BriskHostTables {
  std::vector<float> points;   // [64][1024][60][3] x, y, sigma
  BriskShortPair short_pairs[BRISK_SHORT];
  BriskLongPair long_pairs[BRISK_LONG];
  float scale_list[BRISK_SCALES];
  BriskParams params;
  bool ok = false;
};

// brisk_ref.py choices 1-7
void brisk_build_tables(BriskHostTables &t) {
  constexpr double PI = 3.141592653589793;
  constexpr int ring_n[5] = {1, 10, 14, 15, 20};
  const double mult[5] = {0.0, 2.9, 4.9, 7.4, 10.8};
  float ring_r[5];
  for (int k = 0; k < 5; ++k) ring_r[k] = (float)((double)0.85f * mult[k]);
  const double sigma_scale = (double)1.3f;
  t.points.resize((size_t)BRISK_SCALES * BRISK_ROT * BRISK_POINTS * 3);
  float *out = t.points.data();
  bool sigma_ok = true;
  for (int s = 0; s < BRISK_SCALES; ++s) {
    t.scale_list[s] = (float)std::pow(2.0, s * std::log2(30.0) / BRISK_SCALES);
    const double sc = (double)t.scale_list[s];
    float sigma[5];
    int size = 0;
    for (int ring = 0; ring < 5; ++ring) {
      sigma[ring] = ring == 0 ? (float)(sigma_scale * sc * 0.5) : (float)(sigma_scale * sc * (double)ring_r[ring] * std::sin(PI / ring_n[ring]));
      sigma_ok = sigma_ok && sigma[ring] >= 0.5f;   // (OpenCV's bilinear branch for smaller sigmas is not built)
      size = std::max(size, (int)std::ceil(sc * (double)ring_r[ring] + (double)sigma[ring]) + 1);
    }
    t.params.size_list[s] = size;
    for (int rot = 0; rot < BRISK_ROT; ++rot) {
      const double theta = (double)rot * 2 * PI / (double)BRISK_ROT;
      for (int ring = 0; ring < 5; ++ring)
        for (int num = 0; num < ring_n[ring]; ++num) {
          const double alpha = (double)num * 2 * PI / (double)ring_n[ring];
          *out++ = (float)(sc * (double)ring_r[ring] * std::cos(alpha + theta));
          *out++ = (float)(sc * (double)ring_r[ring] * std::sin(alpha + theta));
          *out++ = sigma[ring];
        }
    }
  }
  const double d_long_sq = (double)8.2f * (double)8.2f, d_short_sq = (double)5.85f * (double)5.85f;
  const float *p = t.points.data();   // scale 0, rotation 0
  int n_short = 0, n_long = 0;
  for (int i = 1; i < BRISK_POINTS; ++i)
    for (int j = 0; j < i; ++j) {
      const double dx = (double)p[3 * j] - (double)p[3 * i], dy = (double)p[3 * j + 1] - (double)p[3 * i + 1];
      const double n2 = dx * dx + dy * dy;
      if (n2 > d_long_sq) {
        if (n_long < BRISK_LONG) t.long_pairs[n_long] = BriskLongPair{(unsigned char)i, (unsigned char)j, (short)(int)(dx / n2 * 2048.0 + 0.5), (short)(int)(dy / n2 * 2048.0 + 0.5), 0};
        ++n_long;
      } else if (n2 < d_short_sq) {
        if (n_short < BRISK_SHORT) t.short_pairs[n_short] = BriskShortPair{(unsigned char)i, (unsigned char)j};
        ++n_short;
      }
    }
  t.params.basic_size_06 = 12.0f * 0.6f;
  const float lb = (float)std::log(30.0) / 0.693147180559945f;
  t.params.scales_over_lb = (float)BRISK_SCALES / lb;
  t.ok = sigma_ok && n_short == BRISK_SHORT && n_long == BRISK_LONG;
}

const BriskHostTables &brisk_tables() {
  static BriskHostTables t;
  static std::once_flag once;
  std::call_once(once, [] { brisk_build_tables(t); });
  return t;
}

// the tables on the device: uploaded on a context's first BRISK call (the point table is 47 MB: a one-off cost, include/spvo.h).  A call that
// fails half way is started over by the next: tables_ready is set last, and the grow list frees what the failed call left.
int brisk_upload_tables(spvo_ctx *c, const BriskHostTables &t) {
  auto &k = c->brisk;
  if (int rc = grow(c, wait_for_nothing(), {plain(k.points, t.points.size()), plain(k.long_pairs, BRISK_LONG), plain(k.short_pairs, BRISK_SHORT), zeroed(k.cnt, 4)})) return rc;
  k.h_n.reset();   // (re-allocated behind the uploads, below)
  HIP_TRY(c, hipMemcpy(k.points, t.points.data(), t.points.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(k.long_pairs, t.long_pairs, sizeof t.long_pairs, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(k.short_pairs, t.short_pairs, sizeof t.short_pairs, hipMemcpyHostToDevice));
  return grow(c, wait_for_nothing(), {plain(k.h_n, 4)});
}

int brisk_ensure_tables(spvo_ctx *c) {
  auto &k = c->brisk;
  if (k.tables_ready) return SPVO_OK;
  const BriskHostTables &t = brisk_tables();
  if (!t.ok) return fail(c, SPVO_ERR_STATE, "BRISK: the pattern tables failed their own checks (512 short pairs, 870 long pairs, every sigma >= 0.5)");
  if (int rc = brisk_upload_tables(c, t)) return rc;
  k.tables_ready = true;
  return SPVO_OK;
}

// the integral image for rows x cols, the keypoint buffers and their pinned mirrors for n rows (grown geometrically: a keypoint count that
// creeps up from call to call reallocates rarely), the values0 buffers only for a call that asks for them
int brisk_ensure(spvo_ctx *c, int rows, int cols, int n, bool want_values0) {
  auto &k = c->brisk;
  hipStream_t st = c->stream2;
  const size_t need = (size_t)(rows + 1) * (cols + 1);
  if (need > k.integ.count())
    if (int rc = grow(c, wait_for(st), {plain(k.integ, need)})) return rc;
  if (n > k.kp_cap) {
    const int cap = (int)std::min<long long>(std::max<long long>(n, 2ll * k.kp_cap), 0x7FFFFFFF);
    k.kp_cap = 0;   // a failed allocation below leaves a context that spvo_destroy and a later call can still handle
    if (int rc = grow(c, wait_for(st), {plain(k.xy, (size_t)2 * cap), plain(k.size, cap), plain(k.angle, cap), plain(k.kept, cap), plain(k.kscale, cap), plain(k.desc, (size_t)cap * BRISK_BYTES),
                                        plain(k.h_kept, cap), plain(k.h_angle, cap), plain(k.h_desc, (size_t)cap * BRISK_BYTES)}))
      return rc;
    k.kp_cap = cap;
  }
  if (want_values0 && n > k.v0_cap) {
    const int cap = std::max(n, k.kp_cap);
    k.v0_cap = 0;
    if (int rc = grow(c, wait_for(st), {plain(k.values0, (size_t)cap * BRISK_POINTS), plain(k.h_values0, (size_t)cap * BRISK_POINTS)})) return rc;
    k.v0_cap = cap;
  }
  return SPVO_OK;
}
}  // namespace

int spvo_int::brisk_check_image(spvo_ctx *c, const char *who, int rows, int cols) {
  if ((long long)rows * cols * 255 >= (1ll << 31)) return fail(c, SPVO_ERR_INVALID, "%s: %d x %d pixels do not fit the int32 integral image", who, rows, cols);
  return SPVO_OK;
}

int spvo_int::brisk_chain_ensure(spvo_ctx *c, int rows, int cols, int cap) {
  if (int rc = brisk_ensure_tables(c)) return rc;
  return brisk_ensure(c, rows, cols, cap, false);
}

// spvo_brisk_describe's launches without its two host round trips: the keypoints are the detector's list where it lies (cls.xy, cls.resp,
// cls.counters), the rows go straight into the slot.  kept / kscale / angle and the integral image are shared by the two images of a pair,
// which is correct in stream order.
int spvo_int::brisk_chain_enqueue(spvo_ctx *c, int rows, int cols, float size, int cap, int most, const ChainOut &o) {
  auto &b = c->cls;
  auto &k = c->brisk;
  hipStream_t st = c->stream2;
  uint8_t *desc = reinterpret_cast<uint8_t *>(o.d_desc);
  hipLaunchKernelGGL(brisk_integral_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, b.im, rows, cols, k.integ);
  hipLaunchKernelGGL(brisk_integral_cols_kernel, dim3((cols + 1 + 255) / 256), dim3(256), 0, st, rows, cols, k.integ);
  hipLaunchKernelGGL(brisk_compact_list_kernel, dim3(1), dim3(1024), 0, st, b.xy, b.resp, b.counters, size, rows, cols, brisk_tables().params, cap, k.kept, k.kscale, o.kresp, o.cnt);
  // (the describe kernel reads its row count at cnt[0]: handed cnt + 2, it describes min(kept, cap) rows)
  hipLaunchKernelGGL(brisk_describe_kernel, dim3(std::min((std::max(most, 1) + 3) / 4, BRISK_DESCRIBE_BLOCKS)), dim3(256), 0, st, b.im, k.integ, rows, cols, b.xy, k.kept, k.kscale, o.cnt + 2, k.points,
                     k.long_pairs, k.short_pairs, k.angle, desc, nullptr);
  hipLaunchKernelGGL(brisk_slot_finish_kernel, dim3(32), dim3(256), 0, st, b.counters, o.cnt, b.xy, k.kept, k.angle, o.kresp, reinterpret_cast<const uint4 *>(desc), cap, o.d_kp, o.d_n, o.h_n, o.h_kp,
                     reinterpret_cast<uint4 *>(o.h_desc));
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// The same behind the BRISK detector (spvo_brisk_detect_pair): the keypoints are the detector's records where brisk_refine_kernel left them,
// each with a size of its own, so ONE launch applies the keep flag and the border rule and leaves the packed coordinate list the describe
// kernel reads (spvo_ctx::brisk.xy: kept[k] = k); its grid is fixed by the slot capacity, the count is read on the device.
int spvo_int::brisk_pair_chain_enqueue(spvo_ctx *c, int rows, int cols, int cap, const BriskDetKeypoint *rec, const int *keep, const int *det_counters, int det_cap,
                                       BriskDetKeypoint *crec, const ChainOut &o, BriskDetKeypoint *h_kp) {
  auto &b = c->cls;
  auto &k = c->brisk;
  hipStream_t st = c->stream2;
  uint8_t *desc = reinterpret_cast<uint8_t *>(o.d_desc);
  hipLaunchKernelGGL(brisk_integral_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, b.im, rows, cols, k.integ);
  hipLaunchKernelGGL(brisk_integral_cols_kernel, dim3((cols + 1 + 255) / 256), dim3(256), 0, st, rows, cols, k.integ);
  hipLaunchKernelGGL(brisk_pair_compact_kernel, dim3(1), dim3(1024), 0, st, rec, keep, det_counters, det_cap, rows, cols, brisk_tables().params, cap, k.xy, k.kept, k.kscale, crec, o.cnt);
  hipLaunchKernelGGL(brisk_describe_kernel, dim3(std::min((cap + 3) / 4, BRISK_DESCRIBE_BLOCKS)), dim3(256), 0, st, b.im, k.integ, rows, cols, k.xy, k.kept, k.kscale, o.cnt + 2, k.points, k.long_pairs,
                     k.short_pairs, k.angle, desc, nullptr);
  hipLaunchKernelGGL(brisk_pair_finish_kernel, dim3(32), dim3(256), 0, st, det_counters, o.cnt, crec, k.angle, reinterpret_cast<const uint4 *>(desc), cap, o.d_kp, o.d_n, o.h_n, h_kp,
                     reinterpret_cast<uint4 *>(o.h_desc));
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

extern "C" {

int spvo_brisk_tables(int scale, float *points, int32_t *short_pairs, int32_t *long_pairs, float *scale_list, int32_t *size_list) {
  if (points && (scale < 0 || scale >= BRISK_SCALES)) return fail(nullptr, SPVO_ERR_INVALID, "spvo_brisk_tables: scale must be 0 .. %d", BRISK_SCALES - 1);
  const BriskHostTables &t = brisk_tables();
  if (!t.ok) return fail(nullptr, SPVO_ERR_STATE, "BRISK: the pattern tables failed their own checks (512 short pairs, 870 long pairs, every sigma >= 0.5)");
  const size_t slice = (size_t)BRISK_ROT * BRISK_POINTS * 3;
  if (points) std::memcpy(points, t.points.data() + (size_t)scale * slice, slice * sizeof(float));
  if (short_pairs)
    for (int k = 0; k < BRISK_SHORT; ++k) { short_pairs[2 * k] = t.short_pairs[k].i; short_pairs[2 * k + 1] = t.short_pairs[k].j; }
  if (long_pairs)
    for (int k = 0; k < BRISK_LONG; ++k) {
      long_pairs[4 * k] = t.long_pairs[k].i; long_pairs[4 * k + 1] = t.long_pairs[k].j;
      long_pairs[4 * k + 2] = t.long_pairs[k].wdx; long_pairs[4 * k + 3] = t.long_pairs[k].wdy;
    }
  if (scale_list) std::memcpy(scale_list, t.scale_list, sizeof t.scale_list);
  if (size_list) std::memcpy(size_list, t.params.size_list, sizeof t.params.size_list);
  return SPVO_OK;
}

int spvo_brisk_describe(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, const float *xy, const float *size, int n, int32_t *kept, float *angle, uint8_t *desc,
                        int32_t *values0, int *n_kept) {
  if (!c || !n_kept || rows <= 0 || cols <= 0 || n < 0 || (n > 0 && (!xy || !size || !kept || !desc)) || (img && stride < (size_t)cols)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  *n_kept = 0;
  if (int rc = brisk_check_image(c, "spvo_brisk_describe", rows, cols)) return rc;
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(size[i]) || !(size[i] > 0)) return fail(c, SPVO_ERR_INVALID, "spvo_brisk_describe: keypoint %d has size %g", i, (double)size[i]);
  if (int rc = require_idle(c)) return rc;
  auto &b = c->cls;
  if (!img && (b.rows != rows || b.cols != cols))
    return fail(c, SPVO_ERR_STATE, "spvo_brisk_describe: no image of %d x %d is resident (call spvo_gftt_detect / spvo_fast_detect first, or pass the image)", rows, cols);
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream2;
  if (img) {
    if (int rc = classic_upload_image(c, img, rows, cols, stride)) return rc;
  }
  if (n == 0) {
    HIP_TRY(c, hipStreamSynchronize(st));   // (the caller's image may be in flight)
    return SPVO_OK;
  }
  if (int rc = brisk_ensure_tables(c)) return rc;
  if (int rc = brisk_ensure(c, rows, cols, n, values0 != nullptr)) return rc;
  auto &k = c->brisk;
  HIP_TRY(c, hipMemcpyAsync(k.xy, xy, (size_t)2 * n * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(k.size, size, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(brisk_integral_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, b.im, rows, cols, k.integ);
  hipLaunchKernelGGL(brisk_integral_cols_kernel, dim3((cols + 1 + 255) / 256), dim3(256), 0, st, rows, cols, k.integ);
  hipLaunchKernelGGL(brisk_compact_kernel, dim3(1), dim3(1024), 0, st, k.xy, k.size, n, rows, cols, brisk_tables().params, k.kept, k.kscale, k.cnt);
  hipLaunchKernelGGL(brisk_describe_kernel, dim3(std::min((n + 3) / 4, BRISK_DESCRIBE_BLOCKS)), dim3(256), 0, st, b.im, k.integ, rows, cols, k.xy, k.kept, k.kscale, k.cnt, k.points, k.long_pairs, k.short_pairs, k.angle,
                     k.desc, values0 ? k.values0 : nullptr);
  hipLaunchKernelGGL(brisk_finish_kernel, dim3(32), dim3(256), 0, st, k.cnt, k.kept, k.angle, reinterpret_cast<const uint32_t *>(k.desc.get()), values0 ? k.values0.get() : nullptr, k.h_n, k.h_kept, k.h_angle,
                     reinterpret_cast<uint32_t *>(k.h_desc.get()), values0 ? k.h_values0.get() : nullptr);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(st));   // the one wait of the call
  const int m = std::min(std::max(k.h_n[0], 0), n);
  *n_kept = m;
  if (m > 0) {
    std::memcpy(kept, k.h_kept, (size_t)m * sizeof(int));
    if (angle) std::memcpy(angle, k.h_angle, (size_t)m * sizeof(float));
    std::memcpy(desc, k.h_desc, (size_t)m * BRISK_BYTES);
    if (values0) std::memcpy(values0, k.h_values0, (size_t)m * BRISK_POINTS * sizeof(int));
  }
  return SPVO_OK;
}

}  // extern "C"
