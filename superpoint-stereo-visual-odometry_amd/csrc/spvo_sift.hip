// spvo_sift.hip -- the classic front end's SIFT detector + descriptor (sift.hip.h): plan of the pyramid, scratch in the context (grown on
// shape change, nothing allocated per call in steady state), the launch chain, and the final ordering.  OpenCV's total order (x, y, size,
// angle, response, octave) makes the output independent of the order in which the kernels appended candidates.  spvo_sift_detect sorts
// and removes duplicates on the HOST after one copy of the records (a few thousand rows); spvo_sift_detect_pair does both on the device
// (sift.hip.h: key, rank, unique, gather) and leaves a stereo pair's features in two SIFT slots for spvo_match_l2_slots.  Byte equality
// of the two: the host's records are built by ONE function (sift_record) from {candidate, offsets, angle bits}, which the device hands
// over per final row; the device-computed size is a sort key only, and rows of one candidate get identical keys on the device as on the
// host, so ties and duplicates are the same.  Runs on the solver's stream (stream2), like the rest of the classic front end.
// spvo_sift_describe is the extractor alone on a caller's records: it reads the u8 image the Shi-Tomasi / FAST / BRISK / AKAZE detectors and
// the other extractors keep resident (spvo_ctx::cls), builds a Gaussian-only pyramid in the same buffer and describes in one launch.
// spvo_classic_sift_pair is that extractor behind the Shi-Tomasi / FAST detector for both images of a stereo pair, the list never leaving
// the device: detector chain (spvo_classic.hip), base level, the describe kernel into a SIFT slot.
// sift_link_pair is such a call around a detector that reports an octave (BRISK, AKAZE: spvo_brisk_sift_pair and spvo_akaze_sift_pair
// in the detectors' objects hand it their chain as three functions): the extractor's pyramid for octaves 0 .. the detector's highest,
// reduced to the levels a layer-0 record reads, and the describe kernel on the records where they lie (SiftLinkIO).  spvo_sift_link_debug
// runs that link on a caller's list.
// spvo_sift_brisk_pair is the detector in front of the BRISK extractor's chain (spvo_brisk.hip: brisk_pair_chain_enqueue), a
// PairCall<BinPairFamily> into the binary slots: the pyramid of the shared resident image, the orientation-only instantiation of
// sift_describe_kernel, the ordering, and sift_records_kernel, which presents the ordered list as a detector's list.
// The three SIFT-slot pair calls are a PairCall<SiftPairFamily> (pair_call.hip.h: staging, slots, temporal partner, prematch, the one wait, the
// capacity rule) around their own allocations and chains.
#include "spvo_internal.hip.h"
#include "pair_call.hip.h"
#include "sift.hip.h"

#include <numeric>

namespace {
constexpr int SIFT_MIN_SIDE = 6;   // 2 x 6 = 12 > 2 x border: the first octave has an interior; the octave rule then gives >= 2 octaves

// the images spvo_sift_detect, spvo_sift_detect_pair, spvo_sift_describe and spvo_classic_sift_pair (`who`, for the error text) refuse
int sift_check_image(spvo_ctx *c, const char *who, int rows, int cols) {
  if (rows < SIFT_MIN_SIDE || cols < SIFT_MIN_SIDE) return fail(c, SPVO_ERR_INVALID, "%s: images of at least %d x %d (the first octave needs an interior)", who, SIFT_MIN_SIDE, SIFT_MIN_SIDE);
  if ((size_t)rows * cols > ((size_t)1 << 26)) return fail(c, SPVO_ERR_INVALID, "%s: image too large", who);
  return SPVO_OK;
}

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
  if (px > s.img.count() || pyr_floats > s.pyr.count()) {
    const size_t npx = std::max(px, s.img.count()), npyr = std::max(pyr_floats, s.pyr.count());
    if (int rc = grow(c, wait_for(st), {plain(s.img, npx), plain(s.pyr, npyr)})) return rc;
  }
  if (cand_cap > s.cand_cap) {
    s.cand_cap = 0;
    if (int rc = grow(c, wait_for(st), {plain(s.cand_pos, cand_cap), plain(s.cand_off, cand_cap), plain(s.kp, cand_cap), plain(s.desc, (size_t)cand_cap * 128)})) return rc;
    s.cand_cap = cand_cap;
  }
  if (!s.counters) return grow(c, wait_for_nothing(), {plain(s.counters, 4)});
  return SPVO_OK;
}

// the pyramid of the u8 image `src` (rows x cols, packed): 1 + 5 launches per octave.  doubled: the base is the 2x upsampled image (first
// octave -1), else the image at its own size (first octave 0: spvo_sift_describe).  with_dog: every difference of Gaussians is written by
// the blur that completes it; without, P holds Gaussian levels only.  base_only: ONE launch, layer 0 of the first octave (records that all lie
// there: spvo_classic_sift_pair).  link: only the levels a list reads whose records all have layer 0 -- layers 0 .. 3 of every octave
// but the last (the next octave derives from layer 3) and layer 0 of the last (layer 1 comes with the same launch when the octave is not
// the first); a layer depends only on the one before, so these are bit for bit the levels of the full pyramid
int sift_enqueue_pyramid(spvo_ctx *c, const uint8_t *src, int rows, int cols, const SiftPyr &P, bool doubled = true, bool with_dog = true, bool base_only = false, bool link = false) {
  hipStream_t st = c->stream2;
  const double k = std::pow(2.0, 1.0 / 3.0), sigma = 1.6;
  SiftTaps tp[SIFT_GAUSS];
  if (!sift_taps(std::sqrt(std::max(sigma * sigma - (doubled ? 4 : 1) * 0.5 * 0.5, 0.01)), tp[0])) return fail(c, SPVO_ERR_INVALID, "spvo_sift_detect: blur radius above %d", SIFT_MAX_R);
  for (int i = 1; i < SIFT_GAUSS; ++i) {
    const double prev = std::pow(k, (double)(i - 1)) * sigma, total = prev * k;
    if (!sift_taps(std::sqrt(total * total - prev * prev), tp[i])) return fail(c, SPVO_ERR_INVALID, "spvo_sift_detect: blur radius above %d", SIFT_MAX_R);
  }
  for (int o = 0; o < P.n_oct; ++o) {
    const int h = P.h[o], w = P.w[o];
    const size_t lvl = (size_t)h * w;
    float *G = P.pyr + P.g_off[o], *D = with_dog ? P.pyr + P.d_off[o] : nullptr;
    const dim3 grid((w + SIFT_TW - 1) / SIFT_TW, (h + SIFT_TH - 1) / SIFT_TH);
    const int top = !link ? SIFT_GAUSS - 1 : o == P.n_oct - 1 ? 0 : SIFT_LAYERS;   // the highest layer built
    if (o == 0) {
      if (doubled) hipLaunchKernelGGL(sift_blur_kernel<2>, grid, dim3(256), 0, st, (const void *)src, rows, cols, G, (float *)nullptr, (float *)nullptr, h, w, tp[0]);
      else hipLaunchKernelGGL(sift_blur_kernel<3>, grid, dim3(256), 0, st, (const void *)src, rows, cols, G, (float *)nullptr, (float *)nullptr, h, w, tp[0]);
      if (base_only || top == 0) break;
      hipLaunchKernelGGL(sift_blur_kernel<0>, grid, dim3(256), 0, st, (const void *)G, h, w, G + lvl, D, (float *)nullptr, h, w, tp[1]);
    } else {
      const float *below = P.pyr + P.g_off[o - 1] + (size_t)SIFT_LAYERS * P.h[o - 1] * P.w[o - 1];
      hipLaunchKernelGGL(sift_blur_kernel<1>, grid, dim3(256), 0, st, (const void *)below, P.h[o - 1], P.w[o - 1], G + lvl, D, G, h, w, tp[1]);
    }
    for (int i = 2; i <= top; ++i)
      hipLaunchKernelGGL(sift_blur_kernel<0>, grid, dim3(256), 0, st, (const void *)(G + (size_t)(i - 1) * lvl), h, w, G + (size_t)i * lvl, D ? D + (size_t)(i - 1) * lvl : nullptr, (float *)nullptr,
                         h, w, tp[i]);
  }
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// extrema -> refinement -> orientation + descriptor, behind the pyramid.  describe = false: the orientation-only instantiation -- the raw
// rows {candidate, angle bits} without the 128-float rows (spvo_sift_brisk_pair)
int sift_enqueue_features(spvo_ctx *c, const SiftPyr &P, bool describe = true) {
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
  if (describe)
    hipLaunchKernelGGL(sift_describe_kernel<true>, dim3(std::min(s.cand_cap, 8192)), dim3(64), 0, st, P, (const int4 *)s.cand_pos, (const float4 *)s.cand_off, s.counters, s.cand_cap, s.kp,
                       s.desc, s.cand_cap);
  else
    hipLaunchKernelGGL(sift_describe_kernel<false>, dim3(std::min(s.cand_cap, 8192)), dim3(64), 0, st, P, (const int4 *)s.cand_pos, (const float4 *)s.cand_off, s.counters, s.cand_cap, s.kp,
                       s.desc, s.cand_cap);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// the keypoint record of a raw row (tests/sift_ref.py: candidate_record), the first octave being -1: coordinates and size are halved
spvo_sift_keypoint sift_record(const int4 &p, const float4 &f, int angle_bits) {
  const int o = p.x, layer = p.y;
  const float scale = std::ldexp(1.f, o);
  spvo_sift_keypoint k;
  k.x = (((float)p.w + f.z) * scale) * 0.5f;
  k.y = (((float)p.z + f.y) * scale) * 0.5f;
  k.size = (float)(1.6 * std::pow(2.0, ((double)layer + (double)f.x) / 3.0) * std::ldexp(1.0, o));
  std::memcpy(&k.angle, &angle_bits, sizeof(float));
  k.response = std::fabs(f.w);
  const int packed = o + (layer << 8) + ((int)std::nearbyint((f.x + 0.5f) * 255.f) << 16);
  k.octave = (packed & ~255) | ((packed - 1) & 255);
  return k;
}

// the ordering stage's scratch for `n` raw rows
int sift_order_ensure(spvo_ctx *c, int n) {
  auto &s = c->sift;
  if (!s.ord_n)
    if (int rc = grow(c, wait_for_nothing(), {plain(s.ord_n, 2)})) return rc;
  if (n <= s.ord_cap) return SPVO_OK;
  s.ord_cap = 0;
  if (int rc = grow(c, wait_for(c->stream2), {plain(s.keys, n), plain(s.sorted, n), plain(s.order, n)})) return rc;
  s.ord_cap = n;
  return SPVO_OK;
}

// keys[0 .. min(*n_ptr, cap)) -> order, ord_n[0]: rank, duplicate removal.  `sorted` is cleared first: keys that are no total order
// (a NaN in a caller's records) may leave ranks unused, and every entry read must be a row
int sift_enqueue_sort(spvo_ctx *c, const int *n_ptr, int cap) {
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  HIP_TRY(c, hipMemsetAsync(s.sorted, 0, (size_t)std::max(cap, 1) * sizeof(int), st));
  hipLaunchKernelGGL(sift_rank_kernel, dim3(std::min(std::max((cap + 255) / 256, 1), 256)), dim3(256), 0, st, (const SiftKey *)s.keys, n_ptr, cap, s.sorted);
  hipLaunchKernelGGL(sift_unique_kernel, dim3(1), dim3(1024), 0, st, (const SiftKey *)s.keys, (const int *)s.sorted, n_ptr, cap, s.order, s.ord_n);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// the raw rows of the image just described -> `slot` and the host's mirrors of image k, behind sift_enqueue_features
int sift_enqueue_order(spvo_ctx *c, SiftSlot &slot, int k) {
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  hipLaunchKernelGGL(sift_key_kernel, dim3(std::min((s.cand_cap + 255) / 256, 256)), dim3(256), 0, st, (const int4 *)s.cand_pos, (const float4 *)s.cand_off, (const int2 *)s.kp,
                     (const int *)s.counters, s.cand_cap, s.keys);
  if (int rc = sift_enqueue_sort(c, s.counters + 1, s.cand_cap)) return rc;
  hipLaunchKernelGGL(sift_gather_kernel, dim3(64), dim3(256), 0, st, (const int *)s.order, (const int *)s.ord_n, (const int *)s.counters, (const int2 *)s.kp, (const int4 *)s.cand_pos,
                     (const float4 *)s.cand_off, (const float *)s.desc, s.slot_cap, slot.d_desc, slot.d_sqn, slot.d_src, slot.d_n, s.hm_desc + (size_t)k * s.slot_cap * 128,
                     s.h_src + (size_t)k * s.slot_cap, s.h_n + 4 * k);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// spvo_sift_brisk_pair's buffers for lists of `n` rows
int sift_brisk_ensure(spvo_ctx *c, int n) {
  auto &s = c->sift;
  if (!s.brk_cnt)
    if (int rc = grow(c, wait_for_nothing(), {zeroed(s.brk_cnt, 2 * 4), plain(s.hb_n, 2 * 4)})) return rc;
  if (n <= s.brk_cap) return SPVO_OK;
  s.brk_cap = 0;
  if (int rc = grow(c, wait_for(c->stream2), {plain(s.brk_rec, (size_t)n), plain(s.brk_crec, (size_t)n), plain(s.brk_keep, (size_t)n), plain(s.hb_src, (size_t)2 * n)})) return rc;
  s.brk_cap = n;
  return SPVO_OK;
}

// the raw rows of the image just given its orientations -> the ordered list as a detector's list in brk_rec / brk_keep / brk_cnt + 4 k and
// the sources' mirrors of image k, behind sift_enqueue_features; list_cap = s.cand_cap <= s.brk_cap
int sift_enqueue_records(spvo_ctx *c, int k) {
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  hipLaunchKernelGGL(sift_key_kernel, dim3(std::min((s.cand_cap + 255) / 256, 256)), dim3(256), 0, st, (const int4 *)s.cand_pos, (const float4 *)s.cand_off, (const int2 *)s.kp,
                     (const int *)s.counters, s.cand_cap, s.keys);
  if (int rc = sift_enqueue_sort(c, s.counters + 1, s.cand_cap)) return rc;
  hipLaunchKernelGGL(sift_records_kernel, dim3(32), dim3(256), 0, st, (const int *)s.order, (const int *)s.ord_n, (const int *)s.counters, s.cand_cap, (const SiftKey *)s.keys,
                     (const int2 *)s.kp, (const int4 *)s.cand_pos, (const float4 *)s.cand_off, s.brk_rec, s.brk_keep, s.brk_cnt + 4 * k, s.hb_src + (size_t)k * s.brk_cap, s.hb_n + 4 * k);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// what sift_slots_ensure forgets when it re-allocates everything the slot capacity sizes: the slots are empty afterwards
void sift_release_slots(spvo_ctx *c) {
  auto &s = c->sift;
  for (SiftSlot &sl : s.slots) slot_rewrite(sl);
  s.pair.mcache.invalidate();
  s.slot_cap = 0; s.pair.last_slot_l = -1;
}

// the SIFT slots and the call's own buffers for `cap` rows per slot and images of `px` bytes; growing un-fills every slot
int sift_slots_ensure(spvo_ctx *c, int cap, size_t px) {
  auto &s = c->sift;
  if (int rc = s.pair.ensure(c, px)) return rc;
  if (cap <= s.slot_cap) return SPVO_OK;
  HIP_TRY(c, hipDeviceSynchronize());   // (a match may still read the slots where the L2 matcher runs)
  s.match_pending = false;
  sift_release_slots(c);
  std::vector<GrowEntry> list;
  for (SiftSlot &sl : s.slots) list.insert(list.end(), {zeroed(sl.d_desc, (size_t)cap * 256), zeroed(sl.d_sqn, (size_t)cap + 4), zeroed(sl.d_src, cap), zeroed(sl.d_n, 1)});
  list.insert(list.end(), {plain(s.h_src, (size_t)2 * cap), plain(s.hm_desc, (size_t)2 * cap * 128), plain(s.h_n, 4 * 4)});
  if (int rc = grow(c, wait_for_nothing(), list)) return rc;
  s.slot_cap = cap;
  return SPVO_OK;
}

// spvo_set_prematch for an entry point that fills two SIFT slots, in three steps (the other two: SiftPairFamily).  The
// matches are enqueued before the counts are known: scratch for full slots, results spaced by the matcher's capacity
int sift_prematch_ensure(spvo_ctx *c) {
  auto &s = c->sift;
  if (!c->prematch) return SPVO_OK;
  if (int rc = ensure_match(c, s.slot_cap, s.slot_cap)) return rc;
  if (s.h_match_cap != c->match_cap) {
    HIP_TRY(c, hipDeviceSynchronize());
    s.match_pending = false;
    s.h_match_cap = 0;
    s.pair.mcache.invalidate();
    if (int rc = grow(c, wait_for_nothing(), {plain(s.h_match, (size_t)2 * c->match_cap)})) return rc;
    s.h_match_cap = c->match_cap;
  }
  return SPVO_OK;
}
// The SIFT slots' side of the resident-pair protocol (pair_call.hip.h lists what a family is): features on the solver's stream, matches
// where the L2 matcher runs (PostScope), so the chains wait for the matches of the call before
struct SiftPairFamily {
  static constexpr int SLOTS = N_SIFT_SLOTS, CAP_MAX = SIFT_SLOT_MAX;
  static constexpr bool OUT_NEEDS_BUFFERS = true, FORGETS_AFTER_WAIT = false;
  static PairStage &pair(spvo_ctx *c) { return c->sift.pair; }
  static const int *h_n(spvo_ctx *c) { return c->sift.h_n; }
  static SlotState &slot(spvo_ctx *c, int i) { return c->sift.slots[i]; }
  static void rewrite(spvo_ctx *c, int i) { slot_rewrite(c->sift.slots[i]); }
  static bool partner_ok(spvo_ctx *c, int prev) { return c->sift.slots[prev].filled; }
  // a match of an earlier call (or of spvo_sift_detect_pair's attempt before) may still read the slots where the L2 matcher runs
  static int before_chains(spvo_ctx *c) {
    if (c->sift.match_pending) HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->sift.pair.ev_match, 0));
    return SPVO_OK;
  }
  // the two standard matches (slot_l -> partner[0], the stereo one, and -> partner[1], the temporal one, or -1) as ONE set of launches
  // behind the features (pair.ev_feat), counts read on the device
  static int enqueue_prematch(spvo_ctx *c, int slot_l, const int partner[2], int) {
    auto &s = c->sift;
    if (!c->prematch) return SPVO_OK;
    PostScope post(c);
    MatchReq req[2];
    int njobs = 0;
    const SiftSlot &a = s.slots[slot_l];
    for (int k = 0; k < 2; ++k) {
      if (partner[k] < 0) continue;
      const SiftSlot &b = s.slots[partner[k]];
      req[njobs++] = MatchReq{a.d_desc, b.d_desc, s.slot_cap, s.slot_cap, a.d_n, b.d_n, a.d_sqn, b.d_sqn};
    }
    HIP_TRY(c, hipStreamWaitEvent(c->post, s.pair.ev_feat, 0));
    if (int rc = enqueue_matches(c, req, njobs, c->pm_selector, c->pm_cross, c->pm_ratio, s.h_match)) return rc;
    HIP_TRY(c, hipEventRecord(s.pair.ev_match, c->post));
    s.match_pending = true;
    return SPVO_OK;
  }
  // ... and, once both slots are filled, where their results will be: job `job`'s lands in cache entry `job`
  static void record_prematch(spvo_ctx *c, int slot_l, const int partner[2], int) {
    auto &s = c->sift;
    if (!c->prematch) return;
    for (int k = 0, job = 0; k < 2; ++k) {
      if (partner[k] < 0) continue;
      s.pair.mcache.record(job, slot_l, partner[k], s.slots[slot_l].gen, s.slots[partner[k]].gen, c->pm_selector, c->pm_cross, c->pm_ratio, s.h_match + (size_t)job * c->match_cap);
      ++job;
    }
  }
};
// the mirrors commit copies image k's rows from: records of `kp_bytes` in each half's front of h_src (NULL: the caller converts), rows of 128 floats
PairMirror sift_mirror(spvo_ctx *c, int k, bool records, size_t kp_bytes) {
  auto &s = c->sift;
  return PairMirror{records ? s.h_src + (size_t)k * s.slot_cap : nullptr, kp_bytes, s.hm_desc + (size_t)k * s.slot_cap * 128, 128 * sizeof(float)};
}

// spvo_sift_describe's (and spvo_sift_link_debug's) device copies of a caller's n records and their rows
int sift_given_ensure(spvo_ctx *c, int n) {
  auto &s = c->sift;
  if (n <= s.given_cap) return SPVO_OK;
  const int cap = (int)std::min<long long>(std::max<long long>(n, 2ll * s.given_cap), 0x7FFFFFFF);   // (grown geometrically: a count that creeps up reallocates rarely)
  s.given_cap = 0;
  if (int rc = grow(c, wait_for(c->stream2), {plain(s.given_kp, cap), plain(s.given_desc, (size_t)cap * 128)})) return rc;
  s.given_cap = cap;
  return SPVO_OK;
}

// the pyramid buffer grown to `pyr_floats`
int sift_pyr_ensure(spvo_ctx *c, size_t pyr_floats) {
  auto &s = c->sift;
  if (pyr_floats <= s.pyr.count()) return SPVO_OK;
  return grow(c, wait_for(c->stream2), {plain(s.pyr, pyr_floats)});
}

// ---- the link behind a detector whose records carry an octave (spvo_brisk_sift_pair, spvo_akaze_sift_pair, spvo_sift_link_debug)
// the Gaussian-only pyramid of a rows x cols image at its own size, octaves 0 .. max_octave: spvo_sift_describe's layout with first = 0
size_t sift_link_plan(int rows, int cols, int max_octave, SiftPyr &P) {
  P = SiftPyr{};
  P.n_oct = max_octave + 1;
  size_t off = 0;
  for (int o = 0, h = rows, w = cols; o <= max_octave; ++o, h /= 2, w /= 2) {
    P.h[o] = h; P.w[o] = w;
    P.g_off[o] = (long long)off; P.d_off[o] = 0;
    off += (size_t)SIFT_GAUSS * h * w;
  }
  return off;
}

// the host cannot see which octaves the records name, so the shape must have every octave the pyramid is built for
int sift_link_check_octave(spvo_ctx *c, const char *who, int rows, int cols, int max_octave) {
  if (max_octave < 0 || max_octave >= SIFT_MAX_OCT) return fail(c, SPVO_ERR_INVALID, "%s: max_octave must be 0 .. %d", who, SIFT_MAX_OCT - 1);
  if ((std::min(rows, cols) >> max_octave) < 1)
    return fail(c, SPVO_ERR_INVALID, "%s: a %d x %d image has no octave %d (the pyramid is built up to it, whichever octaves the keypoints name)", who, rows, cols, max_octave);
  return SPVO_OK;
}

// the pyramid buffer, the counts and room for `list_cap` kept indices
int sift_link_ensure(spvo_ctx *c, size_t pyr_floats, int list_cap) {
  auto &s = c->sift;
  if (int rc = sift_pyr_ensure(c, pyr_floats)) return rc;
  if (!s.lnk_cnt)
    if (int rc = grow(c, wait_for_nothing(), {zeroed(s.lnk_cnt, 4)})) return rc;
  if (list_cap > s.lnk_cap) {
    s.lnk_cap = 0;
    if (int rc = grow(c, wait_for(c->stream2), {plain(s.lnk_kept, (size_t)list_cap)})) return rc;
    s.lnk_cap = list_cap;
  }
  return SPVO_OK;
}

// Behind a detector's chain on the image resident in spvo_ctx::cls: the keep flags as a list of indices (where the list has flags or
// `compact` asks for the list anyway), the pyramid's levels that are read, and the describe launch on spvo_classic_sift_pair's fixed grid --
// FORM 0, the kernel body of spvo_sift_describe -- with the count read on the device
int sift_link_enqueue(spvo_ctx *c, int rows, int cols, const SiftPyr &P, SiftLinkIO io, bool compact) {
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  if (io.s.keep || compact) {
    hipLaunchKernelGGL(sift_link_compact_kernel, dim3(1), dim3(1024), 0, st, io.s.keep, io.s.n_ptr, std::min(io.s.n_cap, s.lnk_cap), s.lnk_kept, s.lnk_cnt);
    io.kept = s.lnk_kept; io.n_kept = s.lnk_cnt;
  } else {
    io.kept = io.n_kept = nullptr;
  }
  if (int rc = sift_enqueue_pyramid(c, c->cls.im, rows, cols, P, false, false, false, true)) return rc;
  io.max_octave = P.n_oct - 1;
  const int waves = std::min(std::max(tuning("sift_pair_waves_per_cu", 4), 1), 64) * c->num_cus;   // (diagnostic: the grid NOTES.md measures the default against)
  hipLaunchKernelGGL((sift_describe_given_kernel<0, SiftLinkIO>), dim3(waves), dim3(64), 0, st, P, 0, io);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}
}  // namespace

// A detector that reports an octave + SIFT of a stereo pair into two SIFT slots: spvo_classic_sift_pair's protocol around the detector's
// chain (det.enqueue) and sift_link_enqueue, image by image in stream order.  The detector's lists, the kept indices and the pyramid are
// the left image's first and the right image's afterwards: the describe launch of an image, the last of its chain, has put its counts
// into the pinned h_n before the next image's chain clears anything.  A slot's d_src holds the SiftKey records; the mirror h_src holds the
// detector's own records, `stride` bytes each.
int spvo_int::sift_link_pair(spvo_ctx *c, const SiftLinkDetector &det, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int slot_l, int slot_r,
                             int slot_capacity, const PairOut &out_l, const PairOut &out_r) {
  static_assert(sizeof(SiftKey) <= sizeof(SiftSrc) && sizeof(AkazeKp) <= sizeof(SiftSrc), "a slot's source array and its mirror hold the records");
  const char *who = det.who;
  const int cap = slot_capacity;
  PairCall<SiftPairFamily> pc(c, who, SiftPairFamily{}, out_l, out_r);
  int rc;
  if ((rc = pc.check(slot_l, slot_r)) || (rc = pc.check_capacity(cap)) || (rc = det.check()) || (rc = sift_check_image(c, who, rows, cols)) ||
      (rc = sift_link_check_octave(c, who, rows, cols, det.max_octave)) || (rc = pc.open()))
    return rc;
  auto &s = c->sift;
  s.rows = s.cols = 0;   // the pyramid buffer holds the levels that are read of each image in turn: nothing spvo_sift_debug_level could serve
  SiftPyr P{};
  const size_t pyr_floats = sift_link_plan(rows, cols, det.max_octave, P);
  SiftLinkSrc src{};
  // every allocation before the first launch of the chain; the image buffer before the detector's layout, which points into it
  if ((rc = classic_image_ensure(c, rows, cols)) || (rc = det.prepare(src))) return rc;
  if (src.stride <= 0 || src.stride % 4 || src.stride > (int)sizeof(SiftSrc)) return fail(c, SPVO_ERR_STATE, "%s: records of %d bytes", who, src.stride);
  if ((rc = sift_link_ensure(c, pyr_floats, src.keep ? src.n_cap : 0)) || (rc = sift_slots_ensure(c, cap, (size_t)rows * cols)) || (rc = sift_prematch_ensure(c))) return rc;
  P.pyr = s.pyr;
  if ((rc = pc.load(img_l, img_r, rows, cols, stride))) return rc;
  char *const h_rec = reinterpret_cast<char *>(s.h_src.get());
  for (int k = 0; k < 2; ++k) {   // left chain, then the right one
    if ((rc = det.enqueue(pc.image(k)))) return rc;
    const SiftSlot &t = s.slots[pc.slots[k]];
    SiftLinkIO io{};
    io.s = src;
    io.slot_cap = cap;
    io.s_desc = t.d_desc; io.s_sqn = t.d_sqn; io.s_rec = reinterpret_cast<SiftKey *>(t.d_src.get()); io.d_n = t.d_n;
    io.h_desc = s.hm_desc + (size_t)k * s.slot_cap * 128;
    io.h_rec = h_rec + (size_t)k * s.slot_cap * sizeof(SiftSrc);
    io.h_n = s.h_n + 4 * k; io.h_k = s.h_n + 8 + 4 * k;
    if ((rc = sift_link_enqueue(c, rows, cols, P, io, false))) return rc;
  }
  if ((rc = pc.submit())) return rc;
  pc.count(0); pc.count(1);
  // (kept: the BRISK and AKAZE callers answer a detector overflow with SPVO_ERR_STATE -- the detectors size their lists from the image, so
  // the flag cannot be set; were it, the counts would be wrong)
  if ((s.h_n[1] || s.h_n[5]) && det.overflow_is_capacity) return fail(c, SPVO_ERR_CAPACITY, "%s: corner buffer overflow in the %s image", who, s.h_n[1] ? "left" : "right");
  if (s.h_n[1] || s.h_n[5]) return fail(c, SPVO_ERR_STATE, "%s: the candidate list overflowed although it is sized from the image", who);
  const PairMirror mirrors[2] = {sift_mirror(c, 0, true, (size_t)src.stride), sift_mirror(c, 1, true, (size_t)src.stride)};   // (the detector's own records)
  return pc.commit(mirrors);
}

void spvo_int::sift_release(spvo_ctx *c) {
  auto &s = c->sift;
  sift_release_slots(c);
  s.pair.release();
}

extern "C" {

int spvo_sift_detect(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, spvo_sift_keypoint *kp_out, float *desc_out, int cap, int *n_out) {
  if (!c || !img || !n_out || rows <= 0 || cols <= 0 || stride < (size_t)cols || cap < 0 || (cap > 0 && (!kp_out || !desc_out))) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (int rc = sift_check_image(c, "spvo_sift_detect", rows, cols)) return rc;
  if (!c->pendq.empty()) return fail(c, SPVO_ERR_STATE, "detector submissions are in flight: complete them with spvo_detect_wait first");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  *n_out = 0;
  c->akaze.valid = false;   // SIFT keeps an image of its own, but the last detector call owns what is resident: the AKAZE scale space's claim ends (spvo_akaze_describe(img = NULL))
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  SiftPyr P{};
  const size_t pyr_floats = sift_plan(rows, cols, P);
  s.rows = s.cols = 0;   // nothing resident until the pyramid is enqueued
  int cand_cap = std::max(s.cand_cap, std::max(8192, (int)((size_t)4 * rows * cols / 16)));
  if (int rc = sift_ensure(c, rows, cols, pyr_floats, cand_cap)) return rc;
  P.pyr = s.pyr;
  HIP_TRY(c, hipMemcpy2DAsync(s.img, cols, img, stride, cols, rows, hipMemcpyHostToDevice, st));
  if (int rc = sift_enqueue_pyramid(c, s.img, rows, cols, P)) return rc;
  s.plan = P; s.rows = rows; s.cols = cols; s.gauss_only = false;
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
  s.h_rec.resize(n_kp);
  s.h_order.resize(n_kp);
  for (int i = 0; i < n_kp; ++i) {
    s.h_rec[i] = sift_record(s.h_pos[s.h_kp[i].x], s.h_off[s.h_kp[i].x], s.h_kp[i].y);
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

int spvo_sift_slot_rows(spvo_ctx *c, int slot, int *n) {
  if (!c || !n || slot < 0 || slot >= N_SIFT_SLOTS) return fail(c, SPVO_ERR_INVALID, "bad argument");
  const SiftSlot &s = c->sift.slots[slot];
  if (!s.filled) return fail(c, SPVO_ERR_STATE, "SIFT slot %d holds no features (spvo_sift_detect_pair fills it)", slot);
  *n = s.n;
  return SPVO_OK;
}

int spvo_sift_detect_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int slot_l, int slot_r, int slot_capacity,
                          spvo_sift_features *out_l, spvo_sift_features *out_r) {
  if (!c || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  PairCall<SiftPairFamily> pc(c, "spvo_sift_detect_pair", SiftPairFamily{}, pair_out(out_l), pair_out(out_r));
  int rc;
  if ((rc = pc.check(slot_l, slot_r)) || (rc = pc.check_capacity(slot_capacity)) || (rc = sift_check_image(c, pc.who, rows, cols)) || (rc = pc.open())) return rc;
  c->akaze.valid = false;   // as spvo_sift_detect: the AKAZE scale space's claim ends
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  SiftPyr P{};
  const size_t pyr_floats = sift_plan(rows, cols, P), px = (size_t)rows * cols;
  s.rows = s.cols = 0;   // nothing resident until a pyramid is enqueued
  const int cand_cap = std::max(s.cand_cap, std::max(8192, (int)((size_t)4 * rows * cols / 16)));
  if ((rc = sift_ensure(c, rows, cols, pyr_floats, cand_cap)) || (rc = sift_order_ensure(c, s.cand_cap)) || (rc = sift_slots_ensure(c, slot_capacity, px))) return rc;
  pc.cap = s.slot_cap;   // (kept: this entry point's capacity rule is the slots' own capacity, the largest slot_capacity seen: what sift_gather_kernel truncates at)
  if ((rc = sift_prematch_ensure(c))) return rc;
  P.pyr = s.pyr;
  if ((rc = pc.load(img_l, img_r, rows, cols, stride))) return rc;
  for (int attempt = 0;; ++attempt) {
    for (int k = 0; k < 2; ++k) {   // left chain, then the right one: the one resident pyramid is reused in stream order
      s.rows = s.cols = 0;
      HIP_TRY(c, hipMemcpyAsync(s.img, pc.image(k), px, hipMemcpyHostToDevice, st));
      if ((rc = sift_enqueue_pyramid(c, s.img, rows, cols, P))) return rc;
      s.plan = P; s.rows = rows; s.cols = cols; s.gauss_only = false;
      if ((rc = sift_enqueue_features(c, P)) || (rc = sift_enqueue_order(c, s.slots[pc.slots[k]], k))) return rc;
    }
    if ((rc = pc.submit())) return rc;
    int most = 0;
    for (int k = 0; k < 2; ++k) most = std::max(most, std::max(s.h_n[4 * k + 1], s.h_n[4 * k + 2]));
    if (most <= s.cand_cap) break;
    // more candidates (or raw rows) than the lists hold: grow them to what was counted and run the pair again (a second wait)
    if (attempt >= 2) return fail(c, SPVO_ERR_CAPACITY, "spvo_sift_detect_pair: %d candidates / keypoints do not fit", most);
    if (s.match_pending) HIP_TRY(c, wait_event(s.pair.ev_match));
    if ((rc = sift_ensure(c, rows, cols, pyr_floats, most + 1024)) || (rc = sift_order_ensure(c, s.cand_cap)) || (rc = SiftPairFamily::before_chains(c))) return rc;
  }
  pc.count(0); pc.count(1);
  const PairMirror mirrors[2] = {sift_mirror(c, 0, false, 0), sift_mirror(c, 1, false, 0)};   // (the records are built from the sources below)
  if ((rc = pc.commit(mirrors))) return rc;
  spvo_sift_features *const outs[2] = {out_l, out_r};
  for (int k = 0; k < 2; ++k) {
    const SiftSrc *src = s.h_src + (size_t)k * s.slot_cap;
    for (int i = 0, n = pc.ncopy(k); i < n; ++i) outs[k]->kp[i] = sift_record(src[i].pos, src[i].off, __builtin_bit_cast(int, src[i].angle));
  }
  return SPVO_OK;
}

// SIFT keypoints with BRISK descriptors, pair-resident in the BINARY slots (64-byte rows): per image what spvo_sift_detect(img) followed by
// spvo_brisk_describe on its x, y, size hands out, byte for byte.  spvo_brisk_detect_pair's protocol (PairCall<BinPairFamily>); the chain of
// an image is staged image -> resident image (spvo_ctx::cls) -> the SIFT pyramid of THAT image -> candidates and orientations without the
// SIFT rows -> key / rank / unique -> sift_records_kernel -> brisk_pair_chain_enqueue.  The overflow rule is spvo_sift_detect_pair's.
// The size: sift_key_kernel's `size` is a sort key elsewhere; here it picks the BRISK scale index and lands in the record, so behind the
// wait the host rebuilds every final row's record with sift_record from the mirrored sources and compares the sizes bit for bit.  An
// image with a size that differs (none is expected, ever) gets the host's records uploaded and the extractor's chain once more: a second
// wait.  Tuning "sift_brisk_recheck" = 1 (diagnostic) forces that pass for both images.
int spvo_sift_brisk_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int slot_l, int slot_r, int slot_capacity,
                         spvo_brisk_features *out_l, spvo_brisk_features *out_r) {
  if (!c || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  static_assert(sizeof(spvo_brisk_keypoint) == sizeof(BriskDetKeypoint) && sizeof(SiftKey) == sizeof(BriskDetKeypoint), "record layout");
  const char *who = "spvo_sift_brisk_pair";
  const int cap = slot_capacity, row_bytes = 64;
  PairCall<BinPairFamily> pc(c, who, BinPairFamily{row_bytes}, pair_out(out_l), pair_out(out_r));
  int rc;
  if ((rc = pc.check(slot_l, slot_r)) || (rc = pc.check_capacity(cap))) return rc;
  if (cap > 32768) return fail(c, SPVO_ERR_INVALID, "%s: slot_capacity must be 1 .. 32768", who);
  if ((rc = sift_check_image(c, who, rows, cols)) || (rc = brisk_check_image(c, who, rows, cols)) || (rc = pc.open())) return rc;
  c->akaze.valid = false;   // as spvo_sift_detect_pair: the AKAZE scale space's claim ends
  auto &s = c->sift;
  auto &bb = c->bin;
  hipStream_t st = c->stream2;
  SiftPyr P{};
  const size_t pyr_floats = sift_plan(rows, cols, P), px = (size_t)rows * cols;
  s.rows = s.cols = 0;   // nothing resident until a pyramid is enqueued
  const int cand_cap = std::max(s.cand_cap, std::max(8192, (int)((size_t)4 * rows * cols / 16)));
  // every allocation and the BRISK point table before the first launch of the chain
  if ((rc = classic_slots_ensure(c, cap, px)) || (rc = classic_image_ensure(c, rows, cols)) || (rc = brisk_chain_ensure(c, rows, cols, cap)) ||
      (rc = sift_ensure(c, rows, cols, pyr_floats, cand_cap)) || (rc = sift_order_ensure(c, s.cand_cap)) || (rc = sift_brisk_ensure(c, std::max(s.cand_cap, cap))))
    return rc;
  P.pyr = s.pyr;
  if ((rc = pc.load(img_l, img_r, rows, cols, stride))) return rc;
  // the extractor's chain of image k on the list in brk_rec / brk_cnt + 4 k, against the resident image
  const auto extractor = [&](int k) -> int {
    const BinarySlot &t = bb.slots[pc.slots[k]];
    const ChainOut out{bb.d_cnt + k * BIN_COUNTER_INTS, bb.d_kresp, t.d_kp, t.d_desc, t.d_n, bb.h_n + 4 * k, nullptr, bb.h_desc + (size_t)k * cap * row_bytes};
    return brisk_pair_chain_enqueue(c, rows, cols, cap, s.brk_rec, s.brk_keep, s.brk_cnt + 4 * k, s.brk_cap, s.brk_crec, out, bb.h_bkp + (size_t)k * cap);
  };
  for (int attempt = 0;; ++attempt) {
    for (int k = 0; k < 2; ++k) {   // left chain, then the right one: the resident image, the pyramid and the lists are reused in stream order
      s.rows = s.cols = 0;
      if ((rc = classic_image_from_staged(c, pc.image(k), rows, cols)) || (rc = sift_enqueue_pyramid(c, c->cls.im, rows, cols, P))) return rc;
      s.plan = P; s.rows = rows; s.cols = cols; s.gauss_only = false;
      if ((rc = sift_enqueue_features(c, P, false)) || (rc = sift_enqueue_records(c, k)) || (rc = extractor(k))) return rc;
    }
    if ((rc = pc.submit())) return rc;
    int most = 0;
    for (int k = 0; k < 2; ++k) most = std::max(most, std::max(s.hb_n[4 * k + 1], s.hb_n[4 * k + 2]));
    if (most <= s.cand_cap) break;
    // more candidates (or raw rows) than the lists hold: grow them to what was counted and run the pair again (a second wait)
    if (attempt >= 2) {
      pc.count(0); pc.count(1);
      return fail(c, SPVO_ERR_CAPACITY, "%s: %d candidates / keypoints do not fit", who, most);
    }
    HIP_TRY(c, hipStreamSynchronize(st));   // (the prematches of the attempt read the slots on this stream)
    if ((rc = sift_ensure(c, rows, cols, pyr_floats, most + 1024)) || (rc = sift_order_ensure(c, s.cand_cap)) || (rc = sift_brisk_ensure(c, std::max(s.cand_cap, cap)))) return rc;
  }
  // the sizes the device used against sift_record's
  const bool force = tuning("sift_brisk_recheck", 0) == 1;
  bool redo[2] = {force, force};
  for (int k = 0; k < 2 && !force; ++k) {
    const SiftSrc *src = s.hb_src + (size_t)k * s.brk_cap;
    for (int i = 0, n = std::min(std::max(s.hb_n[4 * k], 0), s.brk_cap); i < n && !redo[k]; ++i)
      redo[k] = __builtin_bit_cast(int, sift_record(src[i].pos, src[i].off, __builtin_bit_cast(int, src[i].angle)).size) != src[i].pad[0];
  }
  if (redo[0] || redo[1]) {
    const int n_rows[2] = {std::min(std::max(s.hb_n[0], 0), s.brk_cap), std::min(std::max(s.hb_n[4], 0), s.brk_cap)};
    s.hb_rec.resize((size_t)n_rows[0] + n_rows[1] + 1);   // (each image's records in a part of their own: a copy may read them until the wait)
    for (int k = 0; k < 2; ++k) {   // (the right image is staged again behind a left pass: it is the resident one afterwards)
      if (!redo[k] && !(k == 1 && redo[0])) continue;
      if ((rc = classic_image_from_staged(c, pc.image(k), rows, cols))) return rc;
      if (!redo[k]) continue;
      const SiftSrc *src = s.hb_src + (size_t)k * s.brk_cap;
      BriskDetKeypoint *h_rec = s.hb_rec.data() + (k ? n_rows[0] : 0);
      const int n = n_rows[k];
      for (int i = 0; i < n; ++i) {
        const spvo_sift_keypoint r = sift_record(src[i].pos, src[i].off, __builtin_bit_cast(int, src[i].angle));
        h_rec[i] = BriskDetKeypoint{r.x, r.y, r.size, r.angle, r.response, r.octave};
      }
      if (n > 0) HIP_TRY(c, hipMemcpyAsync(s.brk_rec, h_rec, (size_t)n * sizeof(BriskDetKeypoint), hipMemcpyHostToDevice, st));
      if ((rc = extractor(k))) return rc;
    }
    if ((rc = pc.submit())) return rc;   // the second wait
  }
  pc.count(0); pc.count(1);
  if (bb.h_n[1] || bb.h_n[5]) return fail(c, SPVO_ERR_STATE, "%s: the lists overflowed although they were grown to what was counted", who);
  const PairMirror mirrors[2] = {{bb.h_bkp, sizeof(BriskDetKeypoint), bb.h_desc, (size_t)row_bytes},
                                 {bb.h_bkp + cap, sizeof(BriskDetKeypoint), bb.h_desc + (size_t)cap * row_bytes, (size_t)row_bytes}};
  return pc.commit(mirrors);
}

// Shi-Tomasi / FAST + SIFT of a stereo pair into two SIFT slots.  Per image: the detector's chain on the resident u8 image (spvo_classic.hip),
// the SIFT base level of that image -- every record lies on octave 0, layer 0 -- and sift_describe_given_kernel on the detector's list,
// whose sink is the slot and the pinned mirrors.  A slot's d_src and the mirror h_src hold the 24-byte RECORDS here (SiftKey), not sources.
// The grid is fixed: four waves per CU stride over the records, whose number only the device knows (32 KB of LDS per wave: five per CU fit
// on paper and measure 18 % slower than four, NOTES.md).
int spvo_classic_sift_pair(spvo_ctx *c, const spvo_classic_opts *opts, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, int slot_l, int slot_r,
                           spvo_sift_features *out_l, spvo_sift_features *out_r) {
  static_assert(sizeof(SiftKey) <= sizeof(SiftSrc) && sizeof(spvo_sift_keypoint) == sizeof(SiftKey), "a slot's source array holds the records");
  if (!c || !opts || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  const int kind = opts->kind, cap = opts->slot_capacity;
  if (kind != SPVO_CLASSIC_GFTT_SIFT && kind != SPVO_CLASSIC_FAST_SIFT)
    return fail(c, SPVO_ERR_INVALID, "spvo_classic_sift_pair: kind %d (SPVO_CLASSIC_GFTT_SIFT or SPVO_CLASSIC_FAST_SIFT; the other kinds are spvo_classic_detect's)", kind);
  PairCall<SiftPairFamily> pc(c, "spvo_classic_sift_pair", SiftPairFamily{}, pair_out(out_l), pair_out(out_r));
  int rc;
  if ((rc = pc.check(slot_l, slot_r)) || (rc = pc.check_capacity(cap)) || (rc = classic_detector_check(c, pc.who, opts, rows, cols)) || (rc = sift_check_image(c, pc.who, rows, cols)) ||
      (rc = pc.open()))
    return rc;
  c->akaze.valid = false;   // as spvo_sift_detect_pair: the AKAZE scale space's claim ends
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  const size_t px = (size_t)rows * cols;
  s.rows = s.cols = 0;   // the pyramid buffer holds one level of each image in turn: nothing spvo_sift_debug_level could serve
  if ((rc = classic_image_ensure(c, rows, cols)) || (rc = sift_pyr_ensure(c, px)) || (rc = sift_slots_ensure(c, cap, px)) || (rc = sift_prematch_ensure(c))) return rc;
  SiftPyr P{};
  P.n_oct = 1; P.h[0] = rows; P.w[0] = cols; P.pyr = s.pyr;
  if ((rc = pc.load(img_l, img_r, rows, cols, stride))) return rc;
  const int waves = std::min(std::max(tuning("sift_pair_waves_per_cu", 4), 1), 64) * c->num_cus;   // (diagnostic: the grid NOTES.md measures the default against)
  for (int k = 0; k < 2; ++k) {   // left chain, then the right one: the resident image, the detector's list and the base level are reused in stream order
    if ((rc = classic_detector_enqueue(c, opts, pc.image(k), rows, cols))) return rc;
    if ((rc = sift_enqueue_pyramid(c, c->cls.im, rows, cols, P, false, false, true))) return rc;
    const SiftSlot &t = s.slots[pc.slots[k]];
    const SiftDetectorIO io{c->cls.xy,
                            c->cls.resp,
                            c->cls.counters,
                            SiftKey{0.f, 0.f, kind == SPVO_CLASSIC_GFTT_SIFT ? 5.f : 7.f, -1.f, 0.f, 0},   // KeyPoint::convert(corners, keypoints, blockSize = 5) / KeyPoint(x, y, 7.f, -1, score)
                            cap,
                            t.d_desc,
                            t.d_sqn,
                            reinterpret_cast<SiftKey *>(t.d_src.get()),
                            t.d_n,
                            s.hm_desc + (size_t)k * s.slot_cap * 128,
                            reinterpret_cast<SiftKey *>(s.h_src + (size_t)k * s.slot_cap),
                            s.h_n + 4 * k};
    hipLaunchKernelGGL((sift_describe_given_kernel<0, SiftDetectorIO>), dim3(waves), dim3(64), 0, st, P, 0, io);
    HIP_TRY(c, hipGetLastError());
  }
  if ((rc = pc.submit())) return rc;
  // (kept: this entry point answers a detector overflow with SPVO_ERR_CAPACITY, image by image as the counts are taken)
  for (int k = 0; k < 2; ++k) {
    pc.count(k);
    if (s.h_n[4 * k + 1]) return fail(c, SPVO_ERR_CAPACITY, "spvo_classic_sift_pair: key buffer overflow in the %s image", k ? "right" : "left");
  }
  const PairMirror mirrors[2] = {sift_mirror(c, 0, true, sizeof(SiftKey)), sift_mirror(c, 1, true, sizeof(SiftKey))};
  return pc.commit(mirrors);
}

// tests/sift_describe_ref.py.  Everything a record can be refused for is checked on the host before anything is touched; the kernel then
// indexes levels that exist.
int spvo_sift_describe(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, const spvo_sift_keypoint *kp, int n, float *desc) {
  static_assert(sizeof(spvo_sift_keypoint) == sizeof(SiftKey), "keypoint records differ");
  if (!c || rows <= 0 || cols <= 0 || n < 0 || (n > 0 && (!kp || !desc)) || (img && stride < (size_t)cols)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (int rc = sift_check_image(c, "spvo_sift_describe", rows, cols)) return rc;
  int lo = 0, hi = 0;   // the octaves the list spans, 0 included
  for (int i = 0; i < n; ++i) {
    const spvo_sift_keypoint &k = kp[i];
    if (!std::isfinite(k.x) || !std::isfinite(k.y) || !std::isfinite(k.size) || !std::isfinite(k.angle) || !(k.size > 0))
      return fail(c, SPVO_ERR_INVALID, "spvo_sift_describe: keypoint %d has x %g, y %g, size %g, angle %g", i, (double)k.x, (double)k.y, (double)k.size, (double)k.angle);
    int o = k.octave & 255;
    if (o >= 128) o -= 256;
    const int layer = (k.octave >> 8) & 255;
    if (o < -1 || layer >= SIFT_GAUSS) return fail(c, SPVO_ERR_INVALID, "spvo_sift_describe: keypoint %d has octave %d, layer %d (octaves from -1, layers 0 .. %d)", i, o, layer, SIFT_GAUSS - 1);
    if (o > 0 && (o >= 31 || (std::min(rows, cols) >> o) < 1)) return fail(c, SPVO_ERR_INVALID, "spvo_sift_describe: keypoint %d: a %d x %d image has no octave %d", i, rows, cols, o);
    lo = std::min(lo, o); hi = std::max(hi, o);
  }
  const int first = lo, n_oct = hi - lo + 1;
  if (n_oct > SIFT_MAX_OCT) return fail(c, SPVO_ERR_INVALID, "spvo_sift_describe: %d octaves (at most %d)", n_oct, SIFT_MAX_OCT);
  if (int rc = require_idle(c)) return rc;
  auto &b = c->cls;
  if (!img && (b.rows != rows || b.cols != cols))
    return fail(c, SPVO_ERR_STATE, "spvo_sift_describe: no image of %d x %d is resident (call a detector first, or pass the image)", rows, cols);
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream2;
  if (img) {
    if (int rc = classic_upload_image(c, img, rows, cols, stride)) return rc;
  }
  if (n == 0) {
    HIP_TRY(c, hipStreamSynchronize(st));   // (the caller's image may be in flight)
    return SPVO_OK;
  }
  auto &s = c->sift;
  SiftPyr P{};
  P.n_oct = n_oct;
  size_t pyr_floats = 0;
  for (int o = 0, h = first < 0 ? 2 * rows : rows, w = first < 0 ? 2 * cols : cols; o < n_oct; ++o, h /= 2, w /= 2) {
    P.h[o] = h; P.w[o] = w;
    P.g_off[o] = (long long)pyr_floats; P.d_off[o] = 0;
    pyr_floats += (size_t)SIFT_GAUSS * h * w;
  }
  s.rows = s.cols = 0;   // nothing resident until the pyramid is enqueued
  if (int rc = sift_pyr_ensure(c, pyr_floats)) return rc;
  if (int rc = sift_given_ensure(c, n)) return rc;
  P.pyr = s.pyr;
  HIP_TRY(c, hipMemcpyAsync(s.given_kp, kp, (size_t)n * sizeof(SiftKey), hipMemcpyHostToDevice, st));
  if (int rc = sift_enqueue_pyramid(c, b.im, rows, cols, P, first < 0, false)) return rc;
  s.plan = P; s.rows = rows; s.cols = cols; s.gauss_only = true; s.first = first;
  // (diagnostic, tuning "sift_describe_form": 1 = the staged form NOTES.md measures against the columns)
  if (tuning("sift_describe_form", 0) == 1)
    hipLaunchKernelGGL((sift_describe_given_kernel<1, SiftGivenIO>), dim3(std::min(n, 65536)), dim3(64), 0, st, P, first, SiftGivenIO{s.given_kp, n, s.given_desc});
  else
    hipLaunchKernelGGL((sift_describe_given_kernel<0, SiftGivenIO>), dim3(std::min(n, 65536)), dim3(64), 0, st, P, first, SiftGivenIO{s.given_kp, n, s.given_desc});
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(desc, s.given_desc, (size_t)n * 128 * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));   // the one wait of the call
  return SPVO_OK;
}

// The link of spvo_brisk_sift_pair / spvo_akaze_sift_pair on a caller's list (test hook): sift_link_enqueue -- compaction by the keep flags,
// the levels that are read of octaves 0 .. max_octave, the describe launch on the fixed grid with the count read on the device -- against the
// image already resident.  Everything a record can be refused for is checked before anything is touched.
int spvo_sift_link_debug(spvo_ctx *c, int rows, int cols, const spvo_sift_keypoint *kp, const uint8_t *keep, int n, int max_octave, int32_t *kept, float *desc, int *n_kept) {
  static_assert(sizeof(spvo_sift_keypoint) == sizeof(SiftKey), "keypoint records differ");
  if (!c || !n_kept || rows <= 0 || cols <= 0 || n < 0 || (n > 0 && (!kp || !kept || !desc))) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (int rc = sift_check_image(c, "spvo_sift_link_debug", rows, cols)) return rc;
  if (int rc = sift_link_check_octave(c, "spvo_sift_link_debug", rows, cols, max_octave)) return rc;
  for (int i = 0; i < n; ++i) {
    const spvo_sift_keypoint &k = kp[i];
    if (!std::isfinite(k.x) || !std::isfinite(k.y) || !std::isfinite(k.size) || !std::isfinite(k.angle) || !(k.size > 0))
      return fail(c, SPVO_ERR_INVALID, "spvo_sift_link_debug: keypoint %d has x %g, y %g, size %g, angle %g", i, (double)k.x, (double)k.y, (double)k.size, (double)k.angle);
    int o = k.octave & 255;
    if (o >= 128) o -= 256;
    const int layer = (k.octave >> 8) & 255;
    if (o < 0 || o > max_octave || layer != 0)
      return fail(c, SPVO_ERR_INVALID, "spvo_sift_link_debug: keypoint %d has octave %d, layer %d (octaves 0 .. %d, layer 0: the link builds no other level)", i, o, layer, max_octave);
  }
  if (int rc = require_idle(c)) return rc;
  auto &b = c->cls;
  if (b.rows != rows || b.cols != cols) return fail(c, SPVO_ERR_STATE, "spvo_sift_link_debug: no image of %d x %d is resident (call a detector first)", rows, cols);
  *n_kept = 0;
  if (n == 0) return SPVO_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  SiftPyr P{};
  const size_t pyr_floats = sift_link_plan(rows, cols, max_octave, P);
  s.rows = s.cols = 0;   // the pyramid buffer will hold the levels the link reads: nothing spvo_sift_debug_level could serve
  int rc;
  if ((rc = sift_link_ensure(c, pyr_floats, n)) || (rc = sift_given_ensure(c, n))) return rc;
  if (keep && (size_t)n > s.lnk_keep.count())
    if ((rc = grow(c, wait_for(st), {plain(s.lnk_keep, (size_t)n)}))) return rc;
  P.pyr = s.pyr;
  std::vector<int> flags, h_kept((size_t)n);
  std::vector<float> h_desc((size_t)n * 128);
  HIP_TRY(c, hipStreamSynchronize(st));   // (the pageable copies below read the caller's and these buffers when they are enqueued)
  HIP_TRY(c, hipMemcpyAsync(s.given_kp, kp, (size_t)n * sizeof(SiftKey), hipMemcpyHostToDevice, st));
  if (keep) {
    flags.assign(keep, keep + n);
    HIP_TRY(c, hipMemcpyAsync(s.lnk_keep, flags.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(c, hipMemcpyAsync(s.lnk_cnt + 1, &n, sizeof(int), hipMemcpyHostToDevice, st));
  SiftLinkIO io{};
  io.s = SiftLinkSrc{reinterpret_cast<const char *>(s.given_kp.get()), (int)sizeof(SiftKey), (int)offsetof(SiftKey, x), (int)offsetof(SiftKey, y), (int)offsetof(SiftKey, size),
                     (int)offsetof(SiftKey, angle), (int)offsetof(SiftKey, response), (int)offsetof(SiftKey, octave), keep ? s.lnk_keep : nullptr, s.lnk_cnt + 1, n, nullptr, nullptr, 0};
  io.slot_cap = n;
  io.h_desc = s.given_desc;
  if ((rc = sift_link_enqueue(c, rows, cols, P, io, true))) return rc;
  // into staging first: a failure below leaves the caller's buffers as they were
  int m = 0;
  HIP_TRY(c, hipMemcpyAsync(&m, s.lnk_cnt, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h_kept.data(), s.lnk_kept, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h_desc.data(), s.given_desc, (size_t)n * 128 * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));   // the one wait of the call
  m = std::min(std::max(m, 0), n);
  std::memcpy(kept, h_kept.data(), (size_t)m * sizeof(int));
  std::memcpy(desc, h_desc.data(), (size_t)m * 128 * sizeof(float));
  *n_kept = m;
  return SPVO_OK;
}

// spvo_sift_brisk_pair's chain of ONE image up to sift_records_kernel (test hook): the image becomes the resident one, and the records the
// BRISK chain would read come back.  describe != 0 runs the describing instantiation of sift_describe_kernel in the other's place.
int spvo_sift_records_debug(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, int describe, spvo_sift_keypoint *rec, int cap, int *n_out) {
  static_assert(sizeof(spvo_sift_keypoint) == sizeof(BriskDetKeypoint), "record layout");
  if (!c || !img || !n_out || rows <= 0 || cols <= 0 || stride < (size_t)cols || cap < 0 || (cap > 0 && !rec)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (int rc = sift_check_image(c, "spvo_sift_records_debug", rows, cols)) return rc;
  if (int rc = require_idle(c)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  *n_out = 0;
  c->akaze.valid = false;
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  SiftPyr P{};
  const size_t pyr_floats = sift_plan(rows, cols, P);
  s.rows = s.cols = 0;
  const int cand_cap = std::max(s.cand_cap, std::max(8192, (int)((size_t)4 * rows * cols / 16)));
  int rc;
  if ((rc = sift_ensure(c, rows, cols, pyr_floats, cand_cap)) || (rc = sift_order_ensure(c, s.cand_cap)) || (rc = sift_brisk_ensure(c, s.cand_cap))) return rc;
  P.pyr = s.pyr;
  if ((rc = classic_upload_image(c, img, rows, cols, stride)) || (rc = sift_enqueue_pyramid(c, c->cls.im, rows, cols, P))) return rc;
  s.plan = P; s.rows = rows; s.cols = cols; s.gauss_only = false;
  if ((rc = sift_enqueue_features(c, P, describe != 0)) || (rc = sift_enqueue_records(c, 0))) return rc;
  HIP_TRY(c, hipStreamSynchronize(st));
  if (std::max(s.hb_n[1], s.hb_n[2]) > s.cand_cap) return fail(c, SPVO_ERR_CAPACITY, "spvo_sift_records_debug: %d candidates / %d keypoints do not fit", s.hb_n[1], s.hb_n[2]);
  const int n = std::min(std::max(s.hb_n[0], 0), s.brk_cap);
  if (std::min(n, cap) > 0) HIP_TRY(c, hipMemcpy(rec, s.brk_rec, (size_t)std::min(n, cap) * sizeof(BriskDetKeypoint), hipMemcpyDeviceToHost));
  *n_out = n;
  return SPVO_OK;
}

int spvo_sift_order_debug(spvo_ctx *c, const spvo_sift_keypoint *rec, int n, int32_t *order, int *n_kept) {
  static_assert(sizeof(spvo_sift_keypoint) == sizeof(SiftKey), "keypoint records differ");
  if (!c || !n_kept || n < 0 || n > (1 << 20) || (n > 0 && (!rec || !order))) return fail(c, SPVO_ERR_INVALID, "bad argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  *n_kept = 0;
  auto &s = c->sift;
  hipStream_t st = c->stream2;
  if (int rc = sift_order_ensure(c, std::max(n, 1))) return rc;
  HIP_TRY(c, hipStreamSynchronize(st));
  if (n) HIP_TRY(c, hipMemcpyAsync(s.keys, rec, (size_t)n * sizeof(SiftKey), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(s.ord_n + 1, &n, sizeof(int), hipMemcpyHostToDevice, st));
  if (int rc = sift_enqueue_sort(c, s.ord_n + 1, n)) return rc;
  int kept = 0;
  HIP_TRY(c, hipMemcpyAsync(&kept, s.ord_n, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (kept > 0) HIP_TRY(c, hipMemcpy(order, s.order, (size_t)kept * sizeof(int), hipMemcpyDeviceToHost));
  *n_kept = kept;
  return SPVO_OK;
}

int spvo_sift_debug_level(spvo_ctx *c, int octave, int layer, int dog, float *out, int *rows, int *cols) {
  if (!c) return fail(c, SPVO_ERR_INVALID, "null context");
  auto &s = c->sift;
  if (s.rows == 0) return fail(c, SPVO_ERR_STATE, "spvo_sift_debug_level: no pyramid is resident (call spvo_sift_detect first)");
  if (dog && s.gauss_only) return fail(c, SPVO_ERR_STATE, "spvo_sift_debug_level: the resident pyramid is spvo_sift_describe's, which builds no difference of Gaussians");
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
