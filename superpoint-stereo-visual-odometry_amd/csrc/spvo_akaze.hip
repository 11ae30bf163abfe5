// spvo_akaze.hip -- the classic front end's AKAZE keypoint detector (akaze.hip.h): the tables of a shape (levels, FED step sizes, Gaussian
// taps: built on the host by the formulas tests/akaze_ref.py lists, spvo_akaze_tables), the chain of launches of spvo_akaze_detect, the
// order-dependent suppression between candidates on the host (rule 11: the restatement's loop over the copied candidate list), the
// test hooks, spvo_akaze_describe (akaze_mldb.hip.h: orientation and MLDB descriptor on the scale space that chain leaves resident), and
// spvo_akaze_detect_pair (detector + descriptor of a stereo pair in one submission into two binary slots of 61-byte rows, by
// the resident-pair protocol of pair_call.hip.h, with rule 11 on the device: akaze_suppress.hip.h; spvo_akaze_orb_pair and
// spvo_akaze_brisk_pair: the same call with the octave-aware ORB extractor or the BRISK extractor behind rule 11).
// Runs on the solver's stream (stream2) with the image resident in spvo_ctx::cls -- it stays there for a spvo_brisk_describe(img = NULL)
// that follows -- and owns everything else it needs (spvo_ctx::akaze).
#include "spvo_internal.hip.h"
#include "pair_call.hip.h"
#include "akaze.hip.h"
#include "akaze_mldb.hip.h"
#include "akaze_suppress.hip.h"

namespace {
constexpr int AK_SUBLEVELS = 4;

struct AkTables {
  int n = 0, octaves = 0;
  int oh[AKAZE_MAX_OCTAVES] = {0}, ow[AKAZE_MAX_OCTAVES] = {0};
  int octave[AKAZE_MAX_LEVELS] = {0}, sigma_size[AKAZE_MAX_LEVELS] = {0}, nsteps[AKAZE_MAX_LEVELS] = {0};   // nsteps[i]: the transition i - 1 -> i
  float esigma[AKAZE_MAX_LEVELS] = {0};
  std::vector<float> tau;
  AkazeTaps g0{}, g1{};
};

bool is_prime(int n) {
  if (n < 2) return false;
  for (int d = 2; d * d <= n; ++d)
    if (n % d == 0) return false;
  return true;
}

// rule 1: fed_tau_by_process_time(t, 1, 0.25, reordering) in float, appended to `out`; -> the number of steps
int fed_tau(float t, std::vector<float> &out) {
#pragma clang fp contract(off)
  const float tau_max = 0.25f;
  const int n = (int)std::ceil(sqrtf(3.0f * t / tau_max + 0.25f) - 0.5f - 1.0e-8f);
  if (n <= 0) return 0;
  const float scale = 3.0f * t / (tau_max * (float)(n * (n + 1)));
  const float c = 1.0f / (4.0f * (float)n + 2.0f), d = scale * tau_max / 2.0f;
  std::vector<float> tauh((size_t)n);
  for (int k = 0; k < n; ++k) {
    const float h = cosf((float)M_PI * (2.0f * (float)k + 1.0f) * c);
    tauh[k] = d / (h * h);
  }
  const int kappa = n / 2;
  int prime = n + 1;
  while (!is_prime(prime)) ++prime;
  for (int k = 0, l = 0; l < n; ++k, ++l) {
    int index;
    while ((index = ((k + 1) * kappa) % prime - 1) >= n) ++k;
    out.push_back(tauh[index]);
  }
  return n;
}

// rule 2
AkazeTaps gaussian_taps(double sigma) {
  AkazeTaps t{};
  const int ksize = (int)std::ceil(2.0 * (1.0 + (sigma - 0.8) / 0.3)) | 1;
  t.r = std::min(ksize / 2, AKAZE_BLUR_R);
  double v[2 * AKAZE_BLUR_R + 1], sum = 0;
  for (int i = -t.r; i <= t.r; ++i) sum += v[i + t.r] = std::exp(-((double)i * i) / (2.0 * sigma * sigma));
  for (int j = 0; j <= t.r; ++j) t.g[j] = (float)(v[j + t.r] / sum);
  return t;
}

AkTables make_tables(int rows, int cols) {
#pragma clang fp contract(off)
  AkTables T;
  for (int o = 0; o < AKAZE_MAX_OCTAVES; ++o) {
    const int h = (int)(rows / (double)(1 << o)), w = (int)(cols / (double)(1 << o));
    if (o > 0 && (w < 80 || h < 40)) break;
    T.oh[o] = h; T.ow[o] = w; T.octaves = o + 1;
    for (int j = 0; j < AK_SUBLEVELS; ++j, ++T.n) {
      T.octave[T.n] = o;
      T.esigma[T.n] = 1.6f * powf(2.f, (float)j / (float)AK_SUBLEVELS + (float)o);
      T.sigma_size[T.n] = (int)std::nearbyint(T.esigma[T.n] * 1.5f / (float)(1 << o));
    }
  }
  for (int i = 1; i < T.n; ++i) {
    const float e1 = 0.5f * T.esigma[i] * T.esigma[i], e0 = 0.5f * T.esigma[i - 1] * T.esigma[i - 1];
    T.nsteps[i] = fed_tau(e1 - e0, T.tau);
  }
  T.g0 = gaussian_taps(1.6);
  T.g1 = gaussian_taps(1.0);
  return T;
}

int level_border(int sigma_size) {
#pragma clang fp contract(off)
  return (int)std::nearbyint(10.0f * sqrtf(2.0f) * (float)sigma_size) + 1;
}

size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }
dim3 grid_of(int w, int h) { return dim3((w + 63) / 64, (h + 3) / 4, 1); }

// layout, tables and buffers for a rows x cols image
int ak_ensure(spvo_ctx *c, int rows, int cols) {
  auto &d = c->akaze;
  hipStream_t st = c->stream2;
  d.valid = false;
  if (!d.stat)
    if (int rc = grow(c, wait_for_nothing(), {zeroed(d.stat, AKAZE_STAT_INTS)})) return rc;
  if (d.rows == rows && d.cols == cols) return SPVO_OK;
  d.rows = d.cols = 0;
  const AkTables T = make_tables(rows, cols);
  size_t planes = 0, tabs = 0, off[AKAZE_MAX_LEVELS], tab_off[AKAZE_MAX_OCTAVES] = {0};
  long long cand = 0;
  for (int i = 0; i < T.n; ++i) {
    const int h = T.oh[T.octave[i]], w = T.ow[T.octave[i]], b = level_border(T.sigma_size[i]);
    off[i] = planes;
    planes += 6 * align64((size_t)h * w);
    cand += (long long)((std::max(h - 2 * b, 0) + 1) / 2) * ((std::max(w - 2 * b, 0) + 1) / 2);   // strict maxima do not touch, diagonally either
  }
  bool exact[AKAZE_MAX_OCTAVES] = {false};
  for (int o = 1; o < T.octaves; ++o) {
    exact[o] = T.oh[o - 1] == 2 * T.oh[o] && T.ow[o - 1] == 2 * T.ow[o];
    if (!exact[o]) { tab_off[o] = tabs; tabs += (size_t)T.ow[o] + T.oh[o]; }
  }
  d.h_tabs.assign(std::max<size_t>(tabs, 1), BriskAreaTap{});
  for (int o = 1; o < T.octaves; ++o)
    if (!exact[o] && !(brisk_area_tab(T.ow[o - 1], T.ow[o], d.h_tabs.data() + tab_off[o]) && brisk_area_tab(T.oh[o - 1], T.oh[o], d.h_tabs.data() + tab_off[o] + T.ow[o])))
      return fail(c, SPVO_ERR_STATE, "AKAZE detector: the area taps of octave %d (%d x %d from %d x %d) failed their own checks", o, T.oh[o], T.ow[o], T.oh[o - 1], T.ow[o - 1]);
  const size_t scratch = 2 * align64((size_t)rows * cols);
  if (planes > d.plane_cap || scratch > d.scratch_cap || tabs > d.tab_cap || cand > d.cand_cap) {
    const size_t np = std::max(planes, d.plane_cap), ns = std::max(scratch, d.scratch_cap), nt = std::max(std::max<size_t>(tabs, 1), d.tab_cap);
    const int nc = (int)std::min<long long>(std::max<long long>(std::max<long long>(cand, 1), d.cand_cap), 0x7FFFFFFF);
    d.plane_cap = d.scratch_cap = d.tab_cap = 0; d.cand_cap = 0;   // a failed allocation below leaves a context that spvo_destroy and a later call can still handle
    if (int rc = grow(c, wait_for(st), {plain(d.planes, np), plain(d.scratch, ns), plain(d.tabs, nt), plain(d.keys, nc), zeroed(d.rank, nc), plain(d.rec, nc)})) return rc;
    d.plane_cap = np; d.scratch_cap = ns; d.tab_cap = nt; d.cand_cap = nc;
  }
  HIP_TRY(c, hipMemcpyAsync(d.tabs, d.h_tabs.data(), d.h_tabs.size() * sizeof(BriskAreaTap), hipMemcpyHostToDevice, st));
  d.lv = AkazeLevels{};
  d.lv.n = T.n;
  for (int i = 0; i < T.n; ++i) {
    AkazeLevel &L = d.lv.l[i];
    L.h = T.oh[T.octave[i]]; L.w = T.ow[T.octave[i]];
    const size_t px = align64((size_t)L.h * L.w);
    L.Lt = d.planes + off[i]; L.Lsmooth = L.Lt + px; L.Lflow = L.Lsmooth + px; L.Ldet = L.Lflow + px; L.Lx = L.Ldet + px; L.Ly = L.Lx + px;
    L.octave = T.octave[i]; L.sigma_size = T.sigma_size[i]; L.border = level_border(T.sigma_size[i]); L.esigma = T.esigma[i];
    d.nsteps[i] = T.nsteps[i];
  }
  HIP_TRY(c, hipMemsetAsync(d.lv.l[0].Lflow, 0, (size_t)rows * cols * sizeof(float), st));   // level 0 has no flow: the plane reads as zeros
  for (int o = 0; o < AKAZE_MAX_OCTAVES; ++o) {
    d.xtab[o] = o >= 1 && o < T.octaves && !exact[o] ? d.tabs + tab_off[o] : nullptr;
    d.ytab[o] = d.xtab[o] ? d.xtab[o] + T.ow[o] : nullptr;
  }
  d.octaves = T.octaves;
  d.h_tau = T.tau;
  d.g0 = T.g0; d.g1 = T.g1;
  d.rows = rows; d.cols = cols;
  return SPVO_OK;
}

// rule 11 over the candidates `cd` (level by level, raster order) -> the indices of the survivors, in the list's order
void ak_suppress(const AkazeLevels &lv, const std::vector<AkazeCand> &cd, std::vector<int> &keep) {
#pragma clang fp contract(off)
  struct Aux { float x, y, size, response; int level, index; };
  std::vector<Aux> aux;
  aux.reserve(cd.size());
  for (size_t i = 0; i < cd.size(); ++i) {
    const AkazeCand &p = cd[i];
    const float ratio = (float)(1 << p.octave), half = 0.5f * (ratio - 1.f), size = lv.l[p.class_id].esigma * 1.5f, size2 = size * size;
    const float px = (float)p.col * ratio, py = (float)p.row * ratio;
    size_t slot = aux.size();
    bool drop = false;
    for (size_t k = 0; k < aux.size(); ++k) {
      if (aux[k].level != p.class_id && aux[k].level != p.class_id - 1) continue;
      const float dx = px - aux[k].x, dy = py - aux[k].y;
      const float dxx = dx * dx, dyy = dy * dy;
      if (dxx + dyy <= size2) {
        if (p.response > aux[k].response) slot = k; else drop = true;
        break;
      }
    }
    if (drop) continue;
    const Aux a{px + half, py + half, size, p.response, p.class_id, (int)i};
    if (slot == aux.size()) aux.push_back(a); else aux[slot] = a;
  }
  keep.clear();
  for (size_t i = 0; i < aux.size(); ++i) {
    bool repeated = false;
    const float size2 = aux[i].size * aux[i].size;
    for (size_t j = i + 1; j < aux.size() && !repeated; ++j) {
      if (aux[j].level != aux[i].level + 1) continue;
      const float dx = aux[i].x - aux[j].x, dy = aux[i].y - aux[j].y;
      const float dxx = dx * dx, dyy = dy * dy;
      repeated = dxx + dyy <= size2 && aux[i].response < aux[j].response;
    }
    if (!repeated) keep.push_back(aux[i].index);
  }
}
// The chain both entry points share: the image into spvo_ctx::cls, the layout of its shape, and every launch up to rule 9 (all six planes
// of every level), enqueued on the solver's stream.  The caller waits, and marks the result resident with ak_mark_resident.
int ak_scale_enqueue(spvo_ctx *c, int rows, int cols);
int ak_scale_space(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride) {
  if (int rc = classic_upload_image(c, img, rows, cols, stride)) return rc;
  if (int rc = ak_ensure(c, rows, cols)) return rc;
  return ak_scale_enqueue(c, rows, cols);
}
// the launches of that chain on the image resident in spvo_ctx::cls (ak_ensure has run for its shape)
int ak_scale_enqueue(spvo_ctx *c, int rows, int cols) {
  hipStream_t st = c->stream2;
  auto &d = c->akaze;
  const AkazeLevels &lv = d.lv;
  const size_t px0 = align64((size_t)rows * cols);
  float *blur1 = d.scratch, *ping = d.scratch + px0;
  const dim3 blk(256);
  auto blur_grid = [](int w, int h) { return dim3((w + AKAZE_TW - 1) / AKAZE_TW, (h + AKAZE_TH - 1) / AKAZE_TH, 1); };
  HIP_TRY(c, hipMemsetAsync(d.stat, 0, AKAZE_STAT_INTS * sizeof(int), st));
  // level 0 (rules 3, 4) and the contrast factor (rule 5; its sigma 1 blur goes to the first scratch plane)
  hipLaunchKernelGGL(akaze_blur_kernel<uint8_t>, blur_grid(cols, rows), blk, 0, st, c->cls.im, lv.l[0].Lt, lv.l[0].Lsmooth, rows, cols, d.g0);
  hipLaunchKernelGGL(akaze_blur_kernel<uint8_t>, blur_grid(cols, rows), blk, 0, st, c->cls.im, blur1, (float *)nullptr, rows, cols, d.g1);
  hipLaunchKernelGGL(akaze_gradmax_kernel, grid_of(cols, rows), blk, 0, st, blur1, rows, cols, d.stat);
  hipLaunchKernelGGL(akaze_hist_kernel, grid_of(cols, rows), blk, 0, st, blur1, rows, cols, d.stat);
  hipLaunchKernelGGL(akaze_contrast_finish_kernel, dim3(1), dim3(64), 0, st, rows, cols, d.octaves, d.stat);
  // rules 6 - 8: every further level
  size_t t0 = 0;
  for (int i = 1; i < lv.n; ++i) {
    const AkazeLevel &L = lv.l[i], &P = lv.l[i - 1];
    const int n = d.nsteps[i];
    const float *start = P.Lt;
    if (L.octave > P.octave) {
      float *half = (n % 2 == 0) ? L.Lt : ping;   // so that the last step's output is L.Lt
      if (d.xtab[L.octave]) hipLaunchKernelGGL(akaze_area_kernel, grid_of(L.w, L.h), blk, 0, st, P.Lt, half, P.w, L.h, L.w, d.xtab[L.octave], d.ytab[L.octave]);
      else hipLaunchKernelGGL(akaze_half_kernel, grid_of(L.w, L.h), blk, 0, st, P.Lt, half, P.w, L.h, L.w);
      start = half;
    }
    hipLaunchKernelGGL(akaze_blur_kernel<float>, blur_grid(L.w, L.h), blk, 0, st, start, L.Lsmooth, (float *)nullptr, L.h, L.w, d.g1);
    hipLaunchKernelGGL(akaze_flow_kernel, grid_of(L.w, L.h), blk, 0, st, L.Lsmooth, L.Lflow, L.h, L.w, d.stat + AKAZE_STAT_K + L.octave);
    if (n == 0 && start != L.Lt) HIP_TRY(c, hipMemcpyAsync(L.Lt, start, (size_t)L.h * L.w * sizeof(float), hipMemcpyDeviceToDevice, st));
    const float *in = start;
    for (int s = 1; s <= n; ++s) {
      float *out = ((n - s) % 2 == 0) ? L.Lt : ping;   // alternates, ends in L.Lt, and never equals `in`
      hipLaunchKernelGGL(akaze_fed_kernel, grid_of(L.w, L.h), blk, 0, st, in, L.Lflow, out, L.h, L.w, 0.5f * d.h_tau[t0 + s - 1]);
      in = out;
    }
    t0 += n;
  }
  // rule 9: the first derivatives stay, per level, for spvo_akaze_describe
  for (int i = 0; i < lv.n; ++i) {
    const AkazeLevel &L = lv.l[i];
    const int s = L.sigma_size;
    float norm, wn;
    {
#pragma clang fp contract(off)
      const float w = 10.0f / 3.0f;
      norm = 1.0f / ((2.0f * (float)s) * (w + 2.0f));
      wn = w * norm;
    }
    hipLaunchKernelGGL(akaze_deriv_kernel, grid_of(L.w, L.h), blk, 0, st, L.Lsmooth, L.Lx, L.Ly, L.h, L.w, s, norm, wn);
    hipLaunchKernelGGL(akaze_det_kernel, grid_of(L.w, L.h), blk, 0, st, L.Lx, L.Ly, L.Ldet, L.h, L.w, s, norm, wn, (float)(s * s * s * s));
  }
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// after the wait: the planes belong to the image now resident; stat: the first AKAZE_STAT_HIST integers as the kernels left them
void ak_mark_resident(spvo_ctx *c, const int *stat) {
  auto &d = c->akaze;
  d.valid = true;
  d.image_gen = c->cls.image_gen;
  for (int o = 0; o < AKAZE_MAX_OCTAVES; ++o) std::memcpy(&d.k[o], &stat[AKAZE_STAT_K + o], sizeof(float));
}

bool ak_resident(const spvo_ctx *c) {
  const auto &d = c->akaze;
  return d.valid && d.image_gen == c->cls.image_gen && c->cls.rows == d.rows && c->cls.cols == d.cols;
}

// what spvo_akaze_detect refuses of its parameters and of the image shape (`who` names the entry point in the error text)
int ak_check(spvo_ctx *c, const char *who, int rows, int cols, float threshold) {
  if (!std::isfinite(threshold) || !(threshold > 0.f)) return fail(c, SPVO_ERR_INVALID, "%s: the threshold must be finite and positive", who);
  if (rows < 16 || cols < 16) return fail(c, SPVO_ERR_INVALID, "%s: images of at least 16 x 16 only", who);
  return brisk_check_image(c, who, rows, cols);
}

// the descriptor's record, angle and row buffers for n keypoints
int ak_kp_ensure(spvo_ctx *c, int n) {
  auto &d = c->akaze;
  if (n <= d.kp_cap) return SPVO_OK;
  d.kp_cap = 0;
  const int cap = std::max(n, 1024);
  if (int rc = grow(c, wait_for(c->stream2), {plain(d.d_kp, (size_t)cap), plain(d.d_angle, (size_t)cap), plain(d.d_desc, (size_t)cap * AKAZE_MLDB_BYTES)})) return rc;
  d.kp_cap = cap;
  return SPVO_OK;
}

// the buffers of the device suppression for lists of n candidates
int ak_sup_ensure(spvo_ctx *c, int n) {
  auto &d = c->akaze;
  if (!d.sup_cnt)
    if (int rc = grow(c, wait_for_nothing(), {zeroed(d.sup_cnt, AKAZE_SUP_INTS)})) return rc;
  if (n <= d.sup_cap) return SPVO_OK;
  d.sup_cap = 0;
  const size_t cap = (size_t)std::max(n, 1024);
  if (int rc = grow(c, wait_for(c->stream2), {plain(d.sup_list, cap), plain(d.sup_idx, cap), plain(d.sup_keep, cap), plain(d.sup_src, cap), plain(d.sup_kp, cap)})) return rc;
  d.sup_cap = (int)cap;
  return SPVO_OK;
}

// spvo_akaze_brisk_pair: the BRISK extractor's tables and buffers for `cap` rows of a rows x cols image, and the lists that present the
// suppression's survivors to it (ak_sup_ensure has run: as many records as the suppression can keep, and no fewer than `cap`)
int ak_brisk_ensure(spvo_ctx *c, int rows, int cols, int cap) {
  auto &d = c->akaze;
  if (int rc = brisk_chain_ensure(c, rows, cols, cap)) return rc;
  const int n = std::max(d.sup_cap, cap);
  if (!d.brk_cnt)
    if (int rc = grow(c, wait_for_nothing(), {zeroed(d.brk_cnt, 4)})) return rc;
  if (n <= d.brk_cap) return SPVO_OK;
  d.brk_cap = 0;
  if (int rc = grow(c, wait_for(c->stream2), {plain(d.brk_rec, (size_t)n), plain(d.brk_crec, (size_t)n), plain(d.brk_keep, (size_t)n)})) return rc;
  d.brk_cap = n;
  return SPVO_OK;
}

// rule 11 and rule 13's flag on the device: the candidates rec[0 .. min(*n_ptr, cap)) -> sup_kp / sup_src, their number in
// sup_cnt[AKAZE_SUP_KEPT] (ak_sup_ensure(cap) has run; only esigma of lv's levels is read)
void ak_suppress_enqueue(spvo_ctx *c, const AkazeLevels &lv, const AkazeCand *rec, const int *n_ptr, int cap) {
  auto &d = c->akaze;
  hipStream_t st = c->stream2;
  hipLaunchKernelGGL(akaze_suppress_first_kernel, dim3(1), dim3(64), 0, st, lv, rec, n_ptr, cap, d.sup_list, d.sup_idx, d.sup_cnt);
  hipLaunchKernelGGL(akaze_suppress_second_kernel, dim3(std::min((cap + 255) / 256, 256)), dim3(256), 0, st, lv, rec, d.sup_list, d.sup_idx, d.sup_cnt, cap, d.sup_keep);
  hipLaunchKernelGGL(akaze_suppress_compact_kernel, dim3(1), dim3(1024), 0, st, rec, d.sup_idx, d.sup_keep, cap, d.sup_cnt, d.sup_kp, d.sup_src);
}

// rules 10, 12, 13 behind the scale space (spvo_akaze_detect and every pair call): extrema -- one launch per octave; an octave with no room
// inside its smallest border has none --, rank, refinement -> the candidates in rec, their number in stat[AKAZE_STAT_NCAND]
void ak_extrema_enqueue(spvo_ctx *c, float threshold) {
  auto &d = c->akaze;
  hipStream_t st = c->stream2;
  const AkazeLevels &lv = d.lv;
  for (int first = 0; first < lv.n; first += AK_SUBLEVELS) {
    const AkazeLevel &L = lv.l[first];
    if (L.h <= 2 * L.border || L.w <= 2 * L.border) continue;
    dim3 eg = grid_of(L.w, L.h);
    eg.z = std::min(AK_SUBLEVELS, lv.n - first);
    hipLaunchKernelGGL(akaze_extrema_kernel, eg, dim3(256), 0, st, lv, first, threshold, 1e-5f, d.keys, d.cand_cap, d.stat);
  }
  classic_rank_enqueue(c, d.keys, d.rank, d.stat + AKAZE_STAT_NCAND, d.cand_cap);
  hipLaunchKernelGGL(akaze_refine_kernel, dim3(32), dim3(256), 0, st, lv, d.keys, d.rank, d.cand_cap, d.stat, d.rec);
}

// A pair call's detector chain (the binary pairs and spvo_akaze_sift_pair): a staged image becomes the resident one, its scale space, the
// launches above and rule 11 on the device, which leaves sup_kp and the AKAZE_SUP_KEPT count for the extractor behind it
int ak_staged_enqueue(spvo_ctx *c, const uint8_t *h_img, int rows, int cols, float threshold) {
  auto &d = c->akaze;
  if (int rc = classic_image_from_staged(c, h_img, rows, cols)) return rc;
  if (int rc = ak_scale_enqueue(c, rows, cols)) return rc;
  ak_extrema_enqueue(c, threshold);
  ak_suppress_enqueue(c, d.lv, d.rec, d.stat + AKAZE_STAT_NCAND, d.cand_cap);
  return SPVO_OK;
}

// behind a pair call's wait: the right image's scale space is resident.  h_n: the family's pinned count block, where the finishing launch of
// image k left its contrast factors at h_n + 8 + 4 k (ak_mark_resident reads them where stat keeps them)
void ak_mark_right_resident(spvo_ctx *c, const int *h_n) {
  int stat[AKAZE_STAT_HIST] = {0};
  std::memcpy(&stat[AKAZE_STAT_K], h_n + 8 + 4, AKAZE_MAX_OCTAVES * sizeof(int));
  ak_mark_resident(c, stat);
}
}  // namespace

extern "C" {

int spvo_akaze_detect(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, float threshold, spvo_akaze_keypoint *kp, int cap, int *n_out) {
  if (!c || !img || !n_out || rows <= 0 || cols <= 0 || stride < (size_t)cols || cap < 0 || (cap > 0 && !kp)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  *n_out = 0;
  if (!std::isfinite(threshold) || !(threshold > 0.f)) return fail(c, SPVO_ERR_INVALID, "spvo_akaze_detect: the threshold must be finite and positive");
  if (rows < 16 || cols < 16) return fail(c, SPVO_ERR_INVALID, "spvo_akaze_detect: images of at least 16 x 16 only");
  if (int rc = brisk_check_image(c, "spvo_akaze_detect", rows, cols)) return rc;
  if (int rc = require_idle(c)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream2;
  if (int rc = ak_scale_space(c, img, rows, cols, stride)) return rc;
  auto &d = c->akaze;
  const AkazeLevels &lv = d.lv;
  ak_extrema_enqueue(c, threshold);
  HIP_TRY(c, hipGetLastError());
  int stat[AKAZE_STAT_HIST];
  HIP_TRY(c, hipMemcpyAsync(stat, d.stat, sizeof stat, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  // (the list holds every strict maximum the borders leave room for, so the overflow flag cannot be set; were it, the count would be wrong)
  if (stat[AKAZE_STAT_OVERFLOW] || stat[AKAZE_STAT_NCAND] > d.cand_cap) return fail(c, SPVO_ERR_STATE, "spvo_akaze_detect: the candidate list overflowed although it is sized from the image");
  ak_mark_resident(c, stat);
  d.h_cand.resize((size_t)stat[AKAZE_STAT_NCAND]);
  if (!d.h_cand.empty()) {
    HIP_TRY(c, hipMemcpyAsync(d.h_cand.data(), d.rec, d.h_cand.size() * sizeof(AkazeCand), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  std::vector<int> keep;
  ak_suppress(lv, d.h_cand, keep);
  int n = 0;
  static_assert(sizeof(spvo_akaze_keypoint) == 28 && sizeof(AkazeCand) == 40, "record layout");
  for (int i : keep) {
    if (!d.h_cand[i].ok) continue;
    if (n < cap) std::memcpy(&kp[n], &d.h_cand[i], sizeof(spvo_akaze_keypoint));   // (the candidate's first seven fields are the record)
    ++n;
  }
  *n_out = n;
  return SPVO_OK;
}

int spvo_akaze_debug_level(spvo_ctx *c, int level, int what, float *out, int *rows, int *cols) {
  if (!c || !rows || !cols || level < 0 || what < 0 || what > 3) return fail(c, SPVO_ERR_INVALID, "bad argument");
  auto &d = c->akaze;
  if (!ak_resident(c)) return fail(c, SPVO_ERR_STATE, "spvo_akaze_debug_level: no spvo_akaze_detect result is resident");
  if (level >= d.lv.n) return fail(c, SPVO_ERR_INVALID, "spvo_akaze_debug_level: the scale space of this image has %d levels", d.lv.n);
  if (int rc = require_idle(c)) return rc;
  const AkazeLevel &L = d.lv.l[level];
  *rows = L.h; *cols = L.w;
  if (!out) return SPVO_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const float *src = what == 0 ? L.Lt : what == 1 ? L.Lsmooth : what == 2 ? L.Lflow : L.Ldet;
  HIP_TRY(c, hipMemcpyAsync(out, src, (size_t)L.h * L.w * sizeof(float), hipMemcpyDeviceToHost, c->stream2));
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  return SPVO_OK;
}

int spvo_akaze_last_contrast(spvo_ctx *c, float *k, int *octaves) {
  if (!c || !k || !octaves) return fail(c, SPVO_ERR_INVALID, "bad argument");
  auto &d = c->akaze;
  if (!ak_resident(c)) return fail(c, SPVO_ERR_STATE, "spvo_akaze_last_contrast: no spvo_akaze_detect result is resident");
  *octaves = d.octaves;
  for (int o = 0; o < AKAZE_MAX_OCTAVES; ++o) k[o] = o < d.octaves ? d.k[o] : 0.f;
  return SPVO_OK;
}

int spvo_akaze_describe(spvo_ctx *c, const uint8_t *img, int rows, int cols, size_t stride, const spvo_akaze_keypoint *kp, int n, float *angle, uint8_t *desc) {
  if (!c || rows <= 0 || cols <= 0 || n < 0 || (n > 0 && (!kp || !angle || !desc)) || (img && stride < (size_t)cols)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (rows < 16 || cols < 16) return fail(c, SPVO_ERR_INVALID, "spvo_akaze_describe: images of at least 16 x 16 only");
  if (int rc = brisk_check_image(c, "spvo_akaze_describe", rows, cols)) return rc;
  if (int rc = require_idle(c)) return rc;
  auto &d = c->akaze;
  if (!img && !(ak_resident(c) && d.rows == rows && d.cols == cols))
    return fail(c, SPVO_ERR_STATE, "spvo_akaze_describe: no spvo_akaze_detect result of a %d x %d image is resident (call spvo_akaze_detect first, or pass the image)", rows, cols);
  {
    // every record against the levels of this shape, before anything is uploaded or written
    int levels, octave[AKAZE_MAX_LEVELS];
    if (d.rows == rows && d.cols == cols) {
      levels = d.lv.n;
      for (int i = 0; i < levels; ++i) octave[i] = d.lv.l[i].octave;
    } else {
      const AkTables T = make_tables(rows, cols);
      levels = T.n;
      std::memcpy(octave, T.octave, sizeof octave);
    }
    for (int i = 0; i < n; ++i) {
      const spvo_akaze_keypoint &p = kp[i];
      if (p.class_id < 0 || p.class_id >= levels) return fail(c, SPVO_ERR_INVALID, "spvo_akaze_describe: keypoint %d has class_id %d; the scale space of this image has %d levels", i, p.class_id, levels);
      if (p.octave != octave[p.class_id]) return fail(c, SPVO_ERR_INVALID, "spvo_akaze_describe: keypoint %d has octave %d; level %d lies on octave %d", i, p.octave, p.class_id, octave[p.class_id]);
      if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.size) || !(p.size > 0.f))
        return fail(c, SPVO_ERR_INVALID, "spvo_akaze_describe: keypoint %d is (%g, %g) of size %g", i, (double)p.x, (double)p.y, (double)p.size);
    }
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream2;
  if (img) {
    if (int rc = ak_scale_space(c, img, rows, cols, stride)) return rc;
    int stat[AKAZE_STAT_HIST];
    HIP_TRY(c, hipMemcpyAsync(stat, d.stat, sizeof stat, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    ak_mark_resident(c, stat);
  }
  if (n == 0) return SPVO_OK;
  if (int rc = ak_kp_ensure(c, n)) return rc;
  static_assert(sizeof(spvo_akaze_keypoint) == sizeof(AkazeKp) && SPVO_AKAZE_DESC_BYTES == AKAZE_MLDB_BYTES, "record layout");
  HIP_TRY(c, hipMemcpyAsync(d.d_kp, kp, (size_t)n * sizeof(AkazeKp), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(akaze_describe_kernel, dim3(std::min(n, 4096)), dim3(64), 0, st, d.lv, d.d_kp, n, (const int *)nullptr, d.d_angle, d.d_desc);
  HIP_TRY(c, hipGetLastError());
  // into staging first: a failure below leaves the caller's buffers as they were
  d.h_angle.resize((size_t)n);
  d.h_desc.resize((size_t)n * AKAZE_MLDB_BYTES);
  HIP_TRY(c, hipMemcpyAsync(d.h_angle.data(), d.d_angle, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(d.h_desc.data(), d.d_desc, (size_t)n * AKAZE_MLDB_BYTES, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  std::memcpy(angle, d.h_angle.data(), (size_t)n * sizeof(float));
  std::memcpy(desc, d.h_desc.data(), (size_t)n * AKAZE_MLDB_BYTES);
  return SPVO_OK;
}

// Rule 11 on the device for a caller's candidate list (test hook): exactly the kernels spvo_akaze_detect_pair runs behind
// akaze_refine_kernel, on records built from (level, row, col, response, ok) and the level tables of a rows x cols image.  Nothing of a
// resident scale space is touched.
int spvo_akaze_suppress_debug(spvo_ctx *c, int rows, int cols, const spvo_akaze_candidate *cand, int n, int32_t *keep, int *n_keep) {
  if (!c || !n_keep || n < 0 || (n > 0 && (!cand || !keep))) return fail(c, SPVO_ERR_INVALID, "bad argument");
  *n_keep = 0;
  if (rows < 16 || cols < 16) return fail(c, SPVO_ERR_INVALID, "spvo_akaze_suppress_debug: images of at least 16 x 16 only");
  const AkTables T = make_tables(rows, cols);
  std::vector<AkazeCand> h((size_t)n);
  for (int i = 0; i < n; ++i) {
    const spvo_akaze_candidate &p = cand[i];
    if (p.level < 0 || p.level >= T.n) return fail(c, SPVO_ERR_INVALID, "spvo_akaze_suppress_debug: candidate %d has level %d; the scale space of this shape has %d levels", i, p.level, T.n);
    if (i > 0 && p.level < cand[i - 1].level) return fail(c, SPVO_ERR_INVALID, "spvo_akaze_suppress_debug: candidate %d has level %d behind level %d (the list goes level by level)", i, p.level, cand[i - 1].level);
    h[i] = AkazeCand{0.f, 0.f, 0.f, 0.f, p.response, T.octave[p.level], p.level, p.row, p.col, p.ok ? 1 : 0};
  }
  if (int rc = require_idle(c)) return rc;
  if (n == 0) return SPVO_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream2;
  auto &d = c->akaze;
  if (int rc = ak_sup_ensure(c, n)) return rc;
  AkazeLevels lv{};
  lv.n = T.n;
  for (int i = 0; i < T.n; ++i) { lv.l[i].octave = T.octave[i]; lv.l[i].esigma = T.esigma[i]; }
  DevBuf<AkazeCand> rec;   // (the hook's own list: freed when the call returns, behind its wait)
  if (int rc = grow(c, wait_for_nothing(), {plain(rec, (size_t)n)})) return rc;
  int cnt[AKAZE_SUP_INTS] = {0, 0, n, 0};
  std::vector<int> src((size_t)n);
  hipError_t e = hipMemcpyAsync(rec, h.data(), (size_t)n * sizeof(AkazeCand), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d.sup_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    ak_suppress_enqueue(c, lv, rec, d.sup_cnt + 2, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(cnt, d.sup_cnt, sizeof cnt, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(src.data(), d.sup_src, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);
  HIP_TRY(c, e);
  HIP_TRY(c, e2);
  const int m = std::min(std::max(cnt[AKAZE_SUP_KEPT], 0), n);
  std::memcpy(keep, src.data(), (size_t)m * sizeof(int));
  *n_keep = m;
  return SPVO_OK;
}

// One submission per stereo pair: the resident-pair protocol (PairCall on the binary slots, pair_call.hip.h) around the detector's chain
// through rule 11 on the device (ak_staged_enqueue), the descriptor on the compacted records and a finishing kernel, image by image
// in stream order.  The scale space, the candidate lists, the suppression's lists and the descriptor's buffers are the left image's first
// and the right image's afterwards: an image's finishing kernel has put its counts into the pinned h_n before the next image's clear.
// The extractor behind rule 11 is the call's: MLDB (spvo_akaze_detect_pair, 61-byte rows), the octave-aware ORB extractor on the kept
// records (spvo_akaze_orb_pair: orb_link.hip.h through spvo_classic.hip, 32-byte rows), or the BRISK extractor (spvo_akaze_brisk_pair:
// the kept records presented to brisk_pair_chain_enqueue as a detector's list, 64-byte rows).  spvo_akaze_sift_pair, below, runs the
// same detector launches as the first link of spvo_sift.hip's sift_link_pair, into the SIFT slots.
}  // extern "C"
namespace {
enum class AkExtract { Mldb, Orb, Brisk };
int akaze_pair(spvo_ctx *c, const char *who, AkExtract ex, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, float threshold, int slot_l, int slot_r,
               int slot_capacity, spvo_akaze_features *out_l, spvo_akaze_features *out_r) {
  if (!c || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  const int cap = slot_capacity, row_bytes = ex == AkExtract::Mldb ? AKAZE_MLDB_BYTES : ex == AkExtract::Orb ? 32 : 64;
  PairCall<BinPairFamily> pc(c, who, BinPairFamily{row_bytes}, pair_out(out_l), pair_out(out_r));
  int rc;
  if ((rc = pc.check(slot_l, slot_r)) || (rc = pc.check_capacity(cap)) || (rc = ak_check(c, who, rows, cols, threshold))) return rc;
  // a kept record's octave is at most that of the shape's last level
  const int max_octave = ex == AkExtract::Orb ? ((c->akaze.rows == rows && c->akaze.cols == cols) ? c->akaze.octaves : make_tables(rows, cols).octaves) - 1 : 0;
  if (ex == AkExtract::Orb)
    if ((rc = orb_link_check(c, who, rows, cols, max_octave))) return rc;
  if ((rc = pc.open())) return rc;
  hipStream_t st = c->stream2;
  auto &bb = c->bin;
  auto &d = c->akaze;
  // every allocation before the first launch of the chain; the image buffer before the layout of its shape
  if ((rc = classic_slots_ensure(c, cap, (size_t)rows * cols)) || (rc = classic_image_ensure(c, rows, cols)) || (rc = ak_ensure(c, rows, cols)) || (rc = ak_sup_ensure(c, d.cand_cap)) ||
      (rc = ex == AkExtract::Mldb ? ak_kp_ensure(c, cap) : ex == AkExtract::Orb ? orb_link_ensure(c, rows, cols, cap) : ak_brisk_ensure(c, rows, cols, cap)))
    return rc;
  if ((rc = pc.load(img_l, img_r, rows, cols, stride))) return rc;
  const AkazeLevels &lv = d.lv;
  const dim3 blk(256);
  for (int k = 0; k < 2; ++k) {
    const BinarySlot &s = bb.slots[pc.slots[k]];
    // the detector through rule 11, then the descriptor on what it leaves, the count read on the device
    if ((rc = ak_staged_enqueue(c, pc.image(k), rows, cols, threshold))) return rc;
    int *h_n = bb.h_n + 4 * k, *h_k = bb.h_n + 8 + 4 * k;
    AkazeKp *h_akp = bb.h_akp + (size_t)k * cap;
    uint8_t *h_desc = bb.h_desc + (size_t)k * cap * row_bytes;
    if (ex == AkExtract::Mldb) {
      hipLaunchKernelGGL(akaze_describe_kernel, dim3(std::min(cap, 4096)), dim3(64), 0, st, lv, d.sup_kp, cap, d.sup_cnt + AKAZE_SUP_KEPT, d.d_angle, d.d_desc);
      hipLaunchKernelGGL(akaze_pair_finish_kernel, dim3(32), blk, 0, st, d.stat, d.cand_cap, d.sup_cnt, d.sup_kp, d.d_angle, d.d_desc, cap, s.d_kp, s.d_desc, s.d_n, h_n, h_k, h_akp, h_desc);
    } else if (ex == AkExtract::Orb) {
      static_assert(offsetof(AkazeKp, x) == 0 && offsetof(AkazeKp, y) == 4 && offsetof(AkazeKp, octave) == 20, "record layout");
      const OrbLinkSrc src{reinterpret_cast<const char *>(d.sup_kp.get()), (int)sizeof(AkazeKp), 0, 4, 20, nullptr, d.sup_cnt + AKAZE_SUP_KEPT, d.sup_cap};
      if ((rc = orb_link_enqueue(c, rows, cols, max_octave, src, cap, reinterpret_cast<uint8_t *>(s.d_desc.get())))) return rc;
      orb_link_finish_akaze(c, d.sup_kp, d.stat, d.cand_cap, cap, s.d_kp, s.d_desc, s.d_n, h_n, h_k, h_akp, h_desc);
    } else {
      // the kept records as a BRISK detector's list, every keep flag set; the tested compaction, describe and finishing launches follow
      // (their 24-byte mirror goes to h_bkp and is not handed out), then the 28-byte mirror
      hipLaunchKernelGGL(akaze_present_brisk_kernel, dim3(32), blk, 0, st, d.stat, d.cand_cap, d.sup_cnt, d.sup_kp, d.brk_cap, d.brk_rec, d.brk_keep, d.brk_cnt);
      const ChainOut out{bb.d_cnt + k * BIN_COUNTER_INTS, bb.d_kresp, s.d_kp, s.d_desc, s.d_n, h_n, nullptr, h_desc};
      if ((rc = brisk_pair_chain_enqueue(c, rows, cols, cap, d.brk_rec, d.brk_keep, d.brk_cnt, d.brk_cap, d.brk_crec, out, bb.h_bkp + (size_t)k * cap))) return rc;
      hipLaunchKernelGGL(akaze_brisk_finish_kernel, dim3(32), blk, 0, st, d.stat, out.cnt, d.brk_crec, c->brisk.angle, cap, h_k, h_akp);
    }
    HIP_TRY(c, hipGetLastError());
  }
  if ((rc = pc.submit())) return rc;
  pc.count(0); pc.count(1);
  // (kept: the AKAZE callers answer a detector overflow with SPVO_ERR_STATE -- the list holds every strict maximum the borders leave room
  // for, so the flag cannot be set; were it, the counts would be wrong)
  if (bb.h_n[1] || bb.h_n[5]) return fail(c, SPVO_ERR_STATE, "%s: the candidate list overflowed although it is sized from the image", who);
  ak_mark_right_resident(c, bb.h_n);   // (kept: also when the capacity rule below answers SPVO_ERR_CAPACITY)
  static_assert(sizeof(spvo_akaze_keypoint) == sizeof(AkazeKp), "record layout");
  const PairMirror mirrors[2] = {{bb.h_akp, sizeof(AkazeKp), bb.h_desc, (size_t)row_bytes},
                                 {bb.h_akp + cap, sizeof(AkazeKp), bb.h_desc + (size_t)cap * row_bytes, (size_t)row_bytes}};
  return pc.commit(mirrors);
}
}  // namespace
extern "C" {

int spvo_akaze_detect_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, float threshold, int slot_l, int slot_r, int slot_capacity,
                           spvo_akaze_features *out_l, spvo_akaze_features *out_r) {
  return akaze_pair(c, "spvo_akaze_detect_pair", AkExtract::Mldb, img_l, img_r, rows, cols, stride, threshold, slot_l, slot_r, slot_capacity, out_l, out_r);
}

// The AKAZE detector with the ORB extractor at the keypoints' octaves, pair-resident: per image what spvo_akaze_detect followed by
// spvo_orb_describe_octaves(img = NULL) hands out, byte for byte, in slots of 32-byte rows
int spvo_akaze_orb_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, float threshold, int slot_l, int slot_r, int slot_capacity,
                        spvo_akaze_features *out_l, spvo_akaze_features *out_r) {
  return akaze_pair(c, "spvo_akaze_orb_pair", AkExtract::Orb, img_l, img_r, rows, cols, stride, threshold, slot_l, slot_r, slot_capacity, out_l, out_r);
}

// The AKAZE detector with the BRISK extractor, pair-resident: per image what spvo_akaze_detect followed by spvo_brisk_describe(img = NULL)
// on its x, y, size hands out, byte for byte, in slots of 64-byte rows
int spvo_akaze_brisk_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, float threshold, int slot_l, int slot_r, int slot_capacity,
                          spvo_akaze_features *out_l, spvo_akaze_features *out_r) {
  return akaze_pair(c, "spvo_akaze_brisk_pair", AkExtract::Brisk, img_l, img_r, rows, cols, stride, threshold, slot_l, slot_r, slot_capacity, out_l, out_r);
}

// The AKAZE detector with the SIFT extractor, pair-resident in the SIFT slots: per image what spvo_akaze_detect followed by
// spvo_sift_describe(img = NULL) on {x, y, size, angle, response, octave} of its records hands out, byte for byte; the host's records keep
// their class_id.  The call is sift_link_pair's (spvo_sift.hip); the detector's part is akaze_pair's chain, ak_staged_enqueue,
// which leaves sup_kp and the AKAZE_SUP_KEPT count on the device.  A kept record's octave is at most that of the shape's last level, so the
// pyramid is built up to it.  Afterwards the right image's scale space is resident, as after spvo_akaze_orb_pair.
int spvo_akaze_sift_pair(spvo_ctx *c, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride, float threshold, int slot_l, int slot_r, int slot_capacity,
                         spvo_akaze_sift_features *out_l, spvo_akaze_sift_features *out_r) {
  if (!c || !img_l || !img_r || !out_l || !out_r || rows <= 0 || cols <= 0 || stride < (size_t)cols) return fail(c, SPVO_ERR_INVALID, "bad argument");
  static_assert(sizeof(spvo_akaze_keypoint) == sizeof(AkazeKp), "record layout");
  const char *who = "spvo_akaze_sift_pair";
  auto &d = c->akaze;
  SiftLinkDetector det;
  det.who = who;
  det.max_octave = ((d.rows == rows && d.cols == cols) ? d.octaves : make_tables(rows, cols).octaves) - 1;   // (make_tables takes any positive shape)
  det.check = [&]() -> int { return ak_check(c, who, rows, cols, threshold); };
  det.prepare = [&](SiftLinkSrc &src) -> int {
    int rc;
    if ((rc = ak_ensure(c, rows, cols)) || (rc = ak_sup_ensure(c, d.cand_cap))) return rc;
    src = SiftLinkSrc{reinterpret_cast<const char *>(d.sup_kp.get()), (int)sizeof(AkazeKp), (int)offsetof(AkazeKp, x), (int)offsetof(AkazeKp, y), (int)offsetof(AkazeKp, size),
                      (int)offsetof(AkazeKp, angle), (int)offsetof(AkazeKp, response), (int)offsetof(AkazeKp, octave), nullptr, d.sup_cnt + AKAZE_SUP_KEPT, d.sup_cap, nullptr, d.stat,
                      d.cand_cap};
    return SPVO_OK;
  };
  det.enqueue = [&](const uint8_t *h_img) -> int {
    if (int rc = ak_staged_enqueue(c, h_img, rows, cols, threshold)) return rc;
    HIP_TRY(c, hipGetLastError());
    return SPVO_OK;
  };
  const int rc = sift_link_pair(c, det, img_l, img_r, rows, cols, stride, slot_l, slot_r, slot_capacity, pair_out(out_l), pair_out(out_r));
  // (kept: both SPVO_OK and SPVO_ERR_CAPACITY are answered behind the wait, and after either the right image's scale space is resident)
  if (rc == SPVO_OK || rc == SPVO_ERR_CAPACITY) ak_mark_right_resident(c, c->sift.h_n);
  return rc;
}

int spvo_akaze_tables(int rows, int cols, int *levels, int32_t *octave, float *esigma, int32_t *sigma_size, int32_t *nsteps, float *tau, int tau_cap, int *n_tau, float *g0, float *g1) {
  if (rows < 16 || cols < 16 || !levels || !n_tau || tau_cap < 0) return SPVO_ERR_INVALID;
  const AkTables T = make_tables(rows, cols);
  *levels = T.n;
  *n_tau = (int)T.tau.size();
  for (int i = 0; i < T.n; ++i) {
    if (octave) octave[i] = T.octave[i];
    if (esigma) esigma[i] = T.esigma[i];
    if (sigma_size) sigma_size[i] = T.sigma_size[i];
    if (nsteps && i > 0) nsteps[i - 1] = T.nsteps[i];
  }
  if (tau) std::memcpy(tau, T.tau.data(), std::min<size_t>(T.tau.size(), (size_t)tau_cap) * sizeof(float));
  if (g0) std::memcpy(g0, T.g0.g, (size_t)(T.g0.r + 1) * sizeof(float));
  if (g1) std::memcpy(g1, T.g1.g, (size_t)(T.g1.r + 1) * sizeof(float));
  return SPVO_OK;
}

}  // extern "C"
