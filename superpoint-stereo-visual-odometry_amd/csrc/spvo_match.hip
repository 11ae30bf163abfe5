// spvo_match.hip -- descriptor matching (matchDescriptors, feature_detection_base.cpp:434-500): L2 (K12, K13) and Hamming (K12h).
#include "spvo_internal.hip.h"
#include "match.hip.h"

namespace spvo_int {

int ensure_match(spvo_ctx *c, int na, int nb) {
  const int need = std::max(na, nb);
  if (need <= c->match_cap) return SPVO_OK;
  const int cap = std::max(need, std::max(c->cfg.max_keypoints, 1024));
  HIP_TRY(c, hipDeviceSynchronize());
  // the capacity drops to 0 first: an allocation failure further down leaves a context that spvo_destroy (and a later, smaller
  // request) can still handle
  c->match_cap = 0;
  for (SubmitSet &s : c->sets) set_release_match(s);
  std::vector<GrowEntry> list{zeroed(c->d_ma, (size_t)cap * MATCH_D), zeroed(c->d_mb, (size_t)cap * MATCH_D), zeroed(c->d_match_out, (size_t)4 * cap)};
  const size_t nt = (size_t)(cap + MATCH_TT - 1) / MATCH_TT;
  for (auto &set : c->ms)
    for (MatchScratch &m : set) {
      m.d_out = nullptr;
      list.insert(list.end(), {zeroed(m.d_na, cap + 4), zeroed(m.d_nb, cap + 4),   // K12b reads the norms four at a time
                               zeroed(m.d_best_d2, (size_t)cap * 2), zeroed(m.d_dt, (size_t)cap * match_ldt(cap)), zeroed(m.d_cand, (size_t)cap * nt * MATCH_C),
                               zeroed(m.d_meta, (size_t)cap * nt), zeroed(m.d_best_idx, (size_t)cap * 2), zeroed(m.d_train_best, cap), zeroed(m.d_a8, (size_t)cap * MATCH_D),
                               zeroed(m.d_b8, (size_t)cap * MATCH_D), zeroed(m.d_qa8, cap), zeroed(m.d_qb8, cap)});
    }
  c->h_match_tmp.reset();   // (re-allocated behind the sets' mirrors, below)
  if (int rc = grow(c, wait_for_nothing(), list)) return rc;
  for (int k4 = 0; k4 < 4; ++k4) c->ms[k4 >> 1][k4 & 1].d_out = c->d_match_out + (size_t)k4 * cap;
  for (SubmitSet &s : c->sets) HIP_TRY(c, hipHostMalloc((void **)&s.h_match_out, (size_t)2 * cap * sizeof(int2)));
  if (int rc = grow(c, wait_for_nothing(), {plain(c->h_match_tmp, cap)})) return rc;
  c->match_cap = cap;
  return SPVO_OK;
}

// Enqueue 1 or 2 matches as ONE set of launches (blockIdx.z / .y = job) and one result copy:
// packed {train_idx, distance bits} for job k lands at host_out + k*match_cap.
int enqueue_matches(spvo_ctx *c, const MatchReq *req_in, int njobs, int selector, int cross_check, float ratio, int2 *host_out) {
  MatchJobs jobs;
  int na_max = 0, nb_max = 0;
  // NN + cross-check is cv::batchDistance's crosscheck: the search runs from the TRAIN rows to the query rows, so the
  // two sides change places for the distance GEMM and the re-rank; match_select_cross_kernel writes one entry per
  // query row again
  const bool swap = selector == SPVO_SELECT_NN && cross_check;
  // host_out is pinned memory of the context (h_match_out / h_match_tmp): the kernels that decide a row write its entry there
  // themselves -- 8 bytes per row over PCIe -- instead of a 16 KB copy behind them (a 19 us blit launch between the merge and the
  // event the host waits for).
  MatchReq req[2];
  for (int k = 0; k < njobs; ++k) {
    req[k] = req_in[k];
    if (swap) {
      std::swap(req[k].dA, req[k].dB); std::swap(req[k].na, req[k].nb);
      std::swap(req[k].na_ptr, req[k].nb_ptr); std::swap(req[k].sqA, req[k].sqB);
    }
    MatchScratch &m = c->ms[c->ms_set & 1][k];
    MatchJob &j = jobs.j[k];
    j.A = req[k].dA; j.B = req[k].dB;
    j.na = req[k].na; j.nb = req[k].nb;
    j.na_ptr = req[k].na_ptr; j.nb_ptr = req[k].nb_ptr;
    j.nA = req[k].sqA ? req[k].sqA : m.d_na;
    j.nB = req[k].sqB ? req[k].sqB : m.d_nb;
    j.dt = m.d_dt; j.cand = m.d_cand; j.meta = m.d_meta; j.best_d2 = m.d_best_d2; j.best_idx = m.d_best_idx; j.train_best = m.d_train_best; j.out = host_out + (size_t)k * c->match_cap;
    j.A8 = j.B8 = nullptr;
    j.qA8 = j.qB8 = nullptr;
    if (c->match_fp8) {
      hipLaunchKernelGGL(desc_to_fp8_kernel, dim3((req[k].na + 3) / 4), dim3(256), 0, c->post, req[k].dA, req[k].na, req[k].na_ptr, m.d_a8, m.d_qa8);
      hipLaunchKernelGGL(desc_to_fp8_kernel, dim3((req[k].nb + 3) / 4), dim3(256), 0, c->post, req[k].dB, req[k].nb, req[k].nb_ptr, m.d_b8, m.d_qb8);
      j.A8 = m.d_a8; j.B8 = m.d_b8;
      j.qA8 = m.d_qa8; j.qB8 = m.d_qb8;
    }
    na_max = std::max(na_max, req[k].na);
    nb_max = std::max(nb_max, req[k].nb);
    if (!req[k].sqA) hipLaunchKernelGGL(row_sqnorm_kernel, dim3((req[k].na + 3) / 4), dim3(256), 0, c->post, req[k].dA, req[k].na, req[k].na_ptr, m.d_na);
    if (!req[k].sqB) hipLaunchKernelGGL(row_sqnorm_kernel, dim3((req[k].nb + 3) / 4), dim3(256), 0, c->post, req[k].dB, req[k].nb, req[k].nb_ptr, m.d_nb);
    if (swap) HIP_TRY(c, hipMemsetAsync(m.d_train_best, 0xFF, (size_t)req[k].nb * sizeof(unsigned long long), c->post));
  }
  if (njobs == 1) jobs.j[1] = jobs.j[0];
  const int groups = (nb_max + MATCH_TT - 1) / MATCH_TT;
  const int ldt = match_ldt(c->match_cap);
  const double fl = 2.0 * na_max * nb_max * MATCH_D * njobs;
  ScopedStage st(c, stage_id(c, "match"), fl, 4.0 * (na_max + nb_max) * MATCH_D * njobs);
  const size_t lds = MATCH_LDS_BYTES;
  static bool attr[64] = {};
  if (!attr[c->cfg.device & 63]) {
    HIP_TRY(c, hipFuncSetAttribute((const void *)match_gemm_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(c, hipFuncSetAttribute((const void *)match_gemm_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr[c->cfg.device & 63] = true;
  }
  // Default: the fused form -- the distance tile is reduced per query row in LDS (K12a) and a short merge (K12m) finishes the row;
  // dt never goes to HBM.  The fp8 shortlist mode (and tuning "match_fused" = 0, for A/B measurements) keeps the two-kernel form that
  // writes every dt and reads it back.  Column tiles are lanes of the merge: capacities beyond 64 tiles use the unfused form.
  const bool fused_on = tuning("match_fused", 1) != 0;
  const int nt_stride = (c->match_cap + MATCH_TT - 1) / MATCH_TT;
  const bool fused = fused_on && !c->match_fp8 && nt_stride <= 64;
  const int gx = groups, gy = (na_max + MATCH_QT - 1) / MATCH_QT;
  const dim3 gg(8 * ((gx * gy * njobs + 7) / 8));   // one-dimensional: XCD-contiguous chunks of the tile order (see the kernel)
  {
    ScopedStage sg(c, stage_id(c, "match_gemm"), fl, 4.0 * (na_max + nb_max) * MATCH_D * njobs);
    if (c->match_fp8) hipLaunchKernelGGL((match_gemm_kernel<true, false>), gg, dim3(256), MATCH_LDS_BYTES_FP8, c->post, jobs, ldt, 0.f, 0, gx, gy, njobs);
    else if (fused) hipLaunchKernelGGL((match_gemm_kernel<false, true>), gg, dim3(256), lds, c->post, jobs, ldt, MATCH_ERR_REL, nt_stride, gx, gy, njobs);
    else hipLaunchKernelGGL((match_gemm_kernel<false, false>), gg, dim3(256), lds, c->post, jobs, ldt, 0.f, 0, gx, gy, njobs);
  }
  {
    ScopedStage sr(c, stage_id(c, "match_rerank"));
    const float err = c->match_fp8 ? MATCH_ERR_REL_FP8 : MATCH_ERR_REL;
    const dim3 gr((na_max + 3) / 4, njobs);
    // rows of up to 1024 columns stay in registers between the two passes of the re-rank (8 chunks for 2048 columns
    // measured 2.4x SLOWER than the chunked form: 232 registers, 70 KB of LDS)
    const int nch = !fused && nb_max <= 1024 ? 4 : 0;
    c->match_form[0] = c->match_fp8 ? 1 : 0; c->match_form[1] = fused ? 1 : 0; c->match_form[2] = nch; c->match_form[3] = njobs;   // spvo_match_last_form
    if (fused) hipLaunchKernelGGL(match_merge_kernel<>, gr, dim3(256), sizeof(MatchRerankLds<0>), c->post, jobs, nt_stride, ldt, MATCH_ERR_REL, selector, cross_check, ratio);
    else if (nb_max <= 1024) hipLaunchKernelGGL(match_rerank_kernel<4>, gr, dim3(256), sizeof(MatchRerankLds<4>), c->post, jobs, ldt, err, selector, cross_check, ratio);
    else hipLaunchKernelGGL(match_rerank_kernel<0>, gr, dim3(256), sizeof(MatchRerankLds<0>), c->post, jobs, ldt, err, selector, cross_check, ratio);
  }
  if (swap) hipLaunchKernelGGL(match_select_cross_kernel, dim3((nb_max + 255) / 256, njobs), dim3(256), 0, c->post, jobs);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

void unpack_match(const int2 *packed, int n, int32_t *train_idx, float *distance) {
  for (int i = 0; i < n; ++i) {
    train_idx[i] = packed[i].x;
    std::memcpy(&distance[i], &packed[i].y, sizeof(float));
  }
}

int run_match(spvo_ctx *c, const MatchReq &r, int selector, int cross_check, float ratio, int32_t *train_idx, float *distance) {
  if (r.na == 0) return SPVO_OK;
  if (r.nb == 0) {
    for (int i = 0; i < r.na; ++i) { train_idx[i] = -1; distance[i] = 0.f; }
    return SPVO_OK;
  }
  int rc = enqueue_matches(c, &r, 1, selector, cross_check, ratio, c->h_match_tmp);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->post));
  unpack_match(c->h_match_tmp, r.na, train_idx, distance);
  return SPVO_OK;
}

// One Hamming match between two binary slots OF ONE ROW WIDTH on the solver's stream, counts read on the device (match.hip.h K12t, by the
// slots' width the instantiation for 8 words, or for 16 for any width above 32 bytes): the packed result
// {train_idx, distance bits} of every row of slot_a lands in `host_out` (pinned).  NN + cross-check is cv::batchDistance's crosscheck as in
// spvo_match_hamming: the train rows vote for their nearest query row, then every query row reads its vote.
int enqueue_hamming_slots(spvo_ctx *c, int slot_a, int slot_b, int selector, int cross_check, float ratio, int2 *host_out) {
  static_assert(HAM_SHIFT == HAM_KEY_SHIFT, "the key layout of match.hip.h and the capacity limit of spvo_classic_detect differ");
  auto &bb = c->bin;
  const BinarySlot &a = bb.slots[slot_a], &b = bb.slots[slot_b];
  hipStream_t st = c->stream2;
  const int cap = bb.cap;
  if (a.row_bytes != b.row_bytes)
    return fail(c, SPVO_ERR_INVALID, "binary slot %d holds rows of %d bytes, slot %d rows of %d bytes: only slots of one width are matched", slot_a, a.row_bytes, slot_b, b.row_bytes);
  const bool wide = a.row_bytes > 32;   // (BRISK's 64 bytes, AKAZE's 61 in 16 words)
  const dim3 grid(wide ? (cap + HAM_QB<16> - 1) / HAM_QB<16> : (cap + HAM_QB<8> - 1) / HAM_QB<8>);
  auto launch = [&](const BinarySlot &q, const BinarySlot &t, int mode) {
    if (wide) hipLaunchKernelGGL(match_hamming_tiled_kernel<16>, grid, dim3(256), 0, st, q.d_desc, q.d_n, t.d_desc, t.d_n, cap, mode, ratio, host_out, bb.d_vote);
    else hipLaunchKernelGGL(match_hamming_tiled_kernel<8>, grid, dim3(256), 0, st, q.d_desc, q.d_n, t.d_desc, t.d_n, cap, mode, ratio, host_out, bb.d_vote);
  };
  if (cross_check && selector == SPVO_SELECT_NN) {   // BFMatcher's crossCheck is off for knnMatch (base.cpp:27-28)
    HIP_TRY(c, hipMemsetAsync(bb.d_vote, 0xFF, (size_t)cap * sizeof(unsigned long long), st));
    launch(b, a, 2);
    hipLaunchKernelGGL(match_hamming_cross_slots_kernel, dim3((cap + 255) / 256), dim3(256), 0, st, bb.d_vote, a.d_n, cap, host_out);
  } else {
    launch(a, b, selector == SPVO_SELECT_KNN ? 1 : 0);
  }
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// The launches of one byte-L2 match (match.hip.h K12u) on `st`: rows `row_bytes` wide lying 32 (row_bytes <= 32) or 64 bytes apart, `cap`
// rows at most on either side, the packed result of every row of `a` into `out` (device or pinned memory, cap entries).  U8Rows::n is the
// host's count, or with n_ptr set an upper bound that sizes the grid.  FLANN has no cross-check; the mode exists for the C ABI's argument.
struct U8Rows { const uint32_t *rows; int n; const int *n_ptr; };
static int enqueue_l2u8(spvo_ctx *c, hipStream_t st, const U8Rows &a, const U8Rows &b, int cap, int row_bytes, int selector, int cross_check, float ratio, int2 *out,
                        unsigned long long *vote) {
  const bool wide = row_bytes > 32;
  auto launch = [&](const U8Rows &q, const U8Rows &t, int mode) {
    const dim3 grid((q.n + U8L2_QT - 1) / U8L2_QT);
    if (wide) hipLaunchKernelGGL(match_l2u8_kernel<64>, grid, dim3(256), 0, st, q.rows, q.n, q.n_ptr, t.rows, t.n, t.n_ptr, cap, row_bytes, mode, ratio, out, vote);
    else hipLaunchKernelGGL(match_l2u8_kernel<32>, grid, dim3(256), 0, st, q.rows, q.n, q.n_ptr, t.rows, t.n, t.n_ptr, cap, row_bytes, mode, ratio, out, vote);
  };
  if (cross_check && selector == SPVO_SELECT_NN) {
    HIP_TRY(c, hipMemsetAsync(vote, 0xFF, (size_t)a.n * sizeof(unsigned long long), st));
    launch(b, a, 2);   // every train row votes for its nearest query row
    hipLaunchKernelGGL(match_l2u8_cross_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, vote, a.n, a.n_ptr, cap, out);
  } else {
    launch(a, b, selector == SPVO_SELECT_KNN ? 1 : 0);
  }
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

// enqueue_hamming_slots for the byte-L2 norm: the same slots, stream, vote scratch and result format
int enqueue_l2u8_slots(spvo_ctx *c, int slot_a, int slot_b, int selector, int cross_check, float ratio, int2 *host_out) {
  auto &bb = c->bin;
  const BinarySlot &a = bb.slots[slot_a], &b = bb.slots[slot_b];
  if (a.row_bytes != b.row_bytes)
    return fail(c, SPVO_ERR_INVALID, "binary slot %d holds rows of %d bytes, slot %d rows of %d bytes: only slots of one width are matched", slot_a, a.row_bytes, slot_b, b.row_bytes);
  return enqueue_l2u8(c, c->stream2, U8Rows{a.d_desc, bb.cap, a.d_n}, U8Rows{b.d_desc, bb.cap, b.d_n}, bb.cap, a.row_bytes, selector, cross_check, ratio, host_out, bb.d_vote);
}

// the match a binary pair call enqueues behind its features: spvo_set_binary_prematch_norm's choice
int enqueue_binary_prematch(spvo_ctx *c, int slot_a, int slot_b, int2 *host_out) {
  return c->bin_pm_norm == SPVO_NORM_L2 ? enqueue_l2u8_slots(c, slot_a, slot_b, c->pm_selector, c->pm_cross, c->pm_ratio, host_out)
                                        : enqueue_hamming_slots(c, slot_a, slot_b, c->pm_selector, c->pm_cross, c->pm_ratio, host_out);
}

// Host rows of desc_bytes bytes for the two byte matchers: d_ham_a / d_ham_b grown on demand, the rows zero-padded to nw words (pa, pb:
// the packed copies, the caller's until the stream has been waited for) and sent up on the solver's stream.
static int upload_byte_rows(spvo_ctx *c, const uint8_t *desc_a, int na, const uint8_t *desc_b, int nb, int desc_bytes, int nw, std::vector<uint32_t> &pa, std::vector<uint32_t> &pb) {
  const int need = std::max(na, nb);
  if (need > c->ham_cap) {
    c->ham_cap = 0;
    const int cap = std::max(need, 2048);
    if (int rc = grow(c, wait_for(c->stream2), {zeroed(c->d_ham_a, (size_t)cap * 16), zeroed(c->d_ham_b, (size_t)cap * 16), zeroed(c->d_ham_idx, cap), zeroed(c->d_ham_dist, cap),
                                                zeroed(c->d_ham_vote, cap), zeroed(c->d_ham_out, cap)}))
      return rc;
    c->ham_cap = cap;
  }
  pa.assign((size_t)na * nw, 0u); pb.assign((size_t)nb * nw, 0u);
  for (int i = 0; i < na; ++i) std::memcpy(&pa[(size_t)i * nw], desc_a + (size_t)i * desc_bytes, desc_bytes);
  for (int i = 0; i < nb; ++i) std::memcpy(&pb[(size_t)i * nw], desc_b + (size_t)i * desc_bytes, desc_bytes);
  HIP_TRY(c, hipMemcpyAsync(c->d_ham_a, pa.data(), pa.size() * 4, hipMemcpyHostToDevice, c->stream2));
  HIP_TRY(c, hipMemcpyAsync(c->d_ham_b, pb.data(), pb.size() * 4, hipMemcpyHostToDevice, c->stream2));
  return SPVO_OK;
}

}  // namespace spvo_int

// ===========================================================================
extern "C" {

int spvo_match(spvo_ctx *c, const float *desc_a, int na, const float *desc_b, int nb, int selector, int cross_check, float ratio, int32_t *train_idx, float *distance) {
  if (!c || na < 0 || nb < 0 || (na > 0 && (!desc_a || !train_idx || !distance)) || (nb > 0 && !desc_b)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (selector != SPVO_SELECT_NN && selector != SPVO_SELECT_KNN) return fail(c, SPVO_ERR_INVALID, "bad selector");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc = ensure_match(c, na, nb);
  if (rc) return rc;
  PostScope ps(c);   // behind the queued tails: they share the matcher's scratch
  if (na) HIP_TRY(c, hipMemcpyAsync(c->d_ma, desc_a, (size_t)na * MATCH_D * sizeof(float), hipMemcpyHostToDevice, c->post));
  if (nb) HIP_TRY(c, hipMemcpyAsync(c->d_mb, desc_b, (size_t)nb * MATCH_D * sizeof(float), hipMemcpyHostToDevice, c->post));
  return run_match(c, MatchReq{c->d_ma, c->d_mb, na, nb, nullptr, nullptr, nullptr, nullptr}, selector, cross_check ? 1 : 0, ratio, train_idx, distance);
}

// spvo_match for rows of `dim` floats: zero-padded to MATCH_D columns on the way up (a 2-D copy into cleared buffers)
int spvo_match_l2(spvo_ctx *c, const float *desc_a, int na, const float *desc_b, int nb, int dim, int selector, int cross_check, float ratio, int32_t *train_idx, float *distance) {
  if (!c || na < 0 || nb < 0 || (na > 0 && (!desc_a || !train_idx || !distance)) || (nb > 0 && !desc_b)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (dim < 1 || dim > MATCH_D) return fail(c, SPVO_ERR_INVALID, "spvo_match_l2: rows of 1 .. %d floats", MATCH_D);
  if (selector != SPVO_SELECT_NN && selector != SPVO_SELECT_KNN) return fail(c, SPVO_ERR_INVALID, "bad selector");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc = ensure_match(c, na, nb);
  if (rc) return rc;
  PostScope ps(c);   // behind the queued tails: they share the matcher's scratch
  const size_t row = (size_t)dim * sizeof(float), pitch = (size_t)MATCH_D * sizeof(float);
  if (na && dim < MATCH_D) HIP_TRY(c, hipMemsetAsync(c->d_ma, 0, (size_t)na * pitch, c->post));
  if (nb && dim < MATCH_D) HIP_TRY(c, hipMemsetAsync(c->d_mb, 0, (size_t)nb * pitch, c->post));
  if (na) HIP_TRY(c, hipMemcpy2DAsync(c->d_ma, pitch, desc_a, row, row, na, hipMemcpyHostToDevice, c->post));
  if (nb) HIP_TRY(c, hipMemcpy2DAsync(c->d_mb, pitch, desc_b, row, row, nb, hipMemcpyHostToDevice, c->post));
  return run_match(c, MatchReq{c->d_ma, c->d_mb, na, nb, nullptr, nullptr, nullptr, nullptr}, selector, cross_check ? 1 : 0, ratio, train_idx, distance);
}

// cv::BFMatcher(NORM_HAMMING): binary descriptors of `desc_bytes` bytes per row (ORB 32, BRISK 64, AKAZE 61), see match.hip.h K12h
int spvo_match_hamming(spvo_ctx *c, const uint8_t *desc_a, int na, const uint8_t *desc_b, int nb, int desc_bytes, int selector, int cross_check, float ratio,
                       int32_t *train_idx, float *distance) {
  if (!c || na < 0 || nb < 0 || (na > 0 && (!desc_a || !train_idx || !distance)) || (nb > 0 && !desc_b)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (selector != SPVO_SELECT_NN && selector != SPVO_SELECT_KNN) return fail(c, SPVO_ERR_INVALID, "bad selector");
  if (desc_bytes <= 0 || desc_bytes > 64) return fail(c, SPVO_ERR_INVALID, "binary descriptors of 1 .. 64 bytes are supported (got %d)", desc_bytes);
  if (na == 0) return SPVO_OK;
  if (nb == 0) {
    for (int i = 0; i < na; ++i) { train_idx[i] = -1; distance[i] = 0.f; }
    return SPVO_OK;
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const int nw = desc_bytes <= 32 ? 8 : 16;
  // rows zero-padded to nw words: padding bits are equal on both sides and add nothing to a distance
  std::vector<uint32_t> pa, pb;
  if (int rc = upload_byte_rows(c, desc_a, na, desc_b, nb, desc_bytes, nw, pa, pb)) return rc;
  hipStream_t st = c->stream2;   // the solver's stream: overlaps detector submissions in flight
  const bool cross = cross_check && selector == SPVO_SELECT_NN;   // BFMatcher's crossCheck is off for knnMatch (base.cpp:27-28)
  auto launch = [&](const uint32_t *A, int n_a, const uint32_t *B, int n_b, int mode) {
    if (nw == 8) hipLaunchKernelGGL(match_hamming_kernel<8>, dim3((n_a + 3) / 4), dim3(256), 0, st, A, n_a, B, n_b, mode, ratio, c->d_ham_idx, c->d_ham_dist, c->d_ham_vote);
    else hipLaunchKernelGGL(match_hamming_kernel<16>, dim3((n_a + 3) / 4), dim3(256), 0, st, A, n_a, B, n_b, mode, ratio, c->d_ham_idx, c->d_ham_dist, c->d_ham_vote);
  };
  if (cross) {
    HIP_TRY(c, hipMemsetAsync(c->d_ham_vote, 0xFF, (size_t)na * sizeof(unsigned long long), st));
    launch(c->d_ham_b, nb, c->d_ham_a, na, 2);   // every train row votes for its nearest query row
    hipLaunchKernelGGL(match_hamming_cross_kernel, dim3((na + 255) / 256), dim3(256), 0, st, c->d_ham_vote, na, c->d_ham_idx, c->d_ham_dist);
  } else {
    launch(c->d_ham_a, na, c->d_ham_b, nb, selector == SPVO_SELECT_KNN ? 1 : 0);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(train_idx, c->d_ham_idx, (size_t)na * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(distance, c->d_ham_dist, (size_t)na * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return SPVO_OK;
}

int spvo_match_slots(spvo_ctx *c, int slot_a, int slot_b, int selector, int cross_check, float ratio, int32_t *train_idx, float *distance) {
  if (!c || slot_a < 0 || slot_a >= N_SLOTS || slot_b < 0 || slot_b >= N_SLOTS) return fail(c, SPVO_ERR_INVALID, "bad slot");
  if (selector != SPVO_SELECT_NN && selector != SPVO_SELECT_KNN) return fail(c, SPVO_ERR_INVALID, "bad selector");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  (void)release_held_if_idle(c);   // (a failing launch is reported by that pair's spvo_detect_wait: launch_group)
  const FeatureSlot &a = c->slots[slot_a], &b = c->slots[slot_b];
  if (a.n > 0 && (!train_idx || !distance)) return fail(c, SPVO_ERR_INVALID, "null output");
  for (int set = 0; set < RING; ++set) {   // already computed alongside the detector (spvo_set_prematch)?
    bool inflight = false;
    for (const auto &q : c->pendq) inflight |= q.ring == set;
    if (inflight) continue;   // that set belongs to a submission in flight
    if (const MatchCache *mc = c->sets[set].mcache.find(slot_a, slot_b, a.gen, b.gen, selector, cross_check ? 1 : 0, ratio)) {
      // the matches were enqueued behind the submission's features; spvo_detect_wait returned when the features were final
      const double tw0 = diag_now_us();
      HIP_TRY(c, wait_event(c->sets[set].ev_tail));
      g_diag.iv_match += diag_now_us() - tw0;
      if (a.n > 0) unpack_match(mc->h_out, a.n, train_idx, distance);
      return SPVO_OK;
    }
  }
  ++g_diag.match_miss;
  for (const auto &q : c->pendq)
    if (q.slot_l == slot_a || q.slot_r == slot_a || q.slot_l == slot_b || q.slot_r == slot_b)
      return fail(c, SPVO_ERR_STATE, "match not precomputed and a detector submission is rewriting the feature slots");
  PostScope ps(c);   // behind the queued tails: they share the matcher's scratch
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc = ensure_match(c, a.n, b.n);
  if (rc) return rc;
  return run_match(c, MatchReq{a.d_desc, b.d_desc, a.n, b.n, nullptr, nullptr, a.d_sqn, b.d_sqn}, selector, cross_check ? 1 : 0, ratio, train_idx, distance);
}

// The Hamming match of two binary slots (spvo_classic_detect).  Served from the call's prematch when it is exactly that match of exactly
// those slot contents (the generation check of spvo_match_slots), computed on the spot otherwise.
int spvo_match_hamming_slots(spvo_ctx *c, int slot_a, int slot_b, int selector, int cross_check, float ratio, int32_t *train_idx, float *distance) {
  if (!c || slot_a < 0 || slot_a >= N_BIN_SLOTS || slot_b < 0 || slot_b >= N_BIN_SLOTS) return fail(c, SPVO_ERR_INVALID, "bad slot");
  if (selector != SPVO_SELECT_NN && selector != SPVO_SELECT_KNN) return fail(c, SPVO_ERR_INVALID, "bad selector");
  auto &bb = c->bin;
  const BinarySlot &a = bb.slots[slot_a], &b = bb.slots[slot_b];
  if (!a.filled || !b.filled) return fail(c, SPVO_ERR_STATE, "binary slot %d holds no features (spvo_classic_detect fills it)", a.filled ? slot_b : slot_a);
  if (a.row_bytes != b.row_bytes)
    return fail(c, SPVO_ERR_INVALID, "binary slot %d holds rows of %d bytes, slot %d rows of %d bytes: only slots of one width are matched", slot_a, a.row_bytes, slot_b, b.row_bytes);
  if (a.n > 0 && (!train_idx || !distance)) return fail(c, SPVO_ERR_INVALID, "null output");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const int cross = cross_check ? 1 : 0;
  if (const MatchCache *mc = bb.pair.mcache.find(slot_a, slot_b, a.gen, b.gen, selector, cross, ratio)) {
    HIP_TRY(c, wait_event(bb.pair.ev_match));
    unpack_match(mc->h_out, a.n, train_idx, distance);
    return SPVO_OK;
  }
  if (a.n == 0) return SPVO_OK;
  int2 *h = bb.h_match + (size_t)2 * bb.cap;
  if (int rc = enqueue_hamming_slots(c, slot_a, slot_b, selector, cross, ratio, h)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  unpack_match(h, a.n, train_idx, distance);
  return SPVO_OK;
}

// MatcherType::FLANN on binary descriptors: the exact L2 nearest neighbours of the rows' bytes (match.hip.h K12u).  spvo_match_hamming's
// argument rules, buffers and stream.
int spvo_match_l2_u8(spvo_ctx *c, const uint8_t *desc_a, int na, const uint8_t *desc_b, int nb, int desc_bytes, int selector, int cross_check, float ratio,
                     int32_t *train_idx, float *distance) {
  if (!c || na < 0 || nb < 0 || (na > 0 && (!desc_a || !train_idx || !distance)) || (nb > 0 && !desc_b)) return fail(c, SPVO_ERR_INVALID, "bad argument");
  if (selector != SPVO_SELECT_NN && selector != SPVO_SELECT_KNN) return fail(c, SPVO_ERR_INVALID, "bad selector");
  if (desc_bytes <= 0 || desc_bytes > 64) return fail(c, SPVO_ERR_INVALID, "binary descriptors of 1 .. 64 bytes are supported (got %d)", desc_bytes);
  if (na == 0) return SPVO_OK;
  if (nb == 0) {
    for (int i = 0; i < na; ++i) { train_idx[i] = -1; distance[i] = 0.f; }
    return SPVO_OK;
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  std::vector<uint32_t> pa, pb;
  if (int rc = upload_byte_rows(c, desc_a, na, desc_b, nb, desc_bytes, desc_bytes <= 32 ? 8 : 16, pa, pb)) return rc;
  hipStream_t st = c->stream2;
  if (int rc = enqueue_l2u8(c, st, U8Rows{c->d_ham_a, na, nullptr}, U8Rows{c->d_ham_b, nb, nullptr}, c->ham_cap, desc_bytes, selector, cross_check ? 1 : 0, ratio, c->d_ham_out,
                            c->d_ham_vote))
    return rc;
  std::vector<int2> packed(na);
  HIP_TRY(c, hipMemcpyAsync(packed.data(), c->d_ham_out, (size_t)na * sizeof(int2), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  unpack_match(packed.data(), na, train_idx, distance);
  return SPVO_OK;
}

// spvo_match_l2_u8 on two binary slots.  Served from the call's prematch when that ran under SPVO_NORM_L2 and is exactly this match of
// exactly these slot contents, computed on the spot otherwise.
int spvo_match_l2_u8_slots(spvo_ctx *c, int slot_a, int slot_b, int selector, int cross_check, float ratio, int32_t *train_idx, float *distance) {
  if (!c || slot_a < 0 || slot_a >= N_BIN_SLOTS || slot_b < 0 || slot_b >= N_BIN_SLOTS) return fail(c, SPVO_ERR_INVALID, "bad slot");
  if (selector != SPVO_SELECT_NN && selector != SPVO_SELECT_KNN) return fail(c, SPVO_ERR_INVALID, "bad selector");
  auto &bb = c->bin;
  const BinarySlot &a = bb.slots[slot_a], &b = bb.slots[slot_b];
  if (!a.filled || !b.filled) return fail(c, SPVO_ERR_STATE, "binary slot %d holds no features (spvo_classic_detect fills it)", a.filled ? slot_b : slot_a);
  if (a.row_bytes != b.row_bytes)
    return fail(c, SPVO_ERR_INVALID, "binary slot %d holds rows of %d bytes, slot %d rows of %d bytes: only slots of one width are matched", slot_a, a.row_bytes, slot_b, b.row_bytes);
  if (a.n > 0 && (!train_idx || !distance)) return fail(c, SPVO_ERR_INVALID, "null output");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const int cross = cross_check ? 1 : 0;
  if (const MatchCache *mc = bb.pair.mcache.find(slot_a, slot_b, a.gen, b.gen, selector, cross, ratio, SPVO_NORM_L2)) {
    HIP_TRY(c, wait_event(bb.pair.ev_match));
    unpack_match(mc->h_out, a.n, train_idx, distance);
    return SPVO_OK;
  }
  if (a.n == 0) return SPVO_OK;
  int2 *h = bb.h_match + (size_t)2 * bb.cap;
  if (int rc = enqueue_l2u8_slots(c, slot_a, slot_b, selector, cross, ratio, h)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream2));
  unpack_match(h, a.n, train_idx, distance);
  return SPVO_OK;
}

int spvo_set_binary_prematch_norm(spvo_ctx *c, int norm) {
  if (!c) return fail(c, SPVO_ERR_INVALID, "null context");
  if (norm != SPVO_NORM_HAMMING && norm != SPVO_NORM_L2) return fail(c, SPVO_ERR_INVALID, "bad norm %d (SPVO_NORM_HAMMING or SPVO_NORM_L2)", norm);
  c->bin_pm_norm = norm;
  c->bin.pair.mcache.invalidate();
  return SPVO_OK;
}

// The L2 match of two SIFT slots (spvo_sift_detect_pair): the slots' rows, counts and squared norms go to the matcher as they lie on the
// device.  Served from the call's prematch when it is exactly that match of exactly those slot contents, computed on the spot otherwise.
int spvo_match_l2_slots(spvo_ctx *c, int slot_a, int slot_b, int selector, int cross_check, float ratio, int32_t *train_idx, float *distance) {
  if (!c || slot_a < 0 || slot_a >= N_SIFT_SLOTS || slot_b < 0 || slot_b >= N_SIFT_SLOTS) return fail(c, SPVO_ERR_INVALID, "bad slot");
  if (selector != SPVO_SELECT_NN && selector != SPVO_SELECT_KNN) return fail(c, SPVO_ERR_INVALID, "bad selector");
  auto &sf = c->sift;
  const SiftSlot &a = sf.slots[slot_a], &b = sf.slots[slot_b];
  if (!a.filled || !b.filled) return fail(c, SPVO_ERR_STATE, "SIFT slot %d holds no features (spvo_sift_detect_pair fills it)", a.filled ? slot_b : slot_a);
  if (a.n > 0 && (!train_idx || !distance)) return fail(c, SPVO_ERR_INVALID, "null output");
  if (a.n == 0) return SPVO_OK;
  if (b.n == 0) {
    for (int i = 0; i < a.n; ++i) { train_idx[i] = -1; distance[i] = 0.f; }
    return SPVO_OK;
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const int cross = cross_check ? 1 : 0;
  if (const MatchCache *mc = sf.pair.mcache.find(slot_a, slot_b, a.gen, b.gen, selector, cross, ratio)) {
    HIP_TRY(c, wait_event(sf.pair.ev_match));
    unpack_match(mc->h_out, a.n, train_idx, distance);
    return SPVO_OK;
  }
  PostScope ps(c);   // behind the queued tails: they share the matcher's scratch
  if (int rc = ensure_match(c, a.n, b.n)) return rc;
  HIP_TRY(c, hipStreamWaitEvent(c->post, sf.pair.ev_feat, 0));   // behind the feature chain (the solver's stream)
  return run_match(c, MatchReq{a.d_desc, b.d_desc, a.n, b.n, a.d_n, b.d_n, a.d_sqn, b.d_sqn}, selector, cross, ratio, train_idx, distance);
}

int spvo_set_prematch(spvo_ctx *c, int enable, int selector, int cross_check, float ratio) {
  if (!c) return fail(c, SPVO_ERR_INVALID, "null context");
  if (selector != SPVO_SELECT_NN && selector != SPVO_SELECT_KNN) return fail(c, SPVO_ERR_INVALID, "bad selector");
  c->prematch = enable != 0;
  c->pm_selector = selector;
  c->pm_cross = cross_check ? 1 : 0;
  c->pm_ratio = ratio;
  for (SubmitSet &s : c->sets) s.mcache.invalidate();
  c->bin.pair.mcache.invalidate();
  c->sift.pair.mcache.invalidate();
  return SPVO_OK;
}

int spvo_set_match_fp8(spvo_ctx *c, int enable) {
  if (!c) return fail(c, SPVO_ERR_INVALID, "null context");
  c->match_fp8 = enable != 0;
  for (SubmitSet &s : c->sets) s.mcache.invalidate();
  c->sift.pair.mcache.invalidate();   // (not the binary slots': a Hamming match does not depend on fp8)
  return SPVO_OK;
}

int spvo_get_match_fp8(const spvo_ctx *c) { return c ? (c->match_fp8 ? 1 : 0) : SPVO_ERR_INVALID; }

int spvo_match_last_form(spvo_ctx *c, int info[4]) {
  if (!c || !info) return fail(c, SPVO_ERR_INVALID, "bad argument");
  for (int i = 0; i < 4; ++i) info[i] = c->match_form[i];
  return SPVO_OK;
}

}  // extern "C"
