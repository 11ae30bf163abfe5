// spvo_net_i8.hip -- INT8 engines (conv_i8.hip.h): what the plan loader prepares of a layer and of the tail, the fusion plan, and the kernel launchers.
#include "spvo_internal.hip.h"
#include "conv_i8.hip.h"
#include "conv_i8_fused.hip.h"
#include "heads_i8.hip.h"

namespace spvo_int {

// ---------------------------------------------------------------- INT8 engines
// what the plan loader prepares of a depthwise 3x3 convolution (spvo_plan.hip)
int prepare_dwconv_i8(spvo_ctx *c, unsigned i, const float *w, const float *b) {
  Op &op = c->ops[i];
  const Tensor &ti = c->tensors[op.in], &to = c->tensors[op.out];
  if (!ti.i8 || !to.i8) return fail(c, SPVO_ERR_IO, "op %u: depthwise convolution of an INT8 engine needs channel counts that are multiples of 16", i);
  std::vector<int8_t> wq;
  std::vector<float> ws;
  quantize_conv_weights(w, op.cout, 9, wq, ws);
  const std::vector<int> wq32(wq.begin(), wq.end());
  // r = fma(f32(acc), qm, bias) with 1 / s_out folded into both constants (oracle/net_int8.py: FOLDING): the kernels' final multiply is by 1
  std::vector<float> qm(op.cout), bq(op.cout);
  const float inv_dw = 1.f / to.scale;
  for (int o = 0; o < op.cout; ++o) { qm[o] = ws[o] * ti.scale; qm[o] = qm[o] * inv_dw; bq[o] = b[o] * inv_dw; }
  op.inv_s_out = 1.f;
  int rc = upload(c, &op.d_wq32, wq32);
  if (rc || (rc = upload(c, &op.d_wsel, pack_dw_wsel(wq.data(), op.cout))) || (rc = upload(c, &op.d_qm, qm))) return rc;
  return upload(c, &op.d_b, bq);
}

// ... of a convolution; `ckg` groups of 16 channels per chunk: the second digit of launch_conv8's keys
int prepare_conv_i8(spvo_ctx *c, unsigned i, const float *w, const float *b) {
  Op &op = c->ops[i];
  const Tensor &ti = c->tensors[op.in], &to = c->tensors[op.out];
  const bool bn = op.flags & FLAG_BN, add = op.flags & FLAG_ADD, pool = op.flags & FLAG_POOL;
  if (ti.i8 != (op.cin != 1)) return fail(c, SPVO_ERR_IO, "op %u: INT8 engine: a %d-channel input tensor stored as %s", i, op.cin, ti.i8 ? "int8" : "fp32");
  // FOLDING (oracle/net_int8.py): quantised output, no residual, and an affine to fold into (the accumulator's, or a BatchNorm --
  // folded where its constants are built, spvo_plan.hip): the kernels then multiply by 1 at the end
  const bool fold = to.i8 && !add && (op.cin > 1 || bn);
  const float inv_fold = to.i8 ? 1.f / to.scale : 0.f;
  op.inv_s_out = fold ? 1.f : inv_fold;
  if (op.cin == 1) {   // fp32 stem
    if (pool || add || (to.i8 && ((op.out_c_off % 16) || (op.cout % 16)))) return fail(c, SPVO_ERR_IO, "op %u: unsupported single-channel-input layer for INT8", i);
    return upload_stem(c, op, w, b);
  }
  const int ckg = (op.ks == 3 || op.cin % 64) ? 2 : 4;   // 32 channels per chunk; 64 for 1x1 layers when they divide
  // (int8_general: whole groups suffice -- cin 16, 48, ... end in a chunk of one group, conv_i8.hip.h ODD)
  const int fit = c->int8_general_req ? 16 : 16 * ckg;
  if (op.cin % fit || op.in_c_off % 16) return fail(c, SPVO_ERR_IO, "op %u: cin %d / channel offset %d do not fit the INT8 chunking (%d)", i, op.cin, op.in_c_off, fit);
  if (to.i8 && ((op.cout % 16) || (op.out_c_off % 16))) return fail(c, SPVO_ERR_IO, "op %u: cout %d / channel offset %d are not multiples of 16", i, op.cout, op.out_c_off);
  if (!to.i8 && (pool || bn || add)) return fail(c, SPVO_ERR_IO, "op %u: pooled / BatchNorm / residual layer with an fp32 output", i);
  if (add) {
    const Tensor &tr = c->tensors[op.residual];
    if (!tr.i8 || tr.ch != op.cout) return fail(c, SPVO_ERR_IO, "op %u: residual tensor is not a %d-channel int8 tensor", i, op.cout);
    op.s_res = tr.scale;
  }
  op.ck = 16 * ckg;
  op.n_chunks = (op.cin + op.ck - 1) / op.ck;
  choose_variant(c, op, ti);
  std::vector<int8_t> wq;
  std::vector<float> ws;
  quantize_conv_weights(w, op.cout, op.cin * op.ks * op.ks, wq, ws);
  std::vector<float> qm((size_t)op.co_tiles * CO_TILE, 0.f), bp((size_t)op.co_tiles * CO_TILE, 0.f);
  for (int o = 0; o < op.cout; ++o) {
    qm[o] = ws[o] * ti.scale; bp[o] = b[o];
    if (fold && !bn) { qm[o] = qm[o] * inv_fold; bp[o] = bp[o] * inv_fold; }   // (with a BatchNorm the BatchNorm's constants carry the factor)
  }
  int rc = upload(c, &op.d_w8, pack_conv_weights_i8(wq.data(), op.cout, op.cin, op.ks, ckg));
  if (rc || (rc = upload(c, &op.d_qm, qm))) return rc;
  return upload(c, &op.d_b, bp);
}

// ... of a stand-alone 2x2/2 max-pool (int8_general; maxpool2_i8_kernel): nothing to upload, the kernel's multiplier is kept in the op
int prepare_maxpool_i8(spvo_ctx *c, unsigned i) {
  Op &op = c->ops[i];
  const Tensor &ti = c->tensors[op.in], &to = c->tensors[op.out];
  if (!ti.i8 || !to.i8) return fail(c, SPVO_ERR_IO, "op %u: max-pool of an INT8 engine between tensors that are not both int8", i);
  if (to.ch != ti.ch) return fail(c, SPVO_ERR_IO, "op %u: max-pool from %d to %d channels", i, ti.ch, to.ch);
  if (to.level != ti.level + 1) return fail(c, SPVO_ERR_IO, "op %u: level mismatch", i);
  // (defensive: a network's size is a multiple of 8 and a level is at most 3 -- engine_file.h --, so behind the level check every map a pool
  // reads is even; no engine file reaches this text and no test covers it)
  if ((ti.H | ti.W) & 1) return fail(c, SPVO_ERR_IO, "op %u: pooling an odd-sized map", i);
  const float inv = 1.f / to.scale;
  op.pool_m = ti.scale * inv;
  return SPVO_OK;
}

// The tail as ONE launch of heads_i8_kernel (heads_i8.hip.h; launch_heads8 below) -- int8 C16 activations of both branches in, fp32 detector
// planes, un-normalised and normalised descriptors out: oracle/net_int8.py's arithmetic for a layer with an fp32 output
int fuse_tail_i8(spvo_ctx *c, const float *payload, const EngineOp &rp, const EngineOp &rd) {
  const Op &pb = c->ops[c->head_start], &db = c->ops[c->head_start + 1];
  const bool plain = tail_is_plain(c, HEADS8_CIN) && c->tensors[pb.in].i8 && c->tensors[db.in].i8 && !c->tensors[pb.out].i8 && !c->tensors[db.out].i8 &&
                     ((pb.in_c_off | db.in_c_off) % 16) == 0;
  if (!plain) return SPVO_OK;
  std::vector<int8_t> wq_p, wq_d;
  std::vector<float> ws_p, ws_d;
  quantize_conv_weights(payload + rp.w_off, pb.cout, pb.cin, wq_p, ws_p);
  quantize_conv_weights(payload + rd.w_off, db.cout, db.cin, wq_d, ws_d);
  std::vector<float> qm((size_t)HEADS8_UNITS * 16, 0.f), bp((size_t)HEADS8_UNITS * 16, 0.f);
  const float *b_p = payload + rp.b_off, *b_d = payload + rd.b_off;
  for (int o = 0; o < pb.cout; ++o) { qm[o] = ws_p[o] * c->tensors[pb.in].scale; bp[o] = b_p[o]; }
  for (int o = 0; o < db.cout; ++o) { qm[16 * HEADS8_DET_UNITS + o] = ws_d[o] * c->tensors[db.in].scale; bp[16 * HEADS8_DET_UNITS + o] = b_d[o]; }
  int rc = upload(c, &c->d_heads_w8, pack_heads_weights_i8(wq_p.data(), pb.cout, wq_d.data()));
  if (rc || (rc = upload(c, &c->d_heads_qm, qm)) || (rc = upload(c, &c->d_heads_b, bp))) return rc;
  c->heads_fused = true;
  return SPVO_OK;
}

template <int KS, int CKG, int WR, int WC, bool POOL, bool RELU, bool OUT_F32, int EPI = 0, bool ODD = false>
int launch_conv8_instance(spvo_ctx *c, const ConvArgs8 &args, hipStream_t stream) {
  return launch_persistent_tiles<ConvTile8<KS, CKG, WR, WC>, conv_i8_kernel<KS, CKG, WR, WC, POOL, RELU, OUT_F32, EPI, ODD>>(c, args, stream);
}

template <int KS, int CKG, int WR, int WC, bool POOL, bool ODD = false>
int launch_conv8_variant(spvo_ctx *c, const ConvArgs8 &a, bool relu, bool out_f32, int epi, hipStream_t stream) {
  if constexpr (KS == 1) {
    if (epi == 1) return launch_conv8_instance<1, CKG, WR, WC, POOL, true, false, 1, ODD>(c, a, stream);
    if (epi == 2) return launch_conv8_instance<1, CKG, WR, WC, POOL, false, false, 2, ODD>(c, a, stream);
  }
  if constexpr (!POOL) {
    if (out_f32) return relu ? launch_conv8_instance<KS, CKG, WR, WC, false, true, true, 0, ODD>(c, a, stream) : launch_conv8_instance<KS, CKG, WR, WC, false, false, true, 0, ODD>(c, a, stream);
  }
  return relu ? launch_conv8_instance<KS, CKG, WR, WC, POOL, true, false, 0, ODD>(c, a, stream) : launch_conv8_instance<KS, CKG, WR, WC, POOL, false, false, 0, ODD>(c, a, stream);
}

// ---------------------------------------------------------------- MobileNet blocks as one launch (conv_i8_fused.hip.h)
// A depthwise 3x3 (+ ReLU) whose only reader is the pointwise 1x1 (+ ReLU [+ BatchNorm] [+ pool]) behind it, both int8, 64 or 128
// channels in, 64 or 128 out: the pointwise op's launch does both (`fused_dw`), the depthwise op launches nothing (`fused_away`).
// If that block is ops 2, 3 of the plan and ops 0, 1 are the sp_mbv1 stem (3x3 1 -> 1 + ReLU on the fp32 input plane, 1x1 1 -> 64 +
// ReLU + BatchNorm into int8), the same launch computes the stem as well (`fused_stem`).
void plan_int8_fusion(spvo_ctx *c) {
  auto readers = [&](int tensor) { int n = 0; for (const auto &o : c->ops) n += (o.in == tensor) + ((o.flags & FLAG_ADD) && o.residual == tensor); return n; };
  for (size_t i = 0; i + 1 < c->ops.size(); ++i) {
    Op &dw = c->ops[i], &pw = c->ops[i + 1];
    if (dw.type != OP_DWCONV || pw.type != OP_CONV || pw.ks != 1 || pw.in != dw.out || pw.in_c_off || pw.out_c_off || pw.cin != dw.cout) continue;
    if (dw.flags != FLAG_RELU || !(pw.flags & FLAG_RELU) || (pw.flags & FLAG_ADD)) continue;
    const Tensor &ti = c->tensors[dw.in], &tm = c->tensors[dw.out], &to = c->tensors[pw.out];
    if (!ti.i8 || !tm.i8 || !to.i8 || (dw.cout != 64 && dw.cout != 128) || (pw.cout != 64 && pw.cout != 128) || to.ch != pw.cout) continue;
    if (readers(dw.out) != 1 || (int)dw.out == c->t_det || (int)dw.out == c->t_desc || !dw.d_wsel || !pw.d_w8) continue;
    if ((pw.flags & FLAG_POOL) && ((ti.H | ti.W) & 1)) continue;
    pw.fused_dw = (int)i;
    dw.fused_away = true;
    if (i == 2) {
      Op &s0 = c->ops[0], &s1 = c->ops[1];
      const bool stem = s0.type == OP_CONV && s0.cin == 1 && s0.cout == 1 && s0.ks == 3 && s0.flags == FLAG_RELU && s0.in == c->t_input && !c->tensors[s0.out].i8 &&
                        s1.type == OP_CONV && s1.cin == 1 && s1.cout == 64 && s1.ks == 1 && s1.flags == (FLAG_RELU | FLAG_BN) && s1.in == s0.out && s1.out == dw.in &&
                        !s1.out_c_off && dw.cout == 64 && readers(s0.out) == 1 && readers(s1.out) == 1 && s1.d_bn_scale;
      if (stem) { pw.fused_stem = true; s0.fused_away = s1.fused_away = true; }
    }
  }
}

template <int G, bool STEM, bool POOL, int EPI>
static int launch_dwpw8_instance(spvo_ctx *c, const DwPwArgs8 &a, hipStream_t stream) {
  using T = DwPwTile<G, STEM>;
  auto k = dwpw_i8_kernel<G, STEM, POOL, EPI>;
  static int per_cu[64] = {};
  const int dev = c->cfg.device & 63;
  if (!per_cu[dev]) {
    HIP_TRY(c, hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, T::LDS_BYTES));
    int n = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)k, DWPW_THREADS, T::LDS_BYTES));
    per_cu[dev] = std::max(n, 1);
  }
  const int n_tiles = a.tiles_x * a.tiles_y * a.batch;
  const int force = tuning("int8_fused", 1);   // (measurements: 2, 3, 4 = one, two, three workgroups per CU)
  const int wg_per_cu = force > 1 ? force - 1 : per_cu[dev];
  c->launch_tiles = n_tiles; c->launch_wgs = std::min(n_tiles, c->num_cus * wg_per_cu);
  c->launch_block = 1000 * G + 100 * (STEM ? 1 : 0) + 10 * (POOL ? 1 : 0) + EPI;   // (spvo_profile_stage_fused)
  hipLaunchKernelGGL(k, dim3(c->launch_wgs), dim3(DWPW_THREADS), T::LDS_BYTES, stream, a);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

static int launch_dwpw8(spvo_ctx *c, const Op &pw, int img0, int batch, hipStream_t stream) {
  const Op &dw = c->ops[pw.fused_dw];
  const Tensor &ti = c->tensors[dw.in], &tm = c->tensors[dw.out], &to = c->tensors[pw.out];
  DwPwArgs8 a;
  a.hp = ti.hp; a.wp = ti.wp; a.H = ti.H; a.W = ti.W;
  a.in = (const int8_t *)ring_ptr(c, ti, img0);
  a.in_per_image = ti.per_image * 4;
  a.dw_wsel = dw.d_wsel; a.dw_qm = dw.d_qm; a.dw_bias = dw.d_b; a.inv_s_dw = dw.inv_s_out;
  a.pw_w = pw.d_w8; a.pw_qm = pw.d_qm; a.pw_bias = pw.d_b; a.bn_scale = pw.d_bn_scale; a.bn_shift = pw.d_bn_shift; a.inv_s_out = pw.inv_s_out;
  a.out = (int8_t *)ring_ptr(c, to, img0);
  a.out_per_image = to.per_image * 4;
  a.out_hp = to.hp; a.out_wp = to.wp; a.cout = pw.cout; a.co_tiles = pw.cout / CO_TILE;
  a.tiles_x = (ti.W + 31) / 32; a.tiles_y = (ti.H + 7) / 8; a.batch = batch;
  const bool keep = c->heads_keep_raw;   // the synchronous entry points expose every tensor (spvo_debug_tensor): the skipped ones are stored too
  if (keep) { a.dbg_dw_out = (int8_t *)(tm.d + (size_t)img0 * tm.per_image); a.dbg_c16_per_image = tm.per_image * 4; }
  const bool pool = pw.flags & FLAG_POOL, bn = pw.flags & FLAG_BN;
  if (pw.fused_stem) {
    const Op &s0 = c->ops[0], &s1 = c->ops[1];
    const Tensor &t0 = c->tensors[s0.in], &t1 = c->tensors[s0.out];
    a.in = nullptr;
    a.in_f32 = ring_ptr(c, t0, img0);
    a.in_per_image = t0.per_image;
    a.w0 = s0.d_w; a.b0 = s0.d_b; a.w1 = s1.d_w; a.b1 = s1.d_b; a.bn1_scale = s1.d_bn_scale; a.bn1_shift = s1.d_bn_shift; a.inv_s_stem = s1.inv_s_out;
    if (keep) { a.dbg_stem_plane = t1.d + (size_t)img0 * t1.per_image; a.dbg_stem_plane_per_image = t1.per_image; a.dbg_stem_out = (int8_t *)(ti.d + (size_t)img0 * ti.per_image); }
    if (pool) return bn ? launch_dwpw8_instance<4, true, true, 1>(c, a, stream) : launch_dwpw8_instance<4, true, true, 0>(c, a, stream);
    return bn ? launch_dwpw8_instance<4, true, false, 1>(c, a, stream) : launch_dwpw8_instance<4, true, false, 0>(c, a, stream);
  }
  if (dw.cout == 64) {
    if (pool) return bn ? launch_dwpw8_instance<4, false, true, 1>(c, a, stream) : launch_dwpw8_instance<4, false, true, 0>(c, a, stream);
    return bn ? launch_dwpw8_instance<4, false, false, 1>(c, a, stream) : launch_dwpw8_instance<4, false, false, 0>(c, a, stream);
  }
  if (pool) return bn ? launch_dwpw8_instance<8, false, true, 1>(c, a, stream) : launch_dwpw8_instance<8, false, true, 0>(c, a, stream);
  return bn ? launch_dwpw8_instance<8, false, false, 1>(c, a, stream) : launch_dwpw8_instance<8, false, false, 0>(c, a, stream);
}

int launch_conv8(spvo_ctx *c, const Op &op, int img0, int batch, hipStream_t stream) {
  if (op.fused_dw >= 0) return launch_dwpw8(c, op, img0, batch, stream);
  const Tensor &ti = c->tensors[op.in];
  const Tensor &to = c->tensors[op.out];
  const float *tin = ring_ptr(c, ti, img0);
  float *tout = ring_ptr(c, to, img0);
  const bool relu = op.flags & FLAG_RELU, pool = op.flags & FLAG_POOL;
  if (op.type == OP_DWCONV) {
    dim3 grid((ti.W + 63) / 64, (ti.H + 3) / 4, batch * (op.cout / 16));
    if (relu) hipLaunchKernelGGL(dwconv3x3_i8_kernel<true>, grid, dim3(256), 0, stream, (const int8_t *)tin, (int8_t *)tout, op.d_wq32, op.d_qm, op.d_b, op.inv_s_out, op.cout / 16, ti.H, ti.W, ti.hp, ti.wp);
    else hipLaunchKernelGGL(dwconv3x3_i8_kernel<false>, grid, dim3(256), 0, stream, (const int8_t *)tin, (int8_t *)tout, op.d_wq32, op.d_qm, op.d_b, op.inv_s_out, op.cout / 16, ti.H, ti.W, ti.hp, ti.wp);
    HIP_TRY(c, hipGetLastError());
    return SPVO_OK;
  }
  if (op.cin == 1) {   // fp32 stem
    dim3 grid((ti.W + 63) / 64, (ti.H + 3) / 4, batch);
#define SPVO_STEM8(KS, RELU, OUTQ) hipLaunchKernelGGL((conv_first_i8_kernel<KS, RELU, OUTQ>), grid, dim3(256), 0, stream, tin, (void *)tout, op.d_w, op.d_b, \
                                                      op.d_bn_scale, op.d_bn_shift, op.inv_s_out, ti.H, ti.W, ti.hp, ti.wp, to.ch, op.out_c_off, op.cout)
    if (to.i8) {
      if (op.ks == 3) { if (relu) SPVO_STEM8(3, true, true); else SPVO_STEM8(3, false, true); }
      else            { if (relu) SPVO_STEM8(1, true, true); else SPVO_STEM8(1, false, true); }
    } else {
      if (op.ks == 3) { if (relu) SPVO_STEM8(3, true, false); else SPVO_STEM8(3, false, false); }
      else            { if (relu) SPVO_STEM8(1, true, false); else SPVO_STEM8(1, false, false); }
    }
#undef SPVO_STEM8
    HIP_TRY(c, hipGetLastError());
    return SPVO_OK;
  }
  ConvArgs8 a;
  a.in = (const int8_t *)tin; a.out = tout; a.wpack = op.d_w8; a.qm = op.d_qm; a.bias = op.d_b;
  a.bn_scale = op.d_bn_scale; a.bn_shift = op.d_bn_shift;
  a.inv_s_out = op.inv_s_out; a.s_res = op.s_res;
  a.H = ti.H; a.W = ti.W;
  a.in_hp = ti.hp; a.in_wp = ti.wp; a.in_gtot = ti.ch / 16; a.in_goff = op.in_c_off / 16;
  a.out_hp = to.hp; a.out_wp = to.wp; a.out_ctot = to.ch; a.out_coff = op.out_c_off;
  a.cout = op.cout; a.n_chunks = op.n_chunks; a.co_tiles = op.co_tiles;
  a.tiles_x = a.tiles_y = 0;
  a.batch = batch;
  a.in_groups = op.cin / 16;
  const int epi = (op.flags & FLAG_BN) ? 1 : (op.flags & FLAG_ADD) ? 2 : 0;
  if (epi == 2) a.residual = (const int8_t *)ring_ptr(c, c->tensors[op.residual], img0);
  const bool out_f32 = !to.i8;
  const int key = op.ks * 10000 + (op.ck / 16) * 1000 + op.wr * 100 + op.wc * 10 + (pool ? 1 : 0);   // ks, groups per chunk, wr, wc, pool: for the error text only (the table is with_tile_variant)
  return with_tile_variant<2, 4, 2>(op.ks, op.ck / 16, op.wr, op.wc, pool, [&](auto v) {
    using V = decltype(v);
    if constexpr (V::CKG == 2) {   // an odd number of 16-channel groups (int8_general): the instances whose last chunk has one group
      if (a.in_groups & 1) return launch_conv8_variant<V::KS, 2, V::WR, V::WC, V::POOL, true>(c, a, relu, out_f32, epi, stream);
    }
    return launch_conv8_variant<V::KS, V::CKG, V::WR, V::WC, V::POOL>(c, a, relu, out_f32, epi, stream);
  }, [&] { return fail(c, SPVO_ERR_INVALID, "no int8 conv kernel variant for key %d", key); });
}

// the fused tail of an INT8 engine (heads_i8.hip.h): ops head_start .. head_start + 2 in one launch
int launch_heads8(spvo_ctx *c, int batch, hipStream_t stream) {
  const Op &pb = c->ops[c->head_start], &db = c->ops[c->head_start + 1];
  const Tensor &ti = c->tensors[pb.in], &te = c->tensors[db.in], &tdet = c->tensors[pb.out], &traw = c->tensors[db.out], &tdesc = c->tensors[c->t_desc];
  const size_t plane = (size_t)ti.hp * ti.wp;
  HeadsArgs8 a;
  a.in_det = (const int8_t *)(ring_ptr(c, ti)) + (size_t)(pb.in_c_off / 16) * plane * 16; a.det_in_per_image = ti.per_image * 4;
  a.in_desc = (const int8_t *)(ring_ptr(c, te)) + (size_t)(db.in_c_off / 16) * plane * 16; a.desc_in_per_image = te.per_image * 4;
  a.in_hp = ti.hp; a.in_wp = ti.wp;
  a.wpack = c->d_heads_w8; a.qm = c->d_heads_qm; a.bias = c->d_heads_b;
  a.det = ring_ptr(c, tdet); a.det_per_image = tdet.per_image;
  a.desc_raw = c->heads_keep_raw ? ring_ptr(c, traw) : nullptr; a.raw_per_image = traw.per_image;
  a.desc = ring_ptr(c, tdesc);
  a.H = ti.H; a.W = ti.W; a.batch = batch;
  const double hbytes = batch * ((double)(pb.cin + db.cin) * ti.H * ti.W + (double)(pb.cout + (a.desc_raw ? 2 : 1) * db.cout) * ti.H * ti.W * 4) + (double)(pb.cout * pb.cin + db.cout * db.cin);
  ScopedStage st(c, stage_id(c, "heads"), (pb.flops_per_image + db.flops_per_image) * batch, hbytes, stream);
  const int ntiles = (batch * ti.H * ti.W + 31) / 32;
  c->heads_kind = 3; c->heads_tiles = c->heads_wgs = ntiles;   // (spvo_profile_stage_fused)
  hipLaunchKernelGGL(heads_i8_kernel<>, dim3(ntiles), dim3(HEADS8_THREADS), 0, stream, a);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

int launch_maxpool_i8(spvo_ctx *c, const Op &op, const Tensor &ti, const Tensor &to, const float *tin, float *tout, int batch, hipStream_t stream) {
  dim3 grid((to.W + 63) / 64, (to.H + 3) / 4, batch * (to.ch / 16));
  hipLaunchKernelGGL(maxpool2_i8_kernel<>, grid, dim3(256), 0, stream, (const int8_t *)tin, (int8_t *)tout, op.pool_m, to.H, to.W, ti.hp, ti.wp, to.hp, to.wp);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

void launch_unpad_c16(const Tensor &t, int batch, float *dst, hipStream_t stream) {
  hipLaunchKernelGGL(unpad_c16_kernel<>, dim3((t.W + 63) / 64, t.H, batch * t.ch), dim3(64), 0, stream, (const int8_t *)t.d, dst, t.ch, t.H, t.W, t.hp, t.wp);
}

}  // namespace spvo_int

