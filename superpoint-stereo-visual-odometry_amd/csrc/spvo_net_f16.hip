// spvo_net_f16.hip -- FP16 engines (conv_f16.hip.h): what the plan loader prepares of a layer, and the kernel launchers.
#include "spvo_internal.hip.h"
#include "conv_f16.hip.h"

namespace spvo_int {

// ---------------------------------------------------------------- FP16 engines
// what the plan loader prepares of a convolution (spvo_plan.hip); `ckg` groups of 8 channels per chunk: the second digit of launch_conv16's keys
int prepare_conv_f16(spvo_ctx *c, unsigned i, const float *w, const float *b) {
  Op &op = c->ops[i];
  const Tensor &ti = c->tensors[op.in], &to = c->tensors[op.out];
  const bool bn = op.flags & FLAG_BN, add = op.flags & FLAG_ADD, pool = op.flags & FLAG_POOL;
  if (ti.f16 != (op.cin != 1)) return fail(c, SPVO_ERR_IO, "op %u: FP16 engine: a %d-channel input tensor stored as %s", i, op.cin, ti.f16 ? "fp16" : "fp32");
  if (op.cin == 1) {   // fp32 plane in: fp32 arithmetic on fp16-rounded weights, fp16 values out
    if (pool || add || (to.f16 && (op.out_c_off % 8))) return fail(c, SPVO_ERR_IO, "op %u: unsupported single-channel-input layer for FP16", i);
    std::vector<float> wr((size_t)op.cout * op.ks * op.ks);
    for (size_t q = 0; q < wr.size(); ++q) wr[q] = (float)(_Float16)w[q];
    return upload_stem(c, op, wr.data(), b);
  }
  const int ckg = (op.ks == 3 || op.cin % 32) ? 2 : 4;   // 16 channels per chunk; 32 for 1x1 layers when they divide
  if (op.cin % (8 * ckg) || op.in_c_off % 8) return fail(c, SPVO_ERR_IO, "op %u: cin %d / channel offset %d do not fit the FP16 chunking (%d)", i, op.cin, op.in_c_off, 8 * ckg);
  if (to.f16 && ((op.cout % 8) || (op.out_c_off % 8))) return fail(c, SPVO_ERR_IO, "op %u: cout %d / channel offset %d are not multiples of 8", i, op.cout, op.out_c_off);
  if ((bn || add) && !to.f16) return fail(c, SPVO_ERR_IO, "op %u: BatchNorm / residual epilogue with an fp32 output", i);
  if (add && (!c->tensors[op.residual].f16 || c->tensors[op.residual].ch != op.cout)) return fail(c, SPVO_ERR_IO, "op %u: residual tensor is not a %d-channel fp16 tensor", i, op.cout);
  if (!to.f16 && pool) return fail(c, SPVO_ERR_IO, "op %u: pooled fp32 output", i);
  op.ck = 8 * ckg;
  op.n_chunks = op.cin / op.ck;
  choose_variant(c, op, ti);
  return upload(c, &op.d_w16, pack_conv_weights_f16(w, b, op.cout, op.cin, op.ks, ckg));
}

template <int KS, int CKG, int WR, int WC, bool POOL, bool RELU, bool OUT_F32, int EPI = 0>
int launch_conv16_instance(spvo_ctx *c, const ConvArgs16 &args, hipStream_t stream) {
  return launch_persistent_tiles<ConvTile16<KS, CKG, WR, WC>, conv_f16_kernel<KS, CKG, WR, WC, POOL, RELU, OUT_F32, EPI>>(c, args, stream);
}

template <int KS, int CKG, int WR, int WC, bool POOL>
int launch_conv16_variant(spvo_ctx *c, const ConvArgs16 &a, bool relu, bool out_f32, hipStream_t stream) {
  if constexpr (!POOL) {
    if (out_f32) return relu ? launch_conv16_instance<KS, CKG, WR, WC, false, true, true>(c, a, stream) : launch_conv16_instance<KS, CKG, WR, WC, false, false, true>(c, a, stream);
  }
  return relu ? launch_conv16_instance<KS, CKG, WR, WC, POOL, true, false>(c, a, stream) : launch_conv16_instance<KS, CKG, WR, WC, POOL, false, false>(c, a, stream);
}

// MobileNet 1x1 layers of an FP16 engine: EPI 1 = ReLU, BatchNorm, ReLU (mbv1); EPI 2 = residual add, ReLU (mbv2)
template <int CKG, int WR, int WC, bool POOL>
int launch_conv16_epi(spvo_ctx *c, const ConvArgs16 &a, int epi, hipStream_t stream) {
  return epi == 1 ? launch_conv16_instance<1, CKG, WR, WC, POOL, true, false, 1>(c, a, stream)
                  : launch_conv16_instance<1, CKG, WR, WC, POOL, false, false, 2>(c, a, stream);
}

int launch_conv16(spvo_ctx *c, const Op &op, int img0, int batch, hipStream_t stream) {
  const Tensor &ti = c->tensors[op.in];
  const Tensor &to = c->tensors[op.out];
  const float *tin = ring_ptr(c, ti, img0);
  float *tout = ring_ptr(c, to, img0);
  const bool relu = op.flags & FLAG_RELU, pool = op.flags & FLAG_POOL;
  if (op.type == OP_DWCONV) {
    dim3 grid((ti.W + 63) / 64, (ti.H + 3) / 4, batch * (op.cout / 8));
    if (relu) hipLaunchKernelGGL(dwconv3x3_f16_kernel<true>, grid, dim3(256), 0, stream, (const _Float16 *)tin, (_Float16 *)tout, op.d_w, op.d_b, op.cout / 8, ti.H, ti.W, ti.hp, ti.wp);
    else hipLaunchKernelGGL(dwconv3x3_f16_kernel<false>, grid, dim3(256), 0, stream, (const _Float16 *)tin, (_Float16 *)tout, op.d_w, op.d_b, op.cout / 8, ti.H, ti.W, ti.hp, ti.wp);
    HIP_TRY(c, hipGetLastError());
    return SPVO_OK;
  }
  if (op.cin == 1) {
    dim3 grid((ti.W + 63) / 64, (ti.H + 3) / 4, batch);
    if (to.f16) {
#define SPVO_FIRST16(KS, RELU) hipLaunchKernelGGL((conv_first_f16_kernel<KS, RELU>), grid, dim3(256), 0, stream, tin, (_Float16 *)tout, op.d_w, op.d_b, \
                                                  op.d_bn_scale, op.d_bn_shift, ti.H, ti.W, ti.hp, ti.wp, to.ch / 8, op.out_c_off / 8, op.cout)
      if (op.ks == 3) { if (relu) SPVO_FIRST16(3, true); else SPVO_FIRST16(3, false); }
      else            { if (relu) SPVO_FIRST16(1, true); else SPVO_FIRST16(1, false); }
#undef SPVO_FIRST16
    } else {   // a stem with fewer than 8 channels stays an fp32 plane that holds fp16 values
#define SPVO_FIRST(KS, RELU) hipLaunchKernelGGL((conv_first_kernel<KS, RELU>), grid, dim3(256), 0, stream, tin, tout, op.d_w, op.d_b, \
                                                op.d_bn_scale, op.d_bn_shift, ti.H, ti.W, ti.hp, ti.wp, to.ch, op.out_c_off, op.cout, 1)
      if (op.ks == 3) { if (relu) SPVO_FIRST(3, true); else SPVO_FIRST(3, false); }
      else            { if (relu) SPVO_FIRST(1, true); else SPVO_FIRST(1, false); }
#undef SPVO_FIRST
    }
    HIP_TRY(c, hipGetLastError());
    return SPVO_OK;
  }
  ConvArgs16 a;
  a.in = (const _Float16 *)tin; a.out = tout; a.wpack = op.d_w16;
  a.H = ti.H; a.W = ti.W;
  a.in_hp = ti.hp; a.in_wp = ti.wp; a.in_gtot = ti.ch / 8; a.in_goff = op.in_c_off / 8;
  a.out_hp = to.hp; a.out_wp = to.wp; a.out_ctot = to.ch; a.out_coff = op.out_c_off;
  a.cout = op.cout; a.n_chunks = op.n_chunks; a.co_tiles = op.co_tiles;
  a.tiles_x = a.tiles_y = 0;
  a.batch = batch;
  const bool out_f32 = !to.f16;
  const int key = op.ks * 10000 + (op.ck / 8) * 1000 + op.wr * 100 + op.wc * 10 + (pool ? 1 : 0);   // ks, groups per chunk, wr, wc, pool: for the error text only (the table is with_tile_variant)
  const int epi = (op.flags & FLAG_BN) ? 1 : (op.flags & FLAG_ADD) ? 2 : 0;
  if (epi) {
    a.bn_scale = op.d_bn_scale; a.bn_shift = op.d_bn_shift;
    if (epi == 2) a.residual = (const _Float16 *)ring_ptr(c, c->tensors[op.residual], img0);
  }
  auto no_variant = [&] {
    return epi ? fail(c, SPVO_ERR_INVALID, "no fp16 conv kernel variant for key %d with epilogue %d", key, epi)
               : fail(c, SPVO_ERR_INVALID, "no fp16 conv kernel variant for key %d", key);
  };
  return with_tile_variant<2, 4, 2>(op.ks, op.ck / 8, op.wr, op.wc, pool, [&](auto v) {
    using V = decltype(v);
    if (!epi) return launch_conv16_variant<V::KS, V::CKG, V::WR, V::WC, V::POOL>(c, a, relu, out_f32, stream);
    if constexpr (V::KS == 1) return launch_conv16_epi<V::CKG, V::WR, V::WC, V::POOL>(c, a, epi, stream);   // (the 1x1 layers have the epilogue forms)
    else return no_variant();
  }, no_variant);
}

int launch_maxpool_f16(spvo_ctx *c, const Tensor &ti, const Tensor &to, const float *tin, float *tout, int batch, hipStream_t stream) {
  dim3 grid((to.W + 63) / 64, (to.H + 3) / 4, batch * (to.ch / 8));
  hipLaunchKernelGGL(maxpool2_f16_kernel<>, grid, dim3(256), 0, stream, (const _Float16 *)tin, (_Float16 *)tout, to.H, to.W, ti.hp, ti.wp, to.hp, to.wp);
  HIP_TRY(c, hipGetLastError());
  return SPVO_OK;
}

void launch_unpad_c8(const Tensor &t, int batch, float *dst, hipStream_t stream) {
  hipLaunchKernelGGL(unpad_c8_kernel<>, dim3((t.W + 63) / 64, t.H, batch * t.ch), dim3(64), 0, stream, (const _Float16 *)t.d, dst, t.ch, t.H, t.W, t.hp, t.wp);
}

}  // namespace spvo_int

