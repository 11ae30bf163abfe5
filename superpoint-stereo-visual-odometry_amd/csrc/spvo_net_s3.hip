// spvo_net_s3.hip -- FP32 engines in split mode (conv_bf16x3.hip.h): what the plan loader prepares of a layer, and the kernel launchers.
#include "spvo_internal.hip.h"
#include "conv_bf16x3.hip.h"

namespace spvo_int {

// ---------------------------------------------------------------- FP32 engines in split mode (bf16x3)
// what the plan loader prepares of a convolution (spvo_plan.hip); `ckg` groups of 8 channels per chunk: 1 for the 3x3 instances launch_conv_s3
// has, 2 for the 1x1 ones
int prepare_conv_s3(spvo_ctx *c, unsigned i, const float *w, const float *b) {
  Op &op = c->ops[i];
  const Tensor &ti = c->tensors[op.in], &to = c->tensors[op.out];
  const bool bn = op.flags & FLAG_BN, add = op.flags & FLAG_ADD, pool = op.flags & FLAG_POOL;
  if (bn || add) return fail(c, SPVO_ERR_IO, "op %u: split-fp32 mode has no BatchNorm / residual epilogue", i);
  if (ti.s3 != (op.cin != 1)) return fail(c, SPVO_ERR_IO, "op %u: split-fp32 mode: unexpected storage of the input tensor", i);
  if (to.s3 && ((op.cout % 8) || (op.out_c_off % 8))) return fail(c, SPVO_ERR_IO, "op %u: cout %d / channel offset %d are not multiples of 8", i, op.cout, op.out_c_off);
  if (!to.s3 && pool) return fail(c, SPVO_ERR_IO, "op %u: pooled fp32 output", i);
  if (op.cin == 1) {
    if (pool || !to.s3) return fail(c, SPVO_ERR_IO, "op %u: unsupported single-channel-input layer for split-fp32 mode", i);
    return upload_stem(c, op, w, b);
  }
  const int ckg = op.ks == 3 ? 1 : 2;
  if (op.cin % (8 * ckg) || op.in_c_off % 8) return fail(c, SPVO_ERR_IO, "op %u: cin %d / channel offset %d do not fit the split-fp32 chunking (%d)", i, op.cin, op.in_c_off, 8 * ckg);
  op.ck = 8 * ckg;
  op.n_chunks = op.cin / op.ck;
  choose_variant(c, op, ti, true);
  return upload(c, &op.d_ws3, pack_conv_weights_s3(w, b, op.cout, op.cin, op.ks, ckg));
}

template <int KS, int CKG, int WR, int WC, bool POOL, bool RELU, bool OUT_F32>
int launch_conv_s3_instance(spvo_ctx *c, const ConvArgsS3 &args, hipStream_t stream) {
  return launch_persistent_tiles<ConvTileS3<KS, CKG, WR, WC>, conv_s3_kernel<KS, CKG, WR, WC, POOL, RELU, OUT_F32>>(c, args, stream);
}

template <int KS, int CKG, int WR, int WC, bool POOL>
int launch_conv_s3_variant(spvo_ctx *c, const ConvArgsS3 &a, bool relu, bool out_f32, hipStream_t stream) {
  if constexpr (!POOL) {
    if (out_f32) return relu ? launch_conv_s3_instance<KS, CKG, WR, WC, false, true, true>(c, a, stream) : launch_conv_s3_instance<KS, CKG, WR, WC, false, false, true>(c, a, stream);
  }
  return relu ? launch_conv_s3_instance<KS, CKG, WR, WC, POOL, true, false>(c, a, stream) : launch_conv_s3_instance<KS, CKG, WR, WC, POOL, false, false>(c, a, stream);
}

int launch_conv_s3(spvo_ctx *c, const Op &op, int img0, int batch, hipStream_t stream) {
  const Tensor &ti = c->tensors[op.in];
  const Tensor &to = c->tensors[op.out];
  const float *tin = ring_ptr(c, ti, img0);
  float *tout = ring_ptr(c, to, img0);
  const bool relu = op.flags & FLAG_RELU, pool = op.flags & FLAG_POOL;
  if (op.cin == 1) {
    dim3 grid((ti.W + 63) / 64, (ti.H + 3) / 4, batch);
#define SPVO_FIRST_S3(KS, RELU) hipLaunchKernelGGL((conv_first_s3_kernel<KS, RELU>), grid, dim3(256), 0, stream, tin, (unsigned short *)tout, op.d_w, op.d_b, \
                                                   ti.H, ti.W, ti.hp, ti.wp, to.ch / 8, op.out_c_off / 8, op.cout)
    if (op.ks == 3) { if (relu) SPVO_FIRST_S3(3, true); else SPVO_FIRST_S3(3, false); }
    else            { if (relu) SPVO_FIRST_S3(1, true); else SPVO_FIRST_S3(1, false); }
#undef SPVO_FIRST_S3
    HIP_TRY(c, hipGetLastError());
    return SPVO_OK;
  }
  ConvArgsS3 a;
  a.in = (const unsigned short *)tin; a.out = tout; a.wpack = op.d_ws3;
  a.H = ti.H; a.W = ti.W;
  a.in_hp = ti.hp; a.in_wp = ti.wp; a.in_gtot = ti.ch / 8; a.in_goff = op.in_c_off / 8;
  a.out_hp = to.hp; a.out_wp = to.wp; a.out_ctot = to.ch; a.out_coff = op.out_c_off;
  a.cout = op.cout; a.n_chunks = op.n_chunks; a.co_tiles = op.co_tiles;
  a.tiles_x = a.tiles_y = 0;
  a.batch = batch;
  const bool out_f32 = !to.s3;
  const int key = op.ks * 1000 + op.wr * 100 + op.wc * 10 + (pool ? 1 : 0);   // for the error text only (the table is with_tile_variant)
  return with_tile_variant<1, 2, 0>(op.ks, op.ck / 8, op.wr, op.wc, pool, [&](auto v) {
    using V = decltype(v);
    return launch_conv_s3_variant<V::KS, V::CKG, V::WR, V::WC, V::POOL>(c, a, relu, out_f32, stream);
  }, [&] { return fail(c, SPVO_ERR_INVALID, "no split-fp32 conv kernel variant for key %d", key); });
}

void launch_unpad_s3(const Tensor &t, int batch, float *dst, hipStream_t stream) {
  hipLaunchKernelGGL(unpad_s3_kernel<>, dim3((t.W + 63) / 64, t.H, batch * t.ch), dim3(64), 0, stream, (const unsigned short *)t.d, dst, t.ch, t.H, t.W, t.hp, t.wp);
}

}  // namespace spvo_int

