// spvo_plan.hip -- the plan loader: an engine file's records (engine_file.h) -> tensors, ops, repacked weights on the device, placement.
// spvo_load_weights, at the bottom, is the list of its steps.  What a convolution needs for ONE engine kind -- refusals, chunking, tile
// variant, packed weights -- is prepared beside that kind's launcher (spvo_net_f32 / _f16 / _s3 / _i8.hip: prepare_conv_*, fuse_tail_*);
// here is what every kind shares.  Part of the extern "C" shim declared in include/spvo.h.
#include "spvo_internal.hip.h"
#include "conv_mfma.hip.h"   // the padded-plane layout every engine kind shares (padded_h, padded_w, CO_TILE)

namespace spvo_int {

void free_plan(spvo_ctx *c) {
  seg_free_all(c);
  for (auto &t : c->tensors) {
    if (t.d) (void)hipFree(t.d);
    for (int r = 1; r < RING; ++r) if (t.dr[r]) (void)hipFree(t.dr[r]);
  }
  for (auto &o : c->ops) dev_free(o.d_w, o.d_b, o.d_bn_scale, o.d_bn_shift, o.d_w16, o.d_w8, o.d_ws3, o.d_wq32, o.d_wsel, o.d_qm, o.d_sched);
  dev_free(c->d_heads_w, c->d_heads_w8, c->d_heads_qm, c->d_heads_b);
  c->heads_fused = false;
  c->heads_kind = c->heads_tiles = c->heads_wgs = 0;
  c->tensors.clear(); c->ops.clear(); c->weights = false; c->fp16 = false; c->int8 = false; c->s3 = false;
}

// Variant choice for a layer.  3x3: every tile variant has a measured rate on perfectly divisible shapes
// (tools/conv_bench sweep, launched back to back; TFLOP/s on 256 CUs) -- the smaller tiles let 2-3 workgroups share
// a CU, whose staging, barriers and output bursts then hide under each other's matrix instructions -- and the
// layer's time is that rate applied to the padded work of the busiest CU: ceil(tiles / CUs) tiles of TH x TW pixels
// (the model reproduces the sweep's times within 4 %).  Chunks of 4 channels (3-4 workgroups per CU) measure a
// further 2-3 % faster in isolation but 4 % SLOWER inside the pipeline, where the chip is shared with the previous
// pair's post-processing and the solver (tools/tune_variants.sh), so they are not offered.
// 1x1: tile by padded work / grid fill.
int choose_variant(const spvo_ctx *c, Op &op, const Tensor &ti, bool split) {
  const int ks = op.ks, H = ti.H, W = ti.W, batch = c->cfg.max_batch, num_cus = c->num_cus, co_tiles = op.co_tiles = (op.cout + CO_TILE - 1) / CO_TILE;
  const bool pool = op.flags & FLAG_POOL;
  int ck = 0;
  struct Cand { int wr, wc, ck; double rate; };
  static const Cand k3_f32[] = {{2, 2, 8, 130.0}, {2, 1, 8, 135.0}, {1, 2, 8, 135.0}, {1, 1, 8, 133.0}};
  // split (bf16x3) kernels: the 8x64 tile reads the fewest operands per matrix instruction (14 ds_read_b128 per 24) and
  // measures 4-9 % faster per pixel than the others (conv1b 263 vs 281 us, conv2b 76 vs 83 us)
  static const Cand k3_s3[] = {{2, 2, 8, 108.0}, {2, 1, 8, 100.0}, {1, 2, 8, 97.0}, {1, 1, 8, 97.0}};
  const Cand *k3 = split ? k3_s3 : k3_f32;
  static const Cand k1[] = {{2, 2, 16, 1.0 / 1.00}, {1, 2, 16, 1.0 / 1.03}, {2, 1, 16, 1.0 / 1.03}, {1, 1, 16, 1.0 / 1.06}};
  const Cand *cands = ks == 3 ? k3 : k1;
  const int nc = 4;
  // tuning "conv_variant" = 10 * wr + wc (diagnostic; read when an engine is loaded): that tile for every layer where it is one of the
  // candidates below, so that a test can run each variant against the oracle; where it is not, and for any other value, the model decides
  auto offered = [&](const Cand &v) {
    if (pool && v.wr != 2) return false;             // a 2x2 pooling window lives in one wave
    return !(ks == 1 && !pool && v.wr == 2 && v.wc == 1);
  };
  const int forced = tuning("conv_variant", 0);
  bool forced_ok = false;
  for (int i = 0; i < nc; ++i) forced_ok |= offered(cands[i]) && 10 * cands[i].wr + cands[i].wc == forced;
  double best = 1e300;
  for (int i = 0; i < nc; ++i) {
    const Cand &v = cands[i];
    if (!offered(v) || (forced_ok && 10 * v.wr + v.wc != forced)) continue;
    const int th = 4 * v.wr, tw = 32 * v.wc;
    const int tx = (W + tw - 1) / tw, ty = (H + th - 1) / th;
    const long tiles = (long)tx * ty * co_tiles * batch;
    double cost;
    if (ks == 3) cost = (double)((tiles + num_cus - 1) / num_cus) * th * tw / v.rate;
    else cost = (double)tx * tw * ty * th / v.rate / std::min(1.0, (double)tiles / num_cus);
    if (cost < best) { best = cost; op.wr = v.wr; op.wc = v.wc; ck = v.ck; }
  }
  return ck;
}

int upload_stem(spvo_ctx *c, Op &op, const float *w, const float *b) {
  const int rc = upload(c, &op.d_w, w, (size_t)op.cout * op.ks * op.ks);
  return rc ? rc : upload(c, &op.d_b, b, (size_t)op.cout);
}

bool tail_is_plain(const spvo_ctx *c, int cin) {
  const Op &pb = c->ops[c->head_start], &db = c->ops[c->head_start + 1], &nm = c->ops[c->head_start + 2];
  return pb.type == OP_CONV && db.type == OP_CONV && nm.type == OP_L2NORM && pb.ks == 1 && db.ks == 1 && pb.flags == 0 && db.flags == 0 &&
         pb.cin == cin && db.cin == cin && pb.cout == 65 && db.cout == 256 && pb.out == c->t_det && pb.out_c_off == 0 &&
         db.out_c_off == 0 && nm.in == db.out && nm.out == c->t_desc && c->tensors[pb.in].level == 3 && c->tensors[db.in].level == 3;
}

namespace {

// 1. the file's bytes (a short read leaves none: not a weight file)
int read_engine_file(spvo_ctx *c, const char *path, std::vector<unsigned char> &buf) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return fail(c, SPVO_ERR_IO, "no such engine file: %s", path);  // nn.cpp:53-55
  std::fseek(f, 0, SEEK_END);
  const long sz = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  buf.resize((size_t)std::max(sz, 0L));
  const size_t got = std::fread(buf.data(), 1, buf.size(), f);
  std::fclose(f);
  if (got != buf.size()) buf.clear();
  return SPVO_OK;
}

// 2. the records as the context's tensors and ops
void build_tensors_and_ops(spvo_ctx *c, const EngineFile &f) {
  c->t_input = (int)f.t_input; c->t_det = (int)f.t_det; c->t_desc = (int)f.t_desc;
  c->fp16 = f.precision == 1;   // engine built for FP16 (engine_generation.py's --fp16; the file name says FP16, nn.cpp:44-49)
  c->int8 = f.precision == 2;   // INT8 engine (BASELINE config 5; no counterpart in the reference): calibrated activation scales in the file
  for (const EngineTensor &r : f.tensors) {
    Tensor t;
    t.ch = r.ch; t.level = r.level;
    t.H = c->H >> t.level; t.W = c->W >> t.level;
    t.hp = padded_h(t.H); t.wp = padded_w(t.W);
    c->tensors.push_back(t);
  }
  for (const EngineOp &r : f.ops) {
    Op op;
    op.type = r.v[0]; op.in = r.v[1]; op.out = r.v[2]; op.out_c_off = r.v[3];
    op.cin = r.v[4] & 0xFFFF; op.in_c_off = r.v[4] >> 16; op.cout = r.v[5]; op.ks = r.v[6]; op.flags = r.v[7];
    op.residual = r.v[8];
    if (op.type == OP_L2NORM) c->tensors[op.out].nhwc = true;
    c->ops.push_back(op);
  }
}

// 3. every tensor's storage class, per engine kind
int assign_storage(spvo_ctx *c, const EngineFile &f, const char *path) {
  const uint32_t nt = (uint32_t)c->tensors.size();
  if (c->int8) {
    if (f.act_scale_off + (uint64_t)nt > f.n_payload) return fail(c, SPVO_ERR_IO, "%s: activation scales out of range", path);
    for (uint32_t t = 0; t < nt; ++t) {
      c->tensors[t].scale = f.payload[f.act_scale_off + t];
      c->tensors[t].i8 = (c->tensors[t].ch % 16) == 0;   // fewer channels (mbv's stem): an fp32 plane
      if (!(c->tensors[t].scale > 0.f)) return fail(c, SPVO_ERR_IO, "%s: tensor %u has no activation scale", path, t);
    }
    c->tensors[c->t_input].i8 = c->tensors[c->t_det].i8 = c->tensors[c->t_desc].i8 = false;   // fp32 bindings
    for (const auto &op : c->ops) {
      if (op.type == OP_L2NORM) c->tensors[op.in].i8 = false;
      if (op.type == OP_MAXPOOL && !c->int8_general_req) return fail(c, SPVO_ERR_IO, "%s: INT8 engines have no stand-alone max-pool (squeeze graph)", path);
    }
  }
  if (c->fp16) {
    // half precision between the fp32 network input and the fp32 outputs (nn.cpp:117): every tensor but the input,
    // output_det, the raw descriptor map and output_desc is C8 fp16
    // (a tensor whose channel count is not a multiple of 8 -- mbv's one-channel stem -- stays an fp32 plane that
    // holds fp16 values)
    for (auto &t : c->tensors) t.f16 = (t.ch % 8) == 0;
    c->tensors[c->t_input].f16 = c->tensors[c->t_det].f16 = c->tensors[c->t_desc].f16 = false;
    for (const auto &op : c->ops)
      if (op.type == OP_L2NORM) c->tensors[op.in].f16 = false;
  }
  c->s3 = c->split_req && !c->fp16 && !c->int8;
  if (c->s3) {
    // split mode: every tensor between the fp32 network input and the fp32 outputs holds bf16 triples
    for (auto &t : c->tensors) t.s3 = true;
    c->tensors[c->t_input].s3 = c->tensors[c->t_det].s3 = c->tensors[c->t_desc].s3 = false;
    for (const auto &op : c->ops) {
      if (op.type == OP_L2NORM) c->tensors[op.in].s3 = false;
      if (op.type != OP_CONV && op.type != OP_L2NORM) return fail(c, SPVO_ERR_IO, "%s: the split-fp32 mode covers convolution + L2-norm graphs (VGG SuperPoint) only", path);
    }
    for (const auto &t : c->tensors) if (t.s3 && (t.ch % 8)) return fail(c, SPVO_ERR_IO, "%s: split-fp32 mode: a %d-channel tensor", path, t.ch);
  }
  return SPVO_OK;
}

// 4. The network's tail end -- the trailing run of unpooled 1x1 convolutions and the L2 normalisation: convPb, convDb + norm --
// is tiny and launch-bound (64 us for 2.2 GFLOP); a submission runs it on the tail stream, where it fills the CUs the next
// pair's trunk leaves idle, instead of on the network stream, which is the one that limits the frame rate.
void find_heads(spvo_ctx *c) {
  c->head_start = c->ops.size();
  if (!tuning("heads_split", 1)) return;   // 0: the heads are ordinary layers of the trunk (no separate placement)
  while (c->head_start > 0) {
    const Op &o = c->ops[c->head_start - 1];
    const bool head = o.type == OP_L2NORM || (o.type == OP_CONV && o.ks == 1 && !(o.flags & FLAG_POOL) && o.cin > 1);
    if (!head) break;
    --c->head_start;
  }
}

// 5. allocate activations (padded planes stay zero outside the interior for ever)
int alloc_activations(spvo_ctx *c) {
  for (size_t ti = 0; ti < c->tensors.size(); ++ti) {
    Tensor &t = c->tensors[ti];
    t.per_image = t.nhwc ? (size_t)t.H * t.W * t.ch : t.s3 ? (size_t)t.ch * t.hp * t.wp * 3 / 2 : (size_t)t.ch * t.hp * t.wp / (t.f16 ? 2 : t.i8 ? 4 : 1);
    // + 24 rows of slack behind the last plane: a 16-row Winograd tile (conv_wino4.hip.h) stages 18 halo rows from its first row
    // on, up to 8 more than a plane padded to a multiple of 8 (+ 2) holds -- rows that only feed outputs below the image, which
    // are never stored, but the last plane's would lie behind the allocation
    const size_t slack = t.nhwc ? 0 : (size_t)24 * t.wp;
    int rc = dev_alloc(c, &t.d, t.per_image * c->B + slack);
    if (rc) return rc;
    bool head_input = false;   // read by the head ops, which a submission runs on its tail stream while the next trunk already runs
    for (size_t q = c->head_start; q < c->ops.size(); ++q) head_input |= c->ops[q].in == (int)ti || ((c->ops[q].flags & FLAG_ADD) && c->ops[q].residual == (int)ti);
    if ((int)ti == c->t_det || (int)ti == c->t_desc || head_input) {   // what a submission's tail reads while the next network pass already runs
      t.dr[0] = t.d;
      for (int r = 1; r < RING; ++r)
        if ((rc = dev_alloc(c, &t.dr[r], t.per_image * c->B + slack))) return rc;
    }
  }
  return SPVO_OK;
}

// 6a. a depthwise 3x3 convolution
int prepare_dwconv(spvo_ctx *c, const EngineFile &f, unsigned i) {
  Op &op = c->ops[i];
  const EngineOp &r = f.ops[i];
  const Tensor &ti = c->tensors[op.in], &to = c->tensors[op.out];
  if (op.ks != 3 || op.cin != op.cout || op.in_c_off || op.out_c_off || ti.ch != op.cin || to.ch != op.cout || to.level != ti.level ||
      (op.flags & ~FLAG_RELU))
    return fail(c, SPVO_ERR_IO, "op %u: unsupported depthwise convolution", i);
  if (r.w_off + (uint64_t)op.cout * 9 > f.n_payload || r.b_off + op.cout > f.n_payload) return fail(c, SPVO_ERR_IO, "op %u: weights out of range", i);
  op.flops_per_image = 2.0 * ti.H * ti.W * op.cout * 9;
  if (c->fp16 && (!ti.f16 || !to.f16)) return fail(c, SPVO_ERR_IO, "op %u: depthwise convolution of an FP16 engine needs channel counts that are multiples of 8", i);
  if (c->int8) return prepare_dwconv_i8(c, i, f.payload + r.w_off, f.payload + r.b_off);
  std::vector<float> wdw(f.payload + r.w_off, f.payload + r.w_off + (size_t)op.cout * 9);
  if (c->fp16) for (auto &q : wdw) q = (float)(_Float16)q;
  return upload_stem(c, op, wdw.data(), f.payload + r.b_off);   // (the same two buffers: [cout][9] weights, bias)
}

// 6b. a convolution, the part every engine kind shares: the epilogues this library executes, the BatchNorm fold, ranges and levels, the
// sibling merge -- then the kind's own function
int prepare_conv(spvo_ctx *c, const EngineFile &f, unsigned i) {
  Op &op = c->ops[i];
  const EngineOp &r = f.ops[i];
  const Tensor &ti = c->tensors[op.in], &to = c->tensors[op.out];
  const uint64_t nfl = f.n_payload;
  const int taps = op.ks * op.ks;
  const bool bn = op.flags & FLAG_BN, add = op.flags & FLAG_ADD;
  if ((bn && (add || !(op.flags & FLAG_RELU))) || (add && (op.flags & FLAG_RELU)))
    return fail(c, SPVO_ERR_IO, "op %u: epilogue flags 0x%x are not a graph order this library executes", i, op.flags);
  if ((bn || add) && op.cin > 1 && op.ks != 1) return fail(c, SPVO_ERR_IO, "op %u: BatchNorm / residual epilogues exist for 1x1 convolutions only", i);
  if (add) {
    const Tensor &tr = c->tensors[op.residual];
    if (op.cin == 1 || tr.ch != op.cout || tr.level != ti.level || tr.nhwc || op.residual == op.out)
      return fail(c, SPVO_ERR_IO, "op %u: bad residual tensor", i);
  }
  if (bn) {
    // ONNX BatchNormalization, inference form, folded to one fma: scale = gamma / sqrt(var + eps)
    if (r.bn_off + 4ull * op.cout + 1 > nfl) return fail(c, SPVO_ERR_IO, "op %u: BatchNorm parameters out of range", i);
    const int co_pad = ((op.cout + CO_TILE - 1) / CO_TILE) * CO_TILE;
    const float *q = f.payload + r.bn_off;
    std::vector<float> sc(co_pad, 0.f), sh(co_pad, 0.f);
    for (int o = 0; o < op.cout; ++o) {
      const double k = (double)q[o] / std::sqrt((double)q[3 * op.cout + o] + (double)q[4 * op.cout]);
      sc[o] = (float)k;
      sh[o] = (float)((double)q[op.cout + o] - (double)q[2 * op.cout + o] * k);
    }
    if (c->int8 && to.i8 && !add) {   // INT8 engines: the chain's last affine absorbs 1 / s_out (oracle/net_int8.py: FOLDING), one fp32 multiply per constant
      const float inv = 1.f / to.scale;
      for (int o = 0; o < op.cout; ++o) { sc[o] = sc[o] * inv; sh[o] = sh[o] * inv; }
    }
    int rc = upload(c, &op.d_bn_scale, sc);
    if (rc || (rc = upload(c, &op.d_bn_shift, sh))) return rc;
  }
  if (op.ks != 1 && op.ks != 3) return fail(c, SPVO_ERR_IO, "op %u: kernel size %d", i, op.ks);
  if (r.w_off + (uint64_t)op.cout * op.cin * taps > nfl || r.b_off + op.cout > nfl) return fail(c, SPVO_ERR_IO, "op %u: weights out of range", i);
  if (op.in_c_off + op.cin > ti.ch || op.out_c_off + op.cout > to.ch) return fail(c, SPVO_ERR_IO, "op %u: channel slice out of range", i);
  const bool pool = op.flags & FLAG_POOL;
  if (to.level != ti.level + (pool ? 1 : 0)) return fail(c, SPVO_ERR_IO, "op %u: level mismatch", i);
  if (pool && ((ti.H | ti.W) & 1)) return fail(c, SPVO_ERR_IO, "op %u: pooling an odd-sized map", i);
  op.flops_per_image = 2.0 * ti.H * ti.W * op.cout * op.cin * taps;
  const float *w = f.payload + r.w_off;
  const float *b = f.payload + r.b_off;
  // Sibling 3x3 layers (same input slice, same flags, adjacent output channel ranges of one tensor -- the two heads' first
  // convolutions convPa / convDa write channels 0..255 and 256..511 of one tensor) run as ONE layer with the output
  // channels concatenated: one launch instead of two, and 480 workgroups on 256 CUs instead of twice 240.
  std::vector<float> wcat, bcat;
  if (!c->s3 && op.ks == 3 && op.cin > 1 && !bn && !add && !pool && (op.cout % CO_TILE) == 0 && i + 1 < f.ops.size() &&
      tuning("merge_siblings", 1)) {
    Op &nx = c->ops[i + 1];
    const EngineOp &rn = f.ops[i + 1];
    if (nx.type == OP_CONV && nx.in == op.in && nx.in_c_off == op.in_c_off && nx.cin == op.cin && nx.ks == op.ks && nx.flags == op.flags &&
        nx.out == op.out && nx.out_c_off == op.out_c_off + op.cout && nx.out_c_off + nx.cout <= to.ch &&
        rn.w_off + (uint64_t)nx.cout * nx.cin * taps <= nfl && rn.b_off + nx.cout <= nfl) {
      wcat.assign(w, w + (size_t)op.cout * op.cin * taps);
      wcat.insert(wcat.end(), f.payload + rn.w_off, f.payload + rn.w_off + (size_t)nx.cout * nx.cin * taps);
      bcat.assign(b, b + op.cout);
      bcat.insert(bcat.end(), f.payload + rn.b_off, f.payload + rn.b_off + nx.cout);
      w = wcat.data();
      b = bcat.data();
      op.cout += nx.cout;
      op.flops_per_image = 2.0 * ti.H * ti.W * op.cout * op.cin * taps;
      nx.merged = true;
    }
  }
  return c->int8 ? prepare_conv_i8(c, i, w, b) : c->fp16 ? prepare_conv_f16(c, i, w, b) : c->s3 ? prepare_conv_s3(c, i, w, b) : prepare_conv_f32(c, i, w, b);
}

// 6. every op: its stage (they keep the plan's order in spvo_profile_get), its checks, its weights on the device
int prepare_ops(spvo_ctx *c, const EngineFile &f) {
  for (unsigned i = 0; i < c->ops.size(); ++i) {
    Op &op = c->ops[i];
    const Tensor &ti = c->tensors[op.in], &to = c->tensors[op.out];
    const char *kind = op.type == OP_DWCONV ? "dwconv" : op.type == OP_CONV ? "conv" : op.type == OP_MAXPOOL ? "pool" : op.type == OP_L2NORM ? "l2norm" : nullptr;
    if (!kind) return fail(c, SPVO_ERR_IO, "op %u: unknown type %d", i, op.type);
    char name[64];
    std::snprintf(name, sizeof name, "%s:%u", kind, i);
    op.stage = stage_id(c, name);
    int rc = SPVO_OK;
    if (op.type == OP_DWCONV) rc = prepare_dwconv(c, f, i);
    else if (op.type == OP_CONV && !op.merged) rc = prepare_conv(c, f, i);
    else if (op.type == OP_MAXPOOL && c->int8) rc = prepare_maxpool_i8(c, i);   // (reached in the int8_general mode only: assign_storage)
    else if (op.type == OP_MAXPOOL && (to.level != ti.level + 1 || to.ch != ti.ch)) rc = fail(c, SPVO_ERR_IO, "op %u: bad pool", i);
    else if (op.type == OP_L2NORM && (ti.ch != 256 || to.ch != 256 || ti.level != 3)) rc = fail(c, SPVO_ERR_IO, "op %u: descriptor tail must be 256 channels at 1/8", i);
    if (rc) return rc;
  }
  return SPVO_OK;
}

// 7. The tail of the SuperPoint graphs -- convPb 256 -> 65, convDb 256 -> 256 (both 1x1, plain, reading two channel ranges of one
// tensor or two tensors), L2 normalisation -- as ONE launch instead of three; tuning "heads_fused" = 0 keeps the plan's ops.
int fuse_tail(spvo_ctx *c, const EngineFile &f) {
  if (c->s3 || c->head_start + 3 != c->ops.size() || !tuning("heads_fused", 1)) return SPVO_OK;
  const EngineOp &rp = f.ops[c->head_start], &rd = f.ops[c->head_start + 1];
  return c->int8 ? fuse_tail_i8(c, f.payload, rp, rd) : fuse_tail_f32(c, f.payload, rp, rd);
}

// 9. placement: what runs where, from the finished plan
void place(spvo_ctx *c) {
  Op *best = nullptr;   // mark the dominant layer
  for (auto &o : c->ops) if (o.type == OP_CONV && (!best || o.flops_per_image > best->flops_per_image)) best = &o;
  if (best) best->dominant = true;
  // a submission's preprocess inside the first layer's launch (conv_first_pre.hip.h): FP32 engines whose first op is the plain 3x3 layer on the input plane
  const Op &o0 = c->ops[0];
  c->pre_fused = !c->fp16 && !c->int8 && !c->s3 && c->head_start >= 1 && o0.type == OP_CONV && o0.cin == 1 && o0.ks == 3 && o0.in == c->t_input && !o0.d_bn_scale &&
                 !(o0.flags & (FLAG_POOL | FLAG_ADD)) && !c->tensors[o0.out].nhwc && (c->W % 8) == 0 && tuning("preprocess_fused", 1) != 0;
  // one tail stream, or two when the caller says so (tuning "tail_streams" = 2: spvo_detect.hip; only with nothing in flight -- the parity
  // of a submission's set selects its stream)
  if (c->pendq.empty()) c->tail_streams = tuning("tail_streams", 0) == 2 ? 2 : 1;
  // where a submission's heads run (spvo_detect.hip): behind the trunk on the network stream when most of the trunk's work is in
  // launches of one 512-thread workgroup per CU (conv_wino4.hip.h), beside which they would starve; on the tail stream otherwise
  double all = 0, big = 0;
  for (const auto &o : c->ops) if (o.type == OP_CONV) { all += o.flops_per_image; if (o.wino4) big += o.flops_per_image; }
  c->heads_on_net = big > 0.8 * all;   // VGG fp32 at 360x1176: 0.95 (on the network stream: 1308 against 1260 frames/s); sp_squeeze: 0.66 (tail stream: 1286 against 1248)
  c->use_graphs = tuning("graphs", 1) == 2 || ((c->fp16 || c->int8) && tuning("graphs", 1) != 0);   // launch segments as HIP graphs: where the host bounds the frame loop
}

// 10. the bindings are SuperPoint's: a one-channel image in, 65 detector planes and a dense descriptor map at 1/8 out
int check_bindings(spvo_ctx *c, const char *path) {
  const Tensor &td = c->tensors[c->t_det];
  const Tensor &ts = c->tensors[c->t_desc];
  if (td.ch != 65 || td.level != 3 || td.nhwc || !ts.nhwc || c->tensors[c->t_input].ch != 1 || c->tensors[c->t_input].level != 0)
    return fail(c, SPVO_ERR_IO, "%s: unexpected output tensors", path);
  return SPVO_OK;
}

}  // namespace
}  // namespace spvo_int

extern "C" int spvo_load_weights(spvo_ctx *c, const char *path) {
  if (!c || !path) return fail(c, SPVO_ERR_INVALID, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  std::vector<unsigned char> bytes;
  int rc = read_engine_file(c, path, bytes);
  if (rc) return rc;
  const EngineFile f = parse_engine_file(bytes.data(), bytes.size(), c->H, path);
  if (f.status) return fail(c, f.status, "%s", f.error.c_str());
  if (!c->pendq.empty()) return fail(c, SPVO_ERR_STATE, "detector submissions are in flight");
  free_plan(c);   // from here on a failure (device allocation, unsupported layer) leaves the context without an engine
  build_tensors_and_ops(c, f);
  if ((rc = assign_storage(c, f, path))) return rc;
  find_heads(c);
  if ((rc = alloc_activations(c))) return rc;
  if ((rc = prepare_ops(c, f))) return rc;
  if ((rc = fuse_tail(c, f))) return rc;
  if (c->int8 && tuning("int8_fused", 1)) plan_int8_fusion(c);
  place(c);
  if ((rc = check_bindings(c, path))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->weights = true;
  return SPVO_OK;
}
