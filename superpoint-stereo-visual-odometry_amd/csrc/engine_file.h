// engine_file.h -- an engine file (SPVW0003; layout: spvo/weights.py) as records.  Plain C++17 without a HIP include: this is the one
// place of the library that reads bytes nobody vouches for, so it also builds into a stand-alone program that runs under the
// sanitizers on the CPU (tools/engine_file_check.cpp, tests/test_engine_file_cpu.py).  The plan loader (spvo_plan.hip) works on the
// records only.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/spvo.h"

namespace spvo_int {

enum { OP_CONV = 1, OP_MAXPOOL = 2, OP_L2NORM = 3, OP_DWCONV = 4 };
enum { FLAG_RELU = 1, FLAG_POOL = 2, FLAG_BN = 4, FLAG_ADD = 8 };

struct EngineTensor { uint32_t ch, level; };
// v: type, in, out, out_c_off, cin | in_c_off << 16, cout, ksize, flags, residual tensor, reserved[3]; the offsets count floats of the payload
struct EngineOp { uint32_t v[12]; uint64_t w_off, b_off, bn_off; };
static_assert(sizeof(EngineTensor) == 8 && sizeof(EngineOp) == 72, "record layout");

struct EngineFile {
  int status = SPVO_OK;              // SPVO_OK, or what spvo_load_weights answers with `error` as its text
  std::string error;
  uint32_t t_input = 0, t_det = 0, t_desc = 0;
  uint32_t precision = 0;            // 0 FP32, 1 FP16, 2 INT8
  uint32_t act_scale_off = 0;        // INT8: where the payload holds one activation scale per tensor
  std::vector<EngineTensor> tensors;
  std::vector<EngineOp> ops;         // in execution order (INT8: convPb moved behind convDa, below)
  const float *payload = nullptr;    // n_payload floats inside the caller's bytes
  uint64_t n_payload = 0;
};

// The records of the file in `data` (4-byte aligned) for a network `H` rows high; `path` is for the texts.  Everything that can be
// checked on the file alone is checked here, BEFORE the loaded plan is dropped: a truncated or corrupt file leaves the engine that was
// loaded before in place.  Ids are compared as unsigned (0xFFFFFFFF is not -1).  What depends on the payload's VALUES or on the
// engine kind (offsets of weights, activation scales, channel counts) is the plan loader's to check.
inline EngineFile parse_engine_file(const unsigned char *data, size_t size, int H, const char *path) {
  EngineFile f;
  auto refuse = [&](const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    f.status = SPVO_ERR_IO;
    f.error = buf;
    return std::move(f);
  };
  if (size < 48 || std::memcmp(data, "SPVW0003", 8) != 0) return refuse("%s is not a SPVW0003 weight file", path);
  uint32_t hdr[8];
  std::memcpy(hdr, data + 8, sizeof hdr);
  const uint32_t nt = hdr[0], no = hdr[1];
  size_t pos = 40;
  if (size < pos + (size_t)nt * 8 + (size_t)no * 72 + 8) return refuse("%s: truncated", path);
  if (hdr[5] > 2) return refuse("%s: unknown precision %u", path, hdr[5]);
  if (nt == 0 || nt > 65536 || no > 65536) return refuse("%s: implausible tensor / op count", path);
  if (hdr[2] >= nt || hdr[3] >= nt || hdr[4] >= nt) return refuse("%s: bad binding tensor ids", path);
  f.t_input = hdr[2]; f.t_det = hdr[3]; f.t_desc = hdr[4]; f.precision = hdr[5]; f.act_scale_off = hdr[6];
  f.tensors.resize(nt);
  std::memcpy(f.tensors.data(), data + pos, (size_t)nt * 8);
  pos += (size_t)nt * 8;
  for (const EngineTensor &t : f.tensors)   // a level is a halving of the network's size that leaves whole rows
    if (t.level > 3 || ((uint32_t)H >> t.level) << t.level != (uint32_t)H) return refuse("%s: bad tensor level", path);
  f.ops.resize(no);
  if (no) std::memcpy(f.ops.data(), data + pos, (size_t)no * 72);
  pos += (size_t)no * 72;
  for (uint32_t i = 0; i < no; ++i)
    if (f.ops[i].v[1] >= nt || f.ops[i].v[2] >= nt || f.ops[i].v[8] >= nt) return refuse("%s: op %u: bad tensor id", path, i);
  std::memcpy(&f.n_payload, data + pos, 8);
  pos += 8;
  if (f.n_payload > (size - pos) / 4) return refuse("%s: truncated payload", path);
  f.payload = (const float *)(data + pos);
  // INT8 engines: the ONNX graphs list the two branches one after the other -- convPa, convPb, convDa, convDb, L2 norm -- so the trailing run
  // of 1x1 layers the tail is made of (spvo_ctx::head_start) would be convDb + norm only.  convPb does not feed convDa: it moves behind it,
  // the tail becomes convPb, convDb, norm as in the VGG plan, and heads_i8_kernel runs it as one launch.  (Tensor ids do not change.)
  if (f.precision == 2 && no >= 5) {
    const EngineOp &A = f.ops[no - 5], &B = f.ops[no - 4], &C = f.ops[no - 3], &D = f.ops[no - 2], &N = f.ops[no - 1];
    const bool branches = A.v[0] == OP_CONV && A.v[6] == 3 && B.v[0] == OP_CONV && B.v[6] == 1 && B.v[1] == A.v[2] && C.v[0] == OP_CONV && C.v[6] == 3 &&
                          C.v[1] != B.v[2] && D.v[0] == OP_CONV && D.v[6] == 1 && D.v[1] == C.v[2] && N.v[0] == OP_L2NORM && N.v[1] == D.v[2] &&
                          !(C.v[7] & FLAG_ADD) && !(B.v[7] & FLAG_ADD);
    if (branches) std::swap(f.ops[no - 4], f.ops[no - 3]);
  }
  return f;
}

}  // namespace spvo_int
