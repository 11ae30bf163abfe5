"""Engine files that spvo_load_weights refuses, one defect each, with the status and a piece of the text the library answers
(tests/test_gpu_engine_file.py; the file-level rows also go through the stand-alone parser, tests/test_engine_file_cpu.py).

A case is a small seeded plan -- three to six ops, 8 .. 64 channels -- for a 64 x 96 network, saved with spvo.weights.save and then
broken in ONE place: one field of one op or tensor before it is saved, or a few bytes of the saved file.  `level` says where the
loader notices:

  "file"   checked on the file's bytes alone, before the loaded plan is dropped (csrc/engine_file.h): the engine loaded before stays
  "late"   checked while the plan is built: the context is left without an engine

BASE, unbroken, is itself a case: it loads at every precision up to the last check and is refused there, because its outputs are
not SuperPoint's.  GOOD is the smallest graph the library accepts (a stem, three pooling steps, the two heads, the L2 norm).
"""
import struct
from typing import Callable, NamedTuple, Optional

import numpy as np

from spvo import weights as W

NET_H, NET_W = 64, 96
IO, STATE = -3, -4                 # SPVO_ERR_IO, SPVO_ERR_STATE (include/spvo.h)
R, P, BN, ADD = W.FLAG_RELU, W.FLAG_POOL, W.FLAG_BN, W.FLAG_ADD


def conv(src, dst, cin, cout, k, flags=R, out_off=0, in_off=0, res=0, type_=W.OP_CONV):
    return dict(type=type_, src=src, dst=dst, cin=cin, cout=cout, k=k, flags=flags, out_off=out_off, in_off=in_off, res=res)


def dwconv(src, dst, ch, flags=R):
    return conv(src, dst, ch, ch, 3, flags, type_=W.OP_DWCONV)


def pool(src, dst, ch):
    return conv(src, dst, ch, ch, 0, 0, type_=W.OP_MAXPOOL)


def norm(src, dst, ch):
    return conv(src, dst, ch, ch, 0, 0, type_=W.OP_L2NORM)


def make_plan(tensors, ops, det, desc, seed=7):
    """tensors: (channels, level) each, tensor 0 the input; ops: conv() / dwconv() / pool() / norm() records; det, desc: the output bindings"""
    rng = np.random.RandomState(seed)
    p = W.Plan()
    for ch, lvl in tensors:
        p.add_tensor(ch, lvl)
    for o in ops:
        op = W.Op(o["type"], o["src"], o["dst"], o["out_off"], o["cin"], o["cout"], o["k"], o["flags"])
        op.in_c_off, op.residual = o["in_off"], o["res"]
        if o["type"] in (W.OP_CONV, W.OP_DWCONV):
            fan = (1 if o["type"] == W.OP_DWCONV else o["cin"]) * o["k"] * o["k"]
            op.weight = (rng.randn(o["cout"], fan) * np.sqrt(2.0 / fan)).astype(np.float32)
            op.bias = (rng.randn(o["cout"]) * 0.05).astype(np.float32)
            if o["flags"] & BN:
                c = o["cout"]
                op.bn = np.concatenate([rng.uniform(0.7, 1.3, c), rng.uniform(0.0, 0.2, c), rng.uniform(0.0, 0.3, c), rng.uniform(0.6, 1.4, c), [1e-5]]).astype(np.float32)
        p.ops.append(op)
    p.input_tensor, p.det_tensor, p.desc_tensor = 0, det, desc
    p.act_scales = np.full(len(tensors), 0.05, np.float32)   # (only an INT8 file carries them)
    return p


# input -> 3x3 stem -> pooled 3x3 -> 1x1 -> linear 3x3 into the (wrong) output binding: channel counts every precision's chunking takes
BASE_TENSORS = [(1, 0), (32, 0), (64, 1), (64, 1), (32, 1)]
BASE_OPS = [conv(0, 1, 1, 32, 3), conv(1, 2, 32, 64, 3, R | P), conv(2, 3, 64, 64, 1), conv(3, 4, 64, 32, 3, 0)]


def base(tensors=None, ops=None, det=None, desc=None):
    """BASE with some tensors / ops replaced ({index: record}) or appended (index = the next one)"""
    t, o = list(BASE_TENSORS), [dict(x) for x in BASE_OPS]
    for i, v in sorted((tensors or {}).items()):
        t[i:i + 1] = [v]
    for i, v in sorted((ops or {}).items()):
        o[i:i + 1] = [v]
    return make_plan(t, o, len(BASE_TENSORS) - 1 if det is None else det, len(BASE_TENSORS) - 1 if desc is None else desc)


def good():
    tensors = [(1, 0), (16, 0), (16, 1), (16, 2), (32, 3), (W.DET_CHANNELS, 3), (W.DESC_CHANNELS, 3), (W.DESC_CHANNELS, 3)]
    ops = [conv(0, 1, 1, 16, 3), pool(1, 2, 16), pool(2, 3, 16), conv(3, 4, 16, 32, 3, R | P), conv(4, 5, 32, W.DET_CHANNELS, 1, 0),
           conv(4, 6, 32, W.DESC_CHANNELS, 1, 0), norm(6, 7, W.DESC_CHANNELS)]
    return make_plan(tensors, ops, 5, 7, seed=11)


# ---- the saved file (layout: spvo/weights.py)
HDR_NT, HDR_NO, HDR_INPUT, HDR_DET, HDR_DESC, HDR_PRECISION, HDR_ACT_OFF = (8 + 4 * i for i in range(7))
OP_IN, OP_W_OFF, OP_BN_OFF = 4, 48, 64      # byte offsets inside a 72-byte op record


def u32(offset, value):
    def patch(b):
        return b[:offset] + struct.pack("<I", value) + b[offset + 4:]
    return patch


def tensor_field(index, field, value):      # field 0 = channels, 1 = level
    return u32(40 + 8 * index + 4 * field, value)


def op_bytes(index, offset, fmt, value):
    def patch(b):
        (nt,) = struct.unpack_from("<I", b, HDR_NT)
        at = 40 + 8 * nt + 72 * index + offset
        return b[:at] + struct.pack(fmt, value) + b[at + struct.calcsize(fmt):]
    return patch


def records_end(b):
    nt, no = struct.unpack_from("<2I", b, HDR_NT)
    return 40 + 8 * nt + 72 * no


class Case(NamedTuple):
    name: str
    engine: str                              # "FP32", "FP16", "INT8", or "SPLIT": an FP32 file loaded with spvo_set_fp32_split
    level: str                               # "file" | "late"
    plan: Callable[[], W.Plan]
    patch: Optional[Callable[[bytes], bytes]]
    code: int
    text: str                                # part of the library's text


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


def _edit(make, fn):
    def build():
        p = make()
        fn(p)
        return p
    return build


def _op(i, **kw):
    """BASE with fields of op i's Plan record changed (the weights stay as they are)"""
    return _edit(base, lambda p: _set(p.ops[i], **kw))


FILE_CASES = [
    Case("short file", "FP32", "file", base, lambda b: b[:40], IO, "is not a SPVW0003 weight file"),
    Case("bad magic", "FP32", "file", base, lambda b: b"SPVW0002" + b[8:], IO, "is not a SPVW0003 weight file"),
    Case("records cut", "FP32", "file", base, lambda b: b[:records_end(b) + 4], IO, ": truncated"),
    Case("unknown precision", "FP32", "file", base, u32(HDR_PRECISION, 7), IO, "unknown precision 7"),
    Case("no tensors", "FP32", "file", base, u32(HDR_NT, 0), IO, "implausible tensor / op count"),
    Case("binding id", "FP32", "file", base, u32(HDR_DET, len(BASE_TENSORS)), IO, "bad binding tensor ids"),
    Case("binding id -1", "FP32", "file", base, u32(HDR_DESC, 0xFFFFFFFF), IO, "bad binding tensor ids"),
    Case("tensor level 4", "FP32", "file", base, tensor_field(2, 1, 4), IO, "bad tensor level"),
    Case("op input id", "FP32", "file", base, op_bytes(1, OP_IN, "<I", len(BASE_TENSORS)), IO, "op 1: bad tensor id"),
    Case("residual id", "FP32", "file", base, op_bytes(2, 32, "<I", 0xFFFFFFFF), IO, "op 2: bad tensor id"),
    Case("payload cut", "FP32", "file", base, lambda b: b[:-4], IO, "truncated payload"),
    Case("payload count", "FP32", "file", base, lambda b: b[:records_end(b)] + struct.pack("<Q", 1 << 62) + b[records_end(b) + 8:], IO, "truncated payload"),
]

LATE_CASES = [
    # ---- every precision reaches the last check with BASE
    Case("outputs fp32", "FP32", "late", base, None, IO, "unexpected output tensors"),
    Case("outputs fp16", "FP16", "late", base, None, IO, "unexpected output tensors"),
    Case("outputs int8", "INT8", "late", base, None, IO, "unexpected output tensors"),
    Case("outputs split", "SPLIT", "late", base, None, IO, "unexpected output tensors"),
    # ---- convolutions, the common part
    Case("BatchNorm without ReLU", "FP32", "late", _op(2, flags=BN), None, IO, "op 2: epilogue flags 0x4 are not a graph order"),
    Case("residual + ReLU", "FP32", "late", _op(2, flags=R | ADD), None, IO, "op 2: epilogue flags 0x9 are not a graph order"),
    Case("BatchNorm on a 3x3", "FP32", "late", _op(1, flags=R | BN), None, IO, "op 1: BatchNorm / residual epilogues exist for 1x1 convolutions only"),
    Case("residual channels", "FP32", "late", _op(2, flags=ADD, residual=4), None, IO, "op 2: bad residual tensor"),
    Case("BatchNorm offset", "FP32", "late", lambda: base(ops={2: conv(2, 3, 64, 64, 1, R | BN)}), op_bytes(2, OP_BN_OFF, "<Q", 1 << 40), IO, "op 2: BatchNorm parameters out of range"),
    Case("kernel size 5", "FP32", "late", _op(1, ksize=5), None, IO, "op 1: kernel size 5"),
    Case("weight offset", "FP32", "late", base, op_bytes(3, OP_W_OFF, "<Q", 1 << 40), IO, "op 3: weights out of range"),
    Case("input slice", "FP32", "late", _op(1, in_c_off=8), None, IO, "op 1: channel slice out of range"),
    Case("output slice", "FP32", "late", _op(2, out_c_off=16), None, IO, "op 2: channel slice out of range"),
    Case("pooled, same level", "FP32", "late", base, tensor_field(2, 1, 0), IO, "op 1: level mismatch"),
    Case("pool channels", "FP32", "late", lambda: base(tensors={5: (32, 2)}, ops={4: pool(3, 5, 64)}), None, IO, "op 4: bad pool"),
    Case("norm of 64 channels", "FP32", "late", lambda: base(tensors={5: (64, 1)}, ops={4: norm(3, 5, 64)}), None, IO, "op 4: descriptor tail must be 256 channels at 1/8"),
    Case("op type 9", "FP32", "late", _op(3, type=9), None, IO, "op 3: unknown type 9"),
    # ---- depthwise convolutions
    Case("depthwise pooled", "FP32", "late", lambda: base(ops={2: dwconv(2, 3, 64, R | P)}), None, IO, "op 2: unsupported depthwise convolution"),
    Case("depthwise weight offset", "FP32", "late", lambda: base(ops={2: dwconv(2, 3, 64)}), op_bytes(2, OP_W_OFF, "<Q", 1 << 40), IO, "op 2: weights out of range"),
    Case("depthwise fp16, 12 channels", "FP16", "late", lambda: base(tensors={1: (12, 0), 5: (12, 0)}, ops={0: conv(0, 1, 1, 12, 3), 1: dwconv(1, 5, 12)}), None, IO,
         "op 1: depthwise convolution of an FP16 engine needs channel counts that are multiples of 8"),
    Case("depthwise int8, 8 channels", "INT8", "late", lambda: base(tensors={1: (8, 0), 5: (8, 0)}, ops={0: conv(0, 1, 1, 8, 3), 1: dwconv(1, 5, 8)}), None, IO,
         "op 1: depthwise convolution of an INT8 engine needs channel counts that are multiples of 16"),
    # ---- FP32 engines
    Case("fp32 pooled stem", "FP32", "late", lambda: base(tensors={1: (32, 1)}, ops={0: conv(0, 1, 1, 32, 3, R | P), 1: conv(1, 2, 32, 64, 3)}), None, IO,
         "op 0: single-channel-input layers have no pooling / residual form"),
    Case("fp32 chunk", "FP32", "late", lambda: base(tensors={1: (12, 0)}, ops={0: conv(0, 1, 1, 12, 3), 1: conv(1, 2, 12, 64, 3, R | P)}), None, IO, "op 1: cin 12 is not a multiple of 8"),
    # ---- FP16 engines
    Case("fp16 storage", "FP16", "late", lambda: base(tensors={1: (12, 0)}, ops={0: conv(0, 1, 1, 12, 3), 1: conv(1, 2, 12, 64, 3, R | P)}), None, IO,
         "op 1: FP16 engine: a 12-channel input tensor stored as fp32"),
    Case("fp16 stem offset", "FP16", "late", _op(0, cout=16, out_c_off=4), None, IO, "op 0: unsupported single-channel-input layer for FP16"),
    Case("fp16 chunk", "FP16", "late", lambda: base(tensors={1: (8, 0)}, ops={0: conv(0, 1, 1, 8, 3), 1: conv(1, 2, 8, 64, 3, R | P)}), None, IO,
         "op 1: cin 8 / channel offset 0 do not fit the FP16 chunking (16)"),
    Case("fp16 cout", "FP16", "late", lambda: base(ops={2: conv(2, 3, 64, 12, 1)}), None, IO, "op 2: cout 12 / channel offset 0 are not multiples of 8"),
    Case("fp16 BatchNorm fp32 out", "FP16", "late", lambda: base(tensors={3: (12, 1)}, ops={2: conv(2, 3, 64, 12, 1, R | BN), 3: conv(2, 4, 64, 32, 3, 0)}), None, IO,
         "op 2: BatchNorm / residual epilogue with an fp32 output"),
    Case("fp16 residual fp32", "FP16", "late", lambda: base(tensors={5: (64, 1)}, ops={2: conv(2, 3, 64, 64, 1, ADD, res=5)}, det=5), None, IO,
         "op 2: residual tensor is not a 64-channel fp16 tensor"),
    Case("fp16 pooled fp32 out", "FP16", "late", lambda: base(tensors={2: (12, 1)}, ops={1: conv(1, 2, 32, 12, 3, R | P), 2: conv(1, 3, 32, 64, 1, R | P)}), None, IO,
         "op 1: pooled fp32 output"),
    # ---- INT8 engines
    Case("int8 scales offset", "INT8", "late", base, u32(HDR_ACT_OFF, 0xFFFFFFF0), IO, "activation scales out of range"),
    Case("int8 no scale", "INT8", "late", _edit(base, lambda p: p.act_scales.__setitem__(2, 0.0)), None, IO, "tensor 2 has no activation scale"),
    Case("int8 max-pool", "INT8", "late", lambda: base(tensors={5: (64, 2)}, ops={4: pool(3, 5, 64)}), None, IO, "INT8 engines have no stand-alone max-pool"),
    Case("int8 storage", "INT8", "late", lambda: base(tensors={1: (8, 0)}, ops={0: conv(0, 1, 1, 8, 3), 1: conv(1, 2, 8, 64, 3, R | P)}), None, IO,
         "op 1: INT8 engine: a 8-channel input tensor stored as fp32"),
    Case("int8 stem cout", "INT8", "late", _op(0, cout=8), None, IO, "op 0: unsupported single-channel-input layer for INT8"),
    Case("int8 chunk", "INT8", "late", lambda: base(tensors={1: (16, 0)}, ops={0: conv(0, 1, 1, 16, 3), 1: conv(1, 2, 16, 64, 3, R | P)}), None, IO,
         "op 1: cin 16 / channel offset 0 do not fit the INT8 chunking (32)"),
    Case("int8 cout", "INT8", "late", lambda: base(ops={2: conv(2, 3, 64, 24, 1)}), None, IO, "op 2: cout 24 / channel offset 0 are not multiples of 16"),
    Case("int8 pooled fp32 out", "INT8", "late", lambda: base(tensors={2: (24, 1)}, ops={1: conv(1, 2, 32, 24, 3, R | P), 2: conv(1, 3, 32, 64, 1, R | P)}), None, IO,
         "op 1: pooled / BatchNorm / residual layer with an fp32 output"),
    Case("int8 residual fp32", "INT8", "late", lambda: base(tensors={5: (64, 1)}, ops={2: conv(2, 3, 64, 64, 1, ADD, res=5)}, det=5), None, IO,
         "op 2: residual tensor is not a 64-channel int8 tensor"),
    # ---- FP32 engines in split mode
    Case("split max-pool", "SPLIT", "late", lambda: base(tensors={5: (64, 2)}, ops={4: pool(3, 5, 64)}), None, IO, "the split-fp32 mode covers convolution + L2-norm graphs"),
    Case("split 12 channels", "SPLIT", "late", lambda: base(tensors={3: (12, 1)}, ops={2: conv(2, 3, 64, 12, 1), 3: conv(2, 4, 64, 32, 3, 0)}), None, IO,
         "split-fp32 mode: a 12-channel tensor"),
    Case("split BatchNorm", "SPLIT", "late", lambda: base(ops={2: conv(2, 3, 64, 64, 1, R | BN)}), None, IO, "op 2: split-fp32 mode has no BatchNorm / residual epilogue"),
    Case("split reads a binding", "SPLIT", "late", lambda: base(tensors={5: (64, 1)}, ops={3: conv(5, 4, 64, 32, 3, 0)}, det=5), None, IO,
         "op 3: split-fp32 mode: unexpected storage of the input tensor"),
    Case("split cout", "SPLIT", "late", lambda: base(ops={2: conv(2, 3, 64, 12, 1)}), None, IO, "op 2: cout 12 / channel offset 0 are not multiples of 8"),
    Case("split pooled fp32 out", "SPLIT", "late", lambda: base(ops={2: conv(2, 3, 64, 64, 1, R), 3: conv(3, 4, 64, 32, 3, P)}, tensors={4: (32, 2)}), None, IO, "op 3: pooled fp32 output"),
    Case("split stem into a binding", "SPLIT", "late", lambda: base(det=1), None, IO, "op 0: unsupported single-channel-input layer for split-fp32 mode"),
    Case("split chunk", "SPLIT", "late", lambda: base(tensors={2: (8, 1)}, ops={1: conv(1, 2, 32, 8, 3, R | P), 2: conv(2, 3, 8, 64, 1)}), None, IO,
         "op 2: cin 8 / channel offset 0 do not fit the split-fp32 chunking (16)"),
]

CASES = FILE_CASES + LATE_CASES


def write(case, path):
    """the case's file at `path`"""
    W.save(case.plan(), path, "FP32" if case.engine == "SPLIT" else case.engine)
    if case.patch:
        with open(path, "rb") as fh:
            b = fh.read()
        with open(path, "wb") as fh:
            fh.write(case.patch(b))
