"""Seeded synthetic graphs that put every instance of the fused INT8 MobileNet block kernel, dwpw_i8_kernel<G, STEM, POOL, EPI>
(csrc/conv_i8_fused.hip.h), and the three fused tails (heads_fused_kernel<false / true>, heads_i8_kernel) in front of the oracle
(tests/test_gpu_fused_blocks.py; checked on the CPU by tests/test_fused_block_cases_cpu.py).

launch_dwpw8 (csrc/spvo_net_i8.hip) dispatches twelve instances: G = 4 or 8 groups of 16 depthwise channels, STEM (the sp_mbv1 stem,
ops 0 .. 3, in the same launch; G = 4 only), POOL, EPI (1: BatchNorm behind the pointwise layer).  Which blocks of a plan fuse is
decided by plan_int8_fusion, restated here as `fusion_table`.  One topology loads as an FP32, an FP16 and an INT8 engine: depthwise
3x3 layers of 64 or 128 channels, pointwise layers 64 / 128 -> 64 / 128.

Three kinds of graph:

  * block_plan(precision, stem_pool, stem_bn), four plans: the stem and a 64 -> 64 block behind it (the four STEM instances), then on
    levels 1 and 2 -- 52 x 100 and 26 x 50 pixels of a 104 x 200 input: a partial 8 x 32 tile in H and in W -- one block per
    (G, POOL, EPI), the four channel pairs among them, a depthwise layer without ReLU (not fusable: dwconv3x3_i8_kernel<false>) and a
    depthwise layer whose output a residual reads as well (two readers: the block stays unfused).  Every block's output is read by a
    later 3x3 layer (the next block's depthwise layer, or a dense one on level 3), so a store into the zero border of a padded plane
    changes a compared tensor.  The tail of the (pooled, no BatchNorm) plan reads its two branches from TWO tensors, the others from
    one merged 512-channel tensor as the VGG plan does.
  * long_block_plan(precision): the eight non-stem instances and a stem instance on LEVEL 0, for 120 x 392 x 2 images: 390 tiles of
    8 x 32 pixels per launch, more than one workgroup per CU has on any chip up to 389 CUs.  Its `part` argument builds a slice of it
    (the oracle's cost is the fused multiply-adds of the level-0 tensors in float64: the slices keep each case to a few seconds).
  * cvc.edge_plan, for the fused tails alone.

INT8 calibration: cvc.prepare takes the maximum of the fp32 graph's values, so its int8 tensors hold no 127 and the fminf(x, 127) arm
of the block kernel's packing would never be taken.  `prepare` here picks scales under which every int8 tensor saturates a little
(saturating_scales).
"""
import numpy as np

from spvo import weights as W
from tests import conv_variant_cases as cvc

EDGE_SIZES = cvc.EDGE_SIZES
LONG_SIZE = cvc.LONG_SIZE
TINY_SIZE = (16, 24)            # 2 x 3 cells: one partial tile of the fused tails holds both images
ENGINES = cvc.ENGINES
CALIB_SIZE = (48, 88)           # where the INT8 scales are found (saturating_scales)
SATURATION = 2e-3
STEMS = [(sp, sb) for sp in (False, True) for sb in (False, True)]     # (stem_pool, stem_bn)
INSTANCES = [(4, 1, p, e) for p in (0, 1) for e in (0, 1)] + [(g, 0, p, e) for g in (4, 8) for p in (0, 1) for e in (0, 1)]
LONG_PARTS = ("g4", "g8u", "g8p", "stem00", "stem10", "stem11")       # slices of long_block_plan, each with its own stem instance
assert len(INSTANCES) == 12


class _Builder(cvc._Builder):
    def dw(self, src, dst, ch, relu=True):
        rng = self.rng
        w = (rng.randn(ch, 1, 3, 3) * np.sqrt(2.0 / 9)).astype(np.float32)
        b = (rng.randn(ch) * 0.1).astype(np.float32)
        op = W.Op(W.OP_DWCONV, src, dst, 0, ch, ch, 3, W.FLAG_RELU if relu else 0, w, b)
        self.p.ops.append(op)
        return op

    def block(self, src, cout, pool=False, bn=False, relu_dw=True):
        """depthwise 3x3 (+ ReLU) and pointwise 1x1 + ReLU [+ BatchNorm] [+ pool] behind it, each into a tensor of its own; the output tensor"""
        cin, lvl = self.p.tensors[src]
        mid = self.tensor(cin, lvl)
        self.dw(src, mid, cin, relu=relu_dw)
        out = self.tensor(cout, lvl + (1 if pool else 0))
        self.conv(mid, out, 0, 0, cin, cout, 1, pool=pool, bn=bn)
        return out

    def stem(self, pool, bn):
        """ops 0 .. 3 of sp_mbv1: 3x3 1 -> 1 + ReLU on the input plane, 1x1 1 -> 64 + ReLU + BatchNorm, then a 64 -> 64 block"""
        t0 = self.p.input_tensor = self.tensor(1, 0)
        t1, t2 = self.tensor(1, 0), self.tensor(64, 0)
        self.conv(t0, t1, 0, 0, 1, 1, 3)
        self.p.ops[-1].weight = np.abs(self.p.ops[-1].weight)          # (a plane that is alive whatever the seed)
        self.conv(t1, t2, 0, 0, 1, 64, 1, bn=True)
        return self.block(t2, 64, pool=pool, bn=bn)

    def tail(self, srcs, two_tensors=False):
        """dense 3x3 readers of the level-3 tensors `srcs` into one tensor, then the heads: cvc's (one merged 512-channel tensor) or two
        256-channel tensors, one per branch"""
        T = self.tensor(64 * len(srcs), 3)
        self.fill([dict(src=s, in_off=0, cin=self.p.tensors[s][0], cout=64, k=3) for s in srcs], T)
        if not two_tensors:
            return self.heads(T, 64 * len(srcs))
        p = self.p
        tp, td = self.tensor(256, 3), self.tensor(256, 3)
        self.conv(T, tp, 0, 0, 64 * len(srcs), 256, 3)
        self.conv(T, td, 0, 0, 64 * len(srcs), 256, 3)
        tr = self.tensor(64, 3)                                         # 3x3 readers of both, compared like every tensor
        self.fill([dict(src=tp, in_off=192, cin=64, cout=32, k=3), dict(src=td, in_off=0, cin=64, cout=32, k=3)], tr)
        p.det_tensor = self.tensor(W.DET_CHANNELS, 3)
        raw = self.tensor(W.DESC_CHANNELS, 3)
        p.desc_tensor = self.tensor(W.DESC_CHANNELS, 3)
        self.conv(tp, p.det_tensor, 0, 0, 256, W.DET_CHANNELS, 1, relu=False)
        self.conv(td, raw, 0, 0, 256, W.DESC_CHANNELS, 1, relu=False)
        p.ops.append(W.Op(W.OP_L2NORM, raw, p.desc_tensor, 0, W.DESC_CHANNELS, W.DESC_CHANNELS))
        return p


def block_plan(precision, stem_pool, stem_bn, seed=21):
    b = _Builder(seed + 2 * int(stem_pool) + int(stem_bn))
    a64 = b.stem(stem_pool, stem_bn)
    if not stem_pool:                                    # level 0 -> 1 through one more pooled block
        a64 = b.block(a64, 64, pool=True, bn=not stem_bn)
    # level 1 (52 x 100 of 104 x 200)
    a128 = b.block(a64, 128, bn=True)                    # (4, 0, 0, 1)  64 -> 128
    a128b = b.block(a128, 128)                           # (8, 0, 0, 0) 128 -> 128
    c64 = b.block(a128b, 64, pool=True, bn=True)         # (8, 0, 1, 1) 128 -> 64
    a64b = b.block(a64, 64)                              # (4, 0, 0, 0)  64 -> 64: a second branch off a64
    c128 = b.block(a64b, 128, pool=True, bn=True)        # (4, 0, 1, 1)  64 -> 128
    # level 2 (26 x 50)
    d64 = b.block(c64, 64, pool=True)                    # (4, 0, 1, 0)  64 -> 64
    d128 = b.block(c128, 128, pool=True)                 # (8, 0, 1, 0) 128 -> 128
    c64b = b.block(c128, 64, bn=True)                    # (8, 0, 0, 1) 128 -> 64: a second branch off c128
    d64b = b.block(c64b, 64, pool=True, relu_dw=False)   # a linear depthwise layer: not fusable
    # a depthwise output with two readers (the pointwise layer and a residual): unfused, MobileNetV2's shape
    m = b.tensor(64, 2)
    b.dw(c64, m, 64)
    n = b.tensor(64, 2)
    b.conv(m, n, 0, 0, 64, 64, 1)
    o = b.tensor(64, 2)
    b.conv(n, o, 0, 0, 64, 64, 1, relu=False, res=m)
    d64c = b.block(o, 64, pool=True, bn=True)            # (4, 0, 1, 1) again, behind the residual
    p = b.tail([d64, d128, d64b, d64c], two_tensors=stem_pool and not stem_bn)
    p.precision = precision
    return p


def long_block_plan(precision, part=None, seed=31):
    """Level 0 at 120 x 392: `part` None is the whole graph -- the (4, 1, 0, 1) stem and the eight non-stem instances; "g4" its four
    G = 4 instances behind that stem, "g8u" / "g8p" the unpooled / pooled two of G = 8, "stem<pool><bn>" another stem instance and
    nothing else on level 0."""
    assert part is None or part in LONG_PARTS
    b = _Builder(seed + (0 if part is None else 1 + LONG_PARTS.index(part)))
    stem_pool, stem_bn = (part[4] == "1", part[5] == "1") if part and part.startswith("stem") else (False, True)
    x64 = b.stem(stem_pool, stem_bn)
    l1 = []
    if stem_pool:
        l1.append(x64)
    elif part and part.startswith("stem"):
        l1.append(b.block(x64, 64, pool=True, bn=True))
    if part in (None, "g4"):
        z64 = b.block(x64, 64, bn=True)                                 # (4, 0, 0, 1)
        l1.append(b.block(z64, 64, pool=True))                          # (4, 0, 1, 0)
        y64 = b.block(x64, 64)                                          # (4, 0, 0, 0)
        l1.append(b.block(y64, 64, pool=True, bn=True))                 # (4, 0, 1, 1)
    if part in (None, "g8u", "g8p"):
        x128 = b.block(x64, 128)                                        # (4, 0, 0, 0) with two tiles of output channels: the 128-channel tensor of the G = 8 blocks
    if part in (None, "g8u"):
        v64 = b.block(x128, 64, bn=True)                                # (8, 0, 0, 1)
        w64 = b.block(x128, 64)                                         # (8, 0, 0, 0)
        l1.append(b.block(v64, 64, pool=True, bn=True))                 # 3x3 readers of the unpooled blocks' outputs
        l1.append(b.block(w64, 64, pool=True))
    if part in (None, "g8p"):
        l1.append(b.block(x128, 64, pool=True))                         # (8, 0, 1, 0)
        l1.append(b.block(x128, 64, pool=True, bn=True))                # (8, 0, 1, 1)
    l3 = [b.block(b.block(t, 64, pool=True), 64, pool=True, bn=True) for t in l1]     # levels 1, 2 -> 3
    p = b.tail(l3)
    p.precision = precision
    return p


def saturating_scales(plan, rounds=8):
    """Activation scales of an INT8 plan under which EVERY int8 tensor of the int8 graph clips: at least SATURATION of its values sit at 127 (or -127, where no ReLU precedes).

    A percentile of the fp32 graph's values does not give that.  Measured on these plans: at 99.0 the first tensors saturate at 1 %,
    but a third of the deeper ones hold no 127 at all, and at 97.0 and 95.0 MORE tensors hold none -- what the layers in front clip
    away is exactly what would have driven a later tensor to the top of its range.  So the scales come from the int8 graph itself: start
    from the fp32 graph's 99.9th percentile, run the oracle, and shrink the scale of every tensor that saturates too little to the
    99.5th percentile of its nonzero values; repeat until none is left (a few rounds: a tensor's new scale changes what the layers
    behind it see).  Done once per plan at CALIB_SIZE on an input of its own (the inputs are noise, alike at every size); the CPU test
    asserts the outcome at every size of the cases."""
    from oracle import net_int8
    x = case_input(*CALIB_SIZE, 2, seed=6)
    s = net_int8.calibrate(plan, [x], percentile=99.9)
    for _ in range(rounds):
        plan.act_scales = s
        _, _, vals = net_int8.forward(plan, x, return_all=True)
        mag = {t: np.abs(v.astype(np.int32)) for t, v in vals.items() if v.dtype == np.int8}
        low = {t: a for t, a in mag.items() if (a == 127).mean() < SATURATION}
        if not low:
            return s
        s = s.copy()
        for t, a in low.items():
            s[t] = np.float32(s[t] * np.percentile(a[a > 0], 99.5) / 127.5)
    raise AssertionError(f"tensors {sorted(low)} still saturate below {SATURATION}")


_scales = {}


def prepare(plan, x=None, key=None):
    """INT8 plans: the saturating scales above (kept per `key`, the arguments the plan was built from)"""
    if plan.precision == "INT8":
        if key is None or key not in _scales:
            _scales[key] = saturating_scales(plan)
        plan.act_scales = _scales[key].copy()
    return plan


case_input = cvc.case_input
reference = cvc.reference


def fusion_table(plan, H=None, Wd=None):
    """plan_int8_fusion (csrc/spvo_net_i8.hip), restated: {index of a pointwise op behind a depthwise op: (G, STEM, POOL, EPI, co_tiles) of
    the block kernel's instance, or None where the two run layer by layer}.  H, Wd: the input size (a pooled block needs even sizes)."""
    from oracle.net_int8 import is_quantized
    ops = plan.ops
    readers = lambda t: sum((o.inp == t) + (bool(o.flags & W.FLAG_ADD) and o.residual == t) for o in ops)
    table = {}
    for i in range(len(ops) - 1):
        dw, pw = ops[i], ops[i + 1]
        if dw.type != W.OP_DWCONV or pw.type != W.OP_CONV or pw.ksize != 1 or pw.inp != dw.out:
            continue
        table[i + 1] = None
        if pw.in_c_off or pw.out_c_off or pw.cin != dw.cout:
            continue
        if dw.flags != W.FLAG_RELU or not (pw.flags & W.FLAG_RELU) or (pw.flags & W.FLAG_ADD):
            continue
        if not (is_quantized(plan, dw.inp) and is_quantized(plan, dw.out) and is_quantized(plan, pw.out)):
            continue
        if dw.cout not in (64, 128) or pw.cout not in (64, 128) or plan.tensors[pw.out][0] != pw.cout:
            continue
        if readers(dw.out) != 1 or dw.out in (plan.det_tensor, plan.desc_tensor):
            continue
        lvl = plan.tensors[dw.inp][1]
        if (pw.flags & W.FLAG_POOL) and H is not None and (((H >> lvl) | (Wd >> lvl)) & 1):
            continue
        stem = False
        if i == 2:
            s0, s1 = ops[0], ops[1]
            stem = (s0.type == W.OP_CONV and (s0.cin, s0.cout, s0.ksize, s0.flags) == (1, 1, 3, W.FLAG_RELU) and s0.inp == plan.input_tensor and
                    not is_quantized(plan, s0.out) and s1.type == W.OP_CONV and (s1.cin, s1.cout, s1.ksize, s1.flags) == (1, 64, 1, W.FLAG_RELU | W.FLAG_BN) and
                    s1.inp == s0.out and s1.out == dw.inp and not s1.out_c_off and dw.cout == 64 and readers(s0.out) == 1 and readers(s1.out) == 1)
        table[i + 1] = (dw.cout // 16, int(stem), int(bool(pw.flags & W.FLAG_POOL)), int(bool(pw.flags & W.FLAG_BN)), pw.cout // 64)
    return table


def fused_writes(plan, table=None):
    """the int8 tensors the fused launches of a plan write: each block's depthwise and pointwise outputs, and the stem's int8 output"""
    table = fusion_table(plan) if table is None else table
    out = set()
    for i, inst in table.items():
        if inst:
            out |= {plan.ops[i].out, plan.ops[i].inp} | ({plan.ops[i - 1].inp} if inst[1] else set())
    return out


def check_loader_rules(plan):
    """cvc.check_loader_rules for the dense layers, and the plan loader's rules for a depthwise layer (csrc/spvo_plan.hip, prepare_dwconv;
    csrc/spvo_net_i8.hip, prepare_dwconv_i8), restated"""
    cvc.check_loader_rules(plan)
    g = {"FP32": 1, "FP16": 8, "INT8": 16}[plan.precision]
    keep = {plan.input_tensor, plan.det_tensor, plan.desc_tensor} | {op.inp for op in plan.ops if op.type == W.OP_L2NORM}
    n = 0
    for i, op in enumerate(plan.ops):
        if op.type != W.OP_DWCONV:
            continue
        n += 1
        (ci, li), (co, lo) = plan.tensors[op.inp], plan.tensors[op.out]
        assert op.ksize == 3 and op.cin == op.cout == ci == co and li == lo and not op.in_c_off and not op.out_c_off, i
        assert not (op.flags & ~W.FLAG_RELU) and op.weight.shape == (op.cout, 1, 3, 3) and op.bias.shape == (op.cout,), i
        assert op.cout % g == 0 and op.inp not in keep and op.out not in keep and op.inp != op.out, i
    return n
