"""Cases for INT8 engines loaded in the "int8_general" mode (spvo_set_int8_general): a stand-alone max-pool between int8 tensors
(maxpool2_i8_kernel) and convolutions whose cin is 16 more than a multiple of 32 (conv_i8_kernel, ODD: a last chunk of one 16-channel
group).  Run on the GPU by tests/test_gpu_int8_general.py against tests/int8_general_ref.py; checked on the CPU by
tests/test_int8_general_cpu.py.

Two graphs:

  * fire_plan(): a miniature of the squeeze graph, levels 0 .. 3.  Stem 1 -> 64, a 3x3 64 -> 64 with fused pool, then three fire modules
    (a 1x1 squeeze to 16, 32 and 48 channels; a 1x1 and a 3x3 expand into the two halves of one tensor) with a stand-alone pool behind
    the first two.  Around them: a 3x3 layer with cin 16 and the POOL flag, pooled 3x3 and 1x1 and unpooled 3x3 layers with cin 48 on channel
    slices of the pooled tensors (a store into the zero border of a pooled plane changes a compared tensor), a 1x1 layer with cin 48
    and BatchNorm, a 1x1 layer with cin 48 and a residual, the detector head 1x1 48 -> 65 with fp32 output (OUT_F32 with an odd
    group count) and the descriptor branch through a 3x3 into 256 channels, a 1x1 with fp32 output and the L2 norm -- in the squeeze
    graph's order (3x3, 1x1, 3x3, 1x1, norm: the library moves the detector head behind the second 3x3, `library_ops`), with a tail that
    is not the plain one and so runs op by op.  One expand layer is linear: the pools see negative bytes.
  * the trained graph, tests/golden/sp_squeeze.spvw.

Scales of fire_plan: oracle.net_int8.calibrate on the case's own input with the plain maximum; then the pooled tensors' scales are SET:
s_o = 2 s_i exactly behind the first module (m = 0.5: ties, round-half-even), s_o ~ 1.37 s_i behind the second (both rounding
directions), and a second pool of the same tensor with s_o ~ 0.73 s_i (m > 1: the clamp at 127 is taken).
"""
import os

import numpy as np

from spvo import weights as W
from tests import conv_variant_cases as cvc

EDGE_SIZES = cvc.EDGE_SIZES          # 104 x 200 and 96 x 168: partial tiles on every level in H and in W; every pooled map is even; the finest pooled outputs are 13 x 25 and 12 x 21
case_input = cvc.case_input
POOL_RATIOS = {"tie": 2.0, "round": 1.37, "clamp": 0.73}     # s_o / s_i of the three stand-alone pools of fire_plan


def fire_plan(seed=41):
    """(plan, {arm: index of its pool op})"""
    b = cvc._Builder(seed)
    p = b.p
    pools = {}

    def pool(src, arm):
        ch, lvl = p.tensors[src]
        dst = b.tensor(ch, lvl + 1)
        p.ops.append(W.Op(W.OP_MAXPOOL, src, dst, 0, ch, ch))
        pools[arm] = len(p.ops) - 1
        return dst

    def fire(src, squeeze, half, relu_1x1=True):
        cin, lvl = p.tensors[src]
        s = b.tensor(squeeze, lvl)
        b.conv(src, s, 0, 0, cin, squeeze, 1)
        e = b.tensor(2 * half, lvl)
        b.conv(s, e, 0, 0, squeeze, half, 1, relu=relu_1x1)
        b.conv(s, e, half, 0, squeeze, half, 3)
        return s, e

    t0 = p.input_tensor = b.tensor(1, 0)
    t1 = b.tensor(64, 0)
    b.conv(t0, t1, 0, 0, 1, 64, 3)
    t2 = b.tensor(64, 1)
    b.conv(t1, t2, 0, 0, 64, 64, 3, pool=True)
    # level 1 (52 x 100 of 104 x 200): fire module 1, squeeze 16
    s1, e1 = fire(t2, 16, 64)
    p1 = pool(e1, "tie")                                             # 128 channels, level 2
    c16 = b.tensor(64, 2)
    b.conv(s1, c16, 0, 0, 16, 64, 3, pool=True)                      # 3x3, cin 16, POOL
    # level 2 (26 x 50): fire module 2, squeeze 32; its 1x1 expand is linear
    s2, e2 = fire(p1, 32, 128, relu_1x1=False)
    p2 = pool(e2, "round")                                           # 256 channels, level 3
    p3 = pool(e2, "clamp")
    q3 = b.tensor(192, 3)
    b.fill([dict(src=p1, in_off=16, cin=48, cout=64, k=3, pool=True),      # 3x3 readers of the pooled tensor p1 (cin 48, pooled) and of c16
            dict(src=p1, in_off=64, cin=48, cout=64, k=1, pool=True),      # 1x1, cin 48, POOL
            dict(src=c16, in_off=0, cin=64, cout=64, k=3, pool=True)], q3)
    # level 3 (13 x 25): fire module 3, squeeze 48
    s3, e3 = fire(p2, 48, 128)
    m = b.tensor(64, 3)
    b.fill([dict(src=p2, in_off=0, cin=48, cout=32, k=3),                  # 3x3 readers of the pooled tensors p2, p3 on 48-channel slices
            dict(src=p3, in_off=208, cin=48, cout=32, k=3, relu=False)], m)
    bn = b.tensor(64, 3)
    b.conv(s3, bn, 0, 0, 48, 64, 1, bn=True)                          # 1x1, cin 48, BatchNorm
    rs = b.tensor(64, 3)
    b.conv(s3, rs, 0, 0, 48, 64, 1, relu=False, res=bn)               # 1x1, cin 48, residual
    d48 = b.tensor(48, 3)                                             # what the detector head reads
    b.fill([dict(src=q3, in_off=32, cin=48, cout=16, k=1),
            dict(src=rs, in_off=0, cin=64, cout=16, k=3),
            dict(src=m, in_off=16, cin=48, cout=16, k=3)], d48)
    p.det_tensor = b.tensor(W.DET_CHANNELS, 3)
    da = b.tensor(256, 3)
    raw = b.tensor(W.DESC_CHANNELS, 3)
    p.desc_tensor = b.tensor(W.DESC_CHANNELS, 3)
    b.conv(d48, p.det_tensor, 0, 0, 48, W.DET_CHANNELS, 1, relu=False)     # detector head: fp32 output, three groups in
    b.conv(e3, da, 0, 0, 256, 256, 3)
    b.conv(da, raw, 0, 0, 256, W.DESC_CHANNELS, 1, relu=False)
    p.ops.append(W.Op(W.OP_L2NORM, raw, p.desc_tensor, 0, W.DESC_CHANNELS, W.DESC_CHANNELS))
    p.precision = "INT8"
    return p, pools


def prepare_fire(plan, pools, x):
    """calibrated scales (plain maximum of the fp32 graph on `x`), then the three pooled tensors' scales set from their inputs'"""
    from oracle import net_int8
    s = net_int8.calibrate(plan, [x], percentile=100.0)
    for arm, i in pools.items():
        op = plan.ops[i]
        s[op.out] = np.float32(np.float32(POOL_RATIOS[arm]) * s[op.inp])
    plan.act_scales = s
    return plan


def golden_images():
    from PIL import Image
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "images")
    return [np.asarray(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d)) if f.endswith(".png")]


def image_input(H, Wd, batch, images=None):
    """crops of the golden images as network input [batch, 1, H, Wd] in [0, 1]; a different crop per image of the batch"""
    images = golden_images() if images is None else images
    xs = []
    for k in range(batch):
        img = images[k % len(images)]
        y0, x0 = 40 + 16 * (k // len(images)), 60 + 37 * k
        xs.append(img[y0:y0 + H, x0:x0 + Wd].astype(np.float32) / 255.0)
    return np.stack(xs)[:, None]


def trained_plan(x):
    """tests/golden/sp_squeeze.spvw as an INT8 plan, calibrated on the first image of `x` (as test_int8_engine_is_bit_exact does)"""
    from oracle import net_int8
    plan = W.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sp_squeeze.spvw"))
    plan.act_scales = net_int8.calibrate(plan, [x[:1]])
    plan.precision = "INT8"
    return plan


def odd_group_convs(plan):
    """indices of the dense convolutions whose cin is 16 more than a multiple of 32"""
    return [i for i, op in enumerate(plan.ops) if op.type == W.OP_CONV and op.cin > 1 and op.cin % 32 == 16]


def stand_alone_pools(plan):
    return [i for i, op in enumerate(plan.ops) if op.type == W.OP_MAXPOOL]


def library_ops(plan):
    """the plan's ops in the order the library numbers its stages ("conv:<index>"): csrc/engine_file.h moves convPb behind convDa when an
    INT8 file ends in 3x3, 1x1, 3x3, 1x1, L2 norm (two branches), so that the trailing run of 1x1 layers holds both heads"""
    ops = list(plan.ops)
    if len(ops) >= 5:
        A, B, C, D, N = ops[-5:]
        if (A.type == W.OP_CONV and A.ksize == 3 and B.type == W.OP_CONV and B.ksize == 1 and B.inp == A.out and C.type == W.OP_CONV and C.ksize == 3 and
                C.inp != B.out and D.type == W.OP_CONV and D.ksize == 1 and D.inp == C.out and N.type == W.OP_L2NORM and N.inp == D.out and
                not (C.flags & W.FLAG_ADD) and not (B.flags & W.FLAG_ADD)):
            ops[-4], ops[-3] = ops[-3], ops[-4]
    return ops
