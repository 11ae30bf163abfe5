"""Seeded synthetic graphs that put every tile variant of the direct FP32, the FP16 and the INT8 convolution kernels in front of the
oracle (tests/test_gpu_conv_variants.py; checked on the CPU by tests/test_conv_variant_cases_cpu.py).

The launchers dispatch on (kernel size, input channels per chunk, wr, wc, pooled) -- csrc/spvo_net_f32.hip, spvo_net_f16.hip,
spvo_net_i8.hip -- and the plan loader (csrc/spvo_core.hip) picks the chunk from cin: 1x1 layers of an FP16 engine take 32 channels
per chunk when cin % 32 == 0 and 16 otherwise, those of an INT8 engine 64 when cin % 64 == 0 and 32 otherwise.  `narrow` below is the
cin that lands on the small chunk: 48 for FP32 / FP16 plans, 96 for INT8 plans; every other channel count is shared (3x3 layers read
multiples of 32 channels, 1x1 layers on the wide chunk read 64, every slice and every cout is a multiple of 16), so one topology
loads at all three precisions.

Two graphs:

  * edge_plan: ~30 small layers on levels 0 .. 3.  Every layer kind the launchers accept -- 3x3 ReLU / linear / pooled, 1x1 on either
    chunk plain / pooled / BatchNorm / residual / pooled with an epilogue -- sits on level 2, where a 104 x 200 input is 26 x 50 pixels:
    a partial tile in H and in W for every tile shape (4 or 8 rows, 32 or 64 columns), with a cout of 48, 80 or 96 (a partial tile of
    64 output channels).  Layers that share an output tensor write adjacent channel ranges in DESCENDING order of offset, so a layer
    that overruns its partial output-channel tile destroys what its neighbour wrote before it; and every tensor a layer under test
    writes is read by a 3x3 layer, so a write into the zero border of a padded plane changes a compared tensor.
  * long_plan: the same layer kinds with 192 output channels on level 0, for 120 x 392 x 2 images: more tiles than a persistent
    grid has workgroups, so every variant walks several tiles per workgroup and prefetches across them.
"""
import numpy as np

from spvo import weights as W

EDGE_SIZES = [(104, 200), (96, 168)]   # 104 x 200 -> 52 x 100 -> 26 x 50 -> 13 x 25;  96 x 168 -> 48 x 84 -> 24 x 42 -> 12 x 21
LONG_SIZE = (120, 392)
ENGINES = ("FP32", "FP16", "INT8")


def narrow_cin(precision):
    return 96 if precision == "INT8" else 48


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.p = W.Plan()

    def tensor(self, ch, level):
        return self.p.add_tensor(ch, level)

    def conv(self, src, dst, out_off, in_off, cin, cout, k, relu=True, pool=False, bn=False, res=None):
        rng = self.rng
        w = (rng.randn(cout, cin, k, k) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
        b = (rng.randn(cout) * 0.1).astype(np.float32)
        flags = (W.FLAG_RELU if relu else 0) | (W.FLAG_POOL if pool else 0) | (W.FLAG_BN if bn else 0) | (W.FLAG_ADD if res is not None else 0)
        op = W.Op(W.OP_CONV, src, dst, out_off, cin, cout, k, flags, w, b)
        op.in_c_off = in_off
        if res is not None:
            op.residual = res
        if bn:   # gamma, beta, mean, var, eps: scales around 1, shifts around 0 (the layer keeps its magnitude and most of its support)
            op.bn = np.concatenate([rng.uniform(0.7, 1.3, cout), rng.uniform(0.0, 0.2, cout), rng.uniform(0.0, 0.3, cout),
                                    rng.uniform(0.6, 1.4, cout), [1e-5]]).astype(np.float32)
        self.p.ops.append(op)
        return op

    def fill(self, writers, dst):
        """writers of one tensor, in execution order: the first gets the HIGHEST channel range, so that each later writer's
        partial output-channel tile ends where an earlier writer's data begins"""
        off = self.p.tensors[dst][0]
        for kw in writers:
            off -= kw["cout"]
            self.conv(dst=dst, out_off=off, **kw)
        assert off == 0, off

    def heads(self, src, cin):
        p = self.p
        t = self.tensor(512, 3)
        self.conv(src, t, 0, 0, cin, 256, 3)          # convPa / convDa: siblings the loader merges into one launch
        self.conv(src, t, 256, 0, cin, 256, 3)
        self.conv(t, self.tensor(64, 3), 0, 192, 128, 64, 3)   # a 3x3 reader of their output (across the boundary of the two), compared like every tensor
        p.det_tensor = self.tensor(W.DET_CHANNELS, 3)
        raw = self.tensor(W.DESC_CHANNELS, 3)
        p.desc_tensor = self.tensor(W.DESC_CHANNELS, 3)
        self.conv(t, p.det_tensor, 0, 0, 256, W.DET_CHANNELS, 1, relu=False)     # with "heads_fused" = 0: the fp32-output instances, cout 65
        self.conv(t, raw, 0, 256, 256, W.DESC_CHANNELS, 1, relu=False)
        p.ops.append(W.Op(W.OP_L2NORM, raw, p.desc_tensor, 0, W.DESC_CHANNELS, W.DESC_CHANNELS))
        return p


def edge_plan(precision, seed=11):
    N = narrow_cin(precision)
    b = _Builder(seed)
    t0 = b.p.input_tensor = b.tensor(1, 0)
    # level 0: stem, a 1x1 layer, a pooled 3x3 layer
    t1, t1b = b.tensor(64, 0), b.tensor(64, 0)
    b.conv(t0, t1, 0, 0, 1, 64, 3)
    b.conv(t1, t1b, 0, 0, 64, 64, 1)
    t2 = b.tensor(64, 1)
    b.conv(t1b, t2, 0, 0, 64, 64, 3, pool=True)
    # level 1: two sibling 3x3 layers the loader merges (64 + 96 = 160 output channels in one launch), then pooled layers of every kind
    t3 = b.tensor(160, 1)
    b.conv(t2, t3, 0, 0, 64, 64, 3)
    b.conv(t2, t3, 64, 0, 64, 96, 3)
    t4 = b.tensor(192, 2)
    b.fill([dict(src=t3, in_off=0, cin=64, cout=64, k=1, pool=True),
            dict(src=t3, in_off=64, cin=N, cout=80, k=1, pool=True),
            dict(src=t3, in_off=32, cin=128, cout=48, k=3, pool=True)], t4)
    # level 2 (26 x 50 of 104 x 200): every unpooled kind ...
    t5 = b.tensor(128, 2)
    b.fill([dict(src=t4, in_off=0, cin=192, cout=48, k=3),                           # siblings the loader does NOT merge (flags, slices and order differ)
            dict(src=t4, in_off=64, cin=128, cout=80, k=3, relu=False)], t5)
    tR = b.tensor(96, 2)                                                              # the residual input of the layers below
    b.conv(t5, tR, 0, 0, 64, 96, 1)
    t6 = b.tensor(256, 2)
    b.fill([dict(src=t5, in_off=0, cin=64, cout=80, k=1),
            dict(src=t5, in_off=16, cin=N, cout=48, k=1, relu=False),
            dict(src=t5, in_off=64, cin=64, cout=80, k=1, bn=True),
            dict(src=t5, in_off=32, cin=N, cout=48, k=1, bn=True)], t6)
    t7 = b.tensor(192, 2)
    b.fill([dict(src=t6, in_off=176, cin=64, cout=96, k=1, relu=False, res=tR),
            dict(src=t6, in_off=0, cin=N, cout=96, k=1, relu=False, res=tR)], t7)
    # ... and every pooled kind, 26 x 50 -> 13 x 25; each of t5, t6, t7, tR has a 3x3 reader among them
    t8 = b.tensor(704, 3)
    b.fill([dict(src=t7, in_off=0, cin=192, cout=48, k=3, pool=True),
            dict(src=t6, in_off=0, cin=256, cout=80, k=3, relu=False, pool=True),
            dict(src=t6, in_off=128, cin=64, cout=48, k=1, pool=True),
            dict(src=t6, in_off=48, cin=N, cout=80, k=1, pool=True),
            dict(src=t7, in_off=0, cin=64, cout=48, k=1, bn=True, pool=True),
            dict(src=t7, in_off=96, cin=N, cout=96, k=1, relu=False, res=tR, pool=True),
            dict(src=t7, in_off=64, cin=64, cout=96, k=1, relu=False, res=tR, pool=True),
            dict(src=t7, in_off=32, cin=N, cout=80, k=1, bn=True, pool=True),
            dict(src=tR, in_off=0, cin=96, cout=64, k=3, pool=True),
            dict(src=t5, in_off=0, cin=128, cout=64, k=3, pool=True)], t8)
    p = b.heads(t8, 704)
    p.precision = precision
    return p


def long_plan(precision, seed=12):
    N = narrow_cin(precision)
    b = _Builder(seed)
    a0 = b.p.input_tensor = b.tensor(1, 0)
    a1 = b.tensor(32, 0)
    b.conv(a0, a1, 0, 0, 1, 32, 3)
    a2 = b.tensor(192, 0)
    b.conv(a1, a2, 0, 0, 32, 192, 3)
    a3 = b.tensor(192, 0)
    b.conv(a2, a3, 0, 0, 64, 192, 1)
    # 192 output channels = 3 tiles of 64 per layer: 2340 tiles of 4 x 32, 1260 of 4 x 64, 1170 of 8 x 32, 630 of 8 x 64 pixels at 120 x 392 x 2,
    # against persistent grids measured on 256 CUs at no more than 1536, 768, 768 and 256 workgroups (6, 3, 3 and 1 per CU: registers
    # bound them, not the LDS) -- every tile shape walks more than one tile per workgroup with half as many tiles to spare
    A = b.tensor(576, 0)
    b.fill([dict(src=a2, in_off=64, cin=64, cout=192, k=1, relu=False, res=a3),
            dict(src=a2, in_off=64, cin=N, cout=192, k=1),
            dict(src=a2, in_off=96, cin=N, cout=192, k=1, bn=True)], A)
    B = b.tensor(1056, 1)
    b.fill([dict(src=a1, in_off=0, cin=32, cout=192, k=3, pool=True),
            dict(src=a2, in_off=128, cin=64, cout=192, k=1, pool=True),
            dict(src=a2, in_off=0, cin=64, cout=192, k=1, relu=False, res=a3, pool=True),
            dict(src=a2, in_off=32, cin=N, cout=192, k=1, pool=True),
            dict(src=a2, in_off=80, cin=N, cout=192, k=1, bn=True, pool=True),
            dict(src=A, in_off=128, cin=128, cout=32, k=3, pool=True),     # 3x3 readers of the level-0 tensors: slices across the writers' boundaries
            dict(src=A, in_off=320, cin=128, cout=32, k=3, pool=True),
            dict(src=a3, in_off=32, cin=128, cout=32, k=3, pool=True)], B)
    Cn = b.tensor(32, 2)
    b.conv(B, Cn, 0, 0, 1056, 32, 3, pool=True)
    D = b.tensor(64, 3)
    b.conv(Cn, D, 0, 0, 32, 64, 3, pool=True)
    p = b.heads(D, 64)
    p.precision = precision
    return p


def case_input(H, Wd, batch, seed=5):
    return np.random.RandomState(seed).rand(batch, 1, H, Wd).astype(np.float32)


def prepare(plan, x):
    """INT8 plans: activation scales from the fp32 graph on the very input of the case, plain maximum (no value of the fp32 graph
    saturates; the int8 graph's own values exceed the range by a rounding step at most)"""
    if plan.precision == "INT8":
        from oracle import net_int8
        plan.act_scales = net_int8.calibrate(plan, [x], percentile=100.0)
    return plan


def reference(plan, x):
    """(det, desc NCHW, {tensor: values}) of the oracle that defines the plan's precision"""
    from oracle import net, net_int8
    return net_int8.forward(plan, x, return_all=True) if plan.precision == "INT8" else net.forward(plan, x, return_all=True)


def check_loader_rules(plan):
    """The plan loader's channel rules (csrc/spvo_core.hip, "INT8 engines" / "FP16 engines" / the FP32 direct kernel), restated"""
    prec = plan.precision
    g = {"FP32": 1, "FP16": 8, "INT8": 16}[prec]                 # channels per storage group
    keep = {plan.input_tensor, plan.det_tensor, plan.desc_tensor} | {op.inp for op in plan.ops if op.type == W.OP_L2NORM}
    low = lambda t: prec != "FP32" and t not in keep and plan.tensors[t][0] % g == 0   # stored as fp16 / int8
    for i, op in enumerate(plan.ops):
        if op.type != W.OP_CONV:
            continue
        ci_t, lv_i = plan.tensors[op.inp]
        co_t, lv_o = plan.tensors[op.out]
        pool, bn, add, relu = (bool(op.flags & f) for f in (W.FLAG_POOL, W.FLAG_BN, W.FLAG_ADD, W.FLAG_RELU))
        assert op.in_c_off + op.cin <= ci_t and op.out_c_off + op.cout <= co_t, i
        assert lv_o == lv_i + (1 if pool else 0), i
        assert not (bn and (add or not relu)) and not (add and relu), i
        assert not ((bn or add) and op.cin > 1 and op.ksize != 1), i
        if add:
            assert plan.tensors[op.residual] == (op.cout, lv_i) and op.residual != op.out, i
        if op.cin == 1:
            assert not pool and not add, i
            continue
        if prec == "FP32":
            assert op.cin % (8 if op.ksize == 3 else 16) == 0, i
            continue
        chunk = g * (2 if (op.ksize == 3 or op.cin % (4 * g)) else 4)
        assert low(op.inp) and op.cin % chunk == 0 and op.in_c_off % g == 0, i
        if low(op.out):
            assert op.cout % g == 0 and op.out_c_off % g == 0, i
        else:
            assert not (pool or bn or add), i
        if add:
            assert low(op.residual), i


def conv_kinds(plan):
    """per dense convolution (op index): (ks, chunk kind "wide" / "narrow" / "3x3", pooled, epilogue 0 / 1 / 2, relu, level of its input)"""
    N = narrow_cin(plan.precision)
    out = {}
    for i, op in enumerate(plan.ops):
        if op.type == W.OP_CONV and op.cin > 1:
            kind = "3x3" if op.ksize == 3 else ("narrow" if op.cin == N else "wide")
            epi = 1 if op.flags & W.FLAG_BN else 2 if op.flags & W.FLAG_ADD else 0
            out[i] = (op.ksize, kind, bool(op.flags & W.FLAG_POOL), epi, bool(op.flags & W.FLAG_RELU), plan.tensors[op.inp][1])
    return out
