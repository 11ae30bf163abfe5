"""The fourth item of the F(4x4,3x3) Winograd kernel (conv_wino4.hip.h, ITEM = 3; spvo_set_tuning "wino4_item" = 3): item 2 with the
instructions that compute no value of the result cut down -- the two DMA bases as running 64-bit scalars (one add per chunk step, a
fresh base per tile step), the LDS side of every DMA and the operand bases swapped between their two buffers instead of rebuilt from
the item's parity, the role test on one scalar kept in place, the counted operand waits with their pieces as inputs only, the raw-tile
and store addresses of the transform kept per wave group, and the row pass written out instruction by instruction.  Same matrix
instructions, same order, same operands, same transform arithmetic: every tensor must come out with IDENTICAL BITS as from items 0
and 2.  The comparisons are np.array_equal on uint32 views, never a tolerance (the method of test_gpu_wino4_item2.py).  A running
pointer that goes wrong does so where a cursor crosses from one tile into the next or where a tile has an odd number of items: a
wrong raw tile or filter slab staged, so a difference, or a run that does not repeat.
"""
import numpy as np
import pytest

import oracle  # noqa: F401

pytestmark = pytest.mark.gpu


def _input(sample_images, H, W, batch):
    xs = []
    for b in range(batch):
        img = sample_images[b % len(sample_images)]
        if img.shape[0] < H + 5 or img.shape[1] < W + 20 + 3 * b:
            img = np.pad(img, ((0, max(0, H + 5 - img.shape[0])), (0, max(0, W + 20 + 3 * b - img.shape[1]))), mode="wrap")
        xs.append(img[5:5 + H, 20 + 3 * b:20 + 3 * b + W].astype(np.float32) / 255.0)
    return np.stack(xs)[:, None]


def _awkward_plan(seed):
    """The graph of test_gpu_network.py::test_winograd_kernels_on_awkward_layer_shapes: channel counts that are not multiples of 64
    (partial output tiles), 16 .. 72 input channels (4 .. 18 items per tile: odd and even chains, both sides of n_chunks < 5), a linear
    layer, pooled and unpooled layers at every level."""
    from spvo import weights as Wm
    rng = np.random.RandomState(seed)
    p = Wm.Plan()
    cur = p.add_tensor(1, 0)
    p.input_tensor = cur
    layers = [(1, 16, True, False), (16, 72, True, True), (72, 24, False, False), (24, 40, True, True), (40, 48, True, False), (48, 16, True, True), (16, 32, True, False)]
    level = 0
    for ci, co, relu, pool in layers:
        if pool:
            level += 1
        nxt = p.add_tensor(co, level)
        w = (rng.randn(co, ci, 3, 3) * np.sqrt(2.0 / (ci * 9))).astype(np.float32)
        b = (rng.randn(co) * 0.05).astype(np.float32)
        p.ops.append(Wm.Op(Wm.OP_CONV, cur, nxt, 0, ci, co, 3, (Wm.FLAG_RELU if relu else 0) | (Wm.FLAG_POOL if pool else 0), w, b))
        cur = nxt
    det, draw, desc = p.add_tensor(Wm.DET_CHANNELS, 3), p.add_tensor(Wm.DESC_CHANNELS, 3), p.add_tensor(Wm.DESC_CHANNELS, 3)
    for out, co in ((det, Wm.DET_CHANNELS), (draw, Wm.DESC_CHANNELS)):
        w = (rng.randn(co, 32, 1, 1) * np.sqrt(1.0 / 32)).astype(np.float32)
        p.ops.append(Wm.Op(Wm.OP_CONV, cur, out, 0, 32, co, 1, 0, w, (rng.randn(co) * 0.05).astype(np.float32)))
    p.ops.append(Wm.Op(Wm.OP_L2NORM, draw, desc, 0, Wm.DESC_CHANNELS, Wm.DESC_CHANNELS))
    p.det_tensor, p.desc_tensor = det, desc
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(plan, path, x, H, W, tuning, item, wino4_stages, **switches):
    """One context with "wino4_item" = item: the kernel family of the given stages, every tensor the library exposes, both outputs."""
    from spvo import capi
    tuning(wino4_item=item, **switches)
    ctx = capi.Context(net_height=H, net_width=W)
    ctx.load_weights(path)
    fams = [ctx.stage_kernel(f"conv:{i}")[0] for i in wino4_stages]
    det, desc = ctx.forward(x)
    out = {"det": _bits(det), "desc": _bits(desc)}
    for tid, (ch, lvl) in enumerate(plan.tensors):
        if tid in (plan.input_tensor, plan.desc_tensor):
            continue
        out[f"tensor {tid}"] = _bits(ctx.debug_tensor(tid, x.shape[0], ch, lvl))
    ctx.close()
    return fams, out


def _assert_same_bits(old, new):
    assert old.keys() == new.keys()
    for k in old:
        assert old[k].shape == new[k].shape and np.array_equal(old[k], new[k]), (k, int((old[k] != new[k]).sum()), old[k].size)


@pytest.mark.parametrize("H,W", [(96, 168), (104, 200), (120, 392)])
def test_item3_agrees_bit_for_bit_with_items_0_and_2_on_awkward_layer_shapes(H, W, sample_images, tuning, tmp_path):
    """Partial tiles, cout not a multiple of 64, 4 .. 18 items per tile (odd and even chains, so that a tile hands either buffer parity to
    its successor), one-tile workgroups (static assignment), pooled and unpooled epilogues."""
    from spvo import weights as Wm
    plan = _awkward_plan(3)
    path = str(tmp_path / "awkward.spvw")
    Wm.save(plan, path)
    x = _input(sample_images, H, W, 2)
    res = {}
    for item in (0, 2, 3):
        fams, res[item] = _run(plan, path, x, H, W, tuning, item, range(1, 7), winograd_min_tiles=1, wino4_min_tiles=1, wino4=1)
        assert all(f == "conv_wino4_kernel" for f in fams), (item, fams)
    _assert_same_bits(res[0], res[3])
    _assert_same_bits(res[2], res[3])


@pytest.fixture(scope="module")
def vgg_192x640(sample_images):
    return _input(sample_images, 192, 640, 2)


def _vgg_3x3_stages(plan):
    from spvo import weights as Wm
    return [i for i, op in enumerate(plan.ops) if op.type == Wm.OP_CONV and op.ksize == 3 and op.cin > 1]


def test_item3_agrees_bit_for_bit_with_item_0_on_vgg_192x640(vgg_weights_path, vgg_plan, vgg_192x640, tuning):
    """conv1b is 480 tiles of 16 items here (two rounds on 256 CUs): the dynamic tile assignment, the item that publishes a tile's
    successor and prefetch cursors that cross from one tile into the next -- the smallest shape that reaches those paths."""
    res, fams = {}, {}
    stages = _vgg_3x3_stages(vgg_plan)
    for item in (0, 3):
        fams[item], res[item] = _run(vgg_plan, vgg_weights_path, vgg_192x640, 192, 640, tuning, item, stages)
    assert fams[0] == fams[3] and fams[3][0] == "conv_wino4_kernel", fams   # (conv1b; the deepest layers have too few tiles for this kernel)
    _assert_same_bits(res[0], res[3])


def test_item3_repeats_bit_for_bit(vgg_weights_path, vgg_plan, vgg_192x640, tuning):
    """Twenty runs of one input on item 3: every run equals the first."""
    from spvo import capi
    tuning(wino4_item=3)
    ctx = capi.Context(net_height=192, net_width=640)
    ctx.load_weights(vgg_weights_path)
    assert ctx.stage_kernel(f"conv:{_vgg_3x3_stages(vgg_plan)[0]}")[0] == "conv_wino4_kernel"

    def once():
        det, desc = ctx.forward(vgg_192x640)
        out = [_bits(det).copy(), _bits(desc).copy()]
        for tid, (ch, lvl) in enumerate(vgg_plan.tensors):
            if tid not in (vgg_plan.input_tensor, vgg_plan.desc_tensor):
                out.append(_bits(ctx.debug_tensor(tid, 2, ch, lvl)).copy())
        return out
    first = once()
    for run in range(1, 20):
        for k, (a, b) in enumerate(zip(first, once())):
            assert np.array_equal(a, b), (run, k, int((a != b).sum()))
    ctx.close()

