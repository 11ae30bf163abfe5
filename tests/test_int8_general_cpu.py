"""The reference of the "int8_general" mode (tests/int8_general_ref.py) and its cases (tests/int8_general_cases.py), on the CPU.

  * on a plan without stand-alone pools the reference IS oracle.net_int8.forward, bit for bit on every tensor;
  * on fire_plan the three pools take the arms they were built for -- ties, both rounding directions, the clamp -- and a pooled value
    that is not clamped lies within half a step of its input's real value;
  * the trained graph runs through the reference; and how many FP32 keypoints its INT8 form keeps is printed (a recorded figure).
"""
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import net_int8
from spvo import weights as W
from tests import int8_general_cases as igc
from tests import int8_general_ref as ref
from tests.conftest import GOLDEN


def test_reference_is_the_oracle_without_stand_alone_pools():
    plan = W.load(os.path.join(GOLDEN, "sp_mbv1.spvw"))
    x = igc.image_input(64, 96, 2)
    plan.act_scales = net_int8.calibrate(plan, [x[:1]])
    plan.precision = "INT8"
    assert not igc.stand_alone_pools(plan)
    det, desc, vals = ref.forward(plan, x, return_all=True)
    odet, odesc, ovals = net_int8.forward(plan, x, return_all=True)
    assert set(vals) == set(ovals)
    for t in vals:
        assert vals[t].dtype == ovals[t].dtype and np.array_equal(vals[t], ovals[t]), t
    assert np.array_equal(det, odet) and np.array_equal(desc, odesc)
    assert ref.forward(plan, x)[0].shape == det.shape             # (the two-value form)


@pytest.fixture(scope="module")
def fire():
    H, Wd = igc.EDGE_SIZES[0]
    x = igc.case_input(H, Wd, 2)
    plan, pools = igc.fire_plan()
    igc.prepare_fire(plan, pools, x)
    return plan, pools, x, ref.forward(plan, x, return_all=True)[2]


def test_fire_plan_is_the_miniature_the_mode_is_for(fire):
    plan, pools, _, _ = fire
    assert sorted(pools) == ["clamp", "round", "tie"] and sorted(pools.values()) == igc.stand_alone_pools(plan)
    odd = [plan.ops[i] for i in igc.odd_group_convs(plan)]
    kinds = {(op.cin, op.ksize, bool(op.flags & W.FLAG_POOL), bool(op.flags & W.FLAG_BN), bool(op.flags & W.FLAG_ADD), net_int8.is_quantized(plan, op.out)) for op in odd}
    for want in [(16, 1, False, False, False, True), (16, 3, False, False, False, True), (16, 3, True, False, False, True), (48, 1, False, False, False, True),
                 (48, 3, False, False, False, True), (48, 3, True, False, False, True), (48, 1, True, False, False, True), (48, 1, False, True, False, True), (48, 1, False, False, True, True),
                 (48, 1, False, False, False, False)]:
        assert want in kinds, want
    det = [op for op in plan.ops if op.out == plan.det_tensor]
    assert len(det) == 1 and det[0].cin == 48 and plan.tensors[det[0].inp][0] == 48
    # the squeeze graph's order: a 3x3 between the two 1x1 heads (which the library moves: igc.library_ops)
    assert [(o.type, o.ksize) for o in plan.ops[-4:]] == [(W.OP_CONV, 1), (W.OP_CONV, 3), (W.OP_CONV, 1), (W.OP_L2NORM, 0)]
    assert [plan.ops.index(o) for o in igc.library_ops(plan)][-5:] == [len(plan.ops) - k for k in (5, 3, 4, 2, 1)]
    for op in plan.ops:
        if op.type == W.OP_MAXPOOL:
            assert net_int8.is_quantized(plan, op.inp) and net_int8.is_quantized(plan, op.out)
            assert plan.tensors[op.inp][0] == plan.tensors[op.out][0] and plan.tensors[op.out][1] == plan.tensors[op.inp][1] + 1
    for H, Wd in igc.EDGE_SIZES:
        for op in plan.ops:
            if op.type == W.OP_MAXPOOL or op.flags & W.FLAG_POOL:
                lvl = plan.tensors[op.inp][1]
                assert (H >> lvl) % 2 == 0 and (Wd >> lvl) % 2 == 0


def test_pool_arms_are_hit_and_the_error_is_half_a_step(fire):
    plan, pools, _, vals = fire
    s = plan.act_scales.astype(np.float32)
    seen = {}
    for arm, i in pools.items():
        op = plan.ops[i]
        s_i, s_o = s[op.inp], s[op.out]
        m = ref.pool_multiplier(s_i, s_o)
        qo, mx = ref.maxpool_i8(vals[op.inp], s_i, s_o)
        assert np.array_equal(qo, vals[op.out])
        v = (mx.astype(np.float32) * m).astype(np.float32)             # the one fp32 product per value
        frac = v.astype(np.float64) - np.floor(v.astype(np.float64))
        sat = np.abs(v) > 127
        seen[arm] = dict(m=float(m), tie=int((frac == 0.5).sum()), down=int(((frac > 0) & (frac < 0.5) & ~sat).sum()), up=int(((frac > 0.5) & ~sat).sum()),
                         clamp=int(sat.sum()), negative=int((mx < 0).sum()))
        # not clamped: |q_o s_o - max(q_i) s_i| <= s_o / 2, plus one fp32 ulp of the product (m is a rounded quotient, v a rounded product)
        real_in = mx.astype(np.float64) * np.float64(s_i)
        real_out = qo.astype(np.float64) * np.float64(s_o)
        ulp = np.spacing(np.abs(v)).astype(np.float64) * np.float64(s_o)
        assert (np.abs(real_out - real_in)[~sat] <= (np.float64(s_o) / 2 + ulp)[~sat]).all(), arm
        assert (np.abs(qo) <= 127).all()
    print(seen)
    assert seen["tie"]["m"] == 0.5 and seen["tie"]["tie"] > 0
    odd = vals[plan.ops[pools["tie"]].inp]
    q_tie = vals[plan.ops[pools["tie"]].out]
    mx = ref.pool_max(odd)
    assert np.array_equal(q_tie[mx == 5], np.full((mx == 5).sum(), 2)) and np.array_equal(q_tie[mx == 7], np.full((mx == 7).sum(), 4))   # half-even: 2.5 -> 2, 3.5 -> 4
    assert (mx == 5).any() and (mx == 7).any()
    assert seen["round"]["down"] > 0 and seen["round"]["up"] > 0 and seen["round"]["negative"] > 0
    assert seen["clamp"]["m"] > 1 and seen["clamp"]["clamp"] > 0 and (vals[plan.ops[pools["clamp"]].out] == 127).any()


def test_trained_graph_runs_through_the_reference():
    H, Wd = igc.EDGE_SIZES[0]
    x = igc.image_input(H, Wd, 2)
    plan = igc.trained_plan(x)
    assert len(igc.stand_alone_pools(plan)) == 2 and {plan.ops[i].cin for i in igc.odd_group_convs(plan)} == {16, 48}
    with pytest.raises(NotImplementedError):
        net_int8.forward(plan, x)
    det, desc, vals = ref.forward(plan, x, return_all=True)
    assert np.isfinite(det).all() and np.isfinite(desc).all()
    for t, v in vals.items():
        if v.dtype == np.int8:
            assert v.min() < v.max(), t


def test_keypoint_overlap_with_the_fp32_graph_is_recorded(sample_images):
    """Recorded, not a bar: the share of the FP32 graph's keypoints (oracle front end, 120 x 392, the golden images) that the INT8 graph,
    calibrated on the first image, finds at the same pixel."""
    import copy
    from oracle import frontend as fe, net
    H, Wd = 120, 392
    P = np.eye(3, 4)
    x = np.stack([fe.to_network_input(fe.preprocess(img, P, H, Wd)[0]) for img in sample_images])[:, None]
    plan = igc.trained_plan(x)
    p32 = copy.copy(plan)
    p32.precision, p32.act_scales = "FP32", None
    d32, _ = net.forward(p32, x)
    d8, _ = ref.forward(plan, x)
    found = total = n8 = 0
    for k in range(len(x)):
        a = {tuple(r) for r in fe.nms(fe.heatmap(d32[k])).tolist()}
        b = {tuple(r) for r in fe.nms(fe.heatmap(d8[k])).tolist()}
        found, total, n8 = found + len(a & b), total + len(a), n8 + len(b)
    print(f"sp_squeeze INT8 (int8_general) at {H} x {Wd}: {found} of {total} FP32 keypoints found again ({100.0 * found / max(total, 1):.1f} %), {n8} INT8 keypoints")
    assert total > 0 and n8 > 0
