"""The synthetic graphs of tests/conv_variant_cases.py, checked without a GPU: they obey the plan loader's channel rules, contain
every layer kind the convolution launchers dispatch on, and their oracle outputs are able to show a fault (dense, unsaturated).
Also the library's side of the variant tests that needs no device: the "conv_variant" switch and the query are exported."""
import time

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import weights as W
from tests import conv_variant_cases as cvc

PLANS = [("edge", cvc.edge_plan), ("long", cvc.long_plan)]


def test_conv_variant_switch_and_query_are_exported():
    from spvo import capi
    lib = capi.load()
    assert "spvo_profile_stage_variant" in capi.SYMBOLS and hasattr(lib, "spvo_profile_stage_variant")
    assert hasattr(capi.Context, "stage_variant")
    try:
        capi.set_tuning("conv_variant", 21)
        assert capi.get_tuning("conv_variant", 0) == 21
        with pytest.raises(capi.SpvoError):
            capi.set_tuning("conv_variant_", 21)
        with pytest.raises(capi.SpvoError):
            capi.set_tuning("no_such_switch", 1)
    finally:
        capi.clear_tuning()
    assert capi.get_tuning("conv_variant", 0) == 0


@pytest.mark.parametrize("precision", cvc.ENGINES)
@pytest.mark.parametrize("name,build", PLANS)
def test_plans_obey_the_loader_rules(name, build, precision):
    plan = build(precision)
    cvc.check_loader_rules(plan)
    # every tensor is written completely (no channel gaps: a gap would be zeros on both sides of every comparison)
    written = {t: np.zeros(ch, bool) for t, (ch, _) in enumerate(plan.tensors)}
    for op in plan.ops:
        if op.type == W.OP_CONV:
            assert not written[op.out][op.out_c_off:op.out_c_off + op.cout].any(), "overlapping writers"
            written[op.out][op.out_c_off:op.out_c_off + op.cout] = True
        else:
            written[op.out][:] = True
    assert all(w.all() for t, w in written.items() if t != plan.input_tensor)
    # a plan is the same graph whenever it is built
    again = build(precision)
    assert all(np.array_equal(a.weight, b.weight) for a, b in zip(plan.ops, again.ops) if a.weight is not None)


@pytest.mark.parametrize("precision", cvc.ENGINES)
def test_edge_plan_holds_every_layer_kind(precision):
    plan = cvc.edge_plan(precision)
    kinds = cvc.conv_kinds(plan)
    have = {(ks, kind, pool, epi) for ks, kind, pool, epi, _, _ in kinds.values()}
    want = {(3, "3x3", False, 0), (3, "3x3", True, 0)}
    for kind in ("wide", "narrow"):
        want |= {(1, kind, pool, epi) for pool in (False, True) for epi in (0, 1, 2)}
    assert want <= have, want - have
    assert any(ks == 3 and not relu for ks, _, _, _, relu, _ in kinds.values())                      # a linear 3x3 layer
    assert {lvl for ks, *_, lvl in kinds.values() if ks == 3} == {0, 1, 2, 3} and {lvl for ks, *_, lvl in kinds.values() if ks == 1} >= {0, 1, 2, 3}
    # every kind sits on level 2 with a partial tile of 64 output channels (26 x 50 pixels of a 104 x 200 input: partial in H and W too)
    on2 = {(ks, kind, pool, epi) for i, (ks, kind, pool, epi, _, lvl) in kinds.items() if lvl == 2 and plan.ops[i].cout % 64}
    assert want <= on2, want - on2
    couts = {plan.ops[i].cout for i in kinds}
    assert {48, 80} <= couts and W.DET_CHANNELS in couts and W.DESC_CHANNELS in couts
    assert any(plan.ops[i].in_c_off for i in kinds)
    N = cvc.narrow_cin(precision)
    assert N % (32 if precision != "INT8" else 64) and all(plan.ops[i].cin % (32 if precision != "INT8" else 64) == 0 for i, k in kinds.items() if k[1] == "wide")
    # every tensor a convolution writes (but the network outputs) has a 3x3 reader
    outputs = {plan.det_tensor, plan.desc_tensor} | {op.inp for op in plan.ops if op.type == W.OP_L2NORM}
    outputs |= set(range(len(plan.tensors))) - {op.inp for op in plan.ops}      # (the 3x3 reader of the heads' input writes a tensor nothing reads)
    read3 = {op.inp for op in plan.ops if op.type == W.OP_CONV and op.ksize == 3}
    assert {plan.ops[i].out for i in kinds} - outputs <= read3
    # writers of one tensor: where a later one ends on a partial tile, the channels behind it were written EARLIER
    for i in kinds:
        op = plan.ops[i]
        end = op.out_c_off + op.cout
        if op.cout % 64 and end < plan.tensors[op.out][0]:
            nb = [j for j, o in enumerate(plan.ops) if o.type == W.OP_CONV and o.out == op.out and o.out_c_off == end]
            assert nb and nb[0] < i, (i, nb)
    # siblings: the loader's merge condition (csrc/spvo_core.hip, "Sibling 3x3 layers"), restated -- both outcomes occur
    def merges(a, b):
        return (a.ksize == 3 and a.cin > 1 and not (a.flags & ~W.FLAG_RELU) and a.cout % 64 == 0 and b.type == W.OP_CONV and (b.inp, b.in_c_off, b.cin, b.ksize, b.flags, b.out)
                == (a.inp, a.in_c_off, a.cin, a.ksize, a.flags, a.out) and b.out_c_off == a.out_c_off + a.cout)
    sib = [(merges(a, b)) for a, b in zip(plan.ops, plan.ops[1:]) if a.type == b.type == W.OP_CONV and a.out == b.out and a.ksize == b.ksize == 3]
    assert True in sib and False in sib


_timing = {}


@pytest.mark.parametrize("precision", cvc.ENGINES)
@pytest.mark.parametrize("name,build", PLANS)
def test_references_can_show_a_fault(name, build, precision):
    """At 96 x 168: in every compared tensor at least a quarter of the values are nonzero, and in every int8 tensor fewer than 1 % sit
    at +-127 -- conditions on the seeds and weight scales of the synthetic plans, met by the oracle alone."""
    H, Wd = cvc.EDGE_SIZES[1]
    x = cvc.case_input(H, Wd, 2)
    plan = cvc.prepare(build(precision), x)
    t0 = time.perf_counter()
    det, desc, vals = cvc.reference(plan, x)
    _timing[(name, precision)] = time.perf_counter() - t0
    print(f"{name} plan, {precision} oracle at {H} x {Wd} x 2: {_timing[(name, precision)]:.2f} s")
    for tid, (ch, lvl) in enumerate(plan.tensors):
        if tid == plan.input_tensor:
            continue
        v = vals[tid]
        assert v.shape == (2, ch, H >> lvl, Wd >> lvl) and np.isfinite(v.astype(np.float64)).all()
        nz = float((v != 0).mean())
        assert nz >= 0.25, (name, precision, tid, nz)
        for c0 in range(0, ch, 16):   # ... and no writer's channel range is dead either
            assert (v[:, c0:c0 + 16] != 0).mean() >= 0.1, (name, precision, tid, c0)
        if v.dtype == np.int8:
            sat = float((np.abs(v.astype(np.int32)) == 127).mean())
            assert sat < 0.01, (name, precision, tid, sat)
    assert np.allclose(np.linalg.norm(desc, axis=1), 1.0, atol=1e-5)
