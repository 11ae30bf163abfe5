"""The synthetic graphs of tests/fused_block_cases.py, checked without a GPU from the oracle and `fusion_table` (the restatement of
plan_int8_fusion) alone: together they hold the twelve instances of dwpw_i8_kernel at the edges where the instances differ, they obey the
plan loader's rules, and their oracle values are able to show a fault -- every int8 tensor a fused block writes clips at 127 and holds
zeros.  Also the library's side that needs no device: the fused-launch report is exported."""
import time

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import weights as W
from tests import fused_block_cases as fbc

BLOCK_PLANS = [(f"block-pool{int(sp)}-bn{int(sb)}", lambda prec, sp=sp, sb=sb: fbc.block_plan(prec, sp, sb)) for sp, sb in fbc.STEMS]
LONG_PLANS = [(f"long-{part or 'all'}", lambda prec, part=part: fbc.long_block_plan(prec, part)) for part in (None,) + fbc.LONG_PARTS]
ORACLE_CASES = [(n, b, H, Wd, 2) for n, b in BLOCK_PLANS for H, Wd in fbc.EDGE_SIZES] + [BLOCK_PLANS[0] + (104, 200, 1)] + [(n, b) + fbc.LONG_SIZE + (2,) for n, b in LONG_PLANS[1:]]


def _blocks(plan, H, Wd):
    """(instance, co_tiles, level, partial tile in W, in H) of every fused block"""
    out = []
    for i, inst in fbc.fusion_table(plan, H, Wd).items():
        if inst:
            lvl = plan.tensors[plan.ops[i - 1].inp][1]
            out.append((inst[:4], inst[4], lvl, (Wd >> lvl) % 32 != 0, (H >> lvl) % 8 != 0))
    return out


def test_fused_report_is_exported():
    from spvo import capi
    lib = capi.load()
    assert "spvo_profile_stage_fused" in capi.SYMBOLS and hasattr(lib, "spvo_profile_stage_fused") and hasattr(capi.Context, "stage_fused")


@pytest.mark.parametrize("precision", fbc.ENGINES)
@pytest.mark.parametrize("name", [n for n, _ in BLOCK_PLANS + LONG_PLANS])
def test_plans_obey_the_loader_rules(name, precision):
    build = dict(BLOCK_PLANS + LONG_PLANS)[name]
    plan = build(precision)
    assert fbc.check_loader_rules(plan) >= 3                  # (the depthwise layers among them: the new op kind)
    written = {t: np.zeros(ch, bool) for t, (ch, _) in enumerate(plan.tensors)}
    for op in plan.ops:
        assert not written[op.out][op.out_c_off:op.out_c_off + op.cout].any(), "overlapping writers"
        written[op.out][op.out_c_off:op.out_c_off + op.cout] = True
    assert all(w.all() for t, w in written.items() if t != plan.input_tensor)
    again = build(precision)
    assert all(np.array_equal(a.weight, b.weight) for a, b in zip(plan.ops, again.ops) if a.weight is not None)
    # the tail is one the loader fuses (csrc/spvo_plan.hip, find_heads / tail_is_plain): exactly convPb, convDb, L2 norm behind a 3x3 layer
    pb, db, nm = plan.ops[-3:]
    assert plan.ops[-4].ksize == 3 and (pb.ksize, pb.cin, pb.cout, pb.flags, pb.out) == (1, 256, W.DET_CHANNELS, 0, plan.det_tensor)
    assert (db.ksize, db.cin, db.cout, db.flags) == (1, 256, W.DESC_CHANNELS, 0) and nm.type == W.OP_L2NORM and nm.inp == db.out and nm.out == plan.desc_tensor
    # the fusion plan does not depend on the precision the topology is loaded at (only INT8 engines use it)
    assert fbc.fusion_table(plan) == fbc.fusion_table(build("INT8"))


def test_block_plans_hold_the_twelve_instances_at_their_edges():
    """Over the four block plans at the two edge sizes: exactly the twelve instances; each non-stem instance with a partial 8 x 32 tile in
    W and in H (levels 1 and 2 of 104 x 200 are 52 x 100 and 26 x 50), each stem instance with a partial tile in W.  A stem block lies on
    level 0, whose height is a multiple of 8 at every size the loader accepts: a partial tile in H cannot occur there."""
    seen = {}
    for _, build in BLOCK_PLANS:
        plan = build("INT8")
        for H, Wd in fbc.EDGE_SIZES:
            for inst, co, lvl, pw_, ph in _blocks(plan, H, Wd):
                f = seen.setdefault(inst, dict(W=False, H=False, co=set()))
                f["W"] |= pw_
                f["H"] |= ph
                f["co"].add(co)
                assert (lvl == 0) >= bool(inst[1])
    assert set(seen) == set(fbc.INSTANCES), set(seen) ^ set(fbc.INSTANCES)
    assert all(f["W"] for f in seen.values()) and all(f["H"] for inst, f in seen.items() if not inst[1]), seen
    assert all(H % 8 == 0 for H, _ in fbc.EDGE_SIZES + [fbc.LONG_SIZE, fbc.TINY_SIZE])
    for G in (4, 8):                                           # one and two tiles of 64 output channels
        assert set().union(*(f["co"] for inst, f in seen.items() if inst[0] == G and not inst[1])) == {1, 2}, G


@pytest.mark.parametrize("name", [n for n, _ in BLOCK_PLANS])
def test_block_plan_topology(name):
    plan = dict(BLOCK_PLANS)[name]("INT8")
    table = fbc.fusion_table(plan, *fbc.EDGE_SIZES[0])
    insts = [v[:4] for v in table.values() if v]
    assert {(g, p, e) for g, stem, p, e in insts if not stem} == {(g, p, e) for g in (4, 8) for p in (0, 1) for e in (0, 1)}
    assert sum(v[1] for v in insts) == 1 and table[3] and table[3][1] == 1          # the stem block is ops 0 .. 3
    pairs = {(plan.ops[i].cin, plan.ops[i].cout) for i, v in table.items() if v}
    assert pairs == {(64, 64), (64, 128), (128, 64), (128, 128)}
    # the unfused two: a depthwise layer without ReLU, and one whose output a residual reads too
    unfused = [i for i, v in table.items() if v is None]
    assert len(unfused) == 2
    lin = [i for i in unfused if not plan.ops[i - 1].flags & W.FLAG_RELU]
    res = [i for i in unfused if any(o.flags & W.FLAG_ADD and o.residual == plan.ops[i - 1].out for o in plan.ops)]
    assert len(lin) == 1 and len(res) == 1 and lin != res
    # every fused block's output has a 3x3 reader behind it (its depthwise output is read by the block alone, and compared through the debug store)
    read3 = {}
    for j, op in enumerate(plan.ops):
        if op.type != W.OP_L2NORM and op.ksize == 3:
            read3.setdefault(op.inp, j)
    for i, v in table.items():
        assert not v or read3.get(plan.ops[i].out, -1) > i, i
    # blocks branch off one tensor
    srcs = [plan.ops[i - 1].inp for i, v in table.items() if v]
    assert len(set(srcs)) < len(srcs)
    # the tail: two tensors in exactly one plan
    two = plan.ops[-3].inp != plan.ops[-2].inp
    assert two == (name == "block-pool1-bn0")
    if not two:
        assert plan.tensors[plan.ops[-3].inp][0] == 512


def test_long_plan_is_on_level_0():
    """long_block_plan: the eight non-stem instances and a stem instance all read level 0 -- 15 x 13 x 2 = 390 tiles per launch at
    120 x 392 x 2 -- and its parts, which the GPU test runs, together hold all twelve there."""
    H, Wd = fbc.LONG_SIZE
    assert ((H + 7) // 8) * ((Wd + 31) // 32) * 2 == 390
    on0 = {inst for inst, co, lvl, _, _ in _blocks(fbc.long_block_plan("INT8"), H, Wd) if lvl == 0}
    assert {i for i in on0 if not i[1]} == {i for i in fbc.INSTANCES if not i[1]} and len({i for i in on0 if i[1]}) == 1
    parts = set()
    for part in fbc.LONG_PARTS:
        parts |= {inst for inst, co, lvl, pw_, _ in _blocks(fbc.long_block_plan("INT8", part), H, Wd) if lvl == 0 and pw_}
    assert parts == set(fbc.INSTANCES)


@pytest.mark.parametrize("name,build,H,Wd,batch", ORACLE_CASES, ids=[f"{c[0]}-{c[2]}x{c[3]}x{c[4]}" for c in ORACLE_CASES])
def test_references_can_show_a_fault(name, build, H, Wd, batch):
    """At every size of the block cases: every int8 tensor a fused launch writes holds at least one 127 (the packing's clamp is taken) and at
    least one 0; every compared tensor is at least a quarter nonzero and no group of 16 channels is dead; no tensor saturates above 1 %."""
    x = fbc.case_input(H, Wd, batch)
    t0 = time.perf_counter()
    plan = fbc.prepare(build("INT8"), x, key=name)
    t1 = time.perf_counter()
    det, desc, vals = fbc.reference(plan, x)
    print(f"{name} at {H} x {Wd} x {batch}: scales {t1 - t0:.2f} s, INT8 oracle {time.perf_counter() - t1:.2f} s")
    fused = fbc.fused_writes(plan, fbc.fusion_table(plan, H, Wd))
    assert fused
    rates = {}
    for tid, (ch, lvl) in enumerate(plan.tensors):
        if tid == plan.input_tensor:
            continue
        v = vals[tid]
        assert v.shape == (batch, ch, H >> lvl, Wd >> lvl) and np.isfinite(v.astype(np.float64)).all()
        assert (v != 0).mean() >= 0.25, (tid, float((v != 0).mean()))
        for c0 in range(0, ch, 16):
            assert (v[:, c0:c0 + 16] != 0).mean() >= 0.1, (tid, c0)
        if v.dtype == np.int8:
            rates[tid] = float((np.abs(v.astype(np.int32)) == 127).mean())
            assert rates[tid] < 0.01, (tid, rates[tid])
            if tid in fused:
                assert (v == 127).any() and (v == 0).any() and v.min() >= 0, tid
    print("  saturation per int8 tensor (* written by a fused launch): " + " ".join(f"{t}{'*' if t in fused else ''}:{100 * r:.2f}%" for t, r in rates.items()))
    assert np.allclose(np.linalg.norm(desc, axis=1), 1.0, atol=1e-5)
