"""Every instance of the fused INT8 block kernel dwpw_i8_kernel<G, STEM, POOL, EPI> and the three fused tails (heads_fused_kernel<false>,
heads_fused_kernel<true>, heads_i8_kernel) against the oracle, on the synthetic graphs of tests/fused_block_cases.py.

The shipped graphs reach six of the twelve block instances, and the fused tails only run at product sizes.  Here spvo_profile_stage_fused
reports, per pointwise op and for the tail, which fused launch ran and on what grid; the tests assert that the report equals
fbc.fusion_table(plan) -- the restatement of plan_int8_fusion -- and that the cases together reach every instance with a partial tile in
W, in H (non-stem) and with more tiles than workgroups.

Modes of a configuration (one oracle, shared):
  fused      the default tuning (FP32: "winograd" = 0, as elsewhere): two forward passes on one context, every tensor of both against the
             oracle -- the tensors a fused block skips too, which the synchronous entry points make the kernel store -- and the second
             pass bit-identical to the first.  The FP32 and FP16 engines of the same topology run dwconv3x3_kernel, dwconv3x3_f16_kernel
             and the 1x1 stems at partial shapes here, and all three precisions their fused tail.
  grid       INT8, "int8_fused" = 2: one workgroup per CU, so that a level-0 launch of the long plan (390 tiles at 120 x 392 x 2) has
             more tiles than workgroups: each workgroup walks several tiles, the loader wave prefetches across them.  Asserted from the
             library's report, not from a CU count.
  layerwise  INT8, "int8_fused" = 0: every tensor bit-identical to the fused run (and to the oracle): dwconv3x3_i8_kernel<true / false>,
             conv_first_i8_kernel<3, true, false> and <1, true, true> on partial tiles.
  product    "heads_keep_raw" = 0: no debug stores, desc_raw == NULL -- how a submission runs the kernels.  det, desc and every tensor
             that is not skipped are bit-identical to the fused run.

Bars (the project's, as in tests/test_gpu_conv_variants.py): INT8 every int8 tensor, the fp32 detector output and the un-normalised
descriptors bit for bit, the normalised descriptors within 1e-5; FP32 1e-4 * max(1, max|ref|) per tensor and 1e-4 on the descriptors;
FP16 4e-3 likewise.

Fused tails: the pixels of all images are one flat run of 16-pixel tiles (INT8: 32).  104 x 200 x 2 is 2 x 325 cells: the image boundary
lies inside a tile (325 = 20 * 16 + 5), 41 tiles on 21 workgroups are shares of two tiles and one of one -- the two-tile and the
one-tile step; 96 x 168 x 2 is 504 cells: the last 32-pixel INT8 tile is partial; one image on a context for two; 16 x 24 x 2 is 12
cells: one partial tile that holds both images.  A step WITH A SUCCESSOR (several steps per workgroup) needs more than 32 cells per CU,
8192 on 256 CUs: the product-size tests (tests/test_gpu_network.py, 45 x 147 x 2 and larger) cover it, no large case is added here.
"""
import time

import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import weights as W
from tests import conv_variant_cases as cvc
from tests import fused_block_cases as fbc

pytestmark = pytest.mark.gpu

ENGINE_TUNING = {"FP32": dict(winograd=0), "FP16": {}, "INT8": {}}
MODE_TUNING = {"fused": {}, "grid": dict(int8_fused=2), "layerwise": dict(int8_fused=0), "product": dict(heads_keep_raw=0)}
PLANS = {f"block{int(sp)}{int(sb)}": (lambda e, sp=sp, sb=sb: fbc.block_plan(e, sp, sb)) for sp, sb in fbc.STEMS}       # block<stem_pool><stem_bn>
PLANS.update({f"long-{part}": (lambda e, part=part: fbc.long_block_plan(e, part)) for part in fbc.LONG_PARTS})
PLANS["edge"] = cvc.edge_plan
BIG, MID, TINY = (104, 200), (96, 168), fbc.TINY_SIZE
HEAD_SIZES = {"104x200x2": BIG + (2, 2), "96x168x2": MID + (2, 2), "104x200x1of2": BIG + (1, 2), "16x24x2": TINY + (2, 2)}
HEAD_KIND = {"FP32": 1, "FP16": 2, "INT8": 3}
REL = {"FP32": 1e-4, "FP16": 4e-3}
DESC_TOL = {"FP32": 1e-4, "FP16": 4e-3, "INT8": 1e-5}


def _cases():
    """(engine, plan, size name, mode), the modes of one (engine, plan, size) side by side: they share its oracle"""
    out = []
    for p in [k for k in PLANS if k.startswith("block")]:
        for size in ("104x200x2", "96x168x2"):
            out += [("INT8", p, size, m) for m in ("fused", "layerwise", "product")]
            out += [(e, p, size, m) for e in ("FP32", "FP16") for m in ("fused", "product")]
    out += [("INT8", "block00", "104x200x1of2", m) for m in ("fused", "layerwise")]
    out += [("INT8", f"long-{part}", "120x392x2", "grid") for part in fbc.LONG_PARTS]
    # the fused tails alone: cvc's edge plan at the four sizes, the two-tensor and a one-tensor tail of the block plans at the two left
    for e in fbc.ENGINES:
        out += [(e, "edge", size, "fused") for size in HEAD_SIZES]
        out += [(e, p, size, "fused") for p in ("block10", "block01") for size in ("104x200x1of2", "16x24x2")]
    return out


SIZES = dict(HEAD_SIZES, **{"120x392x2": fbc.LONG_SIZE + (2, 2)})
CASES = _cases()
_refs, _records = {}, {}
_fused_first = {}                                                    # the newest fused run's first pass: what its layerwise / product neighbours compare with
_device_failed = []


def _reference(engine, pname, size, tmpdir):
    key = (engine, pname, size)
    if key not in _refs:
        while len(_refs) >= 2:
            _refs.pop(next(iter(_refs)))
        H, Wd, batch, _ = SIZES[size]
        x = fbc.case_input(H, Wd, batch)
        plan = PLANS[pname](engine)
        plan = cvc.prepare(plan, x) if pname == "edge" else fbc.prepare(plan, x, key=pname)
        path = str(tmpdir / W.engine_name(f"fused_{pname.replace('-', '_')}_{size}", 2, H, Wd, engine))
        W.save(plan, path)
        det, desc, vals = fbc.reference(plan, x)
        _refs[key] = dict(plan=plan, path=path, x=x, det=det, desc=desc.transpose(0, 2, 3, 1), vals=vals, table=fbc.fusion_table(plan, H, Wd))
    return _refs[key]


def _outputs(engine, size, mode, ref):
    """one context, one load, the forward passes of the mode: ([det, desc, {tensor: values}] per pass, fused-launch report per pointwise op,
    the tail's report, reports before the first pass)"""
    from spvo import capi
    H, Wd, batch, max_batch = SIZES[size]
    plan = ref["plan"]
    capi.clear_tuning()
    try:
        for k, v in dict(ENGINE_TUNING[engine], **MODE_TUNING[mode]).items():
            capi.set_tuning(k, v)
        ctx = capi.Context(net_height=H, net_width=Wd, max_batch=max_batch)
        ctx.load_weights(ref["path"])
        assert ctx.engine_precision() == engine
        before = {i: ctx.stage_fused(f"conv:{i}") for i in ref["table"]}
        before["heads"] = ctx.stage_fused("heads")
        passes = []
        for _ in range(1 if mode == "product" else 2):               # ("heads_keep_raw" and the grid of "int8_fused" are read at every pass)
            det, desc = ctx.forward(ref["x"])
            passes.append([det, desc, {tid: ctx.debug_tensor(tid, batch, ch, lvl) for tid, (ch, lvl) in enumerate(plan.tensors)
                                       if tid not in (plan.input_tensor, plan.desc_tensor)}])
        blocks = {i: ctx.stage_fused(f"conv:{i}") for i in ref["table"]}
        heads = ctx.stage_fused("heads")
        kernels = {i: ctx.stage_kernel(f"conv:{i}")[0] for i in ref["table"]}
        ctx.close()
    finally:
        capi.clear_tuning()
    return passes, blocks, heads, before, kernels


def _run(engine, pname, size, mode, tmpdir):
    key = (engine, pname, size, mode)
    if key in _records:
        return _records[key]
    if _device_failed:
        pytest.fail(f"not run: the device call of case {_device_failed[0]} failed before")
    from spvo import capi
    t0 = time.perf_counter()
    ref = _reference(engine, pname, size, tmpdir)
    plan, table = ref["plan"], ref["table"]
    H, Wd, batch, _ = SIZES[size]
    base = None
    if mode in ("layerwise", "product"):
        _run(engine, pname, size, "fused", tmpdir)
        base = _fused_first.get((engine, pname, size)) or _outputs(engine, size, "fused", ref)[0][0]
    try:
        passes, blocks, heads, before, kernels = _outputs(engine, size, mode, ref)
    except capi.SpvoError:
        _device_failed.append(key)
        raise
    fails = []
    if any(v is not None for v in before.values()):
        fails.append(f"a fused launch is reported before the first forward pass: {before}")
    # ---- the tensors a pass without the debug stores leaves untouched
    skipped = set()
    if mode == "product":
        skipped.add(plan.ops[-1].inp)                                 # the un-normalised descriptors (every engine's fused tail)
        if engine == "INT8":
            for i, inst in table.items():
                if inst:
                    skipped |= {plan.ops[i].inp} | ({plan.ops[0].out, plan.ops[1].out} if inst[1] else set())
    # ---- against the oracle
    worst = 0.0
    for n, (det, desc, tens) in enumerate(passes):
        for tid, got in list(tens.items()) + [("det", det)]:
            if tid in skipped:
                continue
            want = ref["det"] if tid == "det" else ref["vals"][tid]
            if engine == "INT8":
                bad = int((got != want.astype(np.float32)).sum())
                if bad:
                    worst = np.inf
                    fails.append(f"pass {n + 1}, tensor {tid}: {bad} of {got.size} values differ from the oracle")
            else:
                err, tol = float(np.abs(got - want).max()), REL[engine] * max(1.0, float(np.abs(want).max()))
                worst = max(worst, err / tol)
                if not err <= tol:
                    fails.append(f"pass {n + 1}, tensor {tid}: {err:.3g} > {tol:.3g}")
        err = float(np.abs(desc - ref["desc"]).max())
        worst = max(worst, err / DESC_TOL[engine])
        if not err <= DESC_TOL[engine]:
            fails.append(f"pass {n + 1}, descriptors: {err:.3g} > {DESC_TOL[engine]:.3g}")
    same = lambda p, q: [tid for tid in p[2] if tid not in skipped and not np.array_equal(p[2][tid], q[2][tid])] + \
        ([] if np.array_equal(p[0], q[0]) else ["det"]) + ([] if np.array_equal(p[1], q[1]) else ["desc"])
    if len(passes) == 2 and same(passes[0], passes[1]):
        fails.append(f"the second pass differs from the first in {same(passes[0], passes[1])}")
    if base is not None and same(passes[0], base):
        fails.append(f"the {mode} run differs from the fused run in {same(passes[0], base)}")
    # ---- the report: which launches were fused, their instance and grid
    rows = []
    for i, inst in table.items():
        lvl = plan.tensors[plan.ops[i - 1].inp][1]
        h, w = H >> lvl, Wd >> lvl
        tiles = ((h + 7) // 8) * ((w + 31) // 32) * batch
        rep = blocks[i]
        if engine != "INT8" or mode == "layerwise" or inst is None:
            if rep is not None:
                fails.append(f"conv:{i} reports a fused launch {rep} where none is planned")
            if engine == "INT8" and kernels[i] != "conv_i8_kernel":
                fails.append(f"conv:{i} runs {kernels[i]}")
            continue
        if rep is None or (rep["G"], rep["STEM"], rep["POOL"], rep["EPI"], rep["co_tiles"]) != inst or kernels[i] != "dwpw_i8_kernel":
            fails.append(f"conv:{i}: the library reports {rep} ({kernels[i]}), plan_int8_fusion restated gives {inst}")
            continue
        if rep["tiles"] != tiles or not 0 < rep["wgs"] <= tiles:
            fails.append(f"conv:{i}: {rep['tiles']} tiles on {rep['wgs']} workgroups, expected {tiles} tiles")
        if mode == "grid" and lvl == 0 and not rep["tiles"] > rep["wgs"]:
            fails.append(f"conv:{i}: {rep['tiles']} tiles on {rep['wgs']} workgroups: no workgroup walks a second tile")
        rows.append(dict(key=inst[:4], co=inst[4], W=w % 32 != 0, H=h % 8 != 0, M=rep["tiles"] > rep["wgs"], tiles=rep["tiles"], wgs=rep["wgs"], op=i))
    cells = batch * (H // 8) * (Wd // 8)
    px = 32 if engine == "INT8" else 16
    htiles = (cells + px - 1) // px
    if heads is None or heads["kind"] != HEAD_KIND[engine] or heads["tiles"] != htiles or not 0 < heads["wgs"] <= (htiles if engine == "INT8" else (htiles + 1) // 2):
        fails.append(f"the fused tail reports {heads}, expected kind {HEAD_KIND[engine]} on {htiles} tiles")
        heads = None
    if mode == "fused":
        _fused_first.clear()
        _fused_first[(engine, pname, size)] = passes[0]
    _records[key] = dict(fails=fails, rows=rows, heads=heads, worst=worst, cells=cells, seconds=time.perf_counter() - t0)
    return _records[key]


@pytest.fixture(scope="module")
def engine_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("fused_blocks")


@pytest.mark.parametrize("engine,pname,size,mode", CASES, ids=["-".join(c) for c in CASES])
def test_fused_case_matches_oracle(engine, pname, size, mode, engine_dir):
    rec = _run(engine, pname, size, mode, engine_dir)
    print(f"{engine} {pname} {size} {mode}: {rec['seconds']:.2f} s with the oracle, worst error / bar = {rec['worst']:.3g}; tail {rec['heads']}; " +
          ", ".join(f"conv:{r['op']}={r['key']}x{r['co']} {r['tiles']}/{r['wgs']}" for r in rec["rows"]))
    assert not rec["fails"], "\n".join(rec["fails"])


def test_cases_cover_the_block_instances(engine_dir):
    """Over the INT8 cases: the instances that ran are exactly launch_dwpw8's twelve; each ran with a partial tile in W and with more
    tiles than workgroups, the non-stem ones with a partial tile in H as well (a stem block reads level 0, whose height is a multiple
    of 8), and G = 4 and G = 8 each with one and with two tiles of 64 output channels."""
    recs = {c: _run(*c, engine_dir) for c in CASES if c[0] == "INT8" and c[3] in ("fused", "grid", "product")}
    seen, co = {}, {}
    for rec in recs.values():
        for r in rec["rows"]:
            seen.setdefault(r["key"], set()).update(f for f in "WHM" if r[f])
            co.setdefault(r["key"][0], set()).add(r["co"])
    print("dwpw_i8_kernel<G, STEM, POOL, EPI> x edges that ran (W / H: partial tile in width / height, M: more tiles than workgroups)")
    for k in sorted(seen):
        print(f"  {k}: {''.join(f if f in seen[k] else '-' for f in 'WHM')}")
    print(f"largest error / bar over {len(recs)} INT8 cases: {max(r['worst'] for r in recs.values()):.3g}")
    for e in ("FP32", "FP16"):
        sub = [_run(*c, engine_dir) for c in CASES if c[0] == e]
        print(f"largest error / bar over {len(sub)} {e} cases: {max(r['worst'] for r in sub):.3g}")
    assert set(seen) == set(fbc.INSTANCES), set(seen) ^ set(fbc.INSTANCES)
    short = {k: "".join(sorted(({"W", "M"} if k[1] else {"W", "H", "M"}) - f)) for k, f in seen.items()}
    assert not any(short.values()), short
    assert co == {4: {1, 2}, 8: {1, 2}}, co


def test_cases_cover_the_fused_tails(engine_dir):
    """The three fused tails at the four sizes, on a one-tensor and on the two-tensor tail; what each size is there for, from the report."""
    table = {}
    for c in CASES:
        if c[3] == "fused" and c[2] in HEAD_SIZES:
            rec = _run(*c, engine_dir)
            if rec["heads"]:
                table.setdefault((c[0], c[2]), []).append((c[1], rec["heads"], rec["cells"]))
    print("fused tail x size: plan tiles/workgroups")
    for (e, size), rows in sorted(table.items()):
        print(f"  {e} {size}: " + ", ".join(f"{p} {h['tiles']}/{h['wgs']}" for p, h, _ in rows))
    assert set(table) == {(e, s) for e in fbc.ENGINES for s in HEAD_SIZES}
    for e in fbc.ENGINES:
        for size in ("104x200x1of2", "16x24x2"):
            assert {"edge", "block10", "block01"} <= {p for p, _, _ in table[(e, size)]}, (e, size)     # block10: the two-tensor tail
        assert {"edge", "block10", "block00"} <= {p for p, _, _ in table[(e, "104x200x2")]}
        for _, h, cells in table[(e, "16x24x2")]:
            assert cells == 12 and h["tiles"] == 1 and h["wgs"] == 1            # one partial tile holds both images
    for e in ("FP32", "FP16"):
        for _, h, cells in table[(e, "104x200x2")]:
            assert (cells // 2) % 16 == 5 and h["tiles"] == 41 and h["wgs"] == 21   # the image boundary inside a tile; shares of two tiles and one of one
        for _, h, cells in table[(e, "104x200x1of2")]:
            assert h["tiles"] == 21 and h["wgs"] == 11 and cells % 16             # a partial last tile, in a one-tile step
    for _, h, cells in table[("INT8", "96x168x2")]:
        assert cells == 504 and cells % 32 and h["tiles"] == h["wgs"] == 16       # the last 32-pixel tile is partial
    for _, h, cells in table[("INT8", "104x200x2")]:
        assert (cells // 2) % 32 and h["tiles"] == 21                              # the image boundary inside a tile
