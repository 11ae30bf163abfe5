"""Every tile variant of conv_mfma_kernel (FP32 direct), conv_f16_kernel and conv_i8_kernel against the oracle.

The plan loader picks a tile per layer from a cost model (csrc/spvo_core.hip, choose_variant), so the rest of the suite runs whichever
variants the model picks at the sizes it uses.  Here the diagnostic switch "conv_variant" (spvo_set_tuning) forces each tile shape in
turn onto the synthetic graphs of tests/conv_variant_cases.py, spvo_profile_stage_variant reports what every layer ran and how its
persistent grid was filled, and the tests assert that the cases together reach the launchers' whole dispatch tables -- each key with a
partial tile in H, in W and in the output channels, and with more tiles than workgroups.

Bars (the project's, unchanged): FP32 1e-4 * max(1, max|ref|) per tensor and 1e-4 on the descriptors; FP16 4e-3 likewise; INT8 every
int8 tensor and the fp32 detector output bit for bit, 1e-5 on the descriptors.  Each case runs the forward pass twice on one context
and wants identical bits (what a first pass wrote outside its tiles is input of the second).

Cross-variant check: a tile shape changes which pixels a wave holds, not the accumulation chain of a pixel -- conv_mfma.hip.h and
conv_f16.hip.h start every accumulator from the bias and walk chunks, taps and channel pairs in one order whatever WR and WC are
(`for c < n_chunks`, `for st < NSTEP`), and the chunk size does not depend on the tile -- so the forced variants of one engine agree
with each other and with the model's choice BIT FOR BIT on every tensor.  INT8 has that from its oracle already.
"""
import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import weights as W
from tests import conv_variant_cases as cvc

pytestmark = pytest.mark.gpu

ENGINE_TUNING = {"FP32": dict(winograd=0, heads_fused=0), "FP16": dict(heads_fused=0), "INT8": dict(heads_fused=0)}   # (the fused tails, and the fused INT8 blocks, which these plans do not contain: tests/test_gpu_fused_blocks.py)
VARIANTS = [0, 11, 12, 21, 22]                                   # 0 = unset: the model's choice
CONFIGS = {                                                      # plan, H, W, batch, max_batch
    "edge-104x200": ("edge", 104, 200, 2, 2),
    "edge-96x168": ("edge", 96, 168, 2, 2),
    "long-120x392": ("long", 120, 392, 2, 2),
    "edge-104x200-one-of-two": ("edge", 104, 200, 1, 2),
    "edge-104x200-max-batch-1": ("edge", 104, 200, 1, 1),
}
CASES = [(e, c, v) for e in cvc.ENGINES for c in list(CONFIGS)[:3] for v in VARIANTS]
CASES += [(e, "edge-104x200-one-of-two", 12) for e in cvc.ENGINES] + [(e, "edge-104x200-max-batch-1", 0) for e in cvc.ENGINES]

# The launchers' dispatch tables as data: (kernel size, input channels per chunk, wr, wc, pooled).
_T3 = [(2, 2, 0), (2, 1, 0), (1, 2, 0), (1, 1, 0), (2, 2, 1), (2, 1, 1)]      # 3x3: four tiles unpooled, the two 8-row tiles pooled
_T1 = [(2, 2, 0), (1, 2, 0), (1, 1, 0), (2, 2, 1), (2, 1, 1)]                 # 1x1: no 8 x 32 tile unpooled
EXPECTED = {
    "FP32": dict(plain=[(3, 8) + t for t in _T3] + [(1, 16) + t for t in _T1], epi=[(1, 16) + t for t in _T1]),
    "FP16": dict(plain=[(3, 16) + t for t in _T3] + [(1, 32) + t for t in _T1] + [(1, 16) + t for t in _T1],
                 epi=[(1, 32) + t for t in _T1] + [(1, 16) + t for t in _T1]),
    "INT8": dict(plain=[(3, 32) + t for t in _T3] + [(1, 64) + t for t in _T1] + [(1, 32) + t for t in _T1],
                 epi=[(1, 64) + t for t in _T1] + [(1, 32) + t for t in _T1]),   # (one table, whose 1x1 entries also take the epilogues)
}
assert [len(EXPECTED[e]["plain"]) for e in cvc.ENGINES] == [11, 16, 16] and [len(EXPECTED[e]["epi"]) for e in cvc.ENGINES] == [5, 10, 10]
REL = {"FP32": 1e-4, "FP16": 4e-3}
DESC_TOL = {"FP32": 1e-4, "FP16": 4e-3, "INT8": 1e-5}


def _allowed(ks, pool, wr, wc):
    """the tiles choose_variant offers a layer"""
    return not (pool and wr != 2) and not (ks == 1 and not pool and (wr, wc) == (2, 1))


_refs, _base, _records = {}, {}, {}
_device_failed = []


def _reference(engine, config, tmpdir):
    """plan, engine file, input and oracle values of a configuration: computed once, shared by its variants (the newest two are kept)"""
    key = (engine, config)
    if key not in _refs:
        while len(_refs) >= 2:
            _refs.pop(next(iter(_refs)))
        kind, H, Wd, batch, _ = CONFIGS[config]
        x = cvc.case_input(H, Wd, batch)
        plan = cvc.prepare((cvc.edge_plan if kind == "edge" else cvc.long_plan)(engine), x)
        path = str(tmpdir / W.engine_name(f"variants_{kind}", 2, H, Wd, engine))
        W.save(plan, path)
        det, desc, vals = cvc.reference(plan, x)
        _refs[key] = dict(plan=plan, path=path, x=x, det=det, desc=desc.transpose(0, 2, 3, 1), vals=vals)
    return _refs[key]


def _outputs(engine, config, variant, ref):
    """one context, one load, two forward passes: ([det, desc, {tensor: values}] per pass, what every convolution ran, failures so far)"""
    from spvo import capi
    _, H, Wd, batch, max_batch = CONFIGS[config]
    plan = ref["plan"]
    fails = []
    capi.clear_tuning()
    try:
        for k, v in ENGINE_TUNING[engine].items():
            capi.set_tuning(k, v)
        if variant:
            capi.set_tuning("conv_variant", variant)
        ctx = capi.Context(net_height=H, net_width=Wd, max_batch=max_batch)
        ctx.load_weights(ref["path"])
    finally:
        capi.clear_tuning()                                       # (read when the engine is loaded)
    assert ctx.engine_precision() == engine
    convs = [i for i, op in enumerate(plan.ops) if op.type == W.OP_CONV and op.cin > 1]
    before = {i: ctx.stage_variant(f"conv:{i}") for i in convs}
    if any(v and (v["tiles"] or v["wgs"]) for v in before.values()):
        fails.append("a layer reports a launch before the first forward pass")
    passes = []
    for _ in range(2):
        det, desc = ctx.forward(ref["x"])
        passes.append([det, desc, {tid: ctx.debug_tensor(tid, batch, ch, lvl) for tid, (ch, lvl) in enumerate(plan.tensors)
                                   if tid not in (plan.input_tensor, plan.desc_tensor)}])
    layers = {}
    for i in convs:
        v = ctx.stage_variant(f"conv:{i}")
        op = plan.ops[i]
        if v is None:                                             # the second of two merged siblings: its channels belong to the launch in front
            prev = plan.ops[i - 1]
            if not (layers.get(i - 1) and prev.out == op.out and prev.out_c_off + prev.cout == op.out_c_off and prev.ksize == op.ksize == 3):
                fails.append(f"conv:{i} reports no tile variant")
            else:
                layers[i - 1]["cout"] += op.cout
            continue
        if (v["ks"], v["pool"]) != (op.ksize, bool(op.flags & W.FLAG_POOL)) or op.cin % v["ck"] or v["tiles"] <= 0 or not 0 < v["wgs"] <= v["tiles"] or v != dict(before[i] or {}, tiles=v["tiles"], wgs=v["wgs"]):
            fails.append(f"conv:{i}: inconsistent report {v}")
        layers[i] = dict(v, cout=op.cout, epi=1 if op.flags & W.FLAG_BN else 2 if op.flags & W.FLAG_ADD else 0, level=plan.tensors[op.inp][1])
    ctx.close()
    return passes, layers, fails


def _run(engine, config, variant, tmpdir):
    key = (engine, config, variant)
    if key in _records:
        return _records[key]
    if _device_failed:
        pytest.fail(f"not run: the device call of case {_device_failed[0]} failed before")
    from spvo import capi
    ref = _reference(engine, config, tmpdir)
    plan = ref["plan"]
    _, H, Wd, batch, _ = CONFIGS[config]
    try:
        passes, layers, fails = _outputs(engine, config, variant, ref)
        base = None
        if engine != "INT8" and variant:                          # the model's own choice on the same engine and input
            if (engine, config) not in _base:
                _base.clear()
                _base[(engine, config)] = _outputs(engine, config, 0, ref)[0][0]
            base = _base[(engine, config)]
        elif engine != "INT8":
            _base.clear()
            _base[(engine, config)] = passes[0]
    except capi.SpvoError:
        _device_failed.append(key)
        raise
    worst = 0.0                                                   # largest error of the case as a fraction of its bar (INT8: 0 or inf)
    for n, (det, desc, tens) in enumerate(passes):
        for tid, got in list(tens.items()) + [("det", det)]:
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
    (d1, s1, t1), (d2, s2, t2) = passes
    diff = [tid for tid in t1 if not np.array_equal(t1[tid], t2[tid])] + ([] if np.array_equal(d1, d2) else ["det"]) + ([] if np.array_equal(s1, s2) else ["desc"])
    if diff:
        fails.append(f"the second pass differs from the first in {diff}")
    if base is not None:
        diff = [tid for tid in t1 if not np.array_equal(t1[tid], base[2][tid])] + ([] if np.array_equal(d1, base[0]) else ["det"]) + ([] if np.array_equal(s1, base[1]) else ["desc"])
        if diff:
            fails.append(f"variant {variant} differs from the model's choice in {diff}")
    for i, v in layers.items():
        if variant and _allowed(v["ks"], v["pool"], variant // 10, variant % 10) and (v["wr"], v["wc"]) != (variant // 10, variant % 10):
            fails.append(f"conv:{i} runs tile ({v['wr']}, {v['wc']}) although {variant} was forced and is a candidate")
        if not _allowed(v["ks"], v["pool"], v["wr"], v["wc"]):
            fails.append(f"conv:{i} runs tile ({v['wr']}, {v['wc']}), which the model never offers it")
    rows = []
    for i, v in layers.items():
        h, w = H >> v["level"], Wd >> v["level"]
        rows.append(dict(key=(v["ks"], v["ck"], v["wr"], v["wc"], int(v["pool"])), epi=v["epi"], H=h % (4 * v["wr"]) != 0, W=w % (32 * v["wc"]) != 0,
                         C=v["cout"] % 64 != 0, M=v["tiles"] > v["wgs"], tiles=v["tiles"], wgs=v["wgs"], op=i))
    _records[key] = dict(fails=fails, rows=rows, worst=worst)
    return _records[key]


@pytest.fixture(scope="module")
def engine_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("conv_variants")


@pytest.mark.parametrize("engine,config,variant", CASES, ids=[f"{e}-{c}-v{v}" for e, c, v in CASES])
def test_variant_matches_oracle(engine, config, variant, engine_dir):
    rec = _run(engine, config, variant, engine_dir)
    print(f"{engine} {config} conv_variant={variant}: worst error / bar = {rec['worst']:.3g}; " +
          ", ".join(f"conv:{r['op']}={r['key']}{'e' if r['epi'] else ''} {r['tiles']}/{r['wgs']}" for r in rec["rows"]))
    assert not rec["fails"], "\n".join(rec["fails"])


@pytest.mark.parametrize("engine", cvc.ENGINES)
def test_cases_cover_the_dispatch_tables(engine, engine_dir):
    """Over the cases of one engine: the keys that ran are exactly the launcher's tables, and each ran with a partial tile in H, in W, in
    the output channels, and with more tiles than workgroups."""
    recs = {(c, v): _run(engine, c, v, engine_dir) for e, c, v in CASES if e == engine}
    seen = {"plain": {}, "epi": {}}
    for rec in recs.values():
        for r in rec["rows"]:
            flags = seen["epi" if r["epi"] else "plain"].setdefault(r["key"], set())
            flags |= {f for f in "HWCM" if r[f]}
    print(f"{engine}: key (ks, channels per chunk, wr, wc, pooled) x edges that ran (H / W / C: partial tile in height / width / output channels, M: more tiles than workgroups)")
    for table in ("plain", "epi"):
        for k in sorted(seen[table], reverse=True):
            print(f"  {table:5s} {k}: {''.join(f if f in seen[table][k] else '-' for f in 'HWCM')}")
    print(f"{engine}: largest error / bar over {len(recs)} cases: {max(r['worst'] for r in recs.values()):.3g}")
    for table in ("plain", "epi"):
        assert set(seen[table]) == set(EXPECTED[engine][table]), (table, set(seen[table]) ^ set(EXPECTED[engine][table]))
        short = {k: "".join(sorted(set("HWCM") - f)) for k, f in seen[table].items() if f != set("HWCM")}
        assert not short, (table, short)
