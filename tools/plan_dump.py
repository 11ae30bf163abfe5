"""What the plan loader decided for an engine, and what the engine then computes: one line per stage in spvo_profile_get order (name,
kernel family and factor, tile variant and grid of its launch in one forward pass of a seeded input), then a SHA-256 of det, desc and
every tensor.  Two builds of the library that print the same lines made the same plan and run the same arithmetic.

usage: plan_dump.py GRAPH HxW PRECISION [name=value ...]      GRAPH: vgg | sp_squeeze | sp_mbv1 | sp_mbv2 | path of a .spvw file
                                                               PRECISION: FP32 | FP16 | INT8 | SPLIT; name=value: spvo_set_tuning
       plan_dump.py --matrix                                   the graphs, sizes, precisions and tunings of profiles/loader_steps.log
SPVO_LIB_DIR selects a side build of the library (spvo/capi.py).
"""
import hashlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "superpoint-stereo-visual-odometry_amd"))
import numpy as np

import oracle  # noqa: F401
from oracle import net_int8
from spvo import capi, weights

SWITCHES = ["winograd", "wino4", "wino4_item", "wino_narrow", "wino_dynamic", "merge_siblings", "heads_fused", "heads_split", "int8_fused", "preprocess_fused"]
TUNINGS = [{}] + [{s: 0} for s in SWITCHES] + [{"conv_variant": v} for v in (11, 12, 21, 22)]
_plans = {}


def plan_of(graph, H, W, precision):
    """the graph's plan at that precision (INT8: calibrated on the first image of the seeded input, as tests/test_gpu_network.py does)"""
    key = (graph, H, W, precision == "INT8")
    if key not in _plans:
        p = weights.vgg_plan() if graph == "vgg" else weights.load(graph if os.path.exists(graph) else os.path.join(ROOT, "tests", "golden", graph + ".spvw"))
        if precision == "INT8":
            p.act_scales = net_int8.calibrate(p, [seeded_input(H, W)[:1]])
        _plans[key] = p
    return _plans[key]


def seeded_input(H, W):
    return np.random.RandomState(0).rand(2, 1, H, W).astype(np.float32)


def dump(graph, H, W, precision, tunings, out=sys.stdout):
    plan = plan_of(graph, H, W, precision)
    capi.clear_tuning()
    for k, v in tunings.items():
        capi.set_tuning(k, v)
    print(f"== {os.path.basename(graph)} {H}x{W} {precision} {' '.join(f'{k}={v}' for k, v in tunings.items())}".rstrip(), file=out)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "engine.spvw")
        weights.save(plan, path, "FP32" if precision == "SPLIT" else precision)
        ctx = capi.Context(net_height=H, net_width=W)
        ctx.set_fp32_split(precision == "SPLIT")
        try:
            ctx.load_weights(path)
        except capi.SpvoError as e:      # (sp_squeeze as INT8: its stand-alone max-pools) -- the answer is the dump
            print("refused:", str(e).replace(path, "<file>"), file=out)
            ctx.close()
            return
    x = seeded_input(H, W)
    det, desc = ctx.forward(x)
    for name in ctx.profile():
        line = name
        if name.split(":")[0] in ("conv", "dwconv"):
            line += " %s %.6g" % ctx.stage_kernel(name)
        if name.startswith("conv:"):
            v = ctx.stage_variant(name)
            line += " " + (" ".join(str(int(v[k])) for k in ("ks", "ck", "wr", "wc", "pool", "tiles", "wgs")) if v else "0 0 0 0 0 0 0")
        print(line, file=out)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    print("det", sha(det), file=out)
    print("desc", sha(desc), file=out)
    for tid, (ch, lvl) in enumerate(plan.tensors):
        if tid not in (plan.input_tensor, plan.desc_tensor):
            print("tensor", tid, sha(ctx.debug_tensor(tid, 2, ch, lvl)), file=out)
    ctx.close()
    capi.clear_tuning()


def matrix():
    for graph, sizes in (("vgg", [(360, 1176), (240, 784), (120, 392), (64, 96)]), ("sp_squeeze", [(360, 1176), (64, 96)]),
                         ("sp_mbv1", [(360, 1176), (64, 96)]), ("sp_mbv2", [(360, 1176), (64, 96)])):
        for H, W in sizes:
            for precision in ("FP32", "FP16", "INT8") + (("SPLIT",) if graph == "vgg" else ()):
                for t in (TUNINGS if precision in ("FP32", "INT8") else [{}]):
                    dump(graph, H, W, precision, t)
                    sys.stdout.flush()


if __name__ == "__main__":
    if sys.argv[1:] == ["--matrix"]:
        matrix()
    else:
        H, W = (int(v) for v in sys.argv[2].split("x"))
        dump(sys.argv[1], H, W, sys.argv[3], {k: int(v) for k, v in (a.split("=") for a in sys.argv[4:])})
