"""INT8 engines in the "int8_general" mode (spvo_set_int8_general / tuning "int8_general"): the squeeze graph as an INT8 engine.

The mode adds a stand-alone 2x2/2 max-pool between int8 tensors (maxpool2_i8_kernel) and convolutions whose cin is 16 more than a
multiple of 32 (conv_i8_kernel's ODD instances: a last chunk of one 16-channel group).  Reference: tests/int8_general_ref.py; cases:
tests/int8_general_cases.py -- the trained graph (tests/golden/sp_squeeze.spvw) and fire_plan, at 104 x 200 and 96 x 168.

Bars (the project's, tests/test_gpu_network.py::test_int8_engine_is_bit_exact): every int8 tensor, every fp32 tensor and the detector
output bit for bit; the L2-normalised descriptors (a float reduction whose order differs) within 1e-5.

With the mode off both files are refused as before, same status and same text (tests/engine_file_cases.py pins the rows).

Not tested: the loader's refusal of a stand-alone pool on an odd-sized map.  No engine file reaches it -- the network's size is a
multiple of 8 and a tensor's level is at most 3 (csrc/engine_file.h), so every map a pool may read has an even height and width.
"""
import numpy as np
import pytest

import oracle  # noqa: F401
from spvo import weights as W
from tests import engine_file_cases as efc
from tests import int8_general_cases as igc
from tests import int8_general_ref as ref

pytestmark = pytest.mark.gpu

CASES = [(kind, H, Wd) for kind in ("trained", "fire") for H, Wd in igc.EDGE_SIZES]
VARIANTS = [11, 12, 21, 22]
DESC_TOL = 1e-5
_refs = {}


@pytest.fixture(scope="module")
def engine_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("int8_general")


def _reference(kind, H, Wd, engine_dir):
    """plan, engine file, input (two images) and reference values of a case: computed once, shared, not changed"""
    key = (kind, H, Wd)
    if key not in _refs:
        if kind == "trained":
            x = igc.image_input(H, Wd, 2)
            plan = igc.trained_plan(x)
        else:
            x = igc.case_input(H, Wd, 2)
            plan, pools = igc.fire_plan()
            igc.prepare_fire(plan, pools, x)
        path = str(engine_dir / W.engine_name(f"general_{kind}", 2, H, Wd, "INT8"))
        W.save(plan, path)
        det, desc, vals = ref.forward(plan, x, return_all=True)
        _refs[key] = dict(plan=plan, path=path, x=x, det=det, desc=desc.transpose(0, 2, 3, 1), vals=vals)
    return _refs[key]


def _context(r, H, Wd, **tuning):
    from spvo import capi
    capi.clear_tuning()
    try:
        for k, v in tuning.items():
            capi.set_tuning(k, v)
        ctx = capi.Context(net_height=H, net_width=Wd)
        ctx.set_int8_general(True)
        ctx.load_weights(r["path"])
    finally:
        capi.clear_tuning()
    assert ctx.engine_precision() == "INT8"
    return ctx


def _compare(ctx, r, fails, tag=""):
    plan = r["plan"]
    det, desc = ctx.forward(r["x"])
    for tid, (ch, lvl) in enumerate(plan.tensors):
        if tid in (plan.input_tensor, plan.desc_tensor):
            continue
        got, want = ctx.debug_tensor(tid, 2, ch, lvl), r["vals"][tid]
        bad = int((got != want.astype(np.float32)).sum())
        if bad:
            fails.append(f"{tag}{'int8' if want.dtype == np.int8 else 'fp32'} tensor {tid}: {bad} of {got.size} values differ from the reference")
    if not np.array_equal(det, r["det"]):
        fails.append(f"{tag}detector output: {int((det != r['det']).sum())} values differ")
    err = float(np.abs(desc - r["desc"]).max())
    if not err <= DESC_TOL:
        fails.append(f"{tag}descriptors: {err:.3g} > {DESC_TOL}")
    return det, desc, err


@pytest.mark.parametrize("kind,H,Wd", CASES, ids=[f"{k}-{h}x{w}" for k, h, w in CASES])
def test_engine_is_bit_exact(kind, H, Wd, engine_dir):
    """Fails without the mode: no such symbol / tuning name, then the loader's refusal of the file."""
    r = _reference(kind, H, Wd, engine_dir)
    plan = r["plan"]
    assert igc.stand_alone_pools(plan) and igc.odd_group_convs(plan)
    ctx = _context(r, H, Wd)
    fails = []
    d1, s1, e1 = _compare(ctx, r, fails, "pass 1, ")
    d2, s2, _ = _compare(ctx, r, fails, "pass 2, ")            # what a first pass wrote outside its tiles is input of the second
    print(f"{kind} {H} x {Wd}: descriptor error {e1:.3g} (bar {DESC_TOL})")
    for i, op in enumerate(igc.library_ops(plan)):
        if op.type == W.OP_MAXPOOL:
            assert ctx.stage_kernel(f"pool:{i}")[0] == "maxpool2_i8_kernel"
        elif op.type == W.OP_CONV and op.cin % 32 == 16:
            v = ctx.stage_variant(f"conv:{i}")
            assert v and (v["ks"], v["ck"]) == (op.ksize, 32) and v["tiles"] > 0, (i, v)
    ctx.close()
    assert np.array_equal(d1, d2) and np.array_equal(s1, s2)
    assert not fails, "\n".join(fails)


def _allowed(ks, pool, wr, wc):
    """the tiles choose_variant offers a layer (tests/test_gpu_conv_variants.py)"""
    return not (pool and wr != 2) and not (ks == 1 and not pool and (wr, wc) == (2, 1))


@pytest.mark.parametrize("variant", VARIANTS)
def test_forced_tiles(variant, engine_dir):
    H, Wd = igc.EDGE_SIZES[0]
    r = _reference("fire", H, Wd, engine_dir)
    plan = r["plan"]
    ctx = _context(r, H, Wd, conv_variant=variant)
    fails = []
    _compare(ctx, r, fails)
    wr, wc = variant // 10, variant % 10
    ran, odd = [], []
    for i, op in enumerate(igc.library_ops(plan)):
        if op.type != W.OP_CONV or op.cin == 1:
            continue
        v = ctx.stage_variant(f"conv:{i}")
        assert v is not None and v["tiles"] > 0, i
        assert (v["ks"], bool(v["pool"])) == (op.ksize, bool(op.flags & W.FLAG_POOL)) and _allowed(v["ks"], v["pool"], v["wr"], v["wc"]), (i, v)
        if _allowed(op.ksize, bool(op.flags & W.FLAG_POOL), wr, wc):
            assert (v["wr"], v["wc"]) == (wr, wc), f"conv:{i} runs tile ({v['wr']}, {v['wc']}) although {variant} was forced and is a candidate"
            ran.append(i)
            if op.cin % 32 == 16:
                odd.append((i, op.cin, op.ksize))
    ctx.close()
    print(f"conv_variant={variant}: forced on stages conv:{ran}; with an odd group count (stage, cin, ks): {odd}")
    assert {k for _, _, k in odd} == {1, 3}, "the forced tile did not reach 1x1 and 3x3 layers with an odd group count"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind", ["trained", "fire"])
def test_batch_independence(kind, engine_dir):
    """Image 1 alone gives image 1 of the pair; four images per launch give two passes of two: the batch index of the pool kernel's grid
    and of the odd-chunk instances' tiles.  (Where a last chunk's missing group is staged from cannot show in any value -- its weights are
    zero --, so this does not guard the read behind the last image: that is a property of the kernel's address code, conv_i8.hip.h.)"""
    H, Wd = igc.EDGE_SIZES[0]
    r = _reference(kind, H, Wd, engine_dir)
    ctx = _context(r, H, Wd)
    x = r["x"]
    d, s = ctx.forward(x)
    assert np.array_equal(d, r["det"])
    d1, s1 = ctx.forward(x[1:2])
    assert np.array_equal(d1[0], d[1]) and np.array_equal(s1[0], s[1])
    more = igc.image_input(H, Wd, 4)[2:] if kind == "trained" else igc.case_input(H, Wd, 2, seed=9)
    x4 = np.concatenate([x, more])
    d4, s4 = ctx.forward(x4)
    dm, sm = ctx.forward(more)
    assert np.array_equal(d4[:2], d) and np.array_equal(s4[:2], s) and np.array_equal(d4[2:], dm) and np.array_equal(s4[2:], sm)
    assert not np.array_equal(dm, d)
    ctx.close()


def test_submissions_replay_launch_segments(engine_dir, golden_dir):
    """The submission path: the same pair submitted and collected for three rounds of the context's eight buffer sets.  A set's launch
    segments go out as plain launches on its first two visits and as replayed graphs from the third on (csrc/launch_segments.hip.h), so
    the third round runs the pool kernel and the odd-chunk instances from graphs.  Every submission gives the synchronous entry point's
    outputs, bit for bit."""
    import os
    from spvo import synth
    H, Wd = igc.EDGE_SIZES[0]
    r = _reference("trained", H, Wd, engine_dir)
    frames, _, P_l, P_r = synth.stereo_sequence(1, os.path.join(golden_dir, "images", "0000000000.png"), seed=0)
    L, R = frames[0]
    ctx = _context(r, H, Wd)
    want = ctx.detect(L, R, P_l, P_r, 0, 1)
    want = {k: np.array(want[k]) for k in ("xy_l", "xy_r", "desc_l", "desc_r")}
    assert len(want["xy_l"]) > 5 and len(want["xy_r"]) > 5
    rounds = 3
    for n in range(rounds * 8):
        ctx.detect_submit(L, R, 2 + 2 * (n % 2), 3 + 2 * (n % 2))
        got = ctx.detect_collect(P_l, P_r)
        for k in want:
            assert np.array_equal(got[k], want[k]), (n, k)
    prof = ctx.profile()
    replayed, plain = prof.get("segment_graph_launch", {}).get("calls", 0), prof.get("segment_plain_launch", {}).get("calls", 0)
    print(f"{rounds * 8} submissions: {replayed} segments replayed from graphs, {plain} as plain launches")
    ctx.close()
    assert replayed > 0 and plain > 0


def _load_error(ctx, path):
    from spvo import capi
    with pytest.raises(capi.SpvoError) as e:
        ctx.load_weights(path)
    return e.value.code, str(e.value)


def test_mode_off_keeps_the_refusals(engine_dir, tmp_path):
    from spvo import capi
    H, Wd = igc.EDGE_SIZES[0]
    files = [_reference(kind, H, Wd, engine_dir)["path"] for kind in ("trained", "fire")]
    pinned = {c.name: c for c in efc.CASES if c.name in ("int8 max-pool", "int8 chunk")}
    assert len(pinned) == 2
    assert capi.load().spvo_set_int8_general(None, 1) == -1           # SPVO_ERR_INVALID
    assert capi.get_tuning("int8_general", 0) == 0
    ctx = capi.Context(net_height=H, net_width=Wd)
    small = capi.Context(net_height=efc.NET_H, net_width=efc.NET_W)
    try:
        for step in ("default", "off after on"):
            if step == "off after on":
                for c in (ctx, small):
                    c.set_int8_general(True)
                    c.set_int8_general(False)
            for path in files:
                code, msg = _load_error(ctx, path)
                assert code == efc.IO and "INT8 engines have no stand-alone max-pool (squeeze graph)" in msg, (step, msg)
            for case in pinned.values():
                path = str(tmp_path / "case.spvw")
                efc.write(case, path)
                code, msg = _load_error(small, path)
                assert code == case.code and case.text in msg, (step, msg)
        # with the mode on the pinned rows pass the two refusals (and end, as the unbroken base plan does, at the bindings)
        small.set_int8_general(True)
        for case in pinned.values():
            path = str(tmp_path / "case.spvw")
            efc.write(case, path)
            code, msg = _load_error(small, path)
            assert code == efc.IO and "unexpected output tensors" in msg, msg
        # the process-wide default, read when a context is created; the call overrides it
        capi.set_tuning("int8_general", 1)
        try:
            c2 = capi.Context(net_height=H, net_width=Wd)
        finally:
            capi.clear_tuning()
        c2.load_weights(files[0])
        assert c2.engine_precision() == "INT8"
        c2.set_int8_general(False)
        assert _load_error(c2, files[0])[0] == efc.IO
        c2.close()
        with pytest.raises(capi.SpvoError):
            capi.set_tuning("int8_generals", 1)
    finally:
        ctx.close()
        small.close()


def test_mode_on_refuses_what_the_pool_kernel_cannot_do(tmp_path):
    from spvo import capi
    bad = {
        "channels": (efc.base(tensors={5: (32, 2)}, ops={4: efc.pool(3, 5, 64)}), "op 4: max-pool from 64 to 32 channels"),
        "level": (efc.base(tensors={5: (64, 1)}, ops={4: efc.pool(3, 5, 64)}), "op 4: level mismatch"),
        "fp32 tensor": (efc.base(tensors={5: (24, 2), 3: (24, 1)}, ops={2: efc.conv(2, 3, 64, 24, 1, 0), 3: efc.conv(2, 4, 64, 32, 3, 0), 4: efc.pool(3, 5, 24)}),
                        "op 4: max-pool of an INT8 engine between tensors that are not both int8"),
    }
    ctx = capi.Context(net_height=efc.NET_H, net_width=efc.NET_W)
    ctx.set_int8_general(True)
    try:
        for name, (plan, text) in bad.items():
            path = str(tmp_path / "bad.spvw")
            W.save(plan, path, precision="INT8")
            code, msg = _load_error(ctx, path)
            print(name, "->", msg)
            assert code == efc.IO and text in msg, (name, msg)
    finally:
        ctx.close()


def test_public_route_calibrate_save_load_forward(tmp_path, sample_images):
    """What bench.py --graph sp_squeeze --precision INT8 does with SPVO_TUNE_INT8_GENERAL unset: scales from the FP32 engine on the
    device (spvo.quant), the file saved and loaded (here with the per-context switch), a forward pass -- equal to the reference."""
    import os
    from spvo import capi, quant
    from tests.conftest import GOLDEN
    assert "SPVO_TUNE_INT8_GENERAL" not in os.environ and capi.get_tuning("int8_general", 0) == 0
    H, Wd = 120, 392
    plan = W.load(os.path.join(GOLDEN, "sp_squeeze.spvw"))
    x = quant.calibration_inputs(plan, sample_images[:2], H, Wd)
    plan.act_scales = quant.calibrate(plan, [x], H, Wd)
    path = str(tmp_path / W.engine_name("sp_squeeze", 2, H, Wd, "INT8"))
    W.save(plan, path, precision="INT8")
    plan = W.load(path)
    assert plan.precision == "INT8"
    ctx = capi.Context(net_height=H, net_width=Wd)
    ctx.set_int8_general(True)
    ctx.load_weights(path)
    assert ctx.engine_precision() == "INT8"
    det, desc = ctx.forward(x)
    ctx.close()
    rdet, rdesc = ref.forward(plan, x)
    assert np.isfinite(det).all() and np.array_equal(det, rdet)
    assert np.abs(desc - rdesc.transpose(0, 2, 3, 1)).max() <= DESC_TOL
