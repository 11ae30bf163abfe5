"""What spvo_load_weights answers to a malformed engine file, and what state it leaves the context in.

Every row of tests/engine_file_cases.py is one load of a file with one defect: the status and the text are pinned.  Three properties
of the context's state, each with bit-equal outputs: a defect found on the file's bytes alone keeps the engine loaded before; a
defect found later leaves the context without an engine; and such a context loads and runs a good engine again as a fresh one does.
"""
import numpy as np
import pytest

from tests import engine_file_cases as cases

pytestmark = pytest.mark.gpu

H, W = cases.NET_H, cases.NET_W


def _x():
    return np.random.RandomState(5).rand(2, 1, H, W).astype(np.float32)


@pytest.fixture(scope="module")
def ctx():
    from spvo import capi
    c = capi.Context(net_height=H, net_width=W)
    yield c
    c.close()


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """the good engine's file, and what a fresh context computes with it"""
    from spvo import capi, weights
    path = str(tmp_path_factory.mktemp("engine") / "good.spvw")
    weights.save(cases.good(), path)
    c = capi.Context(net_height=H, net_width=W)
    c.load_weights(path)
    det, desc = c.forward(_x())
    c.close()
    assert np.isfinite(det).all() and np.isfinite(desc).all() and np.abs(det).max() > 0
    return path, det, desc


@pytest.fixture(scope="module")
def ctx_good(good):
    from spvo import capi
    c = capi.Context(net_height=H, net_width=W)
    c.load_weights(good[0])
    yield c
    c.close()


def _refused(c, case, path):
    from spvo import capi
    cases.write(case, path)
    c.set_fp32_split(case.engine == "SPLIT")
    try:
        with pytest.raises(capi.SpvoError) as e:
            c.load_weights(path)
    finally:
        c.set_fp32_split(False)
    print(case.name, "->", e.value)
    assert e.value.code == case.code
    msg = str(e.value)
    assert msg.endswith(case.text) if case.level == "file" else case.text in msg, msg


def _no_engine(c):
    from spvo import capi
    with pytest.raises(capi.SpvoError) as e:
        c.forward(_x())
    assert e.value.code == cases.STATE
    with pytest.raises(capi.SpvoError) as e:
        c.engine_precision()
    assert e.value.code == cases.STATE


def _same_as(c, good):
    det, desc = c.forward(_x())
    assert np.array_equal(det, good[1]) and np.array_equal(desc, good[2])


@pytest.mark.parametrize("case", cases.CASES, ids=[c.name for c in cases.CASES])
def test_refusal(ctx, case, tmp_path):
    _refused(ctx, case, str(tmp_path / "case.spvw"))


def test_submissions_in_flight(good, sample_images, kitti_P, tmp_path):
    from spvo import capi
    c = capi.Context(net_height=H, net_width=W)
    c.load_weights(good[0])
    c.detect_submit(sample_images[0], sample_images[0], 2, 3)
    with pytest.raises(capi.SpvoError) as e:
        c.load_weights(good[0])
    assert e.value.code == cases.STATE and "detector submissions are in flight" in str(e.value)
    c.detect_collect(*kitti_P)
    _same_as(c, good)                                   # the engine was not touched
    c.close()


@pytest.mark.parametrize("case", cases.FILE_CASES, ids=[c.name for c in cases.FILE_CASES])
def test_file_level_failure_keeps_the_engine(ctx_good, good, case, tmp_path):
    _refused(ctx_good, case, str(tmp_path / "case.spvw"))
    assert ctx_good.engine_precision() == "FP32"
    _same_as(ctx_good, good)


LATE = [c for c in cases.LATE_CASES if c.name in ("kernel size 5", "split max-pool", "outputs int8")]


@pytest.mark.parametrize("case", LATE, ids=[c.name for c in LATE])
def test_late_failure_leaves_no_engine_and_the_context_recovers(good, case, tmp_path):
    from spvo import capi
    c = capi.Context(net_height=H, net_width=W)
    c.load_weights(good[0])
    _refused(c, case, str(tmp_path / "case.spvw"))
    _no_engine(c)
    c.load_weights(good[0])
    _same_as(c, good)
    c.close()
