"""tests/sift_describe_ref.py, the numpy restatement of the SIFT extractor on given keypoints that spvo_sift_describe is built against:
that its descriptor is sift_ref's arithmetic, its pyramids, what it gives for the detector's own records, the float32-versus-float64
yardsticks the GPU test's tolerances are derived from, and what of the new call is visible without a device."""
import ctypes as C
import os

import numpy as np
import pytest

from spvo import capi, host
from tests import sift_cases as sc, sift_describe_cases as dc, sift_describe_ref as sd, sift_ref as sr


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_scl_parameterised_descriptor_is_sift_refs_arithmetic(T):
    """Handed scl = 1.6 * 2^((l + xi) / 3) and the rounded point, sd.descriptor equals sr.descriptor bit for bit -- on every third refined
    candidate of "kitti" and "noise" (all octaves), at the angle of its first orientation peak and at -1."""
    n = 0
    for name in ("kitti", "noise"):
        st = sc.stage(name)
        for (o, l, r, c, xi, xr, xc, _) in st["cand"][::3]:
            G = st["gauss"][o][l]
            ptx, pty = sr.F(c) + xc, sr.F(r) + xr
            peaks = sr.orientations(G, l, r, c, xi, T)
            for angle in ([peaks[0]] if peaks else []) + [sr.F(-1)]:
                want = sr.descriptor(G, l, ptx, pty, xi, angle, T)
                got = sd.descriptor(G, sr._scl(l, xi, T), int(np.rint(ptx)), int(np.rint(pty)), angle, T)
                assert np.array_equal(bits(got), bits(want)), (name, o, l, r, c)
                n += 1
    assert n > 100


def test_unpacking_and_extent():
    o, layer, scale = sd.unpack(np.array([0, 255, 0x0305, 0x7B0201, sd.pack(-1, 4), 254], np.int32))
    assert o.tolist() == [0, -1, 5, 1, -1, -2] and layer.tolist() == [0, 0, 3, 2, 4, 0]
    assert scale.dtype == np.float32 and scale.tolist() == [1.0, 2.0, 1 / 32, 0.5, 2.0, 4.0]
    kp = dc.records([1.0, 2.0], [1.0, 2.0], [3.0, 3.0], [0.0, 0.0], [sd.pack(2, 1), sd.pack(4, 0)])
    assert sd.extent(kp) == (0, 5)                                           # octave 0 is always built
    kp["octave"][0] = sd.pack(-1, 1)
    assert sd.extent(kp) == (-1, 6)
    for bad in (dict(x=np.nan), dict(y=np.inf), dict(size=0.0), dict(size=-1.0), dict(size=np.inf), dict(angle=np.nan), dict(octave=254), dict(octave=sd.pack(0, 6)),
                dict(octave=sd.pack(7, 0))):
        k = dc.records([5.0], [5.0], [3.0], [0.0], [0])
        for f, v in bad.items():
            k[f] = v
        with pytest.raises(ValueError):
            sd.check((64, 96), k)
    sd.check((64, 96), dc.records([5.0], [5.0], [3.0], [-1.0], [sd.pack(6, 5)]))      # 64 >> 6 = 1: the last octave with a level
    with pytest.raises(ValueError):
        sd.check((5, 96), np.zeros(0, sr.KP_DTYPE))


def test_pyramid_shapes_and_levels():
    """first == 0: the level shapes halve rounding down from rows x cols.  A list containing octave -1: the Gaussian levels are
    sift_ref.pyramid's, bit for bit."""
    assert sd.level_shapes(101, 147, 0, 4) == [(101, 147), (50, 73), (25, 36), (12, 18)]
    assert sd.level_shapes(101, 147, -1, 3) == sr.level_shapes(101, 147)[:3]
    img = np.ascontiguousarray(sc.image("strided"))
    g = sd.pyramid(img, 0, 4)
    assert [lv[0].shape for lv in g] == sd.level_shapes(101, 147, 0, 4) and all(len(lv) == 6 and all(a.dtype == np.float32 and a.shape == lv[0].shape for a in lv) for lv in g)
    assert np.array_equal(bits(g[0][0]), bits(sr.blur(img.astype(np.float32), sd.BASE_SIGMA_0)))
    kp = dc.records([5.0, 6.0], [5.0, 6.0], [3.0, 3.0], [0.0, 0.0], [sd.pack(-1, 1), sd.pack(1, 2)])
    first, n_oct = sd.extent(kp)
    assert (first, n_oct) == (-1, 3)
    for name in ("strided", "noise"):
        img = np.ascontiguousarray(sc.image(name))
        g = sd.pyramid(img, first, n_oct)
        want = sc.stage(name)["gauss"]
        for o in range(n_oct):
            for i in range(6):
                assert g[o][i].shape == want[o][i].shape and np.array_equal(bits(g[o][i]), bits(want[o][i])), (name, o, i)


def test_the_detectors_own_records_get_their_own_rows_back():
    """Re-describing sift_cases.reference("kitti")'s records: the two paths differ only in float rounding of position and scale (the record
    carries (c + xc) * 2^o * 0.5 and a size rounded from double), so a value can flip one integer.  Measured: 286 of 287 rows identical,
    largest difference 1."""
    ref = sc.reference("kitti")
    got = sd.describe(sc.image("kitti"), ref["kp"], gauss=sc.stage("kitti")["gauss"])
    d = dc.row_difference(got, ref["desc"])
    print("own records:", int((d == 0).sum()), "of", len(d), "rows identical, largest difference", float(d.max()))
    assert len(d) > 100 and d.max() <= 1


def test_rows_are_in_order_and_an_empty_patch_is_zero():
    img = np.ascontiguousarray(sc.image("noise"))
    kp = dc.records([10.0, -300.0, 40.0, 10.0], [10.0, 20.0, 900.0, 10.0], [7.0, 7.0, 7.0, 7.0], [-1.0, -1.0, -1.0, -1.0], [0, 0, 0, 0])
    d = sd.describe(img, kp)
    assert d.shape == (4, 128) and d.dtype == np.float32
    assert d[0].any() and not d[1].any() and not d[2].any() and np.array_equal(d[3], d[0])
    assert np.array_equal(sd.describe(img, kp[::-1]), d[::-1])
    assert sd.describe(img, kp[:0]).shape == (0, 128)


# per list: records, percentile 99 and maximum of the per-row largest float32 / float64 difference -- measured by the test below
YARDSTICKS = {"fast": (1224, 0.0, 1.0), "handmade": (300, 0.0, 0.0), "brisk_style": (120, 0.0, 0.0)}


@pytest.mark.parametrize("name", list(YARDSTICKS))
def test_float32_versus_float64_yardsticks(name):
    """The descriptor at float32 and at float64 on the same pyramid, row by row: recorded in YARDSTICKS, from which
    tests/test_gpu_sift_describe.py takes its tolerances.  An input may be used on the GPU if its percentile 99 is at most 1."""
    d = dc.row_difference(dc.reference(name), dc.reference(name, "float64"))
    p99, dmax = float(np.percentile(d, 99)), float(d.max())
    print(name, "records", len(d), "percentile 50 / 99 / max", float(np.percentile(d, 50)), p99, dmax, "rows that differ", int((d > 0).sum()))
    assert (len(d), p99, dmax) == YARDSTICKS[name]
    assert p99 <= 1
    if name == "handmade":
        o, layer, _ = sd.unpack(dc.keypoints(name)["octave"])
        assert set(o.tolist()) == set(range(-1, 6)) and set(layer.tolist()) == set(range(6))


def test_the_call_is_declared_and_refuses_a_null_context():
    lib = capi.load()
    assert "spvo_sift_describe" in capi.SYMBOLS and hasattr(lib, "spvo_sift_describe") and callable(capi.Context.sift_describe)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spvo.h")) as f:
        assert "int spvo_sift_describe(spvo_ctx *ctx, const uint8_t *img" in f.read()
    img = (C.c_uint8 * (64 * 96))()
    rec = (C.c_uint8 * 24)()
    out = (C.c_float * 128)()
    assert lib.spvo_sift_describe(None, img, 64, 96, 96, rec, 1, out) == -1
    assert lib.spvo_sift_describe(None, None, 64, 96, 0, None, 0, None) == -1


def test_the_five_pairs_are_in_the_table():
    """kClassicPairs through the refusal text of a pair that does not run (no device is needed to be refused)."""
    img = np.zeros((64, 96), np.uint8)
    P = np.eye(3, 4)
    n, counts, err = host.classic_pair_probe("BRISK", "ORB", img, img, P, P)
    assert n == 0 and not counts.any()
    for d in ("ShiTomasi", "FAST", "ORB", "BRISK", "AKAZE"):
        assert d + " + SIFT" in err, (d, err)
    assert "SIFT + SIFT" in err and "BRISK + ORB" not in err
