"""tests/sift_ref.py, the numpy restatement of SIFT that csrc/sift.hip.h is built against: its structure, two properties of the
algorithm on synthetic images, and the float32-versus-float64 yardsticks the GPU test's tolerances are derived from."""
import math

import numpy as np
import pytest

from tests import sift_cases as sc, sift_ref as sr


def test_level_shapes_and_octave_count_follow_the_rule():
    assert sr.octave_count(120, 392) == 7 and sr.level_shapes(120, 392) == [(240, 784), (120, 392), (60, 196), (30, 98), (15, 49), (7, 24), (3, 12)]
    assert sr.level_shapes(101, 147)[:3] == [(202, 294), (101, 147), (50, 73)]          # odd halving rounds down
    for rows, cols in ((6, 6), (64, 96), (101, 147), (376, 1241)):
        assert sr.octave_count(rows, cols) == int(round(math.log2(2 * min(rows, cols)) - 2)) + 1 >= 1
        gauss, dog = sr.pyramid(np.zeros((rows, cols), np.uint8)) if rows <= 101 else (None, None)
        if gauss is not None:
            assert [g[0].shape for g in gauss] == sr.level_shapes(rows, cols) and all(len(g) == 6 for g in gauss) and all(len(d) == 5 for d in dog)


def test_blur_taps_sum_to_one_and_the_border_map_is_valid_for_any_radius():
    for s in [sr.BASE_SIGMA] + sr.layer_sigmas():
        t = sr.blur_taps(s).astype(np.float64)
        total = 2 * t.sum() - t[0]
        print("sigma %.4f radius %d sum - 1 = %.3g" % (s, len(t) - 1, total - 1))
        assert abs(total - 1) <= np.finfo(np.float32).eps and len(t) - 1 <= 13 and np.all(np.diff(t) < 0)
    for n in (1, 2, 3, 7):
        m = sr.reflect101(np.arange(-40, 40), n)
        assert m.min() >= 0 and m.max() < n
        assert np.array_equal(sr.reflect101(np.arange(n), n), np.arange(n))
    assert list(sr.reflect101(np.arange(-3, 8), 4)) == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1]
    # a level smaller than the blur radius blurs without reading outside it
    assert sr.blur(np.arange(6, dtype=np.float32).reshape(2, 3), sr.layer_sigmas()[5]).shape == (2, 3)


@pytest.mark.parametrize("s0,cx,cy", [(3.0, 60.3, 40.7), (5.0, 64.25, 50.5)])
def test_a_gaussian_blob_is_found_at_its_place_and_scale(s0, cx, cy):
    """Conventions that enter the expectation: the doubled image samples the original at X / 2 - 0.25, so keypoint coordinates are the
    original's + 0.25 (OpenCV's, which does not compensate); `size` is twice the sigma of the NARROWER Gaussian of the difference that
    peaks, and a difference of Gaussians sigma, k sigma responds like the Laplacian at their geometric mean: blob sigma = size / 2 * sqrt(k)."""
    yy, xx = np.mgrid[0:96, 0:128].astype(np.float64)
    img = np.clip(np.rint(40 + 180 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s0 * s0))), 0, 255).astype(np.uint8)
    kp = sr.detect(img)["kp"]
    assert len(kp) >= 1
    best = kp[np.argmax(kp["response"])]
    print("blob", s0, (cx, cy), "->", best)
    assert abs(best["x"] - (cx + 0.25)) <= 0.1 and abs(best["y"] - (cy + 0.25)) <= 0.1
    assert abs(best["size"] / 2 * 2 ** (1 / 6) - s0) <= 0.05 * s0


def test_descriptor_of_the_rotated_image_equals_the_original_at_the_matching_keypoint():
    """np.rot90 maps base-image coordinates (X, Y) to (Y, 2 W - 1 - X): keypoint (x, y) to (y, W - 0.5 - x), and turns every gradient by
    a quarter turn.  Upsampling and blur are symmetric, so first-octave keypoints (no decimation, whose phase does not commute with the
    rotation) reappear with the same descriptor up to float rounding (rows and columns are blurred in the other order): at most one
    unit per value, the rounding to integers."""
    rs = np.random.RandomState(7)
    yy, xx = np.mgrid[0:80, 0:112].astype(np.float64)
    img = np.full(xx.shape, 30.0)
    for _ in range(14):
        cx, cy, s, a = rs.uniform(15, 97), rs.uniform(15, 65), rs.uniform(1.2, 2.5), rs.uniform(60, 200)
        e = rs.uniform(1.5, 2.5)
        th = rs.uniform(0, np.pi)
        u, v = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th), -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        img += a * np.exp(-(u * u / (2 * s * s * e * e) + v * v / (2 * s * s)))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    a, b = sr.detect(img), sr.detect(np.ascontiguousarray(np.rot90(img)))
    W = img.shape[1]
    first = [i for i in range(len(a["kp"])) if (a["kp"]["octave"][i] & 255) == 255]
    assert len(first) >= 5
    turns = set()
    for i in first:
        k = a["kp"][i]
        d = np.hypot(b["kp"]["x"] - k["y"], b["kp"]["y"] - (W - 0.5 - k["x"])) + np.abs(b["kp"]["size"] - k["size"])
        da = (b["kp"]["angle"].astype(np.float64) - float(k["angle"])) % 360
        j = int(np.argmin(d + np.minimum(np.abs(da - 90), np.abs(da - 270)) / 360))
        assert d[j] <= 1e-3, (k, b["kp"][j])
        turn = 90 if abs(da[j] - 90) < abs(da[j] - 270) else 270
        assert abs(da[j] - turn) <= 1e-2
        turns.add(turn)
        assert np.abs(a["desc"][i] - b["desc"][j]).max() <= 1, (k, b["kp"][j])
    assert len(turns) == 1


@pytest.mark.parametrize("name", sc.NAMES)
def test_output_is_sorted_duplicate_free_and_integer(name):
    out = sc.reference(name)
    kp, desc = out["kp"], out["desc"]
    assert len(kp) == len(desc) > 0
    rows = [tuple(r) for r in kp.tolist()]
    assert rows == sorted(rows) and len({r[:4] for r in rows}) == len(rows)
    assert desc.dtype == np.float32 and np.array_equal(desc, np.rint(desc)) and desc.min() >= 0 and desc.max() <= 255
    assert sc.image("flat").shape == (64, 64) and len(sr.detect(sc.image("flat"))["kp"]) == 0
    with pytest.raises(ValueError):
        sr.detect(np.zeros((5, 8), np.uint8))


# figure (a), figure (b) percentile 99 and maximum, largest angle difference in degrees -- measured by the test below
YARDSTICKS = {"kitti": (0.0, 0.0, 0.0, 3.0517578125e-05), "strided": (0.0, 0.0, 0.0, 2.288818359375e-05), "noise": (0.0, 0.0, 0.0, 3.0517578125e-05)}


@pytest.mark.parametrize("name", sc.NAMES)
def test_float32_versus_float64_yardsticks(name):
    """The stages that are not bit-exact (orientation, descriptor) at float32 and at float64 on the same pyramid and candidates: (a) the share
    of keypoints keyed by (octave, layer, row, column, 10-degree bin) on one side only, (b) the per-row largest absolute descriptor
    difference over the common keys.  Recorded in YARDSTICKS, from which tests/test_gpu_sift.py takes its tolerances."""
    c = sc.compare(sc.reference(name), sc.reference(name, "float64"))
    a, b99, bmax, ang = c["share"], float(np.percentile(c["desc"], 99)), float(c["desc"].max()), float(c["angle"].max())
    print(name, "keypoints", len(sc.reference(name)["kp"]), "(a) share on one side", a, "(b) percentile 50 / 99 / max", float(np.percentile(c["desc"], 50)), b99, bmax,
          "angle max", ang)
    assert (a, b99, bmax, ang) == YARDSTICKS[name]
    assert a <= 0.0025      # the condition under which tests/test_gpu_sift.py may use this input
