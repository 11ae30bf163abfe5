"""The numpy restatement of the BRISK extractor (tests/brisk_ref.py) on its own: the tables' invariants, the border rule, rotation
covariance, the regimes of `size`, and the property the GPU parity cases rely on -- none of their rows sits on a rotation boundary."""
import numpy as np
import pytest

from tests import brisk_cases as bc, brisk_ref as br


def test_tables_have_the_pair_counts_and_border_sizes():
    T = br.own_tables()
    assert T["short_pairs"].shape == (512, 2) and T["long_pairs"].shape == (870, 4)
    assert T["points"].shape == (64, 1024, 60, 3) and T["points"][..., 2].min() >= 0.5 and abs(T["points"][..., 2].min() - 0.65) < 1e-6
    assert T["size_list"][0] == 13 and np.all(np.diff(T["size_list"]) >= 0)
    assert T["scale_list"][0] == 1.0 and abs(float(T["scale_list"][63]) * 2 ** (np.log2(30.0) / 64) - 30.0) < 1e-4
    assert (T["short_pairs"][:, 0] > T["short_pairs"][:, 1]).all() and T["short_pairs"].max() < 60 and T["long_pairs"][:, :2].max() < 60
    # every pair is long or short or neither, never both; the weights are what |d| > 8.2 allows
    assert np.abs(T["long_pairs"][:, 2:]).max() <= int(2048 / 8.2 + 1)


def test_scale_index_regimes():
    assert br.scale_index([5.0, 7.0, 7.2]).tolist() == [0, 0, 0]                       # below the basic size: clamped to 0
    assert br.scale_index([12.3, 31.0, 60.0]).tolist() == [10, 27, 40]                  # middle scales
    assert br.scale_index([216.0, 1e6]).tolist() == [63, 63]                           # the cap (7.2 * 30 = 216 is scale 64)
    s = br.scale_index(np.linspace(7.3, 215, 500))
    assert np.all(np.diff(s) >= 0) and s.min() >= 0 and s.max() == 63


def test_border_rule_at_the_four_edges():
    rows, cols = 64, 96
    b = int(br.own_tables()["size_list"][0])
    xy = np.array([[b - 1, 30], [b, 30], [cols - b - 1, 30], [cols - b, 30], [40, b - 1], [40, b], [40, rows - b - 1], [40, rows - b],
                   [b - 0.001, 30], [cols - b - 0.001, 30], [np.nan, 30]], np.float32)
    keep, s = br.border_keep(xy, 7.0, (rows, cols))
    assert keep.tolist() == [1, 2, 5, 6, 9] and (s == 0).all()
    img, xy, size = bc.case("noise_grid")
    r = br.describe(img, xy, size)
    kept_xy = xy[r["kept"]]
    assert 0 < len(r["kept"]) < len(xy) and np.all(np.diff(r["kept"]) > 0)
    assert kept_xy[:, 0].min() == 13 and kept_xy[:, 0].max() == 82 and kept_xy[:, 1].min() == 13 and kept_xy[:, 1].max() == 50
    assert set(np.unique(r["scale"]).tolist()) == {0, 10}                              # sizes 31 and 60 drop everything at 64 x 96


def _blob_image(n=81):
    """smooth and asymmetric, no plateau: an off-centre paraboloid (a gradient of more than one grey level per pixel everywhere near the centre)"""
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    return np.clip(20 + 0.02 * (x - 10) ** 2 + 0.012 * (y + 5) ** 2, 0, 255).astype(np.uint8)


def test_rotating_the_image_by_90_degrees_rotates_the_angle_and_keeps_the_descriptor():
    """The keypoint is the centre pixel, which a quarter turn maps to itself.  The box means are exact area integrals, so the turned image
    offers the same intensities -- but to a rotation-0 pattern whose rings of 10, 14 and 15 points are not invariant under a quarter turn:
    the direction estimate moves by 90 degrees up to that sampling difference (observed on this image: 90.4 degrees, 257 rotation steps;
    bound: 1 degree, 2 steps), and on a smooth image the 512 comparisons do not notice a pattern turned by those few rotation steps."""
    img = np.ascontiguousarray(np.rot90(_blob_image(), 2))
    n = img.shape[0]
    c = (n - 1) // 2
    a = br.describe(img, np.array([[c, c]], np.float32), 7.0)
    rot = np.ascontiguousarray(np.rot90(img, -1))                                      # clockwise on the screen (y points down): angles + 90
    b = br.describe(rot, np.array([[c, c]], np.float32), 7.0)
    assert len(a["kept"]) == len(b["kept"]) == 1 and not a["boundary"][0] and not b["boundary"][0]
    assert 5 < a["angle"][0] < 85                                                      # both angles positive: the truncation of choice 13 treats them alike
    assert abs(float(b["angle"][0]) - float(a["angle"][0]) - 90.0) < 1.0
    assert abs(int(b["theta"][0]) - int(a["theta"][0]) - 256) <= 2
    assert np.array_equal(a["desc"], b["desc"]) and a["desc"].any() and not a["desc"].all()


def test_float_coordinates_and_every_size_regime_run():
    img = bc.smoothed_noise((700, 700), 3)
    xy = np.array([[350.25, 349.5], [330.75, 360.125]], np.float32)
    for size, scale in ((5.0, 0), (12.3, 10), (31.0, 27), (1000.0, 63)):
        r = br.describe(img, xy, size)
        assert r["kept"].tolist() == [0, 1] and (r["scale"] == scale).all()
        assert r["desc"].shape == (2, 64) and r["values0"].min() >= 0 and r["values0"].max() <= 256 * 1024   # (a box mean in 1/1024 grey levels)
        assert 20 < np.unpackbits(r["desc"], axis=1).sum(1).min() and np.unpackbits(r["desc"], axis=1).sum(1).max() < 492
    # a flat image: every box mean is 77 * 1024 up to the truncation of scaling2 = (int)(scaling * area / 1024), which depends on the ring's
    # sigma (4095 instead of 4096 on rings 0, 2 and 4 at scale 0: 78867 instead of 78848).  So under OpenCV's integer rules a flat image does
    # NOT give dir == 0 and an all-zero descriptor: rings differ by 19 / 1024 of a grey level, and comparisons between rings see it.
    flat = br.describe(np.full((64, 96), 77, np.uint8), [[40, 30]], 7.0)
    v = flat["values0"][0]
    ring = np.repeat(np.arange(5), br.RING_N)
    assert all(len(set(v[ring == k].tolist())) == 1 for k in range(5)) and (np.abs(v - 77 * 1024) <= 77 * 1024 // 4095 + 1).all()
    assert set(v.tolist()) == {78848, 78867} and flat["dir"].tolist() == [[5, 1]] and flat["desc"].any()


@pytest.mark.parametrize("name", bc.CASES + ["full_size"])
def test_the_gpu_parity_cases_have_no_row_on_a_rotation_boundary(sample_images, name):
    """What tests/test_gpu_brisk.py compares: no row of the seeded cases lies within 1e-4 rotation steps of a boundary, and the float32 atan2
    picks the same rotation on every row, so the descriptor comparison there excuses nothing.  Full size (golden image 0, FAST keypoints):
    the count is recorded here, the bound is 1 % of the rows."""
    img, xy, size = bc.image_case(name, sample_images)
    r = br.describe(img, xy, size)
    r32 = br.describe(img, xy, size, atan2_float32=True)
    nb = bc.boundary_rows(r)
    print(name, "keypoints", len(xy), "kept", len(r["kept"]), "boundary rows", nb, "theta differs float32 vs float64", int((r["theta"] != r32["theta"]).sum()))
    assert np.array_equal(r["kept"], r32["kept"]) and np.array_equal(r["values0"], r32["values0"])
    differ = r["theta"] != r32["theta"]
    assert not (differ & ~r["boundary"]).any()                                         # a rotation can only change on a boundary row
    if name == "full_size":
        assert len(r["kept"]) > 2000 and nb == FULL_SIZE_BOUNDARY_ROWS and nb <= 0.01 * len(r["kept"])
    else:
        assert nb == 0
        if name not in ("empty",):
            assert len(r["kept"]) > (5 if name == "flat" else 20)


FULL_SIZE_BOUNDARY_ROWS = 0
