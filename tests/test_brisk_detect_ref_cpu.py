"""CPU checks of tests/brisk_detect_ref.py, the numpy restatement that defines the BRISK detector of csrc/brisk_detect.hip.h: the
scale space's shapes and samplers, the purity of the score read that lets the kernels use a dense map, the coverage the parity cases of
tests/brisk_detect_cases.py are meant to have (every layer, the tie branch of isMax2D), and that the detector selects scale."""
import numpy as np
import pytest

from tests import brisk_detect_cases as bc, brisk_detect_ref as bd, classic_ref as cr

f32 = np.float32


def test_layer_shapes_scales_offsets():
    assert bd.layer_shapes(376, 1241) == [(376, 1241), (250, 826), (188, 620), (125, 413), (94, 310), (62, 206)]
    assert bd.layer_shapes(97, 131) == [(97, 131), (64, 86), (48, 65), (32, 43), (24, 32), (16, 21)]
    assert bd.layer_shapes(8, 8) == [(8, 8), (4, 4), (4, 4), (2, 2), (2, 2), (1, 1)]
    assert [float(s) for s in bd.layer_scales()] == [1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert [float(o) for o in bd.layer_offsets()] == [0.0, 0.25, 0.5, 1.0, 1.5, 2.5]
    for name in bc.CASES:
        layers = bc.reference(name)[0]
        assert [L.im.shape for L in layers] == bd.layer_shapes(*bc.case(name)[0].shape)


def test_half_sampler_on_exact_ratios_is_the_rounded_mean():
    img = bc.case("exact")[0]
    layers = bc.reference("exact")[0]
    for i in (2, 3, 4, 5):                                                      # 96 x 144: every half is exact (layers 0 .. 3 have even sizes)
        s = layers[i - 2].im.astype(np.int32)
        assert s.shape == (2 * layers[i].h, 2 * layers[i].w)
        assert np.array_equal(layers[i].im, (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2)
    assert layers[0].im is not None and np.array_equal(layers[0].im, img)


def test_area_taps():
    """the taps of a destination cell are contiguous, at most 6, and their float weights add up to 1 within rounding; two-thirds of an exact
    ratio is the 2 : 1 / 1 : 2 pattern; the inexact case takes the general path on every layer that can: layer 3 is the half of layer 1, whose
    sizes 2 * (n / 3) are even by construction, so it is an exact half for EVERY image"""
    for ssize, dsize in ((144, 96), (131, 86), (97, 48), (65, 32), (8, 4), (5, 2), (3, 1), (1241, 826), (413, 206)):
        for taps in bd.area_tab(ssize, dsize):
            idx = [s for s, _ in taps]
            assert idx == list(range(idx[0], idx[0] + len(idx))) and 0 <= idx[0] and idx[-1] < ssize and len(idx) <= 6
            assert abs(sum(float(a) for _, a in taps) - 1.0) < 1e-6
    t = bd.area_tab(144, 96)
    assert t[0] == [(0, f32(1 / 1.5)), (1, f32(0.5 / 1.5))] and t[1] == [(1, f32(0.5 / 1.5)), (2, f32(1 / 1.5))]
    shapes = bd.layer_shapes(97, 131)
    for i in range(1, 6):
        sh, sw = shapes[0] if i == 1 else shapes[i - 2]
        assert (sh == 2 * shapes[i][0] and sw == 2 * shapes[i][1]) == (i == 3)
    flat = np.full((97, 131), 93, np.uint8)
    assert all((im == 93).all() for im in bd.pyramid(flat))


def test_area_sampler_rounds_ties_to_even():
    src = np.array([[1, 2, 0], [0, 0, 0], [0, 0, 0]], np.uint8)               # 3 x 3 -> 2 x 2 (two-thirds): cell 0 = (1 + 2 / 2) ... / 2.25
    assert bd.resize_area(np.full((3, 3), 7, np.uint8), 2, 2).tolist() == [[7, 7], [7, 7]]
    assert bd.resize_area(src, 2, 2)[0, 0] == int(np.rint(f32(f32(2 / 3) * f32(f32(1 * f32(2 / 3)) + f32(2 * f32(1 / 3))))))
    two = np.array([[1, 2, 3], [0, 0, 0]], np.uint8)                            # 2 x 3 -> 1 x 1: mean 1.0; [[1, 2, 3], [3, 3, 3]]: 2.5 -> 2
    assert bd.resize_area(two, 1, 1)[0, 0] == 1
    half = np.array([[2, 3, 2, 3], [3, 2, 3, 2], [2, 3, 2, 3]], np.uint8)       # 3 x 4 -> 1 x 2 (rows inexact): mean 2.5 -> ties to even = 2
    assert bd.resize_area(half, 1, 2).tolist() == [[2, 2]]
    assert bd.resize_area(half[:2], 1, 2).tolist() == [[3, 3]]                  # the exact half of the same values: (10 + 2) >> 2 = 3


def test_score_read_is_a_pure_function_of_a_dense_map():
    """getAgastScore(x, y, thr) = s >= thr ? s : 0 with a threshold-independent s that is 0 outside the 3-pixel interior: OpenCV's
    cold-cache read (bounds, bisection from thr - 1, zero below thr), restated literally, equals the read of the dense map at every
    threshold tried, and s = the FAST response at threshold 0 less one"""
    img = bc.case("inexact")[0][:40, :48]
    L = bd.Layer(np.ascontiguousarray(img), f32(1), f32(0))
    h, w = img.shape
    assert not L.s[:3].any() and not L.s[-3:].any() and not L.s[:, :3].any() and not L.s[:, -3:].any()
    rng = np.random.RandomState(0)
    pts = [(int(rng.randint(-2, w + 2)), int(rng.randint(-2, h + 2))) for _ in range(400)] + [(x, y) for y in range(3, 12) for x in range(3, 20)]
    seen = 0
    for x, y in pts:
        for thr in (1, 2, 3, 7, 12, 30, 200):
            lazy = bd.lazy_score_9_16(img, x, y, thr)
            assert lazy == L.read(x, y, thr), (x, y, thr)
            seen += lazy > 0
    assert seen > 100
    fast = cr.fast_score(np.ascontiguousarray(img), 0)
    assert np.array_equal(L.s, np.maximum(fast.astype(np.int32) - 1, 0).astype(np.uint8))
    s5 = bd.score_5_8(np.ascontiguousarray(img))
    assert not s5[:2].any() and not s5[:, :2].any() and not s5[-2:].any() and not s5[:, -2:].any() and s5.any()


def test_sub_pixel_read_and_smoothing():
    L = bd.Layer(bc.case("exact")[0], f32(1), f32(0))
    ys, xs = np.nonzero(L.s)
    x, y = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])
    assert L.read_f(f32(x), f32(y)) == L.read(x, y)                              # integer position: the score itself
    v = L.read_f(f32(x + 0.5), f32(y))
    assert v == int(f32(f32(0.5) * f32(L.read(x, y))) + f32(f32(0.5) * f32(L.read(x + 1, y))))
    assert L.read_f(f32(-0.5), f32(2.0)) == 0 and L.read(-1, 0) == 0 and L.read(0, L.h) == 0
    const = np.full((20, 20), 77, np.uint8)                                      # the area branch preserves a constant map, inside and at scale 2, 3.5
    for scale in (2.0, 3.5):
        assert bd.smoothed_value(const, 9.3, 10.7, scale) == 77
    assert bd.smoothed_value(const, 9.25, 10.5, 0.8) == 77                       # the bilinear branch (half-width below 0.5)


def test_blobs_case_reaches_every_layer_and_ties_case_takes_the_tie_branch():
    _, kp, _ = bc.reference("blobs")
    per_layer = np.bincount(kp["octave"], minlength=6)
    print("blobs: keypoints per layer", per_layer.tolist())
    assert (per_layer > 0).all()                                                 # layer 0 (virtual layer below) .. layer 5 (the top layer's path)
    _, kp, stats = bc.reference("ties")
    print("ties:", stats)
    assert stats["ties"] > 0 and stats["tie_rejects"] > 0 and stats["ties"] > stats["tie_rejects"] and len(kp) > 0


@pytest.mark.parametrize("name", bc.CASES + ["full_size"])
def test_keypoints_lie_in_the_image_with_the_layers_size_range(sample_images, name):
    """every keypoint lies inside the image; the top layer's size is 12 * scale(5) exactly, every other layer's is 12 * the REFINED scale
    (refine1D*'s result times the layer's scale, as OpenCV reports it), which lies between the scales of the layers below and above"""
    img, thr = bc.image_case(name, sample_images)
    _, kp, _ = bc.image_reference(name, sample_images)
    h, w = img.shape
    assert len(kp) > 0
    assert (kp["x"] >= 0).all() and (kp["x"] <= w - 1).all() and (kp["y"] >= 0).all() and (kp["y"] <= h - 1).all()
    assert (kp["angle"] == -1).all() and np.isfinite(kp["response"]).all()
    scales = np.array([float(s) for s in bd.layer_scales()])
    # size = 12 * the refined scale, which refine1D* keeps between the scales of the virtual / real layers below and above; the top layer's is its own
    lo = 12 * scales * np.array([0.7, 2 / 3, 0.75, 2 / 3, 0.75, 1.0])
    hi = 12 * scales * np.array([1.5, 4 / 3, 1.5, 4 / 3, 1.5, 1.0])
    o = kp["octave"]
    assert (kp["size"] >= lo[o] * (1 - 1e-6)).all() and (kp["size"] <= hi[o] * (1 + 1e-6)).all()
    top = o == 5
    assert (kp["size"][top] == 72.0).all()
    assert (kp["response"][~top] > thr).all()
    order = o.astype(np.int64)                                                   # layer by layer
    assert (np.diff(order) >= 0).all()


def test_a_blob_of_twice_the_radius_gives_about_twice_the_size():
    """a Gaussian blob at radius r and at 2 r: the strongest keypoint's size ratio lies between 1.5 and 2.7 (one layer step either side of 2)"""
    for r in (2, 3, 4, 5):
        sizes = []
        for rr in (r, 2 * r):
            kp = bd.detect(bc.blob_image((120, 120), [("blob", 60, 60, rr, 150.0)]), 8)
            assert len(kp) > 0
            sizes.append(float(kp["size"][np.argmax(kp["response"])]))
        print("radius", r, "->", sizes, "ratio %.3f" % (sizes[1] / sizes[0]))
        assert 1.5 < sizes[1] / sizes[0] < 2.7
