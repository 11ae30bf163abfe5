"""tests/akaze_ref.py without a GPU: the level and octave rule, what a blob gives, mirror symmetry, the library's tables against the
restatement's own (spvo_akaze_tables needs no device), the restatement's float32-versus-float64 figures on every parity case, and that
the BRISK extractor's own bar holds on the restatement's keypoints -- what tests/test_gpu_akaze.py relies on, checked here first."""
import numpy as np
import pytest

from spvo import capi
from tests import akaze_cases as ac, akaze_ref as ak, brisk_ref as br
from tests.brisk_detect_cases import blob_image

NEW_SYMBOLS = ["spvo_akaze_detect", "spvo_akaze_debug_level", "spvo_akaze_last_contrast", "spvo_akaze_tables"]
SHAPES = {"one_octave": (97, 131), "two_exact": (96, 160), "two_odd": (83, 165), "blobs": (270, 400), "ties": (80, 112), "border": (140, 180), "flat": (48, 64)}


def test_library_exports_the_akaze_entry_points():
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    for name in ("akaze_detect", "akaze_level", "akaze_last_contrast"):
        assert callable(getattr(capi.Context, name))
    assert capi.AKAZE_KP_DTYPE.itemsize == ak.KP_DTYPE.itemsize == 28 and capi.AKAZE_KP_DTYPE.names == ak.KP_DTYPE.names


@pytest.mark.parametrize("shape, octaves", [((97, 131), [(97, 131)]), ((96, 160), [(96, 160), (48, 80)]), ((83, 165), [(83, 165), (41, 82)]),
                                            ((270, 400), [(270, 400), (135, 200), (67, 100)]), ((80, 112), [(80, 112)]), ((140, 180), [(140, 180), (70, 90)]),
                                            ((48, 64), [(48, 64)]), ((375, 1242), [(375, 1242), (187, 621), (93, 310), (46, 155)]),
                                            ((39, 79), [(39, 79)]), ((40, 80), [(40, 80)]), ((80, 160), [(80, 160), (40, 80)]),
                                            ((320, 640), [(320, 640), (160, 320), (80, 160), (40, 80)])])
def test_levels_and_octaves(shape, octaves):
    """rule 1: the octaves of a shape (they stop before the first octave above 0 narrower than 80 or lower than 40, and after 4), four levels
    each with sigma_size 2, 3, 3, 4 and esigma = 1.6 * 2^(j / 4 + o); every transition has steps that sum to its diffusion time"""
    assert ak.octave_shapes(*shape) == octaves
    T = ak.make_tables(*shape)
    n = 4 * len(octaves)
    assert T["octave"].tolist() == [i // 4 for i in range(n)] and T["sigma_size"].tolist() == [2, 3, 3, 4] * len(octaves)
    assert np.allclose(T["esigma"], [1.6 * 2.0 ** (i / 4.0) for i in range(n)], rtol=1e-6)
    assert len(T["nsteps"]) == n - 1 and T["nsteps"].sum() == len(T["tau"]) and (T["nsteps"] >= 1).all()
    etime = 0.5 * T["esigma"].astype(np.float64) ** 2
    t0 = 0
    for i, m in enumerate(T["nsteps"]):
        assert abs(T["tau"][t0:t0 + m].astype(np.float64).sum() - (etime[i + 1] - etime[i])) <= 1e-4 * etime[i + 1]   # a FED cycle of time T
        t0 += m
    assert [ak.level_border(s) for s in (2, 3, 4)] == [29, 43, 58]
    assert len(T["g0"]) == 5 and len(T["g1"]) == 3 and abs(T["g0"][0] + 2 * T["g0"][1:].sum() - 1) < 1e-6 and abs(T["g1"][0] + 2 * T["g1"][1:].sum() - 1) < 1e-6


def test_case_shapes():
    for name, shape in SHAPES.items():
        assert ac.case(name).shape == shape


def test_a_blob_of_the_base_scale_is_found_at_its_centre_on_the_level_of_its_scale():
    """A Gaussian blob of sigma 1.6 -- soffset, the scale of level 0, chosen before anything was run because it is the one blob scale the
    scale space names exactly -- gives a keypoint within one pixel of its centre, on the level whose esigma is nearest to 1.6 (level 0).
    Larger blobs do not have that property (NOTES.md, "AKAZE detector"); what they give is pinned by the next test."""
    cx, cy, sigma = 75, 64, 1.6
    img = blob_image((128, 150), [("blob", cx, cy, 2 * sigma, 150.0)])
    kp = ak.detect(img)
    T = ak.make_tables(*img.shape)
    near = kp[(np.abs(kp["x"] - cx) <= 1) & (np.abs(kp["y"] - cy) <= 1)]
    print("sigma", sigma, "->", [(int(k["class_id"]), float(k["x"]), float(k["y"]), float(k["response"])) for k in near])
    assert len(near) >= 1
    nearest = int(np.argmin(np.abs(T["esigma"] - np.float32(sigma))))
    assert nearest == 0 and nearest in near["class_id"].tolist()
    assert all(k["size"] == np.float32(np.float32(T["esigma"][k["class_id"]] * np.float32(1.5)) * np.float32(2)) and k["angle"] == 0 for k in kp)


# the levels on which the restatement finds every structure of the `blobs` case (three octaves) within one pixel of its centre: recorded
# values, pinned so that a change of the normalisation (rule 9) or of the suppression (rule 11) shows.  In the order of akaze_cases.BLOBS.
BLOB_LEVELS = [[0, 2], [1], [1], [1], [1], [1], [1, 3], [1, 3, 5, 7], [1, 3, 5, 7], [1], [3], [], [0, 1, 3], []]


def test_the_levels_of_every_blob_of_the_blobs_case_are_as_recorded():
    """What the detector does guarantee about scale: rule 11 compares a candidate with the level below only, so a structure whose response
    falls from one level to the next is found again two levels up -- larger blobs come out on alternating levels, up to level 7 (octave 1)
    for sigma 8 and 10 -- and the coarsest level a blob reaches never decreases from sigma 2 to sigma 10.  The sigma 20 blob and the small
    square yield nothing inside the borders."""
    img = ac.case("blobs")
    kp = ac.reference("blobs")[2]
    found = []
    for kind, cx, cy, r, amp in ac.BLOBS:
        near = kp[(np.abs(kp["x"] - cx) <= 1) & (np.abs(kp["y"] - cy) <= 1)]
        found.append(sorted(near["class_id"].tolist()))
        print(kind, (cx, cy), "sigma", r / 2, "-> levels", found[-1], "responses", near["response"].tolist())
    assert found == BLOB_LEVELS
    top = [max(f) for f in found[:9]]                                                  # the blobs of sigma 2 .. 10
    assert top[1:] == sorted(top[1:]) and top[-1] == 7


def test_the_mirror_image_gives_mirrored_candidates_on_ties():
    """left-right mirroring is exact in every rule (sums of a left and a right neighbour commute), so the candidates of the mirrored image
    are the mirrored candidates with the same responses and the negated horizontal offset: equal Ldet across the symmetry axis never
    yields a candidate on one side only.  (The suppression of rule 11 depends on the raster order and is not mirrored.)"""
    img = ac.case("ties")
    assert np.array_equal(img, img[:, ::-1]) and np.array_equal(img, img[::-1])
    w = img.shape[1]
    a = ak.candidates(ak.scale_space(img)[0])
    b = ak.candidates(ak.scale_space(np.ascontiguousarray(img[:, ::-1]))[0])
    total = 0
    for ca, cb in zip(a, b):
        ka = sorted(zip(ca["row"].tolist(), ca["col"].tolist(), ca["response"].tolist(), ca["ox"].tolist(), ca["oy"].tolist()))
        kb = sorted(zip(cb["row"].tolist(), (w - 1 - cb["col"]).tolist(), cb["response"].tolist(), (-cb["ox"]).tolist(), cb["oy"].tolist()))
        assert ka == kb
        total += len(ka)
        cols = set(zip(ca["row"].tolist(), ca["col"].tolist()))
        assert all((r, w - 1 - c) in cols for r, c in cols)                      # the image is its own mirror: so is the candidate set
    assert total > 0
    ldet = ak.scale_space(img)[0][0]["Ldet"]
    assert np.array_equal(ldet, ldet[:, ::-1]) and (ldet[:, w // 2 - 1] == ldet[:, w // 2]).all()   # equal neighbours along the axis


def _ulps(a, b):
    a, b = (np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return int(np.abs(a - b).max()) if a.size else 0


@pytest.mark.parametrize("shape", sorted(set(SHAPES.values())) + [(375, 1242), (16, 16), (320, 640)])
def test_library_tables_equal_the_restatements(shape):
    """spvo_akaze_tables (no device): every integer equals the restatement's; esigma (one powf), the Gaussian taps (exp in double, rounded to
    float) within 1 ulp; the step sizes within 8 ulp -- two libraries' cosf may differ by 2 ulp, squaring doubles that, and the division and
    the rounding of d add one each.  Measured on these shapes: 0, 0 and at most 5."""
    L, R = capi.akaze_tables(*shape), ak.make_tables(*shape)
    for key in ("octave", "sigma_size", "nsteps"):
        assert L[key].dtype == np.int32 and np.array_equal(L[key], R[key]), key
    figures = {key: _ulps(L[key], R[key]) for key in ("esigma", "g0", "g1", "tau")}
    print(shape, "levels", len(L["octave"]), "steps", len(L["tau"]), "ulp", figures)
    assert len(L["tau"]) == len(R["tau"]) and len(L["g0"]) == 5 and len(L["g1"]) == 3
    assert figures["esigma"] <= 1 and figures["g0"] <= 1 and figures["g1"] <= 1 and figures["tau"] <= 8
    levels, _ = ak.scale_space(np.zeros(shape, np.uint8), tables=L) if shape == (16, 16) else (None, None)   # the library's tables are accepted
    assert levels is None or len(levels) == 4


def _unmatched(a, b):
    """records of a without one of b on the same level within half a pixel"""
    return sum(not ((b["class_id"] == r["class_id"]) & (np.abs(b["x"] - r["x"]) < 0.5) & (np.abs(b["y"] - r["y"]) < 0.5)).any() for r in a)


# keypoints at float32, at float64, float32 keypoints without a float64 partner, float64 keypoints without a float32 partner -- measured by
# the test below
YARDSTICKS = {"one_octave": (78, 78, 0, 0), "two_exact": (97, 97, 0, 0), "two_odd": (63, 63, 0, 0), "blobs": (22, 22, 0, 0), "ties": (20, 20, 0, 0),
              "border": (105, 105, 0, 0), "flat": (0, 0, 0, 0), "full_size": (1442, 1442, 0, 0)}


@pytest.mark.parametrize("name", ac.CASES + ["full_size"])
def test_float32_versus_float64_yardsticks(sample_images, name):
    """The restatement at float32 and at float64 (same float32 tables): how close to a decision boundary (threshold, strict maximum,
    suppression, the offsets' bound) the input sits.  An input on which the two disagree on more than 0.25 % of the keypoints is no parity
    case.  No NaN in any plane, the flat image included."""
    img = ac.image_case(name, sample_images)
    levels, k, kp = ac.reference(name, sample_images)
    levels64, k64 = ak.scale_space(img, ft=np.float64)
    kp64 = ak.detect(img, levels=levels64)
    fig = (len(kp), len(kp64), _unmatched(kp, kp64), _unmatched(kp64, kp))
    print(name, img.shape, "k", k.tolist(), "float64", k64.tolist(), "figures", fig, "per level", np.bincount(kp["class_id"], minlength=len(levels)).tolist())
    assert fig == YARDSTICKS[name]
    assert fig[2] + fig[3] <= 0.0025 * max(len(kp), 1)
    assert all(np.isfinite(L[p]).all() for L in levels for p in ("Lt", "Lsmooth", "Lflow", "Ldet")) and np.isfinite(k).all() and (k > 0).all()
    if name == "flat":
        assert k.tolist() == [np.float32(0.03)] and all((L["Ldet"] == 0).all() for L in levels)
    if name == "blobs":
        assert len(levels) == 12 and len(set(kp["class_id"].tolist())) >= 5 and kp["octave"].max() >= 1     # many levels, beyond octave 0
    if name == "full_size":
        assert len(levels) == 16
    if name == "border":                                                                      # candidates right up to the border rule of level 0
        c = ak.candidates(levels)[0]
        assert c["row"].min() == 29 or c["col"].min() == 29 or c["row"].max() == img.shape[0] - 30 or c["col"].max() == img.shape[1] - 30


@pytest.mark.parametrize("name", ["blobs", "one_octave", "full_size"])
def test_the_extractors_bar_holds_on_the_restatements_keypoints(sample_images, name):
    """tests/brisk_ref.py's describe on the restatement's keypoints: rows within one float step of a rotation boundary (which the GPU test
    excuses) are at most 1 % of the kept rows, plus one; at least 4 distinct scale indices occur on blobs"""
    img = ac.image_case(name, sample_images)
    kp = ac.reference(name, sample_images)[2]
    r = br.describe(img, np.stack([kp["x"], kp["y"]], 1), kp["size"])
    print(name, "keypoints", len(kp), "described", len(r["kept"]), "scale indices", sorted(set(r["scale"].tolist())), "boundary rows", int(r["boundary"].sum()))
    assert len(r["kept"]) > 0 and r["boundary"].sum() <= 0.01 * len(r["kept"]) + 1
    if name == "blobs":
        assert len(set(r["scale"].tolist())) >= 4
