"""The numpy restatement of the ORB extractor across octaves (tests/orb_octaves_ref.py) without a GPU: held to the compiled oracle
(oracle/cpu/orb_cpu.inc) where that independent implementation exists -- its own detector's keypoints, every octave --, what the parity
inputs of tests/test_gpu_orb_octaves.py are meant to cover (the reflect zone of the levels from 3 on, the rounding of the border rule),
and the C ABI and the host switch as far as they can be asked without a device."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import cpu_backend
from spvo import capi, host
from tests import orb_octaves_cases as oc, orb_octaves_ref as oo


@pytest.fixture(scope="module")
def cpu():
    c = cpu_backend.CpuBackend(net_height=64, net_width=96)
    yield c
    c.close()


def test_tables_are_the_oracle_s_and_the_library_s(cpu):
    pat, taps = oo.tables()
    cp, ct = cpu.orb_tables()
    assert np.array_equal(pat, cp) and np.array_equal(taps.view(np.uint32), ct.view(np.uint32))
    lp, lt = np.zeros(1024, np.float32), np.zeros(7, np.float32)
    assert capi.load().spvo_orb_tables(lp.ctypes.data_as(C.c_void_p), lt.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(pat, lp) and np.array_equal(taps.view(np.uint32), lt.view(np.uint32))
    assert np.abs(pat).max() == 13 and len(oo.disc_offsets()) == 709


@pytest.mark.parametrize("which", [0, 1])
def test_restatement_equals_the_compiled_oracle_on_its_own_keypoints(cpu, sample_images, which):
    """every keypoint of the oracle's detector, all octaves, handed over in shuffled order: all kept, `kept` the stable grouping by
    octave, the 32 bytes equal, the direction within 1e-5 rad (tests/test_gpu_classic_detectors.py's bound for the same quantity)"""
    img = sample_images[which]
    r = cpu.orb(img)
    n = len(r["xy"])
    perm = np.random.default_rng(which).permutation(n)
    g = oo.describe(img, r["xy"][perm], r["octave"][perm])
    assert n > 1000 and set(r["octave"].tolist()) == set(range(8))
    assert len(g["kept"]) == n
    assert np.array_equal(g["kept"], np.argsort(r["octave"][perm], kind="stable"))
    src = perm[g["kept"]]
    assert np.array_equal(g["octave"], r["octave"][src])
    bad = int((g["desc"] != r["desc"][src]).any(1).sum())
    err = float(np.abs(g["angle"] - r["angle"][src]).max())
    print(img.shape, "keypoints", n, "rows that differ", bad, "largest direction difference", err, "in the reflect zone", int(g["zone"].any(1).sum()))
    assert bad == 0
    assert err <= 1e-5
    assert not g["outside"].any()                        # the oracle's detector keeps 31 pixels from every level's border


def test_brisk_keypoints_reach_into_the_reflect_zone(sample_images):
    """the BRISK restatement's 1214 keypoints on the crop: 716 survive the 31-pixel rule, octaves 0..5 all present, and on each of octaves
    3, 4 and 5 some kept keypoint lies within the patch's reach (19 pixels) of its level's border -- 28 in all, of which 16 really read
    beyond it (on octaves 4 and 5; on octave 3 a kept keypoint lies at least 18 pixels inside, which the disc and these test pairs do not
    exceed)"""
    img, xy, octave = oc.keypoints("brisk", sample_images)
    g = oc.reference("brisk", sample_images)
    zone, outside = g["zone"].any(1), g["outside"].any(1)
    print("keypoints", len(xy), "kept", len(g["kept"]), "per octave", np.bincount(g["octave"], minlength=8).tolist(), "zone", int(zone.sum()), "reads outside", int(outside.sum()))
    assert img.shape == (160, 400) and len(xy) == 1214
    assert len(g["kept"]) == 716
    assert set(g["octave"].tolist()) == set(range(6))
    for o in (3, 4, 5):
        assert zone[g["octave"] == o].any(), o
    assert int(zone.sum()) == 28
    assert not zone[g["octave"] < 3].any() and not (outside & ~zone).any()
    for o in (4, 5):
        assert outside[g["octave"] == o].any(), o
    assert np.array_equal(g["kept"], oo.border_keep(xy, img.shape)[np.argsort(octave[oo.border_keep(xy, img.shape)], kind="stable")])


def test_handmade_keypoints_cross_every_border_and_pin_the_rounding(sample_images):
    """the handmade set: on each of octaves 3..7 every one of the four borders of the level is within reach of some kept keypoint, and from
    octave 5 on (31 / 1.2^5 = 12 < 15) reads really fall beyond every one; the half-integer coordinates are kept or dropped as round
    half to even says"""
    img, xy, octave = oc.keypoints("handmade", sample_images)
    rows, cols = img.shape
    g = oc.reference("handmade", sample_images)
    assert min(min(s) for s in oo.level_shapes(rows, cols)) >= oo.MIN_LEVEL
    for o in range(3, 8):
        s = g["octave"] == o
        assert g["zone"][s].any(0).all(), (o, g["zone"][s].any(0))
    for o in range(5, 8):
        assert g["outside"][g["octave"] == o].any(0).all(), o
    assert not g["zone"][g["octave"] < 3].any()
    kept = set(g["kept"].tolist())

    def index(x, y, o):
        return int(np.nonzero((xy[:, 0] == np.float32(x)) & (xy[:, 1] == np.float32(y)) & (octave == o))[0][0])
    for o in (0, 3, 7):
        for x, y, keep in ((30.5, 60, False), (31.5, 60, True), (32.5, 60, True), (cols - 31.5, 60, True), (cols - 30.5, 60, False), (60, 30.5, False), (60, 31.5, True),
                           (60, rows - 31.5, True), (60, rows - 30.5, False), (100.5, 70.5, True)):
            assert (index(x, y, o) in kept) == keep, (x, y, o)
    for o in range(8):                                 # the corners of the border rule's rectangle are kept at every octave
        for x, y in ((31, 31), (cols - 32, 31), (31, rows - 32), (cols - 32, rows - 32)):
            assert index(x, y, o) in kept
    assert np.array_equal(g["octave"], np.sort(g["octave"])) and len(kept) == len(g["kept"])
    i0 = index(31.5, 60, 0)                            # on the level: rint(31.5) = 32 at octave 0; rint(100.5 / 1) = 100
    assert tuple(g["cxy"][g["kept"].tolist().index(i0)]) == (32, 60)
    assert tuple(g["cxy"][g["kept"].tolist().index(index(100.5, 70.5, 0))]) == (100, 70)


def test_restatement_refuses_what_the_call_refuses(sample_images):
    img = oc.crop(sample_images)
    one = np.array([[100, 80]], np.float32)
    for bad_octave in (8, -1):
        with pytest.raises(ValueError):
            oo.describe(img, one, [bad_octave])
    with pytest.raises(ValueError):
        oo.describe(img, np.array([[np.nan, 80]], np.float32), [0])
    assert oo.level_shapes(64, 96)[4] == (31, 46)
    with pytest.raises(ValueError):
        oo.describe(np.zeros((64, 96), np.uint8), np.array([[40, 32]], np.float32), [4])
    assert len(oo.describe(img, np.zeros((0, 2), np.float32), np.zeros(0, np.int32))["kept"]) == 0


def test_the_call_is_declared_and_refuses_a_null_context():
    lib = capi.load()
    assert "spvo_orb_describe_octaves" in capi.SYMBOLS and hasattr(lib, "spvo_orb_describe_octaves") and callable(capi.Context.orb_describe_octaves)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spvo.h")) as f:
        assert "int spvo_orb_describe_octaves(spvo_ctx *ctx, const uint8_t *img" in f.read()
    img = (C.c_uint8 * (64 * 96))()
    xy = (C.c_float * 2)(40, 32)
    octave = (C.c_int32 * 1)(0)
    kept = (C.c_int32 * 1)()
    desc = (C.c_uint8 * 32)()
    m = C.c_int(0)
    assert lib.spvo_orb_describe_octaves(None, img, 64, 96, 96, xy, octave, 1, kept, None, desc, C.byref(m)) == -1
    assert lib.spvo_orb_describe_octaves(None, None, 64, 96, 0, None, None, 0, None, None, None, C.byref(m)) == -1


def test_the_two_pairs_are_opt_in():
    """without the keyword BRISK + ORB and AKAZE + ORB are refused with one text, which does not name them; with it the pair is not refused
    -- without a device nothing is pushed and the error names the missing device, not the pair"""
    import torch
    img = np.zeros((64, 96), np.uint8)
    P = np.eye(3, 4)
    n, counts, err = host.classic_pair_probe("BRISK", "ORB", img, img, P, P)
    n2, counts2, err2 = host.classic_pair_probe("AKAZE", "ORB", img, img, P, P)
    assert n == 0 and n2 == 0 and not counts.any() and not counts2.any()
    assert err == err2 and "ShiTomasi + SIFT" in err and "BRISK + ORB" not in err and "AKAZE + ORB" not in err
    for d in ("BRISK", "AKAZE"):
        n, counts, err_on = host.classic_pair_probe(d, "ORB", img, img, P, P, orb_octaves=True)
        assert "only these pairs run" not in err_on, err_on
        if not torch.cuda.is_available():
            assert n == 0 and not counts.any() and "spvo_create" in err_on, err_on
    n, counts, err_on = host.classic_pair_probe("SIFT", "ORB", img, img, P, P, orb_octaves=True)      # a pair that still does not run lists the two
    assert n == 0 and "BRISK + ORB" in err_on and "AKAZE + ORB" in err_on and err_on.startswith(err[:err.index("ShiTomasi + SIFT")])
    assert host.classic_pair_probe("BRISK", "ORB", img, img, P, P)[2] == err                            # ... and the switch was reset
