"""The inputs of tests/match_cases.py, checked without a GPU: the case that is built to defeat the fp8 shortlist's first pass does defeat
it (in the float64 model of csrc/match.hip.h's fp8 path) while the oracle keeps its planted neighbours, the bound E8 of the second pass
holds on every pair of every case the GPU runs under fp8, and the library's side that needs no device is in place."""
import ctypes as C

import numpy as np
import pytest

from spvo import capi
from tests import match_cases as mc


def test_last_form_query_is_exported():
    lib = capi.load()
    assert "spvo_match_last_form" in capi.SYMBOLS and hasattr(lib, "spvo_match_last_form") and callable(capi.Context.match_last_form)
    info = (C.c_int * 4)()
    assert lib.spvo_match_last_form(None, info) == -1


def test_fp8_copy_rounds_and_saturates():
    """the model's copy: e4m3 of 16 x, nearest even, +-448 beyond the format's range (what desc_to_fp8_kernel's clamp produces)"""
    x = np.array([1.06 / 16, 1.065 / 16, -1.065 / 16, 1.0625 / 16, 1.1875 / 16, 28.0, 30.0, -1e4, 0.0, 2.0 ** -9 / 16], np.float32)
    want = np.array([1 / 16, 1.125 / 16, -1.125 / 16, 1 / 16, 1.25 / 16, 28.0, 28.0, -28.0, 0.0, 2.0 ** -9 / 16])   # ties go to the even mantissa; 2^-9 is the smallest subnormal
    assert np.array_equal(mc.fp8_copy(x), want)


def test_cases_are_built_once_and_read_only():
    a, b = mc.case(("sizes", 33, 129))
    assert mc.case(("sizes", 33, 129))[0] is a and not a.flags.writeable and not b.flags.writeable
    assert a.dtype == np.float32 and a.shape == (33, 256) and b.shape == (129, 256)
    i0, d0 = mc.expected(("sizes", 33, 129), "KNN", False)
    assert mc.expected(("sizes", 33, 129), "KNN", False)[0] is i0 and not i0.flags.writeable
    # the transposed distances serve the other direction: bit-identical to evaluating the oracle on (b, a)
    assert np.array_equal(mc.sq_distances(("sizes", 33, 129), True), mc.matching.sq_distances(b, a))
    for sel, cross in mc.SELECTORS:
        ri, rd = mc.matching.bf_match(b, a, sel, cross, mc.RATIO)
        gi, gd = mc.expected(("sizes", 33, 129), sel, cross, True)
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd)


def test_rounding_bias_defeats_pass_one_and_not_the_oracle():
    """fp8_rounding_bias: a matcher that stops after the statistical window returns a distractor on (nearly) every planted row -- so the
    GPU test on this case cannot pass without the second pass -- while the brute-force oracle keeps every planted neighbour, also
    through the KNN ratio test."""
    key = ("fp8_rounding_bias",)
    a, b = mc.case(key)
    truth = mc.bias_truth()
    G = mc.BIAS_GROUPS
    assert len(a) == G and len(b) == 3 * G + 200
    d2 = mc.sq_distances(key)
    assert np.array_equal(np.argmin(d2, axis=1), truth)
    idx, _ = mc.expected(key, "KNN", False)
    assert np.array_equal(idx, truth)                                      # the ratio test keeps all 96
    assert np.array_equal(mc.expected(key, "NN", False)[0], truth)
    m = mc.fp8_model(a, b)
    missed = ~m["cand1"][np.arange(G), truth]
    print(f"pass 1 drops the true neighbour on {missed.sum()} of {G} rows; candidates per row {m['cand1'].sum(1).min()} .. {m['cand1'].sum(1).max()}; "
          f"largest |dt8 - d2| / E8 = {(np.abs(m['dt8'] - d2) / m['e8']).max():.4f}")
    assert missed.mean() >= 0.9
    # ... and what pass 1 does keep holds no better answer: its best candidate is a distractor, a wrong index
    masked = np.where(m["cand1"], d2, np.inf)
    assert (np.argmin(masked, axis=1) != truth)[missed].all()
    # the other direction (B -> a): the planted train rows find their query row
    back, _ = mc.expected(key, "NN", False, True)
    assert np.array_equal(back[truth], np.arange(G))


@pytest.mark.parametrize("key", mc.FP8_CASES, ids=lambda k: "-".join(str(p) for p in k))
def test_e8_bounds_the_fp8_distance_on_every_pair(key):
    """|dt8 - d2| <= E8 = 2 (1 + 2^-10) (|a - a8| |b| + |a8| |b - b8|) + 2^-13 (|a|^2 + |b|^2) with d2 the oracle's canonical float32
    distance: the derivation at MATCH_ERR_REL_FP8, validated on the inputs the device sees -- saturated copies included."""
    a, b = mc.case(key)
    if not len(a) or not len(b):
        return
    m = mc.fp8_model(a, b)
    d2 = mc.sq_distances(key).astype(np.float64)
    assert np.isfinite(m["dt8"]).all() and np.isfinite(m["e8"]).all()
    excess = np.abs(m["dt8"] - d2) - m["e8"]
    assert (excess <= 0).all(), (key, float(excess.max()))
    # the true nearest neighbour of every row is therefore within pass 2's reach: its lower bound cannot exceed ANY canonical distance
    # of the row that is not smaller than its own
    i0 = np.argmin(d2, axis=1)
    r = np.arange(len(a))
    assert (m["dt8"][r, i0] - m["e8"][r, i0] <= d2[r, i0]).all()


def test_out_of_range_cases_are_out_of_range():
    """16 |x| > 448 somewhere in every row of the cases test_fp8_out_of_range_rows runs: the conversion has to saturate there"""
    for key in mc.OUT_OF_RANGE:
        a, b = mc.case(key)
        for x in (a, b):
            frac = (np.abs(x).max(axis=1) * mc.FP8_SCALE > mc.FP8_MAX).mean()
            assert frac > (0.99 if key != ("unnormalised",) else 0.5), (key, frac)
