"""MatcherType::FLANN without a GPU: the libraries export the byte-L2 entry points and refuse a NULL context, initMatcher accepts FLANN
for binary, SIFT and SuperPoint descriptors (and BF as before), and the integer arithmetic the kernel uses is the oracle's."""
import ctypes as C

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import matching
from spvo import capi, host
from tests import match_u8_cases as mc

NEW = ["spvo_match_l2_u8", "spvo_match_l2_u8_slots", "spvo_set_binary_prematch_norm"]


def test_libraries_export_the_new_entry_points():
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.SYMBOLS, name
    assert callable(capi.Context.match_l2_u8) and callable(capi.Context.match_l2_u8_slots) and callable(capi.Context.set_binary_prematch_norm)
    hl = host.load()
    for name in ("spvo_host_matcher_probe", "spvo_host_classic_match_matcher", "spvo_host_classic_sequence_matcher", "spvo_host_create_matcher"):
        assert hasattr(hl, name), name


def test_null_context_is_invalid():
    lib = capi.load()
    rows = (C.c_uint8 * 64)()
    idx, dist = (C.c_int32 * 1)(), (C.c_float * 1)()
    assert lib.spvo_match_l2_u8(None, rows, 1, rows, 1, 64, 1, 0, 0.8, idx, dist) == -1
    assert lib.spvo_match_l2_u8_slots(None, 0, 1, 1, 0, 0.8, None, None) == -1
    assert lib.spvo_set_binary_prematch_norm(None, 1) == -1


@pytest.mark.parametrize("args", [("ORB", "ORB", "FLANN", "KNN"), ("SIFT", "SIFT", "FLANN", "NN"), ("SuperPoint", "SuperPoint", "FLANN", "KNN"),
                                  ("ORB", "ORB", "FLANN", "NN"), ("ORB", "ORB", "BF", "KNN"), ("SIFT", "SIFT", "BF", "NN"), ("SuperPoint", "SuperPoint", "BF", "NN")])
def test_init_matcher_accepts_the_matcher(args):
    for cross in (False, True):                                        # FLANN does not look at cross_check
        rc, err = host.matcher_probe(*args, cross_check=cross)
        assert rc == 0 and err == "", (args, cross, err)


def test_matcher_probe_refuses_unknown_names():
    for bad in (("NOPE", "ORB", "BF", "NN"), ("ORB", "NOPE", "BF", "NN"), ("ORB", "ORB", "KDTREE", "NN"), ("ORB", "ORB", "BF", "BEST")):
        with pytest.raises(ValueError):
            host.matcher_probe(*bad)


@pytest.mark.parametrize("width", mc.WIDTHS)
def test_integer_distances_are_the_oracles(width):
    """d2 in integers = sq_distances of the float casts, value for value, and the signed-offset form the int8 matrix cores compute equals
    both: on random rows (65 x 257) and on the extremes"""
    a, b = mc.random_rows(width, 65, 257)
    a[0], b[0] = 0, 255                                                # the largest distance of the width
    a[1], b[1] = 0x7F, 0x80                                            # across the sign boundary
    ref = matching.sq_distances(a.astype(np.float32), b.astype(np.float32))
    d = mc.d2_int(a, b)
    assert d.max() == width * 255 * 255 < 2 ** 24
    assert np.array_equal(d.astype(np.float32), ref) and np.array_equal(ref.astype(np.int64), d)
    s = mc.d2_signed(a, b)
    assert s.dtype == np.int32 and np.array_equal(s.astype(np.int64), d)


def test_special_cases_say_what_they_claim():
    for w in (32, 61, 64):
        a, b = mc.not_hamming(w)
        idx, dist = mc.oracle_match(a, b, "NN", False)
        hidx, _ = matching.bf_match_hamming(a, b, "NN", False)
        assert idx.tolist() == [1, 1, 1] and hidx.tolist() == [0, 0, 0] and np.all(dist == np.float32(np.sqrt(np.float32(8))))
        assert mc.d2_int(a, b)[0].tolist() == [16384, 8]
    a, b = mc.full_range()
    assert mc.d2_int(a, b)[0].tolist() == [4161600, 4161600, 64 * 49]
    idx, dist = mc.oracle_match(a, b, "NN", False)
    assert idx.tolist() == [2, 2] and dist[1] == 0
    assert mc.oracle_match(a[:1], b[:2], "NN", False)[1][0] == np.float32(2040.0)
    got = [int(mc.oracle_match(*mc.ratio_boundary(k0, k1), "KNN", False)[0][0]) for k0, k1 in mc.RATIO_BOUNDARY]
    assert got == [-1, 0, -1, 0]                                       # dropped, kept, dropped, kept
    a, b = mc.sign_and_ties()
    idx, dist = mc.oracle_match(a, b, "NN", False)
    assert idx.tolist() == [11, 11, 11, 5, 5] and dist.tolist() == [0, 0, 0, 0, 8.0]
    cidx, _ = mc.oracle_match(a, b, "NN", True)
    assert cidx[0] == 11 and cidx[3] == 5                              # the first of the train rows that voted for the query
