"""The device-resident classic front end without a GPU: the library exports the new entry points, spvo_default_classic_opts fills the
reference's parameters (feature_detection_classic.cpp:12-47) for each kind, and the calls refuse a NULL context."""
import ctypes as C

import pytest

from spvo import capi

NEW_SYMBOLS = ["spvo_default_classic_opts", "spvo_classic_detect", "spvo_classic_slot_rows", "spvo_match_hamming_slots"]


def test_library_exports_the_resident_entry_points():
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_default_opts_are_the_reference_s_parameters(kind):
    lib = capi.load()
    o = capi.ClassicOpts()
    C.memset(C.byref(o), 0xA5, C.sizeof(o))
    lib.spvo_default_classic_opts(C.byref(o), kind)
    assert o.kind == kind
    assert o.nfeatures == 2000                                                                   # cv::ORB::create(2000, ...)
    assert (o.max_corners, o.quality_level, o.min_distance, o.block_size) == (1000, 0.03, 7.5, 5)   # cv::GFTTDetector::create(1000, 0.03, 7.5, 5, ..)
    assert (o.fast_threshold, o.fast_nonmax) == (10, 1)                                          # cv::FastFeatureDetector::create(10, true)
    assert o.slot_capacity == 8192
    lib.spvo_default_classic_opts(None, kind)                                                    # tolerated


def test_null_context_is_invalid():
    lib = capi.load()
    o = capi.ClassicOpts()
    lib.spvo_default_classic_opts(C.byref(o), 0)
    img = (C.c_uint8 * (64 * 96))()
    fl, fr = capi.ClassicFeatures(0, None, None, 0), capi.ClassicFeatures(0, None, None, 0)
    assert lib.spvo_classic_detect(None, C.byref(o), img, img, 64, 96, 96, 0, 1, C.byref(fl), C.byref(fr)) == -1
    n = C.c_int(0)
    assert lib.spvo_classic_slot_rows(None, 0, C.byref(n)) == -1
    assert lib.spvo_match_hamming_slots(None, 0, 1, 1, 0, 0.8, None, None) == -1
