"""The device-resident BRISK path without a GPU: the libraries export the new entry points, the two new kinds get the reference's detector
parameters, and every new call refuses a NULL context."""
import ctypes as C

from spvo import capi, host


def test_libraries_export_the_new_entry_points():
    lib = capi.load()
    assert hasattr(lib, "spvo_classic_slot_fill_debug")
    assert "spvo_classic_slot_fill_debug" in capi.SYMBOLS
    assert callable(capi.Context.classic_slot_fill)
    assert hasattr(host.load(), "spvo_host_classic_resident_pairs")
    assert host.classic_resident_pairs() == 0                         # no sequence has run in this process


def test_default_opts_of_the_brisk_kinds():
    lib = capi.load()
    assert capi.CLASSIC_KINDS["ShiTomasi+BRISK"] == 3 and capi.CLASSIC_KINDS["FAST+BRISK"] == 4
    for kind in (3, 4):
        o = capi.ClassicOpts()
        lib.spvo_default_classic_opts(C.byref(o), kind)
        assert o.kind == kind
        assert (o.max_corners, o.quality_level, o.min_distance, o.block_size) == (1000, 0.03, 7.5, 5)      # cv::GFTTDetector::create(1000, 0.03, 7.5, 5, ..)
        assert (o.fast_threshold, o.fast_nonmax) == (10, 1)                                                 # cv::FastFeatureDetector::create(10, true)
        assert o.slot_capacity == 8192


def test_null_context_is_invalid():
    lib = capi.load()
    rows = (C.c_uint8 * 64)()
    assert lib.spvo_classic_slot_fill_debug(None, 0, rows, 1, 64) == -1
    img = (C.c_uint8 * (64 * 96))()
    for kind in (3, 4):
        o = capi.ClassicOpts()
        lib.spvo_default_classic_opts(C.byref(o), kind)
        fl, fr = capi.ClassicFeatures(0, None, None, 0), capi.ClassicFeatures(0, None, None, 0)
        assert lib.spvo_classic_detect(None, C.byref(o), img, img, 64, 96, 96, 0, 1, C.byref(fl), C.byref(fr)) == -1
    assert lib.spvo_match_hamming_slots(None, 0, 1, 1, 0, 0.8, None, None) == -1
