"""ShiTomasi / FAST + SIFT resident (spvo_classic_sift_pair), what needs no GPU: the exports, the refusal of a NULL context and the
reference's detector parameters for the two new kinds."""
import ctypes
import os

from spvo import capi


def test_both_libraries_export_the_new_symbols():
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert "spvo_classic_sift_pair" in capi.SYMBOLS and hasattr(lib, "spvo_classic_sift_pair")
    hostlib = ctypes.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libspvo_host.so"))
    assert hasattr(hostlib, "spvo_host_classic_set_sift_describe_resident")
    assert capi.CLASSIC_SIFT_KINDS == {"ShiTomasi": 5, "GFTT": 5, "FAST": 6}


def test_a_null_context_is_invalid():
    lib = ctypes.CDLL(capi.LIB_PATH)
    o = capi.ClassicOpts()
    lib.spvo_default_classic_opts.argtypes = [ctypes.POINTER(capi.ClassicOpts), ctypes.c_int]
    lib.spvo_default_classic_opts.restype = None
    lib.spvo_default_classic_opts(ctypes.byref(o), 6)
    fl, fr = capi.SiftFeatures(0, None, None, 0), capi.SiftFeatures(0, None, None, 0)
    img = (ctypes.c_uint8 * (16 * 16))()
    lib.spvo_classic_sift_pair.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 2
    assert lib.spvo_classic_sift_pair(None, ctypes.byref(o), img, img, 16, 16, 16, 0, 1, ctypes.byref(fl), ctypes.byref(fr)) == -1


def test_default_options_of_the_two_kinds_are_the_references():
    """cv::GFTTDetector::create(1000, 0.03, 7.5, 5, ..) and cv::FastFeatureDetector::create(10, true), slots of 8192 rows"""
    lib = ctypes.CDLL(capi.LIB_PATH)
    lib.spvo_default_classic_opts.argtypes = [ctypes.POINTER(capi.ClassicOpts), ctypes.c_int]
    lib.spvo_default_classic_opts.restype = None
    for kind in (5, 6):
        o = capi.ClassicOpts()
        lib.spvo_default_classic_opts(ctypes.byref(o), kind)
        assert o.kind == kind
        assert (o.max_corners, o.quality_level, o.min_distance, o.block_size) == (1000, 0.03, 7.5, 5)
        assert (o.fast_threshold, o.fast_nonmax) == (10, 1)
        assert o.slot_capacity == 8192
