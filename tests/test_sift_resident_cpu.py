"""The device-resident SIFT path without a GPU: the library exports the new entry points, they are listed in capi.SYMBOLS, and each
refuses a NULL context."""
import ctypes as C

from spvo import capi

NEW_SYMBOLS = ["spvo_sift_detect_pair", "spvo_sift_slot_rows", "spvo_match_l2_slots", "spvo_sift_order_debug"]


def test_library_exports_the_resident_sift_entry_points():
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    for name in ("sift_detect_pair", "sift_slot_rows", "match_l2_slots", "sift_order"):
        assert callable(getattr(capi.Context, name))


def test_null_context_is_invalid():
    lib = capi.load()
    img = (C.c_uint8 * (64 * 96))()
    fl, fr = capi.SiftFeatures(0, None, None, 0), capi.SiftFeatures(0, None, None, 0)
    assert lib.spvo_sift_detect_pair(None, img, img, 64, 96, 96, 0, 1, 1024, C.byref(fl), C.byref(fr)) == -1
    n = C.c_int(0)
    assert lib.spvo_sift_slot_rows(None, 0, C.byref(n)) == -1
    assert lib.spvo_match_l2_slots(None, 0, 1, 1, 0, 0.8, None, None) == -1
    rec = (C.c_uint8 * 24)()
    order = (C.c_int32 * 1)()
    assert lib.spvo_sift_order_debug(None, rec, 1, order, C.byref(n)) == -1
