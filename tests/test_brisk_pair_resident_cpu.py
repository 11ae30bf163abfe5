"""The device-resident BRISK + BRISK path without a GPU: both libraries export the new entry points, the binding lists and wraps the new
call, it refuses a NULL context, and the host class's switch is off by default."""
import ctypes as C
import inspect

from spvo import capi, host


def test_libraries_export_the_new_entry_points():
    lib = capi.load()
    assert hasattr(lib, "spvo_brisk_detect_pair")
    assert "spvo_brisk_detect_pair" in capi.SYMBOLS
    assert callable(capi.Context.brisk_detect_pair)
    assert [f[0] for f in capi.BriskFeatures._fields_] == ["n", "kp", "desc", "cap"]
    hl = host.load()
    assert hasattr(hl, "spvo_host_classic_set_brisk_resident")
    assert hasattr(hl, "spvo_host_classic_resident_pairs")
    assert inspect.signature(host.classic_sequence).parameters["brisk_resident"].default is False
    assert host.classic_resident_pairs() == 0                         # no sequence has run in this process


def test_null_context_is_invalid():
    lib = capi.load()
    img = (C.c_uint8 * (64 * 96))()
    fl, fr = capi.BriskFeatures(0, None, None, 0), capi.BriskFeatures(0, None, None, 0)
    assert lib.spvo_brisk_detect_pair(None, img, img, 64, 96, 96, 30, 3, 0, 1, 8192, C.byref(fl), C.byref(fr)) == -1
