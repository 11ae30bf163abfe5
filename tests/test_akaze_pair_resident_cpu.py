"""AKAZE + AKAZE resident, what needs no GPU: the exports, and the flat restatement of rule 11 (tests/akaze_suppress_cases.py) that
tests/test_gpu_akaze_pair_resident.py holds spvo_akaze_suppress_debug to -- it equals akaze_ref.suppress on every image case, and the
hand-made lists reach every branch of the rule, which the image cases do not."""
import ctypes
import os

import pytest

from spvo import capi
from tests import akaze_cases as ac, akaze_ref as ak, akaze_suppress_cases as sc

NEW = ["spvo_akaze_detect_pair", "spvo_akaze_suppress_debug"]


def test_both_libraries_export_the_new_symbols():
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    hostlib = ctypes.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libspvo_host.so"))
    assert hasattr(hostlib, "spvo_host_classic_set_akaze_resident")
    assert capi.AKAZE_CAND_DTYPE == sc.CAND_DTYPE and capi.AKAZE_CAND_DTYPE.itemsize == 20
    assert ctypes.sizeof(capi.AkazeFeatures) == ctypes.sizeof(capi.BriskFeatures)


def test_a_null_context_is_invalid():
    lib = ctypes.CDLL(capi.LIB_PATH)
    n = ctypes.c_int(7)
    fl, fr = capi.AkazeFeatures(0, None, None, 0), capi.AkazeFeatures(0, None, None, 0)
    lib.spvo_akaze_detect_pair.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    assert lib.spvo_akaze_detect_pair(None, None, None, 96, 160, 160, 0.001, 0, 1, 8192, ctypes.byref(fl), ctypes.byref(fr)) == -1
    lib.spvo_akaze_suppress_debug.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.spvo_akaze_suppress_debug(None, 96, 160, None, 0, None, ctypes.byref(n)) == -1


@pytest.mark.parametrize("name", ac.CASES)
def test_flat_restatement_equals_the_per_level_one(name):
    levels, _, _ = ac.reference(name)
    per_level = ak.candidates(levels)
    cand = sc.from_levels(per_level)
    tables = dict(octave=[L["octave"] for L in levels], esigma=[L["esigma"] for L in levels])
    keep, st = sc.flat_suppress(tables, cand)
    first = [0]
    for c in per_level:
        first.append(first[-1] + len(c["row"]))
    want = [first[lev] + i for lev, i in ak.suppress(levels, per_level) if per_level[lev]["ok"][i]]
    print(name, len(cand), "candidates", len(keep), "kept", st)
    assert keep.tolist() == want
    assert st["same_level"] == st["second_loop"] == st["not_ok"] == 0 and st["max_raised"] <= 1      # what the images do not reach
    if name == "blobs":
        assert (len(cand), st["drops"], st["from_below"]) == (50, 21, 7)


def test_the_lists_reach_every_branch():
    total = dict()
    for name in sc.LISTS:
        rows, cols, t, cand, keep, st = sc.case(name)
        assert len(cand) == 0 or (cand["level"].max() < len(t["octave"]) and (cand["level"][1:] >= cand["level"][:-1]).all())
        for k, v in st.items():
            total[k] = max(total.get(k, 0), v) if k == "max_raised" else total.get(k, 0) + v
    print(total)
    for k in ("drops", "drops_equal", "same_level", "from_below", "below_start", "several_hits", "second_loop", "not_ok"):
        assert total[k] >= 1, k
    assert total["max_raised"] >= 3
    assert [len(sc.case(n)[3]) for n in ("n0", "n1", "n63", "n64", "n65")] == [0, 1, 63, 64, 65]
    assert sc.case("chain")[5]["max_raised"] == 7 and sc.case("chain")[4].tolist() == [7]          # one slot, replaced seven times
    assert sc.case("second_loop_removes")[4].tolist() == [1] and sc.case("second_loop_keeps")[4].tolist() == [0, 1]
    assert len(sc.case("3000_small")[4]) > 1024                                                     # the compaction crosses a chunk
    assert len(sc.case("9000_four_octaves")[4]) > 3072                                              # more entries than the first loop keeps in LDS
