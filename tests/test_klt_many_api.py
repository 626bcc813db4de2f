"""pmv_klt_step_many without a GPU: the two symbols are declared, exported and bound; the argument lists; the header's contract; and the
refusals that need no device (the null context, trackers of another context)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_klt_step_many", "pmv_debug_klt_many_stats"]
INVALID = -2


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def _code():
    return " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())


def test_the_two_symbols_are_declared_exported_and_bound(pmv):
    code = _code()
    lib = pmv.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(\s*pmv_ctx\*" % name, code), f"{name} is not declared in include/pmv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    for method in ("klt_step_many", "debug_klt_many_stats"):
        assert callable(getattr(pmv.Context, method))


def test_the_declared_argument_lists():
    code = _code()
    assert ("int pmv_klt_step_many(pmv_ctx* ctx, int n_trk, const int* ids, const int* prev_slots, const int* cur_slots, int* out_ids, int* out_ages, float* out_xy, "
            "float* out_prev_xy_or_null, int out_stride, int* out_n , int* out_counts8 );") in code
    assert "int pmv_debug_klt_many_stats(pmv_ctx* ctx, long long* out4);" in code


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    doc = text[text.index("A group of trackers in one call"):text.index("int pmv_klt_step_many(")]
    for phrase in ("Result definition", "j * out_stride", "byte for byte", "the order within the group changes nothing", "two trackers may name the same slots",
                   "an empty tracker may sit next to full ones", "the five fields of gftt", "subpix_params", "frames of one size",
                   "names the first tracker that differs from tracker 0 and the field", "no tracker of the group changes its state", "an id named twice",
                   "n_trk > PMV_KLT_MAX_TRACKERS", "out_stride below the largest target", "only after the last wait", "an incomplete block is PMV_ERR_HIP",
                   "at most 12 launches", "at most two waits", "in one copy", "in any mixture", "one-entry geometry table of its own",
                   "pmv_debug_refill_stats does not move"):
        assert phrase in doc, phrase
    scope = doc[doc.index("Out of scope:"):]
    for phrase in ("the session form", "mixed frame sizes", "more than PMV_KLT_MAX_TRACKERS trackers", "everything pmv_klt_step lists"):
        assert phrase in scope, phrase


def test_a_null_context_is_refused(pmv):
    lib = pmv.load_library()
    out = np.full(16, -7, np.int32)
    fl = np.full(16, -7, np.float32)
    big = np.full(4, -7, np.int64)
    vp, ci = C.c_void_p, C.c_int
    lib.pmv_klt_step_many.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp]
    lib.pmv_debug_klt_many_stats.argtypes = [vp, vp]
    o, f = out.ctypes.data, fl.ctypes.data
    assert lib.pmv_klt_step_many(None, 1, o, o, o, o, o, f, f, 2, o, o) == INVALID
    lib.pmv_last_error.restype = C.c_char_p
    assert b"pmv_klt_step_many" in lib.pmv_last_error(None)
    assert lib.pmv_debug_klt_many_stats(None, big.ctypes.data) == INVALID
    assert b"pmv_debug_klt_many_stats" in lib.pmv_last_error(None)
    assert (out == -7).all() and (fl == -7).all() and (big == -7).all()


def test_trackers_of_another_context_are_refused_before_the_library(pmv):
    class Dummy:
        lib, h = None, None
    mine, other = pmv.Context.__new__(pmv.Context), Dummy()
    mine.lib, mine.h = None, None
    trk = pmv.KltTracker(other, 0, 10)
    with pytest.raises(ValueError, match="of this context"):
        pmv.Context.klt_step_many(mine, [trk], [0], [1])
    own = pmv.KltTracker(mine, 0, 10)
    with pytest.raises(ValueError, match="of this context"):
        pmv.Context.klt_step_many(mine, [own, trk], [0, 0], [1, 1])
    with pytest.raises(ValueError, match="one prev_slot and one cur_slot per tracker"):
        pmv.Context.klt_step_many(mine, [own], [0, 0], [1])
