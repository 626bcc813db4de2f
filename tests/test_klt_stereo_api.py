"""The stereo tracker step without a GPU: the five functions and the setting's struct are declared, exported and bound; the argument lists;
the header's contract; and the refusals that need no device (the null context, trackers of another context)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import klt_stereo_common as ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_klt_set_stereo", "pmv_klt_get_stereo", "pmv_klt_step_stereo", "pmv_klt_step_many_stereo", "pmv_debug_klt_stereo_stats"]
INVALID = -2


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def _code():
    return " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())


def test_the_symbols_are_declared_exported_and_bound(pmv):
    code = _code()
    lib = pmv.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(\s*pmv_ctx\*" % name, code), f"{name} is not declared in include/pmv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    assert not hasattr(lib, "pmv_klt_debug_klt_stereo_stats")
    assert "typedef struct pmv_klt_stereo_params { double fb_max_dist; int border; } pmv_klt_stereo_params;" in code
    assert [f[0] for f in pmv.KltStereoParams._fields_] == ["fb_max_dist", "border"]
    for method in ("set_stereo", "step_stereo"):
        assert callable(getattr(pmv.KltTracker, method))
    for method in ("klt_step_many_stereo", "debug_klt_stereo_stats"):
        assert callable(getattr(pmv.Context, method))


def test_the_declared_argument_lists():
    code = _code()
    assert "int pmv_klt_set_stereo(pmv_ctx* ctx, int id, const pmv_klt_stereo_params* p_or_null);" in code
    assert "int pmv_klt_get_stereo(pmv_ctx* ctx, int id, pmv_klt_stereo_params* out, int* out_on);" in code
    assert ("int pmv_klt_step_stereo(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int right_slot, int* out_ids, int* out_ages, float* out_xy, "
            "float* out_prev_xy_or_null, float* out_right_xy, uint8_t* out_right_status, int out_cap, int* out_n, int* out_counts8);") in code
    assert ("int pmv_klt_step_many_stereo(pmv_ctx* ctx, int n_trk, const int* ids, const int* prev_slots, const int* cur_slots, const int* right_slots, "
            "int* out_ids, int* out_ages, float* out_xy, float* out_prev_xy_or_null, float* out_right_xy, uint8_t* out_right_status, int out_stride, "
            "int* out_n , int* out_counts8 );") in code
    assert "int pmv_debug_klt_stereo_stats(pmv_ctx* ctx, long long* out4);" in code
    # the plain steps keep their signatures, and pmv_klt_params is not extended
    assert ("int pmv_klt_step(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int* out_ids, int* out_ages, float* out_xy, float* out_prev_xy_or_null, "
            "int out_cap, int* out_n, int* out_counts8);") in code
    body = code[code.index("typedef struct pmv_klt_params {"):code.index("} pmv_klt_params;")]
    assert "stereo" not in body and "right" not in body


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    doc = text[text.index("Stereo matches in the tracker step"):text.index("typedef struct pmv_klt_stereo_params")]
    for phrase in ("Result definition", "returns exactly those bytes and leaves exactly that state", "the right observations are not state", "except counts8[7]",
                   "pmv_lk_track_fb(ctx, cur_slot, right_slot, xy, n, flags 0)", "st[i] == 1 && bst[i] == 1 && dx * dx + dy * dy <= thr2 && inBorder(rxy[i])",
                   "without contraction", "(float)(fb_max_dist * fb_max_dist)", "round half to even", "the right frame's size",
                   "pmv_lk_track_ex(.., flags 0); ok[i] = st[i] == 1 && inBorder(rxy[i])", "matched or not", "counts8[7] = the number of matched tracks",
                   "0 in pmv_klt_step, which stays so", "a caller pairs by index", "n == 0: nothing is written to the right arrays and counts8[7] = 0",
                   "starts at the left position", "the VINS stereo reverse pass starts at the right position", "VINS applies no border test when its back check is off",
                   "NULL turns it off", "byte for byte its own pmv_klt_step_stereo", "right_slots[j] < 0", "right status all 0", "its right xy are not written",
                   "needs no stereo setting", "may differ from tracker to tracker", "no additional wait", "once, twice with reject_f", "at most twice",
                   "sized by the bound", "the sum of the targets of the trackers with a right slot", "at most 3 launches", "whatever n_trk is",
                   "return their usual bytes", "no tracker's state changes", "without a stereo setting", "the old setting is kept", "before anything is launched",
                   "the message names the tracker", "refused in the same words", "writes the completion word the host checks", "PMV_ERR_HIP",
                   "do not move pmv_debug_klt_stats or pmv_debug_klt_many_stats"):
        assert phrase in doc, phrase
    scope = doc[doc.index("Out of scope:"):]
    for phrase in ("the session form", "a backward pass without the initial guess", "another size", "epipolar", "compacted right lists", "right positions as tracker state"):
        assert phrase in scope, phrase
    # the mono group call no longer offers itself to a stereo pair
    many = text[text.index("A group of trackers in one call"):text.index("int pmv_klt_step_many(")]
    assert "a stereo pair" not in many


def test_a_null_context_is_refused(pmv):
    lib = pmv.load_library()
    lib.pmv_last_error.restype = C.c_char_p
    rc, untouched, _ = ks.raw_step(None, lib, 0, 0, 1, 2, 8)
    assert rc == INVALID and untouched and b"pmv_klt_step" in lib.pmv_last_error(None)
    rc, untouched, _ = ks.raw_many(None, lib, [0, 1], [0, 0], [1, 1], [2, -1], 8)
    assert rc == INVALID and untouched and b"pmv_klt_step_many" in lib.pmv_last_error(None)
    vp = C.c_void_p
    big = np.full(4, -7, np.int64)
    lib.pmv_debug_klt_stereo_stats.argtypes = [vp, vp]
    assert lib.pmv_debug_klt_stereo_stats(None, big.ctypes.data) == INVALID and (big == -7).all()
    assert b"pmv_debug_klt_stereo_stats" in lib.pmv_last_error(None)
    p, on = pmv.KltStereoParams(0.5, 1), C.c_int(-7)
    lib.pmv_klt_set_stereo.argtypes = [vp, C.c_int, vp]
    lib.pmv_klt_get_stereo.argtypes = [vp, C.c_int, vp, vp]
    assert lib.pmv_klt_set_stereo(None, 0, C.addressof(p)) == INVALID and b"pmv_klt_set_stereo" in lib.pmv_last_error(None)
    assert lib.pmv_klt_get_stereo(None, 0, C.addressof(p), C.addressof(on)) == INVALID and on.value == -7
    assert (p.fb_max_dist, p.border) == (0.5, 1)


def test_trackers_of_another_context_are_refused_before_the_library(pmv):
    class Dummy:
        lib, h = None, None
    mine, other = pmv.Context.__new__(pmv.Context), Dummy()
    mine.lib, mine.h = None, None
    trk = pmv.KltTracker(other, 0, 10)
    own = pmv.KltTracker(mine, 0, 10)
    with pytest.raises(ValueError, match="of this context"):
        pmv.Context.klt_step_many_stereo(mine, [own, trk], [0, 0], [1, 1], [2, 2])
    with pytest.raises(ValueError, match="one right_slot per tracker"):
        pmv.Context.klt_step_many_stereo(mine, [own], [0], [1], [2, 3])
