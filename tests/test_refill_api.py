"""pmv_detect_gftt_refill without a GPU: the four symbols are declared, exported and bound; the session form has the single call's
arguments; the header states the rules; and every refusal that needs no device (the null context, the binding's own argument checks)."""
import inspect
import os
import re

import numpy as np
import pytest

import refill_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_detect_gftt_refill", "pmv_batch_detect_gftt_refill", "pmv_debug_refill_mask", "pmv_debug_refill_stats"]
ARGS = ("pmv_ctx* ctx, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const float* track_xy, const int* track_prio_or_null, "
        "int n_tracks, int radius, const uint8_t* base_mask_or_null, int base_stride, uint8_t* out_keep, int* out_xy, int out_cap, int* out_count")


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def _code():
    return " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())


def test_the_four_symbols_are_declared_exported_and_bound(pmv):
    code = _code()
    lib = pmv.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(\s*pmv_ctx\*" % name, code), f"{name} is not declared in include/pmv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    for method in ("detect_gftt_refill", "batch_detect_gftt_refill", "debug_refill_mask", "debug_refill_stats"):
        assert callable(getattr(pmv.Context, method))
    assert pmv.REFILL_MAX_TRACKS == 8192 and "#define PMV_REFILL_MAX_TRACKS 8192" in _header()
    assert pmv.REFILL_MAX_RADIUS == 255 and "#define PMV_REFILL_MAX_RADIUS 255" in _header()


def test_the_declared_argument_lists():
    code = _code()
    assert f"int pmv_detect_gftt_refill({ARGS});" in code
    assert f"int pmv_batch_detect_gftt_refill({ARGS});" in code
    assert "int pmv_debug_refill_mask(pmv_ctx* ctx, uint8_t* out, long long cap, int* w, int* h);" in code
    assert "int pmv_debug_refill_stats(pmv_ctx* ctx, long long* out4);" in code


def test_the_session_method_has_the_single_calls_signature(pmv):
    single = inspect.signature(pmv.Context.detect_gftt_refill)
    assert inspect.signature(pmv.Context.batch_detect_gftt_refill) == single
    assert [(k, p.default) for k, p in single.parameters.items()][1:] == [
        ("slot", inspect.Parameter.empty), ("max_corners", inspect.Parameter.empty), ("tracks", inspect.Parameter.empty), ("radius", inspect.Parameter.empty),
        ("priorities", None), ("base_mask", None), ("quality", 0.01), ("min_dist", 5.0), ("block_size", 3), ("use_harris", False), ("k", 0.04), ("roi", None),
        ("out_cap", None)]


def test_the_header_states_the_rules():
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    doc = text[text.index("The refill of a KLT loop in one call"):text.index("int pmv_debug_refill_mask")]
    for phrase in ("round half to even", "priority descending, then index ascending", "NULL = all equal", "`== 255`", "cv::circle(mask, pt, radius, 0, -1)",
                   "radius 0 is the centre pixel", "NOT x^2 + y^2 <= r^2", "a track outside the region still suppresses tracks inside it",
                   "exactly pmv_detect_gftt_frame with that mask", "refill_twin_mask", "gftt_twin_cell", "nothing is written and nothing is clamped",
                   "in the same order", "the message names the point and the frame size", "min(max_tracks, PMV_REFILL_MAX_TRACKS)", "n_tracks == 0 is legal",
                   "not logged by pmv_record_enable", "Out of scope"):
        assert phrase in doc, phrase
    frame_doc = text[text.index("cv::goodFeaturesToTrack(frame(roi)"):text.index("int pmv_debug_gftt_frame_stats")]
    assert "the mask still comes from the host" not in frame_doc and "pmv_detect_gftt_refill below" in frame_doc
    session = text[text.index("pmv_detect_gftt_refill as a session call"):text.index("int pmv_batch_detect_gftt_refill")]
    for phrase in ("has-mask = true", "ONE k_track_select and ONE k_track_paint launch", "launches and allocates exactly what it did before",
                   "The track list and the base mask are read before the call returns"):
        assert phrase in session, phrase


def test_a_null_context_is_refused_by_every_new_call(pmv):
    lib = pmv.load_library()
    keep, xy, cnt = np.full(4, 9, np.uint8), np.full((4, 2), -7, np.int32), np.full(1, -7, np.int32)
    trk = np.zeros((4, 2), np.float32)
    P = pmv.GfttParams(0.01, 5.0, 3, 0, 0.04)
    for fn in (lib.pmv_detect_gftt_refill, lib.pmv_batch_detect_gftt_refill):
        assert rc.raw_refill_call(None, fn, 0, None, 4, P, trk, None, 4, 3, None, 0, keep, xy, 4, cnt) == rc.INVALID
        assert (keep == 9).all() and (xy == -7).all() and (cnt == -7).all()
    import ctypes as C
    lib.pmv_debug_refill_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.pmv_debug_refill_stats.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.pmv_debug_refill_mask(None, None, 0, None, None) == rc.INVALID
    assert lib.pmv_debug_refill_stats(None, None) == rc.INVALID


def test_the_binding_refuses_malformed_arrays_before_the_library(pmv):
    """(the methods check the shapes first: no context is needed to get that far)"""
    class Dummy:
        lib, h = None, None
    call = lambda **kw: pmv.Context._gftt_refill(Dummy(), None, None, 0, 10, kw.pop("tracks", np.zeros((3, 2), np.float32)), 5, kw.pop("priorities", None),   # noqa: E731
                                                  kw.pop("base_mask", None), 0.01, 5.0, 3, False, 0.04, kw.pop("roi", None), None)
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        call(tracks=np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="one priority per track"):
        call(priorities=np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="roi is"):
        call(roi=(0, 0, 10))
    with pytest.raises(ValueError, match="base_mask must be"):
        call(base_mask=np.zeros((4, 4), np.float32))
