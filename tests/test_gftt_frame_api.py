"""pmv_detect_gftt_frame without a GPU: the three symbols are declared, exported and bound; the session method has the single call's
signature; the header states the rules of the call."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_detect_gftt_frame", "pmv_batch_detect_gftt_frame", "pmv_debug_gftt_frame_stats"]


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def _code():
    return " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())


def test_the_three_symbols_are_declared_exported_and_bound(pmv):
    code = _code()
    lib = pmv.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(\s*pmv_ctx\*" % name, code), f"{name} is not declared in include/pmv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    for method in ("detect_gftt_frame", "batch_detect_gftt_frame", "debug_gftt_frame_stats"):
        assert callable(getattr(pmv.Context, method))
    assert pmv.GFTT_FRAME_MAX_CORNERS == 16384 and "#define PMV_GFTT_FRAME_MAX_CORNERS 16384" in _header()


def test_the_declared_argument_lists():
    code = _code()
    args = ("pmv_ctx* ctx, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const uint8_t* mask, int mask_stride, "
            "int* out_xy, int out_cap, int* out_count")
    assert f"int pmv_detect_gftt_frame({args});" in code
    assert f"int pmv_batch_detect_gftt_frame({args});" in code
    assert "int pmv_debug_gftt_frame_stats(pmv_ctx* ctx, long long* out6);" in code


def test_the_session_method_has_the_single_calls_signature(pmv):
    single = inspect.signature(pmv.Context.detect_gftt_frame)
    assert inspect.signature(pmv.Context.batch_detect_gftt_frame) == single
    assert [(k, p.default) for k, p in single.parameters.items()][1:] == [
        ("slot", inspect.Parameter.empty), ("max_corners", inspect.Parameter.empty), ("quality", 0.01), ("min_dist", 5.0), ("mask", None),
        ("block_size", 3), ("use_harris", False), ("k", 0.04), ("roi", None), ("out_cap", None)]


def test_the_header_states_the_rules():
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())   # (the comment's line starts removed)
    doc = text[text.index("cv::goodFeaturesToTrack(frame(roi)"):text.index("int pmv_debug_gftt_frame_stats")]
    for phrase in ("max_corners <= 0 is cv's \"no limit\"", "returns PMV_ERR_OVERFLOW and writes nothing", "NULL = the whole frame",
                   "cap = max_corners > 0 ? max_corners : out_cap", "min(out_cap, PMV_GFTT_FRAME_MAX_CORNERS)",
                   "a region smaller than 3x3 or not inside the frame (the message names the region and the frame size)",
                   "Status bits of one call never leak into the next", "gftt_twin_cell", "not a lifted limit", "Out of scope"):
        assert phrase in doc, phrase
    session = text[text.index("pmv_detect_gftt_frame as a session call"):text.index("int pmv_batch_detect_gftt_frame")]
    for phrase in ("ONE pass-1 launch and ONE pass-2 launch", "block_size, use_harris, k, has-mask, quality, min_dist, cap, the no-limit flag and the frame layout",
                   "one workgroup per request", "A round without frame requests launches exactly what it launched before", "The mask is read before the call returns"):
        assert phrase in session, phrase
