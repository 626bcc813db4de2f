"""pmv_project_points, pmv_lk_track_fb_levels and the tracker's prediction (pmv_klt_set_prediction, pmv_klt_get_prediction_result) without a
GPU: the functions and the struct are declared, exported and bound; the argument lists; the header's contract; and the refusals that need
no device (the null context)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_project_points", "pmv_lk_track_fb_levels", "pmv_klt_set_prediction", "pmv_klt_get_prediction_result"]
INVALID = -2


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def _code():
    return " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())


def _fields(code, name):
    body = code[code.index("typedef struct %s {" % name):code.index("} %s;" % name)].split("{", 1)[1]
    return [decl.split()[-1] for decl in body.split(";") if decl.strip()]


def test_the_symbols_are_declared_exported_and_bound(pmv):
    code = _code()
    lib = pmv.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(\s*pmv_ctx\*" % name, code), f"{name} is not declared in include/pmv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    for method in ("project_points", "lk_track_fb_levels"):
        assert callable(getattr(pmv.Context, method))
    sig = inspect.signature(pmv.Context.lk_track_fb_levels).parameters
    assert sig["fwd_top_level"].default == -1 and sig["back_top_level"].default == -1 and sig["back"].default is True
    assert _fields(code, "pmv_klt_predict_params") == [f[0] for f in pmv.KltPredictParams._fields_] == ["cam_id", "top_level", "back_top_level", "min_succ"]
    assert C.sizeof(pmv.KltPredictParams) == 16
    sig = inspect.signature(pmv.KltTracker.set_prediction).parameters
    assert list(sig)[1:4] == ["cam_id", "ids", "xyz"] and (sig["top_level"].default, sig["back_top_level"].default, sig["min_succ"].default) == (1, 1, 10)
    assert callable(pmv.KltTracker.get_prediction_result)


def test_the_declared_argument_lists():
    code = _code()
    assert "int pmv_project_points(pmv_ctx* ctx, int cam_id, const double* xyz , int n, float* out_xy, uint8_t* out_ok);" in code
    assert ("int pmv_lk_track_fb_levels(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy , int flags, "
            "int fwd_top_level, int back_top_level, uint8_t* out_status, float* out_err, float* back_xy_or_null, uint8_t* back_status_or_null, "
            "float* back_err_or_null);") in code
    assert ("int pmv_klt_set_prediction(pmv_ctx* ctx, int id, const pmv_klt_predict_params* p_or_null, const int* ids, const double* xyz , int n);") in code
    assert "int pmv_klt_get_prediction_result(pmv_ctx* ctx, int id, int* out4);" in code
    # no step entry point gets a new signature, and pmv_klt_params is not extended
    assert ("int pmv_klt_step(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int* out_ids, int* out_ages, float* out_xy, float* out_prev_xy_or_null, "
            "int out_cap, int* out_n, int* out_counts8);") in code
    body = code[code.index("typedef struct pmv_klt_params {"):code.index("} pmv_klt_params;")]
    assert "predict" not in body and "level" not in body
    # the calls they extend keep their signatures
    assert "int pmv_undistort_points(pmv_ctx* ctx, int cam_id, const float* xy, int n, float* out_xy, uint8_t* out_ok);" in code
    assert ("int pmv_lk_track_fb(pmv_ctx* ctx, int prev_slot, int next_slot, const float* prev_xy, int n, float* next_xy , int flags, "
            "uint8_t* out_status, float* out_err, float* back_xy, uint8_t* back_status, float* back_err);") in code


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    assert re.search(r"pmv_project_points\s+cv::projectPoints without rvec / tvec", text[:text.index("#ifndef PMV_HIP_H")]), "the line of the top table"
    doc = text[text.index("cv::projectPoints without rvec and tvec"):text.index("int pmv_project_points(")]
    for phrase in ("IEEE + - * / only", "without contraction", "x = X / Z; y = Y / Z; r2 = x*x + y*y", "kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)",
                   "xd = x*kr + (2*p1*x*y + p2*(r2 + 2*x*x))", "yd = y*kr + (p1*(r2 + 2*y*y) + 2*p2*x*y)", "u = fx*xd + cx; v = fy*yd + cy", "Z > 0",
                   "before and after their rounding to float", "<= 1e6", "out_xy = (0, 0)", "no NaN is ever written", "parity with a real OpenCV is unpinned",
                   "tests/twin/project_twin.cpp bit for bit", "one launch", "one wait", "n == 0 is legal and launches nothing", "an unknown camera id",
                   "n above max_tracks", "NaN and infinities included, is no error"):
        assert phrase in doc, phrase
    scope = doc[doc.index("Out of scope:"):]
    for phrase in ("rvec / tvec", "cv::fisheye", "thin-prism and tilt", "the session form"):
        assert phrase in scope, phrase
    doc = text[text.index("cv's maxLevel as a per-call argument"):text.index("int pmv_lk_track_fb_levels(")]
    for phrase in ("min(fwd_top_level, L - 1)", "min(back_top_level, L - 1)", "-1 means L - 1", "the bytes of pmv_lk_track_fb", "forward only",
                   "the bytes of pmv_lk_track_ex", "One or two of them NULL: PMV_ERR_INVALID", "a level outside -1 .. 4", "Nothing is clamped except by L",
                   "no slot is emptied", "ONE launch", "workgroup-uniform", "tests/twin/lkx_twin.cpp", "max_level = min(top, the context's max_level)"):
        assert phrase in doc, phrase
    scope = doc[doc.index("Out of scope:"):]
    for phrase in ("the session form", "a per-track level"):
        assert phrase in scope, phrase


def test_the_header_states_the_prediction(pmv):
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    doc = text[text.index("Predicted positions in the tracker step"):text.index("typedef struct pmv_klt_predict_params")]
    for phrase in ("setPrediction", "spaceToPlane", "one-shot", "a refused step leaves it pending", "NULL or n = 0 clears it", "pmv_klt_set_tracks leaves it pending",
                   "No step entry point gets a new signature", "only stage 1 changes", "pmv_project_points(cam_id, xyz[k])", "else xy[i]",
                   "pmv_lk_track_fb_levels(prev_slot, cur_slot, xy, next_xy = guess, PMV_LK_USE_INITIAL_FLOW, top_level, back_top_level, ..)",
                   "forward only", "succ < min_succ", "flags 0, -1, back_top_level", "fell_back = 1", "{1, 0, 0, 0}", "{consumed, joined, succ, fell_back}",
                   "a host copy", "no additional wait", "at most 2 more launches in a single step and at most 2 more in a many-call", "whatever n_trk is",
                   "binary search", "sorts once", "one integer atomic add", "deterministic", "leave at once when succ >= min_succ", "workgroup-uniform",
                   "mix freely", "an id named twice", "top_level outside 0..4", "back_top_level outside -1..4", "min_succ < 0", "n above PMV_REFILL_MAX_TRACKS",
                   "cannot be destroyed"):
        assert phrase in doc, phrase
    scope = doc[doc.index("Out of scope:"):]
    for phrase in ("the session form", "a level per track", "back_top_level for steps without a prediction", "stereo stage 8 at a capped level"):
        assert phrase in scope, phrase


def test_a_null_context_is_refused(pmv):
    lib = pmv.load_library()
    lib.pmv_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    fl, by, db = np.full(8, -7, np.float32), np.full(4, 0xA5, np.uint8), np.full(12, 1.0, np.float64)
    lib.pmv_project_points.argtypes = [vp, ci, vp, ci, vp, vp]
    lib.pmv_lk_track_fb_levels.argtypes = [vp, ci, ci, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp]
    f, b = fl.ctypes.data, by.ctypes.data
    assert lib.pmv_project_points(None, 0, db.ctypes.data, 4, f, b) == INVALID
    assert b"pmv_project_points" in lib.pmv_last_error(None)
    assert lib.pmv_lk_track_fb_levels(None, 0, 1, f, 4, f, 0, 1, 1, b, f, f, b, f) == INVALID
    assert b"pmv_lk_track_fb_levels" in lib.pmv_last_error(None)
    assert lib.pmv_lk_track_fb_levels(None, 0, 1, f, 4, f, 0, 1, 1, b, f, None, None, None) == INVALID
    lib.pmv_klt_set_prediction.argtypes = [vp, ci, vp, vp, vp, ci]
    lib.pmv_klt_get_prediction_result.argtypes = [vp, ci, vp]
    p, ids, out4 = pmv.KltPredictParams(0, 1, 1, 10), np.arange(4, dtype=np.int32), np.full(4, -7, np.int32)
    assert lib.pmv_klt_set_prediction(None, 0, C.addressof(p), ids.ctypes.data, db.ctypes.data, 4) == INVALID
    assert b"pmv_klt_set_prediction" in lib.pmv_last_error(None)
    assert lib.pmv_klt_get_prediction_result(None, 0, out4.ctypes.data) == INVALID
    assert b"pmv_klt_get_prediction_result" in lib.pmv_last_error(None)
    assert (fl == -7).all() and (by == 0xA5).all() and (out4 == -7).all()
