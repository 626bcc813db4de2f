"""Cameras, pmv_undistort_points and the tracker's observation setting without a GPU: the functions and structs are declared, exported and
bound; the argument lists; the header's contract; and the refusals that need no device (the null context)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_camera_create", "pmv_camera_destroy", "pmv_undistort_points", "pmv_klt_set_observe", "pmv_klt_get_observe", "pmv_klt_get_observations",
       "pmv_debug_klt_observe_stats"]
INVALID = -2


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def _code():
    return " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())


def _fields(code, name):
    body = code[code.index("typedef struct %s {" % name):code.index("} %s;" % name)].split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", part.split()[-1]) for part in decl.split(",")]
    return names


def test_the_symbols_are_declared_exported_and_bound(pmv):
    code = _code()
    lib = pmv.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(\s*pmv_ctx\*" % name, code), f"{name} is not declared in include/pmv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    assert "#define PMV_MAX_CAMERAS 16" in _header()
    assert _fields(code, "pmv_camera_params") == [f[0] for f in pmv.CameraParams._fields_] == ["fx", "fy", "cx", "cy", "dist", "iters"]
    assert _fields(code, "pmv_klt_observe_params") == [f[0] for f in pmv.KltObserveParams._fields_] == ["cam_id", "right_cam_id", "dt", "undistorted_f", "f_focal"]
    assert C.sizeof(pmv.CameraParams) == 13 * 8 and C.sizeof(pmv.KltObserveParams) == 32
    for method in ("set_observe", "get_observe", "get_observations"):
        assert callable(getattr(pmv.KltTracker, method))
    for method in ("camera_create", "camera_destroy", "undistort_points", "debug_klt_observe_stats"):
        assert callable(getattr(pmv.Context, method))
    p = pmv.camera_params(1.0, 2.0, 3.0, 4.0, dist=(0.1, 0.2), iters=7)
    assert (p.fx, p.fy, p.cx, p.cy, list(p.dist), p.iters) == (1.0, 2.0, 3.0, 4.0, [0.1, 0.2, 0, 0, 0, 0, 0, 0], 7)


def test_the_declared_argument_lists():
    code = _code()
    assert "int pmv_camera_create(pmv_ctx* ctx, const pmv_camera_params* p, int* out_id);" in code
    assert "int pmv_camera_destroy(pmv_ctx* ctx, int id);" in code
    assert "int pmv_undistort_points(pmv_ctx* ctx, int cam_id, const float* xy, int n, float* out_xy, uint8_t* out_ok);" in code
    assert "int pmv_klt_set_observe(pmv_ctx* ctx, int id, const pmv_klt_observe_params* p_or_null);" in code
    assert "int pmv_klt_get_observe(pmv_ctx* ctx, int id, pmv_klt_observe_params* out, int* out_on);" in code
    assert ("int pmv_klt_get_observations(pmv_ctx* ctx, int id, float* out_un_xy, float* out_vel, uint8_t* out_ok, float* out_right_un_xy_or_null, "
            "uint8_t* out_right_ok_or_null, int cap, int* out_n);") in code
    assert "int pmv_debug_klt_observe_stats(pmv_ctx* ctx, long long* out4);" in code
    # no step entry point gets a new signature, and pmv_klt_params is not extended
    assert ("int pmv_klt_step(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int* out_ids, int* out_ages, float* out_xy, float* out_prev_xy_or_null, "
            "int out_cap, int* out_n, int* out_counts8);") in code
    assert ("int pmv_klt_step_stereo(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int right_slot, int* out_ids, int* out_ages, float* out_xy, "
            "float* out_prev_xy_or_null, float* out_right_xy, uint8_t* out_right_status, int out_cap, int* out_n, int* out_counts8);") in code
    assert ("int pmv_klt_step_many(pmv_ctx* ctx, int n_trk, const int* ids, const int* prev_slots, const int* cur_slots, int* out_ids, int* out_ages, float* out_xy, "
            "float* out_prev_xy_or_null, int out_stride, int* out_n , int* out_counts8 );") in code
    body = code[code.index("typedef struct pmv_klt_params {"):code.index("} pmv_klt_params;")]
    assert "cam" not in body and "observe" not in body and "dt" not in body


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    assert re.search(r"pmv_undistort_points\s+cv::undistortPoints", text[:text.index("#ifndef PMV_HIP_H")]), "the line of the top table"
    doc = text[text.index("cameras and cv::undistortPoints"):text.index("#define PMV_MAX_CAMERAS")]
    for phrase in ("cv::undistortPoints(src CV_32FC2, dst, K, dist)", "no R and no P", "Result definition", "IEEE + - * / only", "without contraction",
                   "ifx = 1.0 / fx and ify = 1.0 / fy are computed once on the host", "x0 = ((double)u - cx) * ifx", "r2 = x*x + y*y",
                   "icdist = (1 + ((k6*r2 + k5)*r2 + k4)*r2) / (1 + ((k3*r2 + k2)*r2 + k1)*r2)", "dX = 2*p1*x*y + p2*(r2 + 2*x*x)", "dY = p1*(r2 + 2*y*y) + 2*p2*x*y",
                   "x = (x0 - dX) * icdist; y = (y0 - dY) * icdist", "still finite after rounding to float", "out_xy = (0, 0)", "no NaN is ever written",
                   "parity with a real OpenCV is unpinned", "tests/twin/lift_twin.cpp bit for bit", "one small device table", "one wait",
                   "n == 0 is legal and launches nothing", "nothing is written, nothing is clamped", "fx or fy zero or not finite", "iters outside 1..50",
                   "an unknown camera id", "beyond 1e6", "the message names the point", "a tracker's observation setting names", "a 17th camera",
                   "n above max_tracks", "pmv_ctx_destroy frees the cameras"):
        assert phrase in doc, phrase
    scope = doc[doc.index("Out of scope:"):]
    for phrase in ("cv::fisheye", "R / P", "thin-prism and tilt", "the session form", "a forward distort_points call"):
        assert phrase in scope, phrase
    doc = text[text.index("Normalised observations and velocities from the tracker step"):text.index("typedef struct pmv_klt_observe_params")]
    for phrase in ("(id, x, y, 1, u, v, vx, vy)", "off by default", "No step entry point gets a new signature", "a bad value keeps the old setting",
                   "a pure function of what the step returns", "(un, ok) = lift(cam_id, xy[i])", "(pun, pok) = lift(cam_id, prev_xy[i])",
                   "ages[i] > 1 && ok && pok", "vel.x = (float)((double)(un.x - pun.x) / dt)", "one float32 operation", "the division is in double",
                   "a new track, whose prev_xy is its own xy", "no per-track state is added", "out_right_ok[i] = right_status[i] && rok", "unmatched tracks are lifted too",
                   "out_right_ok is all 0 and the right xy are not written", "byte for byte those of the same step with the setting off",
                   "a host copy, no device work", "ran with the setting off", "has not stepped since pmv_klt_create or pmv_klt_set_tracks", "cap < n",
                   "reject_f and n1 >= 15", "BEFORE its rounding to float", "q = ((float)(f_focal * xd + w / 2.0), (float)(f_focal * yd + h / 2.0))",
                   "separate double operations", "both of its points are (0, 0)", "counts8[5..6] are unchanged", "its own completion word", "PMV_ERR_HIP",
                   "whatever n_trk is", "leaves at once", "at most one launch more", "no additional wait", "runs under that wait", "pmv_debug_klt_observe_stats",
                   "cannot be destroyed until the setting is cleared"):
        assert phrase in doc, phrase
    scope = doc[doc.index("Out of scope:"):]
    for phrase in ("right-camera velocities", "the session form", "a camera other than cam_id", "cv::fisheye", "thin-prism", "distort_points"):
        assert phrase in scope, phrase
    # the older sections no longer list the lift as missing
    stereo = text[text.index("Stereo matches in the tracker step"):text.index("typedef struct pmv_klt_stereo_params")]
    assert "normalised coordinates and velocities, compacted" not in stereo
    assert "callers with a lens remap the frames first" not in text


def test_a_null_context_is_refused(pmv):
    lib = pmv.load_library()
    lib.pmv_last_error.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    fl, by, it = np.full(8, -7, np.float32), np.full(4, 0xA5, np.uint8), np.full(4, -7, np.int32)
    big = np.full(4, -7, np.int64)
    cam = pmv.camera_params(300.0, 300.0, 160.0, 100.0)
    obs = pmv.KltObserveParams(0, -1, 0.1, 0, 460.0)
    lib.pmv_camera_create.argtypes = [vp, vp, vp]
    lib.pmv_camera_destroy.argtypes = [vp, ci]
    lib.pmv_undistort_points.argtypes = [vp, ci, vp, ci, vp, vp]
    lib.pmv_klt_set_observe.argtypes = [vp, ci, vp]
    lib.pmv_klt_get_observe.argtypes = [vp, ci, vp, vp]
    lib.pmv_klt_get_observations.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp]
    lib.pmv_debug_klt_observe_stats.argtypes = [vp, vp]
    f, b, i = fl.ctypes.data, by.ctypes.data, it.ctypes.data
    for name, rc in (("pmv_camera_create", lib.pmv_camera_create(None, C.addressof(cam), i)), ("pmv_camera_destroy", lib.pmv_camera_destroy(None, 0)),
                     ("pmv_undistort_points", lib.pmv_undistort_points(None, 0, f, 2, f, b)), ("pmv_klt_set_observe", lib.pmv_klt_set_observe(None, 0, C.addressof(obs))),
                     ("pmv_klt_get_observe", lib.pmv_klt_get_observe(None, 0, C.addressof(obs), i)),
                     ("pmv_klt_get_observations", lib.pmv_klt_get_observations(None, 0, f, f, b, f, b, 2, i)),
                     ("pmv_debug_klt_observe_stats", lib.pmv_debug_klt_observe_stats(None, big.ctypes.data))):
        assert rc == INVALID, name
    assert b"pmv_debug_klt_observe_stats" in lib.pmv_last_error(None)
    assert (fl == -7).all() and (by == 0xA5).all() and (it == -7).all() and (big == -7).all()
    assert (obs.cam_id, obs.right_cam_id, obs.dt, obs.undistorted_f, obs.f_focal) == (0, -1, 0.1, 0, 460.0)
