"""pmv_camera_create_fisheye and pmv_fisheye_map_build without a GPU: the functions and the struct are declared, exported and bound; the
argument lists; the header's contract; and the refusals that need no device (the null context and null arguments)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -2


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def _code():
    return " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())


def test_the_symbols_are_declared_exported_and_bound(pmv):
    code = _code()
    lib = pmv.load_library()
    for name in ("pmv_camera_create_fisheye", "pmv_fisheye_map_build"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    assert "typedef struct pmv_fisheye_params { double fx, fy, cx, cy; double k[4]; } pmv_fisheye_params;" in code
    assert "int pmv_camera_create_fisheye(pmv_ctx* ctx, const pmv_fisheye_params* p, int* out_id);" in code
    assert ("int pmv_fisheye_map_build(const double* K9, const double* k4, const double* R9_or_null, const double* newK9_or_null, int w, int h, "
            "float* map_x, float* map_y);") in code
    assert [f[0] for f in pmv.FisheyeParams._fields_] == ["fx", "fy", "cx", "cy", "k"] and C.sizeof(pmv.FisheyeParams) == 8 * 8
    # pmv_camera_params did not grow
    assert C.sizeof(pmv.CameraParams) == 13 * 8
    assert list(inspect.signature(pmv.Context.camera_create_fisheye).parameters) == ["self", "fx", "fy", "cx", "cy", "k"]
    assert list(inspect.signature(pmv.fisheye_map_build).parameters) == ["K", "k", "size", "R", "new_K"]
    p = pmv.fisheye_params(1.0, 2.0, 3.0, 4.0, k=(0.1, 0.2))
    assert (p.fx, p.fy, p.cx, p.cy, list(p.k)) == (1.0, 2.0, 3.0, 4.0, [0.1, 0.2, 0.0, 0.0])
    try:
        pmv.fisheye_params(1.0, 1.0, 0.0, 0.0, k=(0,) * 5)
    except ValueError as e:
        assert "at most 4" in str(e)
    else:
        raise AssertionError("five coefficients were accepted")


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    doc = text[text.index("cv::fisheye cameras: the equidistant model"):text.index("typedef struct pmv_fisheye_params")]
    for phrase in ("Kalibr", "the same table as pmv_camera_create", "pmv_camera_destroy frees it", "A rig may mix models", "No launch and no wait is added",
                   "IEEE + - * / only", "without contraction", "correctly rounded double square root", "pmv_atan", "pmv_tan", "scripts/derive_atan_tan.py",
                   "0x1.921fb54442d18p+0", "two-part pi/2", "2^-40", "mpmath at 50 digits",
                   "a = X / Z; b = Y / Z; r2 = a*a + b*b; r = sqrt(r2); t = pmv_atan(r)", "td = t * (1 + k1*t2 + k2*t4 + k3*t6 + k4*t8)", "s = r > 1e-8 ? td / r : 1.0",
                   "u = fx*(a*s) + cx; v = fy*(b*s) + cy", "r must be finite", "px = ((double)u - cx) * ifx; py = ((double)v - cy) * ify",
                   "td = sqrt(px*px + py*py); if (td > PI_2) td = PI_2", "repeat at most 10 times",
                   "fix = (t*(1 + k1*t2 + k2*t4 + k3*t6 + k4*t8) - td) / (1 + 3*k1*t2 + 5*k2*t4 + 7*k3*t6 + 9*k4*t8)", "if (fabs(fix) < 1e-8) { converged = true; break }",
                   "good = converged && t >= 0 && t <= PI_2", "s = pmv_tan(t) / td", "x = px*s; y = py*s", "no NaN is ever written", "Differences from OpenCV",
                   "did not converge", "not mirrored", "skew is not taken", "Parity with a real OpenCV is unpinned", "tests/twin/fisheye_twin.cpp bit for bit",
                   "cv::fisheye::initUndistortRectifyMap", "by adjugate and determinant", "(-1, -1)", "pmv_remap_map_create", "k[2]", "a 17th camera",
                   "a singular newK R"):
        assert phrase in doc, phrase
    scope = doc[doc.index("Out of scope:"):]
    for phrase in ("skew", "R / P", "Jacobian", "the session form", "omnidirectional"):
        assert phrase in scope, phrase
    # the older sections no longer list the model as missing
    assert "cv::fisheye and other camera models" not in text and "cv::fisheye models are out of scope" not in text
    assert "camera models other than pmv_camera_params'" not in text


def test_the_documents_name_the_remaining_gaps():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "`cv::fisheye` and other camera models" not in design
    for name in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "pmv_camera_create_fisheye" in open(os.path.join(ROOT, name)).read(), name


def test_refusals_that_need_no_device(pmv):
    lib = pmv.load_library()
    lib.pmv_last_error.restype = C.c_char_p
    vp = C.c_void_p
    lib.pmv_camera_create_fisheye.argtypes = [vp, vp, vp]
    p, out = pmv.fisheye_params(190.97, 190.97, 254.93, 256.90, k=(0.003482, 0.000715, -0.002053, 0.000202)), C.c_int(-7)
    assert lib.pmv_camera_create_fisheye(None, C.addressof(p), C.addressof(out)) == INVALID and out.value == -7
    assert b"pmv_camera_create_fisheye" in lib.pmv_last_error(None)
    assert lib.pmv_camera_create_fisheye(None, None, None) == INVALID
    mx = np.full(4, -7, np.float32)
    lib.pmv_fisheye_map_build.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    assert lib.pmv_fisheye_map_build(None, None, None, None, 2, 2, mx.ctypes.data, mx.ctypes.data) == INVALID
    assert b"pmv_fisheye_map_build" in lib.pmv_last_error(None) and (mx == -7).all()
