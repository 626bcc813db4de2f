"""pmv_frames_remap and its companions without a GPU: the new symbols are declared with the documented argument lists, exported and bound;
the binding hands its arguments to the library as declared and refuses wrong ones before the library is touched; the session upload routes
by its remap argument, alone and combined with clahe; the header states the contract."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_remap_map_create", "pmv_remap_map_destroy", "pmv_frames_remap", "pmv_debug_remap_launches", "pmv_batch_frame_upload_remap"]
UPLOAD_REMAP = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]   # .. and the CLAHE parameters' pointer


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def _code():
    return " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())


def test_the_new_symbols_are_declared_exported_and_bound(pmv):
    code = _code()
    lib = pmv.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(\s*pmv_ctx\*" % name, code), f"{name} is not declared in include/pmv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    assert "pmv_undistort_map_build" in pmv.ABI_SYMBOLS and hasattr(lib, "pmv_undistort_map_build")

    def params(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]
    E = inspect.Parameter.empty
    assert params(pmv.undistort_map) == [("K", E), ("dist", E), ("size", E), ("R", None), ("new_K", None)]
    assert params(pmv.Context.remap_map_create)[1:] == [("map_x", E), ("map_y", E)]
    assert params(pmv.Context.remap_map_destroy)[1:] == [("map_id", E)]
    assert params(pmv.Context.frames_remap)[1:] == [("first_slot", E), ("n", E), ("map_id", E), ("border_value", 0)]
    assert params(pmv.Context.batch_frame_upload_remap)[1:] == [("slot", E), ("frame", E), ("remap", E), ("fmt", "gray"), ("clahe", None)]
    assert callable(pmv.Context.debug_remap_launches)


def test_the_declared_argument_lists():
    code = _code()
    for decl in ("int pmv_remap_map_create(pmv_ctx* ctx, int w, int h, const float* map_x, const float* map_y, int* out_id);",
                 "int pmv_remap_map_destroy(pmv_ctx* ctx, int id);",
                 "int pmv_frames_remap(pmv_ctx* ctx, int first_slot, int n, int map_id, int border_value);",
                 "int pmv_debug_remap_launches(pmv_ctx* ctx, long long* out3);",
                 "int pmv_batch_frame_upload_remap(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format, int map_id, "
                 "int border_value, const pmv_clahe_params* clahe_or_null);",
                 "int pmv_undistort_map_build(const double* K9, const double* dist8, const double* R9_or_null, const double* newK9_or_null, int w, int h, "
                 "float* map_x, float* map_y);",
                 # the existing uploads keep their argument lists
                 "int pmv_batch_frame_upload(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format);",
                 "int pmv_batch_frame_upload_clahe(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format, const pmv_clahe_params* p);"):
        assert decl in code, decl


class _Recorder:
    """stands in for the library: records the arguments of every call and reports success"""

    def __init__(self, params):
        self.calls = []
        self.params = params

    def __getattr__(self, name):
        class _Fn:
            argtypes = None

            def __call__(fn, *args):
                seen = list(args)
                if name == "pmv_batch_frame_upload_remap" and seen[-1] is not None:   # the struct lives only during the call: keep its values
                    p = C.cast(seen[-1], C.POINTER(self.params)).contents
                    seen[-1] = (p.clip_limit, p.tiles_x, p.tiles_y)
                if name == "pmv_remap_map_create":
                    w, h = seen[1], seen[2]
                    seen[3] = np.ctypeslib.as_array(seen[3], (h, w)).copy()
                    seen[4] = np.ctypeslib.as_array(seen[4], (h, w)).copy()
                    seen[5]._obj.value = 11
                self.calls.append((name, seen, fn.argtypes))
                return 0
        f = _Fn()
        object.__setattr__(self, name, f)
        return f


def _recording(pmv):
    ctx = object.__new__(pmv.Context)
    ctx.lib, ctx.h = _Recorder(pmv.ClaheParams), None
    return ctx


def test_the_map_calls_pass_their_arguments(pmv):
    ctx = _recording(pmv)
    mx = np.arange(12, dtype=np.float64).reshape(3, 4)          # converted to float32, tight
    my = np.asfortranarray(np.ones((3, 4), np.float32) * 2.5)
    assert ctx.remap_map_create(mx, my) == 11
    name, args, argtypes = ctx.lib.calls[0]
    f32p = C.POINTER(C.c_float)
    assert name == "pmv_remap_map_create" and list(argtypes) == [C.c_void_p, C.c_int, C.c_int, f32p, f32p, C.POINTER(C.c_int)]
    assert args[1:3] == [4, 3] and np.array_equal(args[3], mx.astype(np.float32)) and np.array_equal(args[4], my)
    ctx.remap_map_destroy(np.int64(11))
    assert ctx.lib.calls[1][0] == "pmv_remap_map_destroy" and ctx.lib.calls[1][1][1:] == [11]
    ctx.frames_remap(3, 5, 11)
    ctx.frames_remap(np.int32(0), 1, 2, border_value=200)
    assert ctx.lib.calls[2][0] == "pmv_frames_remap" and list(ctx.lib.calls[2][2]) == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    assert ctx.lib.calls[2][1][1:] == [3, 5, 11, 0] and ctx.lib.calls[3][1][1:] == [0, 1, 2, 200]
    # values the library refuses are the library's to refuse (its status codes are part of the contract): they are passed on
    ctx.frames_remap(0, 1, 99, border_value=256)
    assert ctx.lib.calls[4][1][1:] == [0, 1, 99, 256]
    n = len(ctx.lib.calls)
    for a, b in ((np.zeros((3, 4)), np.zeros((4, 3))), (np.zeros(12), np.zeros(12)), (np.zeros((2, 3, 4)), np.zeros((2, 3, 4)))):
        with pytest.raises(ValueError):
            ctx.remap_map_create(a, b)
    assert len(ctx.lib.calls) == n
    assert ctx.debug_remap_launches() == [0, 0, 0]
    name, _, argtypes = ctx.lib.calls[-1]
    assert name == "pmv_debug_remap_launches" and list(argtypes) == [C.c_void_p, C.POINTER(C.c_longlong)]


def test_the_session_upload_routes_remap_and_its_combination_with_clahe(pmv):
    ctx = _recording(pmv)
    img = np.zeros((48, 64), np.uint8)
    view = np.zeros((60, 80, 3), np.uint8)[5:53, 8:72]
    ctx.batch_frame_upload(2, img)
    ctx.batch_frame_upload_remap(3, img, 5)
    ctx.batch_frame_upload_remap(4, view, (6, 200), "bgr", clahe=(2.0, (4, 3)))
    ctx.batch_frame_upload_remap(5, img, remap=(np.int32(0), np.int64(255)), clahe=(0, (16, 16)))
    ctx.batch_frame_upload(6, img, "gray", clahe=(2.0, (4, 3)))
    (n0, a0, _), (n1, a1, t1), (n2, a2, _), (n3, a3, _), (n4, a4, _) = ctx.lib.calls
    assert n0 == "pmv_batch_frame_upload" and len(a0) == 7 and n4 == "pmv_batch_frame_upload_clahe" and len(a4) == 8
    assert n1 == n2 == n3 == "pmv_batch_frame_upload_remap"
    assert list(t1) == UPLOAD_REMAP + [C.POINTER(pmv.ClaheParams)]
    assert a1[1] == 3 and a1[2].value == img.ctypes.data and a1[3:] == [64, 48, 64, pmv.FRAME_FORMATS["gray"], 5, 0, None]
    # a view is passed in place, with its own address and stride
    assert a2[1] == 4 and a2[2].value == view.ctypes.data and a2[3:] == [64, 48, 240, pmv.FRAME_FORMATS["bgr"], 6, 200, (2.0, 4, 3)]
    assert a3[1] == 5 and a3[3:] == [64, 48, 64, pmv.FRAME_FORMATS["gray"], 0, 255, (0.0, 16, 16)]
    n = len(ctx.lib.calls)
    for bad in (None, 2.0, (1,), (1, 2, 3), (1, 2.0), (True, 0), "1", (None, 0)):
        with pytest.raises(ValueError):
            ctx.batch_frame_upload_remap(0, img, bad)
    for bad in (2.0, (2.0,), (2.0, 8), (None, (8, 8))):
        with pytest.raises(ValueError):
            ctx.batch_frame_upload_remap(0, img, 1, clahe=bad)
    with pytest.raises(ValueError):   # the source checks of the plain call hold
        ctx.batch_frame_upload_remap(0, img.astype(np.float32), 1)
    assert len(ctx.lib.calls) == n


def test_the_header_states_the_contract():
    src = " ".join(_header().replace("*", " ").split())
    maps = src[src.index("A remap map, created once per camera"):src.index("int pmv_remap_map_create")]
    for phrase in ("tight w x h CV_32FC1 maps of cv::remap", "converts them ONCE, on the host", "At most 16 maps per context", "sized by w h",
                   "sx = cvRound(map_x 32.0f)", "which is exact", "half to even", "gives INT_MIN, as cvtss2si does", "ix = saturate_s16(sx >> 5)", "arithmetic shift",
                   "fx = sx & 31", "6 bytes per pixel", "OpenCV 3.4 imgwarp.cpp", "PMV_ERR_CAPACITY - a 17th map", "an unknown id", "while a batch session is open"):
        assert phrase in maps, phrase
    doc = src[src.index("cv::remap(level 0, level 0, map, INTER_LINEAR, BORDER_CONSTANT"):src.index("int pmv_frames_remap")]
    for phrase in ("staged (pmv_frames_stage) or built", "byte for byte what pmv_frame_upload of the remapped image would have left",
                   "whatever build_pyramids says", "front-end stream", "stays legal under the caller's slot rule", "must equal the map's size",
                   "inside the w x h interior of level 0, else border_value", "never read from the slot's own border",
                   "D = ((32 - fy)(32 - fx) tap(ix, iy) + (32 - fy) fx tap(ix + 1, iy) + fy (32 - fx) tap(ix, iy + 1) + fy fx tap(ix + 1, iy + 1) + 512) >> 10",
                   "(sum of w tap + 2^14) >> 15", "32 times the one above", "exactly where fx = fy = 0", "all taps inside, all outside, mixed", "k_remap",
                   "ONE launch per 64 frames", "cannot run in place", "is not sized by n", "level-0 profiling class", "[mem: OpenCV 3.4 imgwarp.cpp",
                   "parity with a real OpenCV is unpinned", "tests/twin/remap_twin.cpp", "nothing is written, nothing is clamped", "an unknown map_id",
                   "border_value outside 0..255", "an empty slot (the message names it)", "names the slot and both sizes",
                   "pmv_frames_stream_begin bracket or a batched run is open", "as for pmv_frames_build", "other interpolations and border modes", "16-bit images",
                   "builds the pyramid twice"):
        assert phrase in doc, phrase
    assert re.search(r"pmv_frames_remap\s+cv::remap\(INTER_LINEAR, BORDER_CONSTANT\)", _header()), "the citation table at the top names the call"
    sess = src[src.index("pmv_batch_frame_upload with the remap of pmv_frames_remap"):src.index("int pmv_batch_frame_upload_remap")]
    for phrase in ("the pyramid is built once", "conversion, then remap, then equalisation", "never gathered over the bus", "ONE k_remap launch for all remap requests",
                   "grows to the largest round seen", "ONE list-form k_pad_level0 launch from that scratch", "counted as a level-0 launch", "the k_pyrdown launches, once",
                   "launches and records exactly what it did before"):
        assert phrase in sess, phrase
    build = src[src.index("The map of cv::initUndistortRectifyMap"):src.index("int pmv_undistort_map_build")]
    for phrase in ("needs no context", "(k1, k2, p1, p2, k3, k4, k5, k6)", "a null R is the identity", "adjugate and determinant",
                   "kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2)", "held to a tolerance", "cv::fisheye", "a singular newK R"):
        assert phrase in build, phrase
