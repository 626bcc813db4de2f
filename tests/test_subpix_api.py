"""pmv_corner_subpix without a GPU: the new symbols are declared, exported and bound with the documented ctypes signatures; the ctypes
mirror of pmv_subpix_params has the header's fields in the header's order and C layout; the binding hands its arguments to the library as
that struct and the point array in place; it refuses wrong arrays before the library is touched; the header states the contract."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_corner_subpix", "pmv_batch_corner_subpix", "pmv_debug_subpix_launches"]
CTYPES = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
_u8p, _f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float)


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
    assert callable(pmv.Context.debug_subpix_launches)
    for method in ("corner_subpix", "batch_corner_subpix"):
        sig = inspect.signature(getattr(pmv.Context, method))
        assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
            ("slot", inspect.Parameter.empty), ("xy", inspect.Parameter.empty), ("win", (5, 5)), ("zero_zone", (-1, -1)), ("max_iter", 30), ("eps", 0.01),
            ("return_info", False)]


def test_the_declared_argument_lists():
    code = _code()
    args = "pmv_ctx* ctx, int slot, float* xy, int n, const pmv_subpix_params* p, uint8_t* out_iters, uint8_t* out_flags"
    assert f"int pmv_corner_subpix({args});" in code
    assert f"int pmv_batch_corner_subpix({args});" in code
    assert "int pmv_debug_subpix_launches(pmv_ctx* ctx, long long* out3);" in code


def test_struct_layout_matches_the_header(pmv):
    src = _header()
    body = src[src.index("typedef struct pmv_subpix_params {"):src.index("} pmv_subpix_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = []
    for t, names in re.findall(r"\b(int|double|float)\s+([\w\s,]+);", body):
        decl += [(t, n.strip()) for n in names.split(",")]
    assert [n for _, n in decl] == ["win_w", "win_h", "zero_w", "zero_h", "max_iter", "eps"]
    assert [(n, CTYPES[t]) for t, n in decl] == list(pmv.SubpixParams._fields_)
    off = 0
    for t, n in decl:
        size = C.sizeof(CTYPES[t])
        off = (off + size - 1) // size * size
        assert getattr(pmv.SubpixParams, n).offset == off, n
        off += size
    assert C.sizeof(pmv.SubpixParams) == (off + 7) // 8 * 8 == 32


class _Recorder:
    """stands in for the library: records the arguments of every call, moves the points as a library would, and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        class _Fn:
            argtypes = None

            def __call__(fn, *args):
                self.calls.append((name, args, fn.argtypes))
                if name.endswith("corner_subpix"):
                    n = args[3]
                    xy = np.ctypeslib.as_array(args[2], shape=(max(n, 1) * 2,))
                    self.seen = xy[:2 * n].copy()
                    xy[:2 * n] += 0.5
                    for k, p in ((5, 3), (6, 9)):
                        if args[k] is not None:
                            np.ctypeslib.as_array(args[k], shape=(max(n, 1),))[:n] = p
                return 0
        f = _Fn()
        object.__setattr__(self, name, f)
        return f


@pytest.mark.parametrize("method, symbol", [("corner_subpix", "pmv_corner_subpix"), ("batch_corner_subpix", "pmv_batch_corner_subpix")])
def test_the_binding_passes_the_struct_and_the_array_in_place(pmv, method, symbol):
    ctx = object.__new__(pmv.Context)
    ctx.lib, ctx.h = _Recorder(), None
    pts = np.asarray([(1.5, 2.5), (10, 20), (30.25, 4)], np.float32)
    keep = pts.copy()
    out, iters, flags = getattr(ctx, method)(2, pts, win=(3, 7), zero_zone=(1, 0), max_iter=40, eps=0.001, return_info=True)
    name, args, argtypes = ctx.lib.calls[0]
    assert name == symbol
    assert list(argtypes) == [C.c_void_p, C.c_int, _f32p, C.c_int, C.POINTER(pmv.SubpixParams), _u8p, _u8p]
    assert args[1] == 2 and args[3] == 3
    p = C.cast(args[4], C.POINTER(pmv.SubpixParams)).contents
    assert (p.win_w, p.win_h, p.zero_w, p.zero_h, p.max_iter, p.eps) == (3, 7, 1, 0, 40, 0.001)
    # the library saw the caller's values, worked in place on the array that is returned, and the caller's array is untouched
    assert np.array_equal(ctx.lib.seen, keep.ravel()) and np.array_equal(pts, keep)
    assert out.shape == (3, 2) and out.dtype == np.float32 and np.array_equal(out, keep + 0.5)
    assert iters.dtype == flags.dtype == np.uint8 and iters.tolist() == [3] * 3 and flags.tolist() == [9] * 3
    # the defaults; without return_info the two outputs are NULL
    out = getattr(ctx, method)(0, pts)
    _, args, _ = ctx.lib.calls[1]
    p = C.cast(args[4], C.POINTER(pmv.SubpixParams)).contents
    assert (p.win_w, p.win_h, p.zero_w, p.zero_h, p.max_iter, p.eps) == (5, 5, -1, -1, 30, 0.01) and args[5] is None and args[6] is None
    assert isinstance(out, np.ndarray) and np.array_equal(out, keep + 0.5)
    # a strided view is read where it is and returned tight; n = 0 is passed on
    big = np.zeros((6, 4), np.float32)
    big[:, 1:3] = 7
    assert np.array_equal(getattr(ctx, method)(0, big[::2, 1:3]), np.full((3, 2), 7.5, np.float32))
    assert getattr(ctx, method)(0, np.zeros((0, 2), np.float32)).shape == (0, 2) and ctx.lib.calls[-1][1][3] == 0
    # refused before the library is touched
    n = len(ctx.lib.calls)
    for bad in (pts.astype(np.float64), pts.astype(np.int32), pts.ravel(), np.zeros((3, 3), np.float32), [(1.0, 2.0)], None):
        with pytest.raises(ValueError):
            getattr(ctx, method)(1, bad)
    for kw in (dict(win=(5,)), dict(zero_zone=(1, 2, 3))):
        with pytest.raises(ValueError):
            getattr(ctx, method)(1, pts, **kw)
    assert len(ctx.lib.calls) == n


def test_the_debug_call_is_bound(pmv):
    ctx = object.__new__(pmv.Context)
    ctx.lib, ctx.h = _Recorder(), None
    assert ctx.debug_subpix_launches() == [0, 0, 0]
    name, _, argtypes = ctx.lib.calls[0]
    assert name == "pmv_debug_subpix_launches" and list(argtypes) == [C.c_void_p, C.POINTER(C.c_longlong)]


def test_the_header_states_the_contract():
    src = " ".join(_header().replace("*", " ").split())
    doc = src[src.index("cv::cornerSubPix(level 0 of `slot`"):src.index("typedef struct pmv_subpix_params")]
    for phrase in ("mask[i][j] = (float)(vy expf(-x x))", "x = (float)(j - win_w) / win_w", "vy = expf(-y y)",
                   "zero_w >= 0 && zero_h >= 0 && 2 zero_w + 1 < 2 win_w + 1 && 2 zero_h + 1 < 2 win_h + 1", "it is ignored and is not an error",
                   "computed on the HOST with libm", "a device expf does not have libm's bits",
                   "getRectSubPix(src, (2 win_w + 3) x (2 win_h + 3), cI)", "0 <= ip.x && ip.x + W < cols && 0 <= ip.y && ip.y + H < rows",
                   "a = max(a, 0.0001f)", "prev = (float)(t s)", "s = (1. - a) / a in double", "only t[j] and t[j-1]", "four float weights a11..a22",
                   "replicated borders", "both sample columns clamp to the same column", "src b1 + src2 b2", "64-pixel REFLECT_101 frame",
                   "does NOT sample it", "replicate-clamped to the real w x h image", "float differences of patch neighbours", "gxx = tgx tgx m",
                   "fabs(det) <= DBL_EPSILON^2", "scale = 1.0 / det", "err is the squared float step", "outside [0, cols) x [0, rows)",
                   "while (++iter < max_iter && err > eps eps)", "|cI.x - cT.x| > win_w or |cI.y - cT.y| > win_h", "ONE order is fixed",
                   "tests/twin/subpix_twin.cpp", "does not depend on n, on the point's position in the launch, or on single versus session form",
                   "the number of position updates made, 0..100", "bit 1 = stopped on the determinant test", "2 = left the frame",
                   "4 = the iteration cap ended the loop with err > eps^2", "8 = reverted to the input position",
                   "cols >= 2 win_w + 5", "cannot fire", "outside the frame too", "OpenCV 3.4 cornersubpix.cpp, samplers.cpp",
                   "nothing is written on any of them", "win_w or win_h outside 1..15", "max_iter outside 1..100", "nothing is clamped",
                   "eps negative or not finite", "not finite or beyond 1e6 in magnitude", "n above max_tracks", "the slot errors of pmv_lk_track",
                   "n == 0 is PMV_OK and launches nothing", "made by the first call on a context"):
        assert phrase in doc, phrase
    gftt = src[src.index("cv::goodFeaturesToTrack with the caller's remaining arguments"):src.index("typedef struct pmv_gftt_params")]
    assert "Out of scope: the Sobel aperture (gradientSize) stays 3" in gftt and "pmv_corner_subpix" in gftt
    assert re.search(r"pmv_corner_subpix\s+cv::cornerSubPix", _header()), "the citation table at the top names the call"
    sess = src[src.index("pmv_corner_subpix as a session call"):src.index("int pmv_batch_corner_subpix")]
    for phrase in ("the same arguments, bits and status codes", "detector combiner", "agree in the six parameters share ONE launch",
                   "launches exactly what it launched before", "wait for the next round"):
        assert phrase in sess, phrase
