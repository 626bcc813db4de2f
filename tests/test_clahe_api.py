"""pmv_frames_clahe without a GPU: the new symbols are declared with the documented argument lists, exported and bound; the ctypes mirror of
pmv_clahe_params has the header's fields in the header's order and C layout; the binding hands its arguments to the library as that struct;
it refuses wrong arguments before the library is touched; the header states the contract."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_frames_clahe", "pmv_batch_frame_upload_clahe", "pmv_debug_clahe_launches"]
CTYPES = {"int": C.c_int, "double": C.c_double, "float": C.c_float}


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
    assert callable(pmv.Context.debug_clahe_launches)
    sig = inspect.signature(pmv.Context.frames_clahe)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [("first_slot", inspect.Parameter.empty), ("n", inspect.Parameter.empty),
                                                                       ("clip_limit", 40.0), ("tiles", (8, 8))]
    sig = inspect.signature(pmv.Context.batch_frame_upload)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [("slot", inspect.Parameter.empty), ("frame", inspect.Parameter.empty), ("fmt", "gray"),
                                                                       ("clahe", None)]


def test_the_declared_argument_lists():
    code = _code()
    assert "int pmv_frames_clahe(pmv_ctx* ctx, int first_slot, int n, const pmv_clahe_params* p);" in code
    assert ("int pmv_batch_frame_upload_clahe(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format, "
            "const pmv_clahe_params* p);") in code
    assert "int pmv_debug_clahe_launches(pmv_ctx* ctx, long long* out3);" in code
    # the plain upload keeps its argument list
    assert "int pmv_batch_frame_upload(pmv_ctx* ctx, int slot, const uint8_t* pixels, int w, int h, int stride, int format);" in code


def test_struct_layout_matches_the_header(pmv):
    src = _header()
    body = src[src.index("typedef struct pmv_clahe_params {"):src.index("} pmv_clahe_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = []
    for t, names in re.findall(r"\b(int|double|float)\s+([\w\s,]+);", body):
        decl += [(t, n.strip()) for n in names.split(",")]
    assert [n for _, n in decl] == ["clip_limit", "tiles_x", "tiles_y"]
    assert [(n, CTYPES[t]) for t, n in decl] == list(pmv.ClaheParams._fields_)
    off = 0
    for t, n in decl:
        size = C.sizeof(CTYPES[t])
        off = (off + size - 1) // size * size
        assert getattr(pmv.ClaheParams, n).offset == off, n
        off += size
    assert C.sizeof(pmv.ClaheParams) == (off + 7) // 8 * 8 == 16


class _Recorder:
    """stands in for the library: records the arguments of every call and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        class _Fn:
            argtypes = None

            def __call__(fn, *args):
                seen = list(args)
                for i, a in enumerate(seen):   # the struct lives only during the call: keep its values
                    if name.endswith("clahe") and i == len(seen) - 1 and a is not None:
                        p = C.cast(a, C.POINTER(self.params)).contents
                        seen[i] = (p.clip_limit, p.tiles_x, p.tiles_y)
                self.calls.append((name, seen, fn.argtypes))
                return 0
        f = _Fn()
        object.__setattr__(self, name, f)
        return f


def _recording(pmv):
    ctx = object.__new__(pmv.Context)
    ctx.lib, ctx.h = _Recorder(), None
    ctx.lib.params = pmv.ClaheParams
    return ctx


def test_frames_clahe_passes_the_struct(pmv):
    ctx = _recording(pmv)
    ctx.frames_clahe(3, 5, clip_limit=2.5, tiles=(4, 3))
    name, args, argtypes = ctx.lib.calls[0]
    assert name == "pmv_frames_clahe"
    assert list(argtypes) == [C.c_void_p, C.c_int, C.c_int, C.POINTER(pmv.ClaheParams)]
    assert args[1:] == [3, 5, (2.5, 4, 3)]
    ctx.frames_clahe(0, 1)   # cv's defaults
    assert ctx.lib.calls[1][1][1:] == [0, 1, (40.0, 8, 8)]
    ctx.frames_clahe(np.int32(2), np.int64(1), clip_limit=np.float32(0), tiles=np.asarray([16, 1]))
    assert ctx.lib.calls[2][1][1:] == [2, 1, (0.0, 16, 1)]
    # values the library refuses are the library's to refuse (its status codes are part of the contract): they are passed on
    ctx.frames_clahe(0, 1, clip_limit=-1.0, tiles=(0, 17))
    assert ctx.lib.calls[3][1][3] == (-1.0, 0, 17)
    # refused before the library is touched: what the struct cannot hold as the caller meant it
    n = len(ctx.lib.calls)
    for kw in (dict(tiles=(8,)), dict(tiles=(8, 8, 8)), dict(tiles=8), dict(tiles=(8.0, 8)), dict(tiles=(True, 8)), dict(tiles=None), dict(clip_limit="2"),
               dict(clip_limit=None), dict(clip_limit=True), dict(clip_limit=(2.0,))):
        with pytest.raises(ValueError):
            ctx.frames_clahe(0, 1, **kw)
    assert len(ctx.lib.calls) == n


def test_batch_frame_upload_routes_by_the_clahe_argument(pmv):
    ctx = _recording(pmv)
    img = np.zeros((48, 64), np.uint8)
    view = np.zeros((60, 80, 3), np.uint8)[5:53, 8:72]
    ctx.batch_frame_upload(2, img)
    ctx.batch_frame_upload(3, img, "gray", clahe=(2.0, (4, 3)))
    ctx.batch_frame_upload(4, view, "bgr", clahe=(0, (16, 16)))
    (n0, a0, _), (n1, a1, t1), (n2, a2, _) = ctx.lib.calls
    assert n0 == "pmv_batch_frame_upload" and len(a0) == 7 and a0[1] == 2
    assert n1 == n2 == "pmv_batch_frame_upload_clahe"
    assert list(t1) == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(pmv.ClaheParams)]
    assert a1[1] == 3 and a1[2].value == img.ctypes.data and a1[3:] == [64, 48, 64, pmv.FRAME_FORMATS["gray"], (2.0, 4, 3)]
    # a view is passed in place, with its own address and stride
    assert a2[1] == 4 and a2[2].value == view.ctypes.data and a2[3:] == [64, 48, 240, pmv.FRAME_FORMATS["bgr"], (0.0, 16, 16)]
    n = len(ctx.lib.calls)
    for bad in (2.0, (2.0,), (2.0, 8), (2.0, (8, 8), 1), "on", (None, (8, 8)), (2.0, (8.5, 8))):
        with pytest.raises(ValueError):
            ctx.batch_frame_upload(0, img, "gray", clahe=bad)
    with pytest.raises(ValueError):   # the source checks of the plain call hold
        ctx.batch_frame_upload(0, img.astype(np.float32), "gray", clahe=(2.0, (8, 8)))
    assert len(ctx.lib.calls) == n


def test_the_debug_call_is_bound(pmv):
    ctx = _recording(pmv)
    assert ctx.debug_clahe_launches() == [0, 0, 0]
    name, _, argtypes = ctx.lib.calls[0]
    assert name == "pmv_debug_clahe_launches" and list(argtypes) == [C.c_void_p, C.POINTER(C.c_longlong)]


def test_the_header_states_the_contract():
    src = " ".join(_header().replace("*", " ").split())
    doc = src[src.index("cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply(level 0, level 0)"):src.index("typedef struct pmv_clahe_params")]
    for phrase in ("staged (pmv_frames_stage) or built", "may differ in size", "byte for byte what pmv_frame_upload of the equalised image would have left",
                   "whatever build_pyramids says", "A second call equalises again", "front-end stream", "stays legal under the caller's slot rule",
                   "w % tiles_x == 0 && h % tiles_y == 0", "tiles_x - w % tiles_x columns", "tiles_y - h % tiles_y rows with REFLECT_101",
                   "still gets a full extra tiles_x or tiles_y", "from the INTERIOR of level 0", "lutScale = (float)255 / area",
                   "max((int)(clip_limit area / 256), 1) : 0", "clamped to area before the cast", "inv_tw = 1.0f / tile_w",
                   "clipped = sum of max(hist[i] - cl, 0)", "batch = clipped / 256", "step = max(256 / residual, 1)",
                   "i % step == 0 && i / step < residual", "saturate_u8(rint((float)sum lutScale))", "half to even", "txf = x inv_tw - 0.5f",
                   "tx2 = min(tx2, tiles_x - 1)", "(lut[ty2][tx1][v] xa1 + lut[ty2][tx2][v] xa) ya", "without contraction", "k_clahe_lut", "k_clahe_apply",
                   "ONE pair of launches per 64 frames", "is not sized by n", "level-0 profiling class", "OpenCV 3.4 clahe.cpp", "tests/twin/clahe_twin.cpp",
                   "nothing is written, nothing is clamped", "tiles_x or tiles_y outside 1..16", "clip_limit negative or not finite",
                   "an empty slot (the message names it)", "pmv_frames_stream_begin bracket or a batched run is open", "as for pmv_frames_build",
                   "cv::equalizeHist", "16-bit images", "builds the pyramid twice"):
        assert phrase in doc, phrase
    assert re.search(r"pmv_frames_clahe\s+cv::CLAHE::apply", _header()), "the citation table at the top names the call"
    sess = src[src.index("pmv_batch_frame_upload with the equalisation of pmv_frames_clahe"):src.index("int pmv_batch_frame_upload_clahe")]
    for phrase in ("NULL is PMV_ERR_INVALID", "the pyramid is built once", "in the same round as plain uploads", "ONE k_clahe_lut launch and ONE k_clahe_apply launch",
                   "ONE in-place k_pad_level0 launch", "counted as a level-0 launch", "launches exactly what it launched before", "grows to the largest round seen"):
        assert phrase in sess, phrase
