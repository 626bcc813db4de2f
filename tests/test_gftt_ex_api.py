"""pmv_detect_gftt_ex without a GPU: the new symbols are declared, exported and bound with the documented ctypes signatures; the ctypes
mirror of pmv_gftt_params has the header's fields in the header's order and C layout; the binding hands its arguments to the library as
that struct, a strided mask in place; the header states the contract."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_detect_gftt_ex", "pmv_debug_gftt_response_ex", "pmv_debug_gftt_general", "pmv_batch_detect_gftt_ex"]
CTYPES = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
_u8p, _i32p, _f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float)


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
    for method in ("detect_gftt_ex", "batch_detect_gftt_ex", "gftt_response_ex", "debug_gftt_general"):
        assert callable(getattr(pmv.Context, method))
    for method in ("detect_gftt_ex", "batch_detect_gftt_ex"):
        sig = inspect.signature(getattr(pmv.Context, method))
        assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
            ("slot", inspect.Parameter.empty), ("cells", inspect.Parameter.empty), ("max_per_cell", inspect.Parameter.empty), ("quality", 0.01),
            ("min_dist", 5.0), ("mask", None), ("block_size", 3), ("use_harris", False), ("k", 0.04)]


def test_the_declared_argument_lists():
    code = _code()
    args = "pmv_ctx* ctx, int slot, const int* cells, int n_cells, int max_per_cell, const pmv_gftt_params* p, const uint8_t* mask, int mask_stride, int* out_xy, int* out_count"
    assert f"int pmv_detect_gftt_ex({args});" in code
    assert f"int pmv_batch_detect_gftt_ex({args});" in code
    assert "int pmv_debug_gftt_response_ex(pmv_ctx* ctx, int slot, const int* cell, const pmv_gftt_params* p, float* out);" in code
    assert "int pmv_debug_gftt_general(pmv_ctx* ctx, int on);" in code


def test_struct_layout_matches_the_header(pmv):
    src = _header()
    body = src[src.index("typedef struct pmv_gftt_params {"):src.index("} pmv_gftt_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"\b(int|double|float)\s+(\w+)\s*;", body)
    assert [n for _, n in decl] == ["quality", "min_dist", "block_size", "use_harris", "k"]
    assert [(n, CTYPES[t]) for t, n in decl] == list(pmv.GfttParams._fields_)
    off = 0
    for t, n in decl:
        size = C.sizeof(CTYPES[t])
        off = (off + size - 1) // size * size
        assert getattr(pmv.GfttParams, n).offset == off, n
        off += size
    assert C.sizeof(pmv.GfttParams) == (off + 7) // 8 * 8 == 32


class _Recorder:
    """stands in for the library: records the arguments of every call and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        class _Fn:
            argtypes = None

            def __call__(fn, *args):
                self.calls.append((name, args, fn.argtypes))
                return 0
        f = _Fn()
        object.__setattr__(self, name, f)
        return f


@pytest.mark.parametrize("method, symbol", [("detect_gftt_ex", "pmv_detect_gftt_ex"), ("batch_detect_gftt_ex", "pmv_batch_detect_gftt_ex")])
def test_the_binding_passes_the_struct_and_the_mask_in_place(pmv, method, symbol):
    ctx = object.__new__(pmv.Context)
    ctx.lib, ctx.h = _Recorder(), None
    big = np.zeros((50, 90), np.uint8)
    mask = big[3:43, 10:70]   # 60x40, row stride 90
    cells = [(0, 0, 60, 40), (5, 5, 20, 20)]
    out = getattr(ctx, method)(1, cells, 7, quality=0.05, min_dist=3.0, mask=mask, block_size=5, use_harris=True, k=0.06)
    assert [o.shape for o in out] == [(0, 2), (0, 2)]
    name, args, argtypes = ctx.lib.calls[0]
    assert name == symbol
    assert list(argtypes) == [C.c_void_p, C.c_int, _i32p, C.c_int, C.c_int, C.POINTER(pmv.GfttParams), _u8p, C.c_int, _i32p, _i32p]
    assert args[1] == 1 and args[3] == 2 and args[4] == 7
    p = C.cast(args[5], C.POINTER(pmv.GfttParams)).contents
    assert (p.quality, p.min_dist, p.block_size, p.use_harris, p.k) == (0.05, 3.0, 5, 1, 0.06)
    assert C.cast(args[6], C.c_void_p).value == mask.ctypes.data and args[7] == 90
    # no mask: a null pointer, stride 0
    getattr(ctx, method)(0, cells, 0)
    _, args, _ = ctx.lib.calls[1]
    p = C.cast(args[5], C.POINTER(pmv.GfttParams)).contents
    assert args[6] is None and args[7] == 0 and args[4] == 0 and (p.quality, p.min_dist, p.block_size, p.use_harris, p.k) == (0.01, 5.0, 3, 0, 0.04)
    # refused before the library is touched: wrong dtype, a mask that does not cover a cell
    n = len(ctx.lib.calls)
    for bad in (np.zeros((40, 60), np.float32), np.zeros((30, 60), np.uint8), np.zeros((40, 60), np.uint8)[:, ::2]):
        with pytest.raises(ValueError):
            getattr(ctx, method)(1, cells, 7, mask=bad)
    assert len(ctx.lib.calls) == n


def test_the_debug_calls_are_bound(pmv):
    ctx = object.__new__(pmv.Context)
    ctx.lib, ctx.h = _Recorder(), None
    ctx.debug_gftt_general(True)
    assert ctx.lib.calls[0][:2] == ("pmv_debug_gftt_general", (None, 1))
    out = ctx.gftt_response_ex(2, (1, 2, 30, 20), block_size=7, use_harris=True, k=0.05)
    name, args, argtypes = ctx.lib.calls[1]
    p = C.cast(args[3], C.POINTER(pmv.GfttParams)).contents
    assert name == "pmv_debug_gftt_response_ex" and out.shape == (20, 30) and out.dtype == np.float32 and (p.block_size, p.use_harris, p.k) == (7, 1, 0.05)
    assert list(argtypes) == [C.c_void_p, C.c_int, _i32p, C.POINTER(pmv.GfttParams), _f32p]


def test_the_header_states_the_contract():
    src = " ".join(_header().replace("*", " ").split())
    doc = src[src.index("cv::goodFeaturesToTrack with the caller's remaining arguments"):src.index("typedef struct pmv_gftt_params")]
    for phrase in ("NULL = no mask", "non-zero byte allows the pixel", "maximum over the ALLOWED pixels", "masked-out ones included", "anchor block_size / 2",
                   "REFLECT_101 on the CELL as often as needed", "1 / (4 block_size 255)", "returns the bytes of pmv_detect_gftt", "k_gftt_cand_general",
                   "block_size outside 1..15", "quality outside (0, 1]", "min_dist negative or not finite", "k not finite while use_harris is set",
                   "mask_stride below the frame width", "nothing is written on any of them", "Out of scope: the Sobel aperture (gradientSize) stays 3",
                   "tests/twin/gftt_twin.cpp"):
        assert phrase in doc, phrase
