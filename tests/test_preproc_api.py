"""pmv_set_frame_preproc and its companions without a GPU: the three symbols are declared with the documented argument lists, exported and
bound; the struct's ctypes mirror follows the header; the binding hands its arguments to the library as declared and refuses wrong ones
before the library is touched; the header states the contract and no longer lists the bracket and the feeder as out of scope."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmv_set_frame_preproc", "pmv_get_frame_preproc", "pmv_debug_preproc_launches"]


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def _code():
    return " ".join(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S).split())


def test_the_three_symbols_are_declared_exported_and_bound(pmv):
    code = _code()
    lib = pmv.load_library()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    for decl in ("int pmv_set_frame_preproc(pmv_ctx* ctx, const pmv_frame_preproc* p_or_null);",
                 "int pmv_get_frame_preproc(pmv_ctx* ctx, pmv_frame_preproc* out);",
                 "int pmv_debug_preproc_launches(pmv_ctx* ctx, long long* out4);",
                 "#define PMV_PREPROC_MAX_MAPS 8"):
        assert decl in code, decl

    def params(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]
    assert params(pmv.Context.set_frame_preproc)[1:] == [("remap", None), ("border_value", 0), ("clahe", None)]
    assert params(pmv.Context.get_frame_preproc) == [("self", inspect.Parameter.empty)]
    assert params(pmv.Context.debug_preproc_launches) == [("self", inspect.Parameter.empty)]


def test_the_struct_mirror_has_the_headers_field_order(pmv):
    code = _code()
    body = code[code.index("typedef struct pmv_frame_preproc {"):code.index("} pmv_frame_preproc;")]
    decl = re.findall(r"\b(int|pmv_clahe_params)\s+(\w+)(\[\w+\])?;", body)
    assert decl == [("int", "n_maps", ""), ("int", "map_ids", "[PMV_PREPROC_MAX_MAPS]"), ("int", "border_value", ""), ("int", "clahe", ""),
                    ("pmv_clahe_params", "clahe_params", "")]
    assert pmv.PREPROC_MAX_MAPS == 8
    fields = pmv.FramePreproc._fields_
    assert [f[0] for f in fields] == [d[1] for d in decl]
    assert fields[0][1] is C.c_int and fields[1][1] is C.c_int * 8 and fields[2][1] is C.c_int and fields[3][1] is C.c_int and fields[4][1] is pmv.ClaheParams
    # the C layout: 11 ints, then the double-aligned parameter struct
    assert pmv.FramePreproc.clahe_params.offset == 48 and C.sizeof(pmv.FramePreproc) == 64
    # the struct is declared after the types it holds and next to the remap calls it refers to
    h = _header()
    assert h.index("} pmv_clahe_params;") < h.index("typedef struct pmv_frame_preproc {") and h.index("int pmv_frames_remap(") < h.index("typedef struct pmv_frame_preproc {")


class _Recorder:
    """stands in for the library: records the arguments of every call and reports success"""

    def __init__(self, pmv):
        self.calls = []
        self.pmv = pmv

    def __getattr__(self, name):
        class _Fn:
            argtypes = None

            def __call__(fn, *args):
                seen = list(args)
                if name == "pmv_set_frame_preproc" and seen[1] is not None:   # the struct lives only during the call: keep its values
                    p = C.cast(seen[1], C.POINTER(self.pmv.FramePreproc)).contents
                    seen[1] = (p.n_maps, list(p.map_ids), p.border_value, p.clahe, (p.clahe_params.clip_limit, p.clahe_params.tiles_x, p.clahe_params.tiles_y))
                if name == "pmv_get_frame_preproc":
                    p = C.cast(seen[1], C.POINTER(self.pmv.FramePreproc)).contents
                    p.n_maps, p.border_value, p.clahe = 2, 200, 1
                    p.map_ids[0], p.map_ids[1] = 4, 9
                    p.clahe_params = self.pmv.ClaheParams(2.0, 8, 3)
                if name == "pmv_debug_preproc_launches":
                    for i in range(4):
                        seen[1][i] = 10 + i
                self.calls.append((name, seen, fn.argtypes))
                return 0
        f = _Fn()
        object.__setattr__(self, name, f)
        return f


def _recording(pmv):
    ctx = object.__new__(pmv.Context)
    ctx.lib, ctx.h = _Recorder(pmv), None
    return ctx


def test_the_binding_passes_its_arguments(pmv):
    ctx = _recording(pmv)
    ctx.set_frame_preproc()
    ctx.set_frame_preproc(remap=5)
    ctx.set_frame_preproc(remap=(np.int32(3), 7), border_value=200, clahe=(2.0, (8, 8)))
    ctx.set_frame_preproc(clahe=(0, (16, 1)))
    ctx.set_frame_preproc(remap=list(range(8)), border_value=np.int64(255))
    (n0, a0, t0), (_, a1, _), (_, a2, _), (_, a3, _), (_, a4, _) = ctx.lib.calls
    assert n0 == "pmv_set_frame_preproc" and list(t0) == [C.c_void_p, C.POINTER(pmv.FramePreproc)]
    assert a0[1] is None, "no arguments: the setting is cleared with a null pointer"
    assert a1[1] == (1, [5, 0, 0, 0, 0, 0, 0, 0], 0, 0, (0.0, 0, 0))
    assert a2[1] == (2, [3, 7, 0, 0, 0, 0, 0, 0], 200, 1, (2.0, 8, 8))
    assert a3[1] == (0, [0] * 8, 0, 1, (0.0, 16, 1))
    assert a4[1] == (8, list(range(8)), 255, 0, (0.0, 0, 0))
    assert ctx.get_frame_preproc() == dict(remap=[4, 9], border_value=200, clahe=(2.0, (8, 3)))
    assert ctx.lib.calls[-1][0] == "pmv_get_frame_preproc" and list(ctx.lib.calls[-1][2]) == [C.c_void_p, C.POINTER(pmv.FramePreproc)]
    assert ctx.debug_preproc_launches() == [10, 11, 12, 13]
    assert ctx.lib.calls[-1][0] == "pmv_debug_preproc_launches" and list(ctx.lib.calls[-1][2]) == [C.c_void_p, C.POINTER(C.c_longlong)]


def test_the_binding_refuses_before_the_library_is_touched(pmv):
    ctx = _recording(pmv)
    bad = [dict(remap=1.0), dict(remap=(1, 2.0)), dict(remap="1"), dict(remap=True), dict(remap=(None,)),   # a non-integer id
           dict(remap=list(range(9))),                                                                     # more than 8 ids
           dict(remap=1, border_value=256), dict(remap=1, border_value=-1), dict(border_value=1.0),
           dict(clahe=(2.0, (17, 8))), dict(clahe=(2.0, (8, 17))), dict(clahe=(2.0, (0, 8))),              # tiles outside 1..16
           dict(clahe=(-1.0, (8, 8))), dict(clahe=(float("nan"), (8, 8))), dict(clahe=(float("inf"), (8, 8))),   # the clip limit
           dict(clahe=2.0), dict(clahe=(2.0, 8)), dict(clahe=(2.0, (8.0, 8))), dict(clahe=(None, (8, 8)))]
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.set_frame_preproc(**kw)
    assert ctx.lib.calls == []


def test_the_header_states_the_contract():
    src = " ".join(_header().replace("*", " ").split())
    doc = src[src.index("Preprocessing of the host frames that the throughput paths take"):src.index("#define PMV_PREPROC_MAX_MAPS")]
    for phrase in ("next to pmv_set_frame_format", "from HOST memory through the feeder", "pmv_frames_stream_begin .. _end bracket, pmv_pipeline_run_streamed and pmv_pipeline_run_batch_streamed",
                   "BGR -> remap -> CLAHE -> border", "byte for byte what pmv_frame_upload of the preprocessed gray image would have left",
                   "pmv_frames_stage -> pmv_frames_remap -> pmv_frames_clahe", "tests/twin/remap_twin.cpp / clahe_twin.cpp", "the library does not touch K9",
                   "(B 1868 + G 9617 + R 4899 + 8192) >> 14", "Staged feeds are untouched", "pmv_frames_stage, pmv_frames_build - are not preprocessed",
                   "keep their own per-call forms", "each sequence uses the map of its own size", "names the sequence and the size",
                   "before any thread starts or any slot changes", "ONE k_remap_src launch in place of the level-0 launch", "no scratch frame",
                   "ONE k_clahe_lut + k_clahe_apply pair", "ONE in-place k_pad_level0 launch", "level-0 profiling class", "one aligned dword",
                   "bytes elsewhere", "a link transaction per tap", "whatever PMV_BATCH_INGEST says", "a caller's pinned buffer as well",
                   "pmv_batch_ingest_stats keeps counting the bytes moved", "A CLAHE-only feed keeps whichever form it would have had",
                   "exactly the launches it made before", "allocates nothing new", "n_maps outside 0..PMV_PREPROC_MAX_MAPS", "two maps of one size",
                   "border_value outside 0..255", "parameters that pmv_frames_clahe would refuse", "bracket or a batched run is open on the context",
                   "stays as it was, and nothing is clamped", "preprocessing of staged feeds"):
        assert phrase in doc, phrase
    maps = src[src.index("A remap map, created once per camera"):src.index("int pmv_remap_map_create")]
    assert "for a map that the current pmv_set_frame_preproc setting names (clear the setting first)" in maps
    assert "pmv_set_frame_preproc" in src[src.index("The format of the host frames that the throughput paths take"):src.index("enum pmv_frame_format")]


def test_the_bracket_and_the_feeder_are_no_longer_out_of_scope():
    src = " ".join(_header().replace("*", " ").split())
    clahe = src[src.index("cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply(level 0, level 0)"):src.index("typedef struct pmv_clahe_params")]
    remap = src[src.index("cv::remap(level 0, level 0, map, INTER_LINEAR, BORDER_CONSTANT"):src.index("int pmv_frames_remap")]
    for doc in (clahe, remap):
        scope = doc[doc.index("Out of scope:"):]
        assert "inside a pmv_frames_stream_begin bracket" not in scope and "inside the feeder" not in scope
        assert "pmv_set_frame_preproc" in scope
    for name in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert "inside the feeder of the two batched runs are not built" not in text and "pmv_set_frame_preproc" in text, name
