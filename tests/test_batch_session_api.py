"""Batch sessions without a GPU: the binding checks dtype, shape, strides, fmt and the sizes before any library call, hands a strided view's
own address and stride to the library unchanged, and the header states every rule of a session at the calls it applies to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoDevice:
    """stands in for the library: any use means the binding reached the device (so every argument check has passed)"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} called before the arguments were checked")


class _Recorder:
    """stands in for the library: records the arguments of every call and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _ctx(pmv, lib):
    ctx = object.__new__(pmv.Context)
    ctx.lib = lib
    ctx.h = None
    return ctx


class _Tensor:
    """what the binding needs of a torch tensor: data_ptr(), shape, stride() in elements, dtype"""

    def __init__(self, arr, dtype="torch.uint8"):
        self.arr, self.shape, self.dtype = arr, arr.shape, dtype

    def data_ptr(self):
        return self.arr.ctypes.data

    def stride(self):
        return tuple(s // self.arr.itemsize for s in self.arr.strides)


def _bad_frames():
    g = np.zeros((48, 64), np.uint8)
    c = np.zeros((48, 64, 3), np.uint8)
    return [
        ("float frame", g.astype(np.float32), "gray"),
        ("int8 frame", g.astype(np.int8), "gray"),
        ("float tensor", _Tensor(g.astype(np.float32), "torch.float32"), "gray"),
        ("gray pixels not contiguous", g[:, ::2], "gray"),
        ("transposed gray", g.T, "gray"),
        ("BGR pixels not contiguous", c[:, ::2], "bgr"),
        ("a channel slice", np.zeros((48, 64, 4), np.uint8)[:, :, :3], "bgr"),
        ("two channels", np.zeros((48, 64, 2), np.uint8), "bgr"),
        ("four channels", np.zeros((48, 64, 4), np.uint8), "bgr"),
        ("gray array as bgr", g, "bgr"),
        ("colour array as gray", c, "gray"),
        ("a stack of frames", np.zeros((2, 48, 64), np.uint8), "gray"),
        ("rows upside down", g[::-1], "gray"),
        ("every row the same (stride 0)", np.broadcast_to(g[0], (48, 64)), "gray"),
        ("unknown fmt", g, "rgb"),
        ("fmt not a string", g, 1),
        ("fmt None", g, None),
        ("a list", [[0] * 64] * 48, "gray"),
    ]


@pytest.mark.parametrize("what, frame, fmt", _bad_frames(), ids=[b[0] for b in _bad_frames()])
def test_frames_the_library_cannot_read_are_refused_before_any_library_call(pmv, what, frame, fmt):
    with pytest.raises(ValueError):
        _ctx(pmv, _NoDevice()).batch_frame_upload(0, frame, fmt)


@pytest.mark.parametrize("n_seq, sizes", [
    (2, [(640.0, 200)]), (2, [(640, 200.5)]), (2, [(640, 200, 3)]), (2, [640, 200]), (2, []), (2, [("640", "200")]), (2, [(True, 200)]), (2, 640),
    (0, [(640, 200)]), (1.5, [(640, 200)]), ("2", [(640, 200)]),
])
def test_sizes_that_are_not_integer_pairs_are_refused_before_any_library_call(pmv, n_seq, sizes):
    with pytest.raises(ValueError):
        _ctx(pmv, _NoDevice()).batch_open(n_seq, sizes)


def test_good_arguments_reach_the_library(pmv):
    with pytest.raises(AssertionError, match="pmv_batch_open"):
        _ctx(pmv, _NoDevice()).batch_open(2, [(640, 200), (np.int32(1241), np.int64(376))])
    with pytest.raises(AssertionError, match="pmv_batch_frame_upload"):
        _ctx(pmv, _NoDevice()).batch_frame_upload(0, np.zeros((48, 64), np.uint8))
    lib = _Recorder()
    _ctx(pmv, lib).batch_open(3, [(640, 200), (333, 121)])
    name, args = lib.calls[0]
    assert name == "pmv_batch_open" and args[1] == 3 and args[3] == 2
    assert [args[2][i] for i in range(4)] == [640, 200, 333, 121]


@pytest.mark.parametrize("fmt", ["gray", "bgr"])
def test_a_strided_view_is_passed_in_place_with_its_own_stride(pmv, fmt):
    """an ROI view at column 3, row 2 of an image 7 pixels wider: the library receives the view's own address and the big image's row
    stride - the view is not copied tight; the same for an object with data_ptr(), shape and stride()"""
    h, w, W = 40, 50, 57
    ch = 3 if fmt == "bgr" else 1
    big = np.zeros((h + 4, W) + ((3,) if ch == 3 else ()), np.uint8)
    view = big[2:2 + h, 3:3 + w]
    assert not view.flags["C_CONTIGUOUS"]
    for frame in (view, _Tensor(view)):
        lib = _Recorder()
        _ctx(pmv, lib).batch_frame_upload(5, frame, fmt)
        (name, args), = lib.calls
        assert name == "pmv_batch_frame_upload"
        _, slot, ptr, aw, ah, stride, f = args
        assert isinstance(ptr, C.c_void_p) and ptr.value == big.ctypes.data + 2 * W * ch + 3 * ch
        assert (slot, aw, ah, stride, f) == (5, w, h, W * ch, pmv.FRAME_FORMATS[fmt])
    # a tight array: its own address, stride = the row's bytes
    tight = np.ascontiguousarray(view)
    lib = _Recorder()
    _ctx(pmv, lib).batch_frame_upload(0, tight, fmt)
    assert lib.calls[0][1][2].value == tight.ctypes.data and lib.calls[0][1][5] == w * ch


def test_the_session_calls_are_declared_exported_and_bound(pmv):
    names = ["pmv_batch_open", "pmv_batch_close", "pmv_batch_frame_upload", "pmv_batch_upload_stats", "pmv_batch_upload_rounds", "pmv_batch_lk_track", "pmv_batch_knn_match",
             "pmv_batch_detect_gftt", "pmv_batch_detect_shitomasi", "pmv_batch_detect_fast", "pmv_batch_pnp_ransac", "pmv_batch_ba_solve",
             "pmv_batch_triangulate_candidates", "pmv_batch_fivepoint_hypotheses"]
    lib = pmv.load_library()
    for n in names:
        assert n in pmv.ABI_SYMBOLS and hasattr(lib, n), n
        assert callable(getattr(pmv.Context, n[len("pmv_"):])), n
    assert callable(pmv.Context.batch_session)


# the calls that exist as X and batch_X; the back-end ones take the sequence first
FRONT_END_PAIRS = ["detect_gftt", "detect_gftt_ex", "corner_subpix", "detect_shitomasi", "detect_fast", "knn_match", "lk_track", "lk_track_ex", "lk_track_fb"]
BACK_END_PAIRS = ["pnp_ransac", "ba_solve", "triangulate_candidates", "fivepoint_hypotheses", "find_essential_mat", "find_fundamental_mat", "recover_pose"]
SIGNATURE_EXCEPTIONS = {}   # name -> why batch_X may differ from X (none does)


def test_every_session_method_has_the_signature_of_its_single_method(pmv):
    """batch_X takes X's arguments under X's names with X's defaults; a back-end call takes `seq` in front of them"""
    import inspect
    for name in FRONT_END_PAIRS + BACK_END_PAIRS:
        if name in SIGNATURE_EXCEPTIONS:
            continue
        single = inspect.signature(getattr(pmv.Context, name))
        params = list(single.parameters.values())
        if name in BACK_END_PAIRS:
            params.insert(1, inspect.Parameter("seq", inspect.Parameter.POSITIONAL_OR_KEYWORD))   # (behind self)
        assert inspect.signature(getattr(pmv.Context, "batch_" + name)) == single.replace(parameters=params), name


def _doc_before(src, decl):
    """the comment block that precedes a declaration, flattened"""
    end = src.index(decl)
    start = src.rindex("/*", 0, end)
    return " ".join(src[start:end].replace("*", " ").split())


def test_the_header_states_the_rules_at_the_calls_they_apply_to():
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    # single-sequence contracts: the session calls have the arguments of the calls they mirror (`seq` after the context for the back-end)
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())

    def args(name):
        a = re.search(r"\b%s\((.*?)\);" % name, flat).group(1)
        return [" ".join(x.split()) for x in a.split(",")]
    for name in ("lk_track", "knn_match", "detect_gftt", "detect_shitomasi", "detect_fast"):
        assert args("pmv_batch_" + name) == args("pmv_" + name), name
    for name in ("pnp_ransac", "ba_solve", "triangulate_candidates", "fivepoint_hypotheses"):
        a = args("pmv_" + name)
        assert args("pmv_batch_" + name) == a[:1] + ["int seq"] + a[1:], name
    opened = _doc_before(src, "int pmv_batch_open(")
    for rule in ("n_seq (1..256", "n_sizes (1..256) distinct (w, h) pairs", "40x40 .. max_w x max_h", "geometry table",
                 # ownership of the context
                 "pmv_pipeline_run_batch, pmv_pipeline_run_batch_streamed and a second pmv_batch_open return PMV_ERR_INVALID",
                 "pmv_batch_open during one of those runs returns PMV_ERR_INVALID",
                 "PMV_ERR_INVALID while session calls are still outstanding",
                 "without an open session is PMV_ERR_INVALID",
                 "single-sequence pmv_ calls stay legal on slots that no session call is using",
                 "pmv_set_frame_format is unaffected",
                 # threads
                 "may be made from any thread at any time", "Error text is per thread", "pmv_thread_error()", "by any number of threads", "one outstanding call per seq and call",
                 "seq outside 0 .. n_seq - 1 is PMV_ERR_INVALID",
                 # results
                 "exactly the bits the single-sequence pmv_ call of the same name returns for the same inputs",
                 "PMV_ERR_DEGENERATE", "PMV_ERR_OVERFLOW", "current pmv_set_ba_mode", "ordering hint", "changes no result",
                 # slots
                 "Slots are the caller's to manage", "must not be uploaded into while a call that reads it is outstanding", "frames k - 1 and k are live",
                 "does not police it"):
        assert rule in opened, rule
    upload = _doc_before(src, "int pmv_batch_frame_upload(")
    for rule in ("`stride` bytes per source row", "any number of threads", "pageable host memory, pinned mapped host memory, or device memory of the context's device",
                 "read IN PLACE", "nothing past the last row's last byte is read", "copied by the calling thread, row by row",
                 "Device memory of another device is PMV_ERR_INVALID", "must have COMPLETED before the call",
                 "the source may be reused and the slot is built", "needs no further ordering", "completion word",
                 "not declared at pmv_batch_open is PMV_ERR_INVALID", "names the size", "stride below w (gray) or 3 w (BGR) is PMV_ERR_CAPACITY",
                 "at most one gray and one BGR level-0 launch and one k_pyrdown launch per level"):
        assert rule in upload, rule
    front = _doc_before(src, "int pmv_batch_lk_track(")
    assert "argument for argument" in front and "combiner" in front
    back = _doc_before(src, "int pmv_batch_pnp_ransac(")
    assert "0 .. n_seq - 1, else PMV_ERR_INVALID" in back and "one outstanding call per seq and call" in back and "pmv_set_ba_mode" in back
    stats = _doc_before(src, "int pmv_batch_upload_stats(")
    assert "{upload rounds, frames uploaded, level-0 launches, pyrDown launches} since pmv_batch_open" in stats
