"""pmv_find_homography, its session form and its diagnostic calls without a GPU: the names are declared, exported and bound with the
documented signatures; the header states the call's rules; every argument error has its code and message and writes nothing
(pmv_debug_homography_check: the call's own check without a context); pmv_debug_homography_iters_table gives the twin's table; the Context
methods marshal their arguments to the right C calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import homography_common as hc
from test_batch_session_api import _Recorder, _ctx, _doc_before

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pmv_find_homography", "pmv_batch_find_homography", "pmv_debug_homography_iters_table", "pmv_debug_homography_check", "pmv_debug_homography_launches"]
INVALID, CAPACITY, DEGENERATE = -2, -3, -5
_f32p, _f64p, _u8p, _ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int)


def test_the_names_are_declared_exported_and_bound(pmv):
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    lib = pmv.load_library()
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, src), n
        assert n in pmv.ABI_SYMBOLS and hasattr(lib, n), n
    for m in ("find_homography", "batch_find_homography"):
        assert callable(getattr(pmv.Context, m)), m


def test_the_signatures_are_the_documented_ones():
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())

    def args(name):
        a = re.search(r"\b%s\((.*?)\);" % name, flat).group(1)
        return [" ".join(x.split()) for x in a.split(",")]
    a = args("pmv_find_homography")
    assert a == ["pmv_ctx* ctx", "const float* p1_xy", "const float* p2_xy", "int n", "double threshold", "double confidence", "int max_iters", "double* H9",
                 "uint8_t* mask", "int* out_found", "int* out_samples_drawn"]
    assert args("pmv_batch_find_homography") == a[:1] + ["int seq"] + a[1:]
    assert args("pmv_debug_homography_iters_table") == ["int n", "double confidence", "double* out_denoms", "double* out_num"]
    assert args("pmv_debug_homography_launches") == ["pmv_ctx* ctx", "long long* out2"]
    assert src.index("int pmv_find_fundamental_mat(") < src.index("int pmv_find_homography(") < src.index("int pmv_batch_open(")


def test_the_header_states_the_calls_rules():
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    find = _doc_before(src, "int pmv_find_homography(")
    for rule in ("[mem: OpenCV 3.4 fundam.cpp, ptsetreg.cpp, lmsolver.cpp; parity with a real OpenCV unpinned like the rest - tests/twin/homography_twin.cpp is the CPU restatement that fixes the bits]",
                 "n pixel positions (x, y) as float32", "H9 row-major, maps image 1 to image 2", "mask n bytes", "out_found 0 = no model (cv returns an empty Mat): H9 untouched, mask all 0",
                 "n == 4: one runKernel", "n < 4 is PMV_ERR_DEGENERATE", "n > max_tracks: PMV_ERR_CAPACITY", "cv::RNG((uint64)-1)", "rng % n", "only the LAST point",
                 "10000 attempts", "{0,1,2}, {0,1,3}, {0,2,3}, {1,2,3}", "< DBL_EPSILON", "Gauss-Jordan with complete pivoting", "H[8] == 0",
                 "float32 throughout", "max(maxGood, 3)", "RANSACUpdateNumIters(confidence, (n - count) / n, 4, niters)", "starting from max_iters",
                 "the mask is the RANSAC model's", "JacobiImpl_", "sqrt(1 + (b / a)^2)", "at most 10 iterations", "Rlo 0.25, Rhi 0.75", "DECOMP_EIG", "FLT_EPSILON",
                 "i mod 64", "xor butterfly 32, 16, .. 1", "max_iters outside 1..10000", "the message names the point", "nothing is written and nothing is clamped",
                 "Not logged by pmv_record_enable", "ONE launch"):
        assert rule in find, rule
    batch = _doc_before(src, "int pmv_batch_find_homography(")
    for rule in ("0 .. n_seq - 1, else PMV_ERR_INVALID", "ONE k_homography_ransac launch", "returns as soon as ITS request is complete", "the bits of the single call",
                 "pmv_debug_homography_launches"):
        assert rule in batch, rule


def test_every_argument_error_has_its_code_and_message_and_writes_nothing(pmv):
    lib = pmv.load_library()
    max_tracks, n = 128, 20
    p1, p2 = (np.ascontiguousarray(p[:n]) for p in hc.points("plane", 2, 64, 0.3))
    big = np.zeros((max_tracks + 1, 2), np.float32)

    def bad(i, j, v):
        q = p1.copy()
        q[i, j] = v
        return q

    def check(p1=p1, p2=p2, n=n, thr=3.0, conf=0.995, max_iters=2000, null=None):
        H, mask = np.full(9, 7.0), np.full(max(n, 1), 9, np.uint8)
        found, drawn = C.c_int(-5), C.c_int(-6)
        msg = C.create_string_buffer(256)
        a = [max_tracks, p1.ctypes.data_as(_f32p), p2.ctypes.data_as(_f32p), n, C.c_double(thr), C.c_double(conf), max_iters, H.ctypes.data_as(_f64p),
             mask.ctypes.data_as(_u8p), C.byref(found), C.byref(drawn), msg]
        if null is not None:
            a[null] = None
        rc = lib.pmv_debug_homography_check(*a)
        untouched = (H == 7.0).all() and (mask == 9).all() and found.value == -5 and drawn.value == -6
        return rc, bool(untouched), msg.value.decode()
    nan, inf = float("nan"), float("inf")
    rows = [(dict(null=i), INVALID, "null argument") for i in (1, 2, 7, 8, 9, 10)] + \
           [(dict(thr=t), INVALID, "threshold") for t in (0.0, -1.0, inf, nan)] + \
           [(dict(conf=c), INVALID, "confidence") for c in (0.0, 1.0, -0.1, 1.01, nan, inf)] + \
           [(dict(max_iters=m), INVALID, "max_iters = %d outside 1..10000" % m) for m in (0, -1, 10001)] + \
           [(dict(p1=bad(3, 1, nan)), INVALID, "point 3 of image 1"), (dict(p2=bad(19, 0, inf)), INVALID, "point 19 of image 2"),
            (dict(p1=bad(0, 0, 1.5e6)), INVALID, "point 0 of image 1"), (dict(p2=bad(7, 1, -1.5e6)), INVALID, "point 7 of image 2"),
            (dict(n=-1), CAPACITY, "max_tracks=128"), (dict(p1=big, p2=big, n=max_tracks + 1), CAPACITY, "max_tracks=128"),
            (dict(n=3), DEGENERATE, "3 correspondences"), (dict(n=0), DEGENERATE, "cv asserts")]
    for kw, code, needle in rows:
        rc, untouched, msg = check(**kw)
        assert (rc, untouched) == (code, True) and needle in msg and msg.startswith("pmv_find_homography: "), (kw, rc, msg)
    for kw in (dict(), dict(n=4), dict(max_iters=1), dict(max_iters=10000), dict(p1=big[:max_tracks], p2=big[:max_tracks], n=max_tracks)):
        assert check(**kw) == (0, True, ""), kw
    # the calls themselves refuse a null context before anything else
    assert lib.pmv_find_homography(None, None, None, 0, C.c_double(3.0), C.c_double(0.995), 2000, None, None, None, None) == INVALID
    assert lib.pmv_debug_homography_launches(None, None) == INVALID


@pytest.mark.parametrize("n", [4, 64, 300, 1024])
def test_the_debug_table_is_the_twins(pmv, n):
    lib = pmv.load_library()
    lib.pmv_debug_homography_iters_table.argtypes = [C.c_int, C.c_double, _f64p, _f64p]
    for conf in (0.995, 0.5):
        den, num = np.full(n + 1, np.nan), C.c_double()
        assert lib.pmv_debug_homography_iters_table(n, conf, den.ctypes.data_as(_f64p), C.byref(num)) == 0
        wden, wnum = hc.twin().iters_table(n, conf)
        assert num.value == wnum and np.array_equal(den.view(np.uint64), wden.view(np.uint64))
    assert lib.pmv_debug_homography_iters_table(-1, 0.99, den.ctypes.data_as(_f64p), C.byref(num)) == INVALID
    assert lib.pmv_debug_homography_iters_table(n, 0.99, None, C.byref(num)) == INVALID


def _addr(p):
    return C.cast(p, C.c_void_p).value


def test_the_context_methods_marshal_their_arguments_to_the_right_calls(pmv):
    n = 17
    rng = np.random.default_rng(3)
    p1, p2 = rng.uniform(0, 300, (n, 2)), rng.uniform(0, 300, (n, 2))   # float64 going in: converted to float32 as cv converts to CV_32F
    for seq in (None, 3):
        lib = _Recorder()
        ctx = _ctx(pmv, lib)
        head = 1 if seq is None else 2
        if seq is None:
            found, H, mask, drawn = ctx.find_homography(p1, p2, threshold=2.5, confidence=0.9, max_iters=77)
        else:
            found, H, mask, drawn = ctx.batch_find_homography(seq, p1, p2, threshold=2.5, confidence=0.9, max_iters=77)
        (name, a), = lib.calls
        assert name == ("pmv_find_homography" if seq is None else "pmv_batch_find_homography") and len(a) == head + 10
        assert seq is None or a[1] == seq
        a = a[head:]
        assert isinstance(a[0], _f32p) and isinstance(a[1], _f32p)
        assert np.array_equal(np.ctypeslib.as_array(a[0], (n, 2)), p1.astype(np.float32)) and np.array_equal(np.ctypeslib.as_array(a[1], (n, 2)), p2.astype(np.float32))
        assert a[2] == n
        assert isinstance(a[3], C.c_double) and a[3].value == 2.5 and isinstance(a[4], C.c_double) and a[4].value == 0.9 and a[5] == 77
        assert _addr(a[6]) == H.ctypes.data and H.shape == (3, 3) and _addr(a[7]) == mask.ctypes.data and mask.shape == (n,) and mask.dtype == np.uint8
        assert found is False and drawn == 0
    with pytest.raises(ValueError):
        _ctx(pmv, _Recorder()).find_homography(p1, p2[:-1])
    lib = _Recorder()   # the defaults are cv's: 3 px, 2000 iterations, confidence 0.995
    _ctx(pmv, lib).find_homography(p1, p2)
    assert lib.calls[0][1][4].value == 3.0 and lib.calls[0][1][5].value == 0.995 and lib.calls[0][1][6] == 2000
