"""pmv_find_fundamental_mat, its session form and its two diagnostic calls without a GPU: the names are declared, exported and bound with
the documented signatures; the header states the call's rules; pmv_debug_fundamental_iters_table gives the twin's table; the Context methods
marshal their arguments to the right C calls."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fundamental_common as fc
from test_batch_session_api import _Recorder, _ctx, _doc_before

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pmv_find_fundamental_mat", "pmv_batch_find_fundamental_mat", "pmv_debug_fundamental_iters_table", "pmv_debug_set_fundamental_r",
         "pmv_debug_fundamental_r", "pmv_debug_whole_rounds"]


def test_the_names_are_declared_exported_and_bound(pmv):
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    lib = pmv.load_library()
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, src), n
        assert n in pmv.ABI_SYMBOLS and hasattr(lib, n), n
    for m in ("find_fundamental_mat", "batch_find_fundamental_mat"):
        assert callable(getattr(pmv.Context, m)), m


def test_the_signatures_are_the_documented_ones():
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())

    def args(name):
        a = re.search(r"\b%s\((.*?)\);" % name, flat).group(1)
        return [" ".join(x.split()) for x in a.split(",")]
    a = args("pmv_find_fundamental_mat")
    assert a == ["pmv_ctx* ctx", "const float* p1_xy", "const float* p2_xy", "int n", "double threshold", "double confidence", "double* F9", "uint8_t* mask",
                 "int* out_found", "int* out_samples_drawn"]
    assert args("pmv_batch_find_fundamental_mat") == a[:1] + ["int seq"] + a[1:]
    assert args("pmv_debug_fundamental_iters_table") == ["int n", "double confidence", "double* out_denoms", "double* out_num"]
    assert src.index("int pmv_find_essential_mat(") < src.index("int pmv_find_fundamental_mat(") < src.index("int pmv_batch_open(")


def test_the_header_states_the_calls_rules():
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    find = _doc_before(src, "int pmv_find_fundamental_mat(")
    for rule in ("[mem: OpenCV 3.4 fundam.cpp, ptsetreg.cpp; parity with a real OpenCV unpinned like the rest - tests/twin/fundamental_twin.cpp is the CPU restatement that fixes the bits]",
                 "n pixel positions (x, y) as float32", "F9 row-major", "mask n bytes", "out_found 0 = no model (cv returns an empty Mat): F9 untouched, mask all 0",
                 "n < 15 is PMV_ERR_DEGENERATE", "LMedS", "n > max_tracks: PMV_ERR_CAPACITY", "cv::RNG((uint64)-1)", "rng % n", "only the LAST point",
                 "FLT_EPSILON", "10000", "no normalisation", "[x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1]", "Gauss-Jordan with complete pivoting",
                 "acos, cos and pow", "HOW MANY roots", "smallest, largest, middle", "fabs(s) > DBL_EPSILON", "max(maxGood, 6)",
                 "RANSACUpdateNumIters(confidence, (n - count) / n, 7, niters)", "No refit on the inliers", "cv silently substitutes 3 and 0.99",
                 "the message names the point", "nothing is written and nothing is clamped", "Not logged by pmv_record_enable", "ONE launch"):
        assert rule in find, rule
    batch = _doc_before(src, "int pmv_batch_find_fundamental_mat(")
    for rule in ("0 .. n_seq - 1, else PMV_ERR_INVALID", "ONE k_fundamental_ransac launch", "returns as soon as ITS request is complete", "One outstanding call per seq and call",
                 "the bits of the single call"):
        assert rule in batch, rule


@pytest.mark.parametrize("n", [15, 64, 300, 1024])
def test_the_debug_table_is_the_twins(pmv, n):
    lib = pmv.load_library()
    _f64p = C.POINTER(C.c_double)
    lib.pmv_debug_fundamental_iters_table.argtypes = [C.c_int, C.c_double, _f64p, _f64p]
    for conf in (0.99, 0.5):
        den, num = np.full(n + 1, np.nan), C.c_double()
        assert lib.pmv_debug_fundamental_iters_table(n, conf, den.ctypes.data_as(_f64p), C.byref(num)) == 0
        wden, wnum = fc.twin().iters_table(n, conf)
        assert num.value == wnum and np.array_equal(den.view(np.uint64), wden.view(np.uint64))
        # ... and the essential call's table kept its meaning: 5 model points
        lib.pmv_debug_essential_iters_table.argtypes = [C.c_int, C.c_double, _f64p, _f64p]
        assert lib.pmv_debug_essential_iters_table(n, conf, den.ctypes.data_as(_f64p), C.byref(num)) == 0
        assert np.array_equal(den.view(np.uint64), fc.twin().iters_table(n, conf, 5)[0].view(np.uint64))
    assert lib.pmv_debug_fundamental_iters_table(-1, 0.99, den.ctypes.data_as(_f64p), C.byref(num)) == -2
    assert lib.pmv_debug_fundamental_iters_table(n, 0.99, None, C.byref(num)) == -2
    assert lib.pmv_debug_set_fundamental_r(65) == -2 and lib.pmv_debug_set_fundamental_r(-1) == -2 and lib.pmv_debug_set_fundamental_r(0) == 0


@pytest.mark.parametrize("env,want", [(None, 64), ("16", 16), ("1", 1), ("0", 1), ("999", 64)])
def test_the_environment_sets_the_round_width(env, want):
    """PMV_FUNDAMENTAL_R is read once, when the library first needs the width: a fresh process per value. The setter overrides it, 0 gives it back."""
    code = ("import importlib, sys; sys.path.insert(0, %r); lib = importlib.import_module('practical-multi-view_amd').load_library(); "
            "a = lib.pmv_debug_fundamental_r(); lib.pmv_debug_set_fundamental_r(8); b = lib.pmv_debug_fundamental_r(); "
            "lib.pmv_debug_set_fundamental_r(0); print(a, b, lib.pmv_debug_fundamental_r())" % ROOT)
    e = {k: v for k, v in os.environ.items() if k != "PMV_FUNDAMENTAL_R"}
    if env is not None:
        e["PMV_FUNDAMENTAL_R"] = env
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out[-3:]] == [want, 8, want]


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
            found, F, mask, drawn = ctx.find_fundamental_mat(p1, p2, threshold=2.5, confidence=0.9)
        else:
            found, F, mask, drawn = ctx.batch_find_fundamental_mat(seq, p1, p2, threshold=2.5, confidence=0.9)
        (name, a), = lib.calls
        assert name == ("pmv_find_fundamental_mat" if seq is None else "pmv_batch_find_fundamental_mat") and len(a) == head + 9
        assert seq is None or a[1] == seq
        a = a[head:]
        assert isinstance(a[0], C.POINTER(C.c_float)) and isinstance(a[1], C.POINTER(C.c_float))
        assert np.array_equal(np.ctypeslib.as_array(a[0], (n, 2)), p1.astype(np.float32)) and np.array_equal(np.ctypeslib.as_array(a[1], (n, 2)), p2.astype(np.float32))
        assert a[2] == n
        assert isinstance(a[3], C.c_double) and a[3].value == 2.5 and isinstance(a[4], C.c_double) and a[4].value == 0.9
        assert _addr(a[5]) == F.ctypes.data and F.shape == (3, 3) and _addr(a[6]) == mask.ctypes.data and mask.shape == (n,) and mask.dtype == np.uint8
        assert found is False and drawn == 0
    with pytest.raises(ValueError):
        _ctx(pmv, _Recorder()).find_fundamental_mat(p1, p2[:-1])
    # the defaults are cv's: threshold 1 px... (cv's own default is 3; the KLT loops this serves pass 1.0), confidence 0.99
    lib = _Recorder()
    _ctx(pmv, lib).find_fundamental_mat(p1, p2)
    assert lib.calls[0][1][4].value == 1.0 and lib.calls[0][1][5].value == 0.99
