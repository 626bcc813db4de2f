"""The triangulator's two whole calls (pmv_find_essential_mat, pmv_recover_pose and their session forms) without a GPU: the names are declared,
exported and bound; the session forms have the single forms' arguments behind `seq`; the header states each call's rules; the host / device
split of RANSACUpdateNumIters reproduces the host function exactly; the Context methods marshal their arguments to the right C calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_batch_session_api import _Recorder, _ctx, _doc_before

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pmv_find_essential_mat", "pmv_recover_pose", "pmv_batch_find_essential_mat", "pmv_batch_recover_pose", "pmv_debug_essential_iters_table"]


def test_the_five_names_are_declared_exported_and_bound(pmv):
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    lib = pmv.load_library()
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, src), n
        assert n in pmv.ABI_SYMBOLS and hasattr(lib, n), n
    for m in ("find_essential_mat", "recover_pose", "batch_find_essential_mat", "batch_recover_pose"):
        assert callable(getattr(pmv.Context, m)), m


def test_the_session_forms_have_the_single_forms_arguments_behind_seq():
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())

    def args(name):
        a = re.search(r"\b%s\((.*?)\);" % name, flat).group(1)
        return [" ".join(x.split()) for x in a.split(",")]
    for name in ("find_essential_mat", "recover_pose"):
        a = args("pmv_" + name)
        assert args("pmv_batch_" + name) == a[:1] + ["int seq"] + a[1:], name
    assert args("pmv_find_essential_mat") == ["pmv_ctx* ctx", "const double* p1_xy", "const double* p2_xy", "int n", "const double* K", "double prob",
                                              "double threshold", "double* E9", "uint8_t* mask", "int* out_found", "int* out_samples_drawn"]
    assert args("pmv_recover_pose") == ["pmv_ctx* ctx", "const double* E9", "const double* p1_xy", "const double* p2_xy", "int n", "const double* K",
                                        "double* R9", "double* t3", "uint8_t* mask", "double* tri4n", "int* out_good"]


def test_the_header_states_each_calls_rules():
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    find = _doc_before(src, "int pmv_find_essential_mat(")
    for rule in ("OpenCVFivePointTri.cpp:24", "n pixel coordinates (x, y) as doubles", "E9 row-major", "mask n bytes",
                 "out_found 0 = no model (cv returns an empty Mat): E9 untouched, mask all 0",
                 "0 <= n <= max_tracks, else PMV_ERR_CAPACITY", "n < 5: no model", "n == 5: one solve without RANSAC", "mask all 1, 0 samples drawn",
                 "Null pointers, prob outside [0, 1], a non-positive or non-finite threshold: PMV_ERR_INVALID", "On an error no output is written",
                 "ONE launch", "Not logged by pmv_record_enable"):
        assert rule in find, rule
    pose = _doc_before(src, "int pmv_recover_pose(")
    for rule in ("OpenCVFivePointTri.cpp:27", "mask is in/out", "4 x n homogeneous", "the winning candidate's count", "0 <= n <= max_tracks, else PMV_ERR_CAPACITY",
                 "null pointers: PMV_ERR_INVALID", "DLT record"):
        assert rule in pose, rule
    batch = _doc_before(src, "int pmv_batch_find_essential_mat(")
    for rule in ("0 .. n_seq - 1, else PMV_ERR_INVALID", "the no-model convention", "0 <= n <= max_tracks else PMV_ERR_CAPACITY", "mask in/out",
                 "returns as soon as ITS request is complete", "One outstanding call per seq and call", "released the seq's request record"):
        assert rule in batch, rule
    table = _doc_before(src, "int pmv_debug_essential_iters_table(")
    for rule in ("n + 1 doubles", "log(1 - prob)", "-infinity", "denom >= 0 || -num >= maxIters", "(-denom) ? maxIters : lrint(num / denom)"):   # (_doc_before drops the `*`)
        assert rule in table, rule
    params = src[src.index("typedef struct pmv_pipeline_params"):src.index("} pmv_pipeline_params;")]
    assert "2 = the whole RANSAC of a call in one launch (pmv_find_essential_mat)" in " ".join(params.replace("*", " ").split())


@pytest.mark.parametrize("n", [5, 6, 64, 300, 1024])
def test_the_iteration_table_and_the_kernels_final_expression_equal_the_host_function(pmv, orc, n):
    """what the kernel does with the table - IEEE multiply, divide, compare, round half to even - in numpy float64, for every inlier count
    and four iteration caps, against RANSACUpdateNumIters as the host code calls it"""
    lib = pmv.load_library()
    prob = 0.99
    denoms = np.full(n + 1, np.nan)
    num = C.c_double()
    lib.pmv_debug_essential_iters_table.argtypes = [C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    assert lib.pmv_debug_essential_iters_table(n, prob, denoms.ctypes.data_as(C.POINTER(C.c_double)), C.byref(num)) == 0
    assert not np.isnan(denoms).any() and denoms[n] == -np.inf and num.value == np.log(1 - prob)
    orc.lib.orc_host_update_num_iters.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int]
    orc.lib.orc_host_update_num_iters.restype = C.c_int
    nm = np.float64(num.value)
    for max_iters in (1000, 500, 37, 1):
        with np.errstate(all="ignore"):
            keep = (denoms >= 0) | (-nm >= np.float64(max_iters) * (-denoms))
            got = np.where(keep, max_iters, np.rint(nm / denoms)).astype(np.int64)
        want = [orc.lib.orc_host_update_num_iters(prob, (n - g) / n, 5, max_iters) for g in range(n + 1)]
        assert got.tolist() == want, max_iters
    assert lib.pmv_debug_essential_iters_table(-1, prob, denoms.ctypes.data_as(C.POINTER(C.c_double)), C.byref(num)) == -2
    assert lib.pmv_debug_essential_iters_table(n, prob, None, C.byref(num)) == -2


def _addr(p):
    return C.cast(p, C.c_void_p).value


def test_the_context_methods_marshal_their_arguments_to_the_right_calls(pmv):
    n = 7
    rng = np.random.default_rng(3)
    p1, p2 = rng.uniform(0, 300, (n, 2)), rng.uniform(0, 300, (n, 2))
    K = np.array([[700.0, 0, 600], [0, 710, 180], [0, 0, 1]])
    for seq in (None, 3):
        lib = _Recorder()
        ctx = _ctx(pmv, lib)
        head = 1 if seq is None else 2
        if seq is None:
            found, E, mask, drawn = ctx.find_essential_mat(p1, p2, K, prob=0.9, threshold=2.5)
        else:
            found, E, mask, drawn = ctx.batch_find_essential_mat(seq, p1, p2, K, prob=0.9, threshold=2.5)
        (name, a), = lib.calls
        assert name == ("pmv_find_essential_mat" if seq is None else "pmv_batch_find_essential_mat") and len(a) == head + 10
        assert seq is None or a[1] == seq
        a = a[head:]
        assert np.array_equal(np.ctypeslib.as_array(a[0], (n, 2)), p1) and np.array_equal(np.ctypeslib.as_array(a[1], (n, 2)), p2)
        assert a[2] == n and np.array_equal(np.ctypeslib.as_array(a[3], (9,)), K.reshape(9))
        assert isinstance(a[4], C.c_double) and a[4].value == 0.9 and isinstance(a[5], C.c_double) and a[5].value == 2.5
        assert _addr(a[6]) == E.ctypes.data and E.shape == (3, 3) and _addr(a[7]) == mask.ctypes.data and mask.shape == (n,) and mask.dtype == np.uint8
        assert found is False and drawn == 0
        # recover_pose: E, the points, K, then the outputs; the caller's mask is copied, not written
        lib = _Recorder()
        ctx = _ctx(pmv, lib)
        Ein = rng.normal(size=(3, 3))
        m_in = np.array([1, 0, 1, 1, 0, 1, 1], np.uint8)
        keep = m_in.copy()
        if seq is None:
            R, t, m, tri, good = ctx.recover_pose(Ein, p1, p2, K, m_in)
        else:
            R, t, m, tri, good = ctx.batch_recover_pose(seq, Ein, p1, p2, K, m_in)
        (name, a), = lib.calls
        assert name == ("pmv_recover_pose" if seq is None else "pmv_batch_recover_pose") and len(a) == head + 10
        assert seq is None or a[1] == seq
        a = a[head:]
        assert np.array_equal(np.ctypeslib.as_array(a[0], (9,)), Ein.reshape(9))
        assert np.array_equal(np.ctypeslib.as_array(a[1], (n, 2)), p1) and np.array_equal(np.ctypeslib.as_array(a[2], (n, 2)), p2) and a[3] == n
        assert np.array_equal(np.ctypeslib.as_array(a[4], (9,)), K.reshape(9))
        assert _addr(a[5]) == R.ctypes.data and _addr(a[6]) == t.ctypes.data and _addr(a[7]) == m.ctypes.data and _addr(a[8]) == tri.ctypes.data
        assert m.ctypes.data != m_in.ctypes.data and np.array_equal(m, keep) and np.array_equal(m_in, keep)
        assert R.shape == (3, 3) and t.shape == (3,) and tri.shape == (4, n) and good == 0
    with pytest.raises(ValueError):
        _ctx(pmv, _Recorder()).find_essential_mat(p1, p2[:-1], K)
