"""pmv_triangulate_tracks, its session form and its diagnostic calls without a GPU: the names are declared, exported and bound with the
documented signatures; the header states the call's rules; every argument error has its code and message and writes nothing
(pmv_debug_tri_tracks_check: the call's own check without a context); the Context methods marshal their arguments to the right C calls;
projections_from_ba_cams gives the matrices of pmv_ba_solve's camera form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc_binding
import tri_tracks_common as tc
from test_batch_session_api import _Recorder, _ctx, _doc_before

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pmv_triangulate_tracks", "pmv_batch_triangulate_tracks", "pmv_debug_tri_tracks_check", "pmv_debug_tri_tracks_launches"]
INVALID, CAPACITY = -2, -3
_f64p, _u8p, _ip = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int)


def test_the_names_are_declared_exported_and_bound(pmv):
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    lib = pmv.load_library()
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, src), n
        assert n in pmv.ABI_SYMBOLS and hasattr(lib, n), n
    for m in ("triangulate_tracks", "batch_triangulate_tracks", "tri_tracks_launches"):
        assert callable(getattr(pmv.Context, m)), m
    assert callable(pmv.projections_from_ba_cams)
    assert (pmv.TRI_OK, pmv.TRI_FEW_VIEWS, pmv.TRI_DEGENERATE, pmv.TRI_DEPTH, pmv.TRI_REPROJ, pmv.TRI_PARALLAX) == (0, 1, 2, 4, 8, 16)
    assert re.search(r"enum \{ PMV_TRI_OK = 0, PMV_TRI_FEW_VIEWS = 1, PMV_TRI_DEGENERATE = 2, PMV_TRI_DEPTH = 4, PMV_TRI_REPROJ = 8, PMV_TRI_PARALLAX = 16 \};", src)
    p = pmv.TriParams()   # the defaults are the call's
    assert (p.min_views, p.refine_iters, p.min_depth, p.max_depth, p.max_reproj, p.min_parallax_deg) == (2, 0, 0.1, np.inf, np.inf, 0.0)
    assert C.sizeof(pmv.TriParams) == 40


def test_the_signatures_are_the_documented_ones():
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())

    def args(name):
        a = re.search(r"\b%s\((.*?)\);" % name, flat).group(1)
        return [" ".join(x.split()) for x in a.split(",")]
    a = args("pmv_triangulate_tracks")
    assert a == ["pmv_ctx* ctx", "const double* P3x4", "int nc", "const double* obs_xy", "const int* cam_idx", "const int* pt_idx", "int n_obs", "int np",
                 "const pmv_tri_params* p_or_null", "double* out_xyz", "uint8_t* out_status", "double* out_err_or_null", "int* out_good"]
    assert args("pmv_batch_triangulate_tracks") == a[:1] + ["int seq"] + a[1:]
    assert args("pmv_debug_tri_tracks_check") == ["int max_cams", "int max_points", "int max_obs"] + [("const " + x) if x.startswith(("double*", "uint8_t*", "int*")) else x
                                                                                                      for x in a[1:]] + ["char* err256"]
    assert args("pmv_debug_tri_tracks_launches") == ["pmv_ctx* ctx", "long long* out2"]
    assert a[3:7] == args("pmv_ba_solve")[5:9]   # the caller hands the same arrays to both calls
    assert src.index("int pmv_triangulate_candidates_ahead(") < src.index("int pmv_triangulate_tracks(") < src.index("int pmv_find_essential_mat(")
    fields = re.search(r"typedef struct pmv_tri_params \{(.*?)\} pmv_tri_params;", flat).group(1)
    assert [" ".join(f.split()) for f in fields.split(";") if f.strip()] == ["int min_views", "int refine_iters", "double min_depth, max_depth", "double max_reproj",
                                                                           "double min_parallax_deg"]


def test_the_header_states_the_calls_rules():
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    doc = _doc_before(src, "enum { PMV_TRI_OK")
    for rule in ("exactly the arrays of pmv_ba_solve", "its third row must give the depth", "projections_from_ba_cams", "[R|t] for normalised observations", "K[R|t] for pixels",
                 "tests/twin/tri_tracks_twin.cpp", "nc <= max_ba_cams, np <= max_ba_points, n_obs <= max_ba_obs, else PMV_ERR_CAPACITY",
                 "np == 0 or n_obs == 0 is valid: nothing is launched, every landmark is FEW_VIEWS", "order of appearance", "stable counting sort", "pt_idx need not be sorted",
                 "a camera may occur twice", "x P[8+k] - P[k] and y P[8+k] - P[4+k]", "row by row in list order from 0", "smallest eigenvalue",
                 "a two-observation landmark whose first camera is [I|0] has its bits", "X = Qh[0..2] / Qh[3]", "Qh[3] == 0 or a non-finite X: PMV_TRI_DEGENERATE",
                 "Gauss-Newton", "explicit adjugate over the determinant", "only if the new cost is strictly smaller", "A zero or non-finite determinant or a non-finite cost",
                 "no early exit, status bits OR-ed", "out_xyz = 0 and out_err = +inf", "in every view, else PMV_TRI_DEPTH", "PMV_TRI_REPROJ", "rms reprojection error",
                 "C = -M^-1 p4 by the adjugate", "only if the gate is on", "det M == 0 is then PMV_ERR_INVALID; the message names the camera", "pairs i < j",
                 "cos(min_parallax_deg pi / 180) from the host's libm", "a non-finite cosine counts as no parallax", "never evaluates a transcendental function",
                 "the message names the observation", "min_views < 2", "refine_iters outside 0..20", "min_depth not finite or max_depth < min_depth", "max_reproj <= 0 or NaN",
                 "min_parallax_deg outside [0, 180)", "nothing is written", "Not logged by pmv_record_enable", "ONE launch", "out_good = landmarks with status 0"):
        assert rule in doc, rule
    batch = _doc_before(src, "int pmv_batch_triangulate_tracks(")
    for rule in ("0 .. n_seq - 1, else PMV_ERR_INVALID", "ONE k_tri_tracks_batch launch", "the bits of the single call", "\"dlt\" role of pmv_batch_stats",
                 "pmv_debug_tri_tracks_launches", "DLT combiner"):
        assert rule in batch, rule


def test_every_argument_error_has_its_code_and_message_and_writes_nothing(pmv):
    lib = pmv.load_library()
    caps = (5, 40, 200)
    sc = tc.scene(5, 40, 3, noise_px=0.5, min_v=2)
    assert len(sc["obs"]) <= caps[2]
    nan, inf = float("nan"), float("inf")

    def check(P=sc["P"], nc=5, obs=sc["obs"], cam=sc["cam"], pt=sc["pt"], n_obs=None, n_pts=40, null=None, default_params=False, **kw):
        n_obs = len(obs) if n_obs is None else n_obs
        P, obs = np.ascontiguousarray(P, np.float64), np.ascontiguousarray(obs, np.float64)
        cam, pt = np.ascontiguousarray(cam, np.int32), np.ascontiguousarray(pt, np.int32)
        xyz, st, err = np.full((max(n_pts, 1), 3), 7.0), np.full(max(n_pts, 1), 9, np.uint8), np.full(max(n_pts, 1), 5.0)
        good = C.c_int(-5)
        msg = C.create_string_buffer(256)
        par = pmv.TriParams(**kw)
        a = [*caps, P.ctypes.data_as(_f64p), nc, obs.ctypes.data_as(_f64p), cam.ctypes.data_as(_ip), pt.ctypes.data_as(_ip), n_obs, n_pts,
             None if default_params else C.byref(par), xyz.ctypes.data_as(_f64p), st.ctypes.data_as(_u8p), err.ctypes.data_as(_f64p), C.byref(good), msg]
        if null is not None:
            a[null] = None
        rc = lib.pmv_debug_tri_tracks_check(*a)
        untouched = (xyz == 7.0).all() and (st == 9).all() and (err == 5.0).all() and good.value == -5
        return rc, bool(untouched), msg.value.decode()

    def with_(arr, idx, v):
        a = np.array(arr).copy()
        a[idx] = v
        return a
    sing = sc["P"].copy()
    sing[2, :, :3] = [[1, 2, 3], [2, 4, 6], [0, 0, 1]]
    rows = [(dict(null=i), INVALID, "null argument") for i in (3, 5, 6, 7, 11, 12, 14)] + \
           [(dict(nc=0), INVALID, "nc = 0"), (dict(nc=-1), INVALID, "nc = -1"),
            (dict(cam=with_(sc["cam"], 17, 5)), INVALID, "observation 17"), (dict(cam=with_(sc["cam"], 0, -1)), INVALID, "observation 0"),
            (dict(pt=with_(sc["pt"], 33, 40)), INVALID, "observation 33"), (dict(pt=with_(sc["pt"], 2, -1)), INVALID, "observation 2"),
            (dict(n_pts=39), INVALID, "index out of range at observation"),
            (dict(P=with_(sc["P"], (3, 1, 2), nan)), INVALID, "camera 3 is not finite"), (dict(P=with_(sc["P"], (0, 0, 0), inf)), INVALID, "camera 0 is not finite"),
            (dict(obs=with_(sc["obs"], (21, 1), nan)), INVALID, "observation 21"), (dict(obs=with_(sc["obs"], (4, 0), -inf)), INVALID, "observation 4"),
            (dict(min_views=1), INVALID, "min_views = 1"), (dict(min_views=0), INVALID, "min_views = 0"),
            (dict(refine_iters=-1), INVALID, "refine_iters = -1 outside 0..20"), (dict(refine_iters=21), INVALID, "refine_iters = 21 outside 0..20"),
            (dict(min_depth=nan), INVALID, "min_depth"), (dict(min_depth=-inf), INVALID, "min_depth"), (dict(min_depth=inf), INVALID, "min_depth"),
            (dict(min_depth=1.0, max_depth=0.5), INVALID, "max_depth = 0.5 below min_depth = 1"), (dict(max_depth=nan), INVALID, "max_depth"),
            (dict(max_reproj=0.0), INVALID, "max_reproj"), (dict(max_reproj=-1.0), INVALID, "max_reproj"), (dict(max_reproj=nan), INVALID, "max_reproj"),
            (dict(min_parallax_deg=-0.1), INVALID, "min_parallax_deg"), (dict(min_parallax_deg=180.0), INVALID, "min_parallax_deg = 180 outside [0, 180)"),
            (dict(min_parallax_deg=nan), INVALID, "min_parallax_deg"),
            (dict(P=sing, min_parallax_deg=1.0), INVALID, "camera 2 has a singular"),
            (dict(P=np.zeros((6, 3, 4)), nc=6), CAPACITY, "exceed capacity 5/40/200"), (dict(n_pts=41), CAPACITY, "np=41"), (dict(n_pts=-1), CAPACITY, "np=-1"),
            (dict(obs=np.zeros((201, 2)), cam=np.zeros(201, np.int32), pt=np.zeros(201, np.int32)), CAPACITY, "n_obs=201"), (dict(n_obs=-1), CAPACITY, "n_obs=-1")]
    for kw, code, needle in rows:
        rc, untouched, msg = check(**kw)
        assert (rc, untouched) == (code, True) and needle in msg and msg.startswith("pmv_triangulate_tracks: "), (kw, rc, msg)
    for kw in (dict(), dict(default_params=True), dict(null=13), dict(P=sing), dict(min_views=2, refine_iters=20, max_depth=inf, max_reproj=inf, min_parallax_deg=179.9),
               dict(min_depth=-5.0, max_depth=-5.0), dict(n_obs=0), dict(n_obs=0, null=5), dict(n_pts=0, n_obs=0, null=11),
               dict(cam=np.r_[sc["cam"], sc["cam"]][:200], pt=np.r_[sc["pt"], sc["pt"]][:200], obs=np.r_[sc["obs"], sc["obs"]][:200])):
        assert check(**kw) == (0, True, ""), kw
    # the calls themselves refuse a null context before anything else
    assert lib.pmv_triangulate_tracks(None, None, 0, None, None, None, 0, 0, None, None, None, None, None) == INVALID
    assert lib.pmv_batch_triangulate_tracks(None, 0, None, 0, None, None, None, 0, 0, None, None, None, None, None) == INVALID
    assert lib.pmv_debug_tri_tracks_launches(None, None) == INVALID


def _addr(p):
    return C.cast(p, C.c_void_p).value


def test_the_context_methods_marshal_their_arguments_to_the_right_calls(pmv):
    sc = tc.scene(3, 11, 4, noise_px=0.5)
    n_obs = len(sc["obs"])
    for seq in (None, 3):
        for par in (None, dict(min_views=3, refine_iters=4, min_depth=0.2, max_depth=50.0, max_reproj=2.0, min_parallax_deg=1.5)):
            lib = _Recorder()
            ctx = _ctx(pmv, lib)
            head = 1 if seq is None else 2
            cam64 = sc["cam"].astype(np.int64)   # converted to int32 on the way in
            if seq is None:
                xyz, status, err, good = ctx.triangulate_tracks(sc["P"], sc["obs"], cam64, sc["pt"], 11, par)
            else:
                xyz, status, err, good = ctx.batch_triangulate_tracks(seq, sc["P"], sc["obs"], cam64, sc["pt"], 11, par)
            (name, a), = lib.calls
            assert name == ("pmv_triangulate_tracks" if seq is None else "pmv_batch_triangulate_tracks") and len(a) == head + 12
            assert seq is None or a[1] == seq
            a = a[head:]
            assert np.array_equal(np.ctypeslib.as_array(a[0], (3, 12)), sc["P"].reshape(3, 12)) and a[1] == 3
            assert np.array_equal(np.ctypeslib.as_array(a[2], (n_obs, 2)), sc["obs"])
            assert isinstance(a[3], _ip) and np.array_equal(np.ctypeslib.as_array(a[3], (n_obs,)), sc["cam"])
            assert np.array_equal(np.ctypeslib.as_array(a[4], (n_obs,)), sc["pt"]) and a[5] == n_obs and a[6] == 11
            if par is None:
                assert a[7] is None
            else:
                p = a[7]._obj
                assert isinstance(p, pmv.TriParams) and (p.min_views, p.refine_iters, p.min_depth, p.max_depth, p.max_reproj, p.min_parallax_deg) == (3, 4, 0.2, 50.0, 2.0, 1.5)
            assert _addr(a[8]) == xyz.ctypes.data and xyz.shape == (11, 3) and _addr(a[9]) == status.ctypes.data and status.shape == (11,) and status.dtype == np.uint8
            assert _addr(a[10]) == err.ctypes.data and err.shape == (11,) and good == 0
    with pytest.raises(ValueError):
        _ctx(pmv, _Recorder()).triangulate_tracks(sc["P"], sc["obs"], sc["cam"][:-1], sc["pt"], 11)


def test_projections_from_ba_cams_have_zero_projection_residual(pmv):
    """points projected through the helper's matrices give orc_binding.ba_residuals <= 1e-9 px (the rounding of a double projection at 1e3 px
    is about 1e-13), and the third row is the depth pz = -p[2] of that form"""
    rng = np.random.default_rng(11)
    nc, n = 6, 50
    cams = np.c_[rng.uniform(-0.2, 0.2, (nc, 3)), rng.uniform(-1, 1, (nc, 3))]
    cams[0, :3] = 0          # no rotation: the first-order branch
    cams[1, :3] = 1e-9
    X = np.c_[rng.uniform(-4, 4, (n, 2)), rng.uniform(-30, -5, n)]   # in front of cameras that look down -z
    cam, pt = np.repeat(np.arange(nc), n).astype(np.int32), np.tile(np.arange(n), nc).astype(np.int32)
    for K in (tc.KMAT, np.eye(3)):
        P = pmv.projections_from_ba_cams(cams, K)
        assert P.shape == (nc, 3, 4)
        uv, depth = tc.project(P[cam], X[pt])
        assert (depth > 1).all()
        r, _ = orc_binding.ba_residuals(cams, X, uv, cam, pt, K)
        print("worst residual", np.abs(r).max())
        assert np.abs(r).max() <= 1e-9
    assert np.array_equal(pmv.projections_from_ba_cams(cams), pmv.projections_from_ba_cams(cams, np.eye(3)))
    # and the twin triangulates them back
    got = tc.twin().run(pmv.projections_from_ba_cams(cams, tc.KMAT), tc.project(pmv.projections_from_ba_cams(cams, tc.KMAT)[cam], X[pt])[0], cam, pt, n, tc.DEFAULTS)
    assert not got["status"].any() and np.allclose(got["xyz"], X, rtol=1e-8)
