"""pmv_lk_track_ex / pmv_lk_track_fb without a GPU: the surface (declared, exported, bound, documented), the CPU twin pinned to the oracle
at flags 0, and the conditions the two scenes must meet for the GPU tests to mean anything (by the twin alone: if one of these fails, the
scene is wrong, not a kernel)."""
import os
import re

import numpy as np
import pytest

import lkx_common as lx

ROOT = lx.ROOT
NEW = ["pmv_lk_track_ex", "pmv_lk_track_fb", "pmv_batch_lk_track_ex", "pmv_batch_lk_track_fb"]


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def test_the_four_symbols_are_declared_exported_and_bound(pmv):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = pmv.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(\s*pmv_ctx\*" % name, code), f"{name} is not declared in include/pmv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pmv.ABI_SYMBOLS
    assert re.search(r"PMV_LK_USE_INITIAL_FLOW\s*=\s*4\b", code) and re.search(r"PMV_LK_GET_MIN_EIGENVALS\s*=\s*8\b", code)
    assert (pmv.LK_USE_INITIAL_FLOW, pmv.LK_GET_MIN_EIGENVALS) == (4, 8)
    for method in ("lk_track_ex", "lk_track_fb", "batch_lk_track_ex", "batch_lk_track_fb"):
        assert callable(getattr(pmv.Context, method))


class _Recorder:
    """stands in for the library: records the arguments of every call and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        object.__setattr__(self, name, fn)
        return fn


def _floats(ptr, n):
    return np.ctypeslib.as_array(ptr, shape=(n,)).copy()


@pytest.mark.parametrize("method, symbol, n_args", [("lk_track_ex", "pmv_lk_track_ex", 9), ("lk_track_fb", "pmv_lk_track_fb", 12),
                                                    ("batch_lk_track_ex", "pmv_batch_lk_track_ex", 9), ("batch_lk_track_fb", "pmv_batch_lk_track_fb", 12)])
def test_the_binding_hands_over_flags_and_the_in_out_array(pmv, method, symbol, n_args):
    ctx = object.__new__(pmv.Context)
    ctx.lib, ctx.h = _Recorder(), None
    pts = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
    init = pts + np.float32(0.5)
    for kw, flags in ((dict(), 0), (dict(init_xy=init), 4), (dict(min_eigenvals=True), 8), (dict(init_xy=init, min_eigenvals=True), 12)):
        ctx.lib.calls.clear()
        out = getattr(ctx, method)(2, 3, pts, **kw)
        (name, args), = ctx.lib.calls
        assert name == symbol and len(args) == n_args and args[1:3] == (2, 3) and args[4] == 3 and args[6] == flags, (name, args)
        assert np.array_equal(_floats(args[3], 6), pts.ravel())
        assert np.array_equal(_floats(args[5], 6), init.ravel() if "init_xy" in kw else np.zeros(6, np.float32)), "the in/out array does not carry the initial flow"
        assert len(out) == (6 if n_args == 12 else 3) and out[0].shape == (3, 2)
        assert out[0] is not init and np.array_equal(init, pts + np.float32(0.5)), "the caller's init_xy must not be the array the library overwrites"
    with pytest.raises(ValueError):
        getattr(ctx, method)(2, 3, pts, init_xy=init[:2])


def test_the_header_states_the_rules():
    src = " ".join(_header().replace("*", " ").split())
    doc = src[src.index("cv::calcOpticalFlowPyrLK with its `flags` argument"):src.index("int pmv_debug_lk_general")]
    for phrase in ("in/out", "next_xy[i] 2^-level", "read, then overwritten", "Without the flag it is output only", "before the threshold test",
                   "the final residual is not computed", "points that end with status 0 included", "flags = 0: the bytes of pmv_lk_track",
                   "An initial flow equal to prev_xy: the same bytes again", "nothing is written", "not finite or beyond 1e6", "flag bits other than the two",
                   "n above max_tracks", "made by the first extended call", "Defined as a composition, bit for bit", "runs no backward pass",
                   "back_status 0, back_err 0, back_xy = the bits of its forward next_xy", "does not threshold", "a track counts once"):
        assert phrase in doc, phrase
    lk = src[src.index("OpenCVLucasKanadeFM.h:9-10"):src.index("typedef struct pmv_lk_params")]
    assert "per-call `flags` argument of pmv_lk_track_ex" in lk
    sess = src[src.index("pmv_lk_track_ex and pmv_lk_track_fb as session calls"):src.index("int pmv_batch_lk_track_ex")]
    for phrase in ("ONE launch", "out4[0]", "counts n tracks", "default order"):
        assert phrase in sess, phrase


PINNED = [(32, 4), (21, 3), (5, 4), (63, 4)]


@pytest.mark.parametrize("size", lx.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("win, max_level", PINNED)
def test_the_twin_is_the_oracle_at_flags_0(pmv, orc, size, win, max_level):
    """byte for byte in all three outputs, and again with an initial flow equal to the points"""
    a, b, pts = lx.pair_a(pmv, *size)
    want = orc.lk_track(a, b, pts, win=win, max_level=max_level)[:3]
    tw = lx.twin()
    for what, got in (("flags 0", tw.track(a, b, pts, win=win, max_level=max_level)), ("init = prev", tw.track(a, b, pts, init=pts, win=win, max_level=max_level))):
        print(what, int(got[1].sum()), "tracked")
        for name, g, r in zip(("xy", "status", "err"), got, want):
            assert np.array_equal(lx.bits(g), lx.bits(r)), f"{what}: {name} differs from orc.lk_track at {np.flatnonzero((lx.bits(g) != lx.bits(r)).reshape(len(pts), -1).any(axis=1))[:8]}"


def test_scene_crop_needs_the_initial_flow(pmv):
    """160x120, (32, 4): without the guess (nearly) nothing arrives, with it most points do"""
    a, b, pts, init = lx.crop(pmv, 160, 120)
    tw = lx.twin()
    plain = tw.track(a, b, pts)
    guided = tw.track(a, b, pts, init=init)
    n0, n1 = lx.near_truth(pts, plain[0], plain[1]), lx.near_truth(pts, guided[0], guided[1])
    print("within 0.5 px of the truth: without initial flow", n0, "with", n1, "of", len(pts))
    assert n0 <= 40 and n1 >= 100


@pytest.mark.parametrize("size", lx.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("win, max_level", [(32, 4), (21, 3)])
def test_scene_pair_a_has_failed_points_with_an_eigenvalue(pmv, size, win, max_level):
    """a kernel that zeroes err when a point fails must be caught: at least 5 status-0 points carry a non-zero err; xy and status are
    those of the call without the flag"""
    a, b, pts = lx.pair_a(pmv, *size)
    tw = lx.twin()
    plain = tw.track(a, b, pts, win=win, max_level=max_level)
    eig = tw.track(a, b, pts, flags=lx.EIG, win=win, max_level=max_level)
    n = int(((eig[1] == 0) & (eig[2] != 0)).sum())
    print("status-0 points with a non-zero err:", n)
    assert n >= 5
    assert np.array_equal(lx.bits(eig[0]), lx.bits(plain[0])) and np.array_equal(eig[1], plain[1])
    assert not np.array_equal(lx.bits(eig[2]), lx.bits(plain[2]))


def test_scene_crop_back_check_keeps_the_good_tracks(pmv):
    a, b, pts, init = lx.crop(pmv, 160, 120)
    for win, max_level in ((32, 4), (21, 3)):
        xy, st, err, bxy, bst, berr = lx.twin().track_fb(a, b, pts, init=init, win=win, max_level=max_level)
        kept = (st > 0) & (bst > 0) & (np.linalg.norm(bxy.astype(np.float64) - pts, axis=1) < 0.5)
        good = kept & (np.linalg.norm(xy.astype(np.float64) - (pts + lx.FLOW), axis=1) < 0.5)
        print(f"win {win}: the back check keeps {int(kept.sum())} tracks, {int(good.sum())} of them within 0.5 px of the truth")
        assert int(kept.sum()) >= 100
        # the stated outputs of tracks that failed forward
        f = st == 0
        assert not bst[f].any() and not berr[f].any() and np.array_equal(lx.bits(bxy[f]), lx.bits(xy[f]))
