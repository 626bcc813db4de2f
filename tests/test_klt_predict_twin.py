"""The tracker step with a prediction (pmv_klt_set_prediction) on the CPU twins alone: the composition of tests/predict_common.py over the LK
twin, the projection twin and klt_common's stages. What is asserted here is what the GPU tests rely on - that the scenes make a predicted
step differ from a plain one, that an all-out-of-frame prediction falls back onto the plain step's bytes, and that the two predictions of the
min_succ boundary have exactly min_succ - 1 and exactly min_succ successes."""
import numpy as np
import pytest

import klt_common as kc
import lkx_common as lx
import predict_common as pc

LKS = [(32, 4), (21, 3)]
MIN_SUCC = 10


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(lx.bits(x), lx.bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("lk", LKS, ids=lambda v: "win%d-level%d" % v)
def test_a_good_prediction_changes_the_step(pmv, size, lk):
    w, h = size
    case = pc.scene_case(pmv, w, h)
    s0 = pc.state_of(case)
    n0 = len(s0["ids"])
    _, plain, res0, a0 = pc.plain_step(case, lk)
    assert res0 == (0, 0, 0, 0)
    flow = np.linalg.norm(a0[0] - s0["xy"], axis=1)[a0[1] == 1]
    print(size, lk, "n0", n0, "largest tracked flow", float(flow.max()), "px")
    assert flow.max() > 20, "the scene has no flow a prediction would help with"
    pred = pc.good_prediction(case, lk)
    guess, joined = pc.guesses_of(pred, s0["ids"], s0["xy"])
    assert joined == n0 and np.abs(guess - pc.truth(case, lk)).max() < 1.5 + 1e-3
    _, out, res, a = pc.predicted_step(case, pred, lk)
    print(size, lk, "plain counts", plain[4].tolist(), "predicted counts", out[4].tolist(), "result", res)
    assert res[0] == 1 and res[1] == n0 and res[2] >= pred["min_succ"] and res[3] == 0 and res[2] == int((a[1] == 1).sum())
    assert out[4][0] == n0 and out[4][3] >= 10, "too few tracks survive the predicted step"
    # at least one track that survives both steps has other bits
    common = np.intersect1d(plain[0][:plain[4][3]], out[0][:out[4][3]])
    ia, ib = np.searchsorted(plain[0][:plain[4][3]], common), np.searchsorted(out[0][:out[4][3]], common)
    equal = int((lx.bits(plain[2][ia]) == lx.bits(out[2][ib])).all(axis=1).sum())
    print(size, lk, "survivors of both steps:", len(common), "bit-equal:", equal)
    assert len(common) >= 10 and equal < len(common)
    # the back level matters too: the same guesses with the backward pass on every level
    _, out_b, res_b, a_b = pc.predicted_step(case, dict(pred, back_top_level=-1), lk)
    assert res_b[:3] == res[:3] and _same(a_b[:3], a[:3])
    if lk == (21, 3) or size == kc.SIZES[0]:   # (203 x 87 at win 32 has two levels: top 1 is the top)
        assert not _same(a_b[3:], a[3:])


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("lk", LKS, ids=lambda v: "win%d-level%d" % v)
def test_an_out_of_frame_prediction_falls_back_onto_the_plain_step(pmv, size, lk):
    w, h = size
    case = pc.scene_case(pmv, w, h)
    s0 = pc.state_of(case)
    _, plain, _, a0 = pc.plain_step(case, lk)
    pred = pc.far_prediction(case, back_top_level=-1)
    guess, joined = pc.guesses_of(pred, s0["ids"], s0["xy"])
    assert joined == len(s0["ids"]) and (guess < -100).all(), "every guess lies more than a window outside the frame"
    _, out, res, a = pc.predicted_step(case, pred, lk)
    assert res == (1, len(s0["ids"]), 0, 1)
    assert _same(out, plain) and _same(a, a0)
    # with the backward pass capped the fall-back is the plain forward pass and another backward pass
    _, out1, res1, a1 = pc.predicted_step(case, dict(pred, back_top_level=0), lk)
    assert res1 == res and _same(a1[:3], a0[:3]) and not _same(a1[3:], a0[3:])
    # min_succ = 0 never falls back, whatever happens: nothing survives
    _, out0, res0, _ = pc.predicted_step(case, dict(pred, min_succ=0), lk)
    assert res0 == (1, len(s0["ids"]), 0, 0) and out0[4][1] == 0 and out0[4][4] > 0


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_min_succ_boundary(pmv, size):
    """predictions built from the twin's own status bytes: in-frame guesses for k tracks that the predicted pass tracks, far ones for the
    rest - exactly k successes. An in-frame guess does not imply status 1, so the tracks are picked by status, not by position."""
    w, h = size
    lk = (21, 3)
    case = pc.scene_case(pmv, w, h)
    s0 = pc.state_of(case)
    pick = pc.boundary_tracks(case, lk, MIN_SUCC)
    assert len(pick) >= MIN_SUCC
    _, plain, _, a0 = pc.plain_step(case, lk)
    for k, fell in ((MIN_SUCC - 1, 1), (MIN_SUCC, 0)):
        pred = pc.partial_prediction(case, lk, pick[:k], min_succ=MIN_SUCC)
        _, out, res, a1 = pc.predicted_step(case, pred, lk)
        print(size, "k", k, "result", res, "counts", out[4].tolist())
        assert res == (1, len(s0["ids"]), k, fell)
        if fell:
            assert _same(a1[:3], a0[:3]), "the fall-back's forward pass is the plain one"
        else:
            assert out[4][1] <= k and set(out[0][:out[4][3]]) <= set(s0["ids"][pick[:k]])
