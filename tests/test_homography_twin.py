"""The CPU twin of pmv_find_homography (tests/twin/homography_twin.cpp) stage by stage: the scenes of homography_common are what they claim
(refusal counts, no-model cases, samples drawn at the cap), the iteration table is the Python expression, the Jacobi routine gives
eigenpairs, the four-point solve and the refit recover a known H, and the LM stage does not increase the squared reprojection error."""
import math

import numpy as np
import pytest

import homography_common as hc


def test_the_scenes_are_what_they_claim():
    tw = hc.twin()
    # plane and rot: no refusal is collinear; it takes outliers for the orientation test to refuse more than the odd subset (a triple that is
    # nearly collinear can change its orientation under the noise and the rounding); a model with most of the true inliers
    for key in (("plane", 1, 63, 0.0), ("plane", 2, 64, 0.3), ("plane", 3, 65, 0.6), ("plane", 1, 300, 0.6), ("rot", 1, 64, 0.0)):
        p1, p2 = hc.points(*key)
        sub, collinear, twisted = tw.subsets(p1, p2, 200)
        assert len(sub) == 200 and collinear == 0 and (twisted > 100 if key[3] > 0 else twisted <= 5), (key, collinear, twisted)
        assert all(len(set(s)) == 4 and 0 <= min(s) and max(s) < len(p1) for s in sub.tolist())
        r = hc.found(key, 3.0)
        assert r["found"] and 0 < r["drawn"] < 2000 and r["mask"].sum() >= 0.7 * (1 - key[3]) * len(p1), (key, r["drawn"], int(r["mask"].sum()))
    # noise: the loop runs into the caller's cap, whatever it is
    for n in (40, 300):
        for cap in (1, 100, 2000):
            assert hc.found(("noise", 5, n, 0.0), 3.0, max_iters=cap)["drawn"] == cap
    # col40: some subsets are refused as collinear, the call still finds the plane; colall: every subset is, getSubset fails at iteration 0
    sub, collinear, _ = tw.subsets(*hc.points("col40", 1, 100, 0.0), 200)
    assert len(sub) == 200 and collinear > 0 and hc.found(("col40", 1, 100, 0.0))["found"]
    sub, collinear, twisted = tw.subsets(*hc.points("colall", 1, 100, 0.0), 3)
    assert len(sub) == 0 and (collinear, twisted) == (10000, 0)
    r = hc.found(("colall", 1, 100, 0.0))
    assert not r["found"] and r["drawn"] == 0 and not r["mask"].any()
    # twist: the orientation test refuses most subsets (more refusals than subsets), the model is the plane of the points that are not mirrored
    sub, collinear, twisted = tw.subsets(*hc.points("twist", 1, 64, 0.0), 200)
    assert len(sub) == 200 and twisted > 2 * 200 and collinear == 0, twisted
    r = hc.found(("twist", 1, 64, 0.0))
    assert r["found"] and not r["mask"][::2].any() and r["mask"][1::2].sum() >= 20
    # tiny: runKernel has no model at n = 4 (no checkSubset in that branch); from 5 points on checkSubset refuses every subset
    p1, p2 = hc.points("tiny", 1, 4, 0.0)
    assert len(np.unique(p2)) == 1 and tw.four_point(p1, p2) is None
    for n in (4, 5):
        r = hc.found(("tiny", 1, n, 0.0))
        assert not r["found"] and r["drawn"] == 0 and not r["mask"].any()
    # n = 4: no RANSAC, no refit
    r = hc.found(("plane", 1, 4, 0.0))
    assert r["found"] and r["drawn"] == 0 and r["mask"].tolist() == [1] * 4 and np.isnan(r["S2"]).all()
    assert np.array_equal(hc.bits(r["H"]), hc.bits(tw.four_point(*hc.points("plane", 1, 4, 0.0))))


def test_check_subset():
    tw = hc.twin()
    sq = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], np.float32)
    assert tw.check_subset(sq, sq + 5) == 0
    assert tw.check_subset(sq, sq[[1, 0, 2, 3]]) == 2          # two corners swapped: the quadrilateral folds over
    assert tw.check_subset(sq, sq * [-1, 1]) == 2              # mirrored: every triple changes its orientation
    line = np.array([[0, 0], [10, 0], [10, 10], [20, 0]], np.float32)   # the LAST point on the line of the first two
    assert tw.check_subset(line, sq) == 1 and tw.check_subset(sq, line) == 1
    quirk = np.array([[0, 0], [10, 0], [20, 0], [5, 7]], np.float32)    # the first three collinear: cv does not look at them
    assert tw.check_subset(quirk, quirk) == 0


@pytest.mark.parametrize("n", [4, 5, 64, 300])
def test_the_iters_table_is_the_python_expression(n):
    tw = hc.twin()
    for conf in (0.995, 0.5):
        den, num = tw.iters_table(n, conf)
        assert num == math.log(1 - conf)
        for g in range(n + 1):
            d = 1.0 - (1.0 - (n - g) / n) ** 4
            assert den[g] == (-math.inf if d < 2.2250738585072014e-308 else math.log(d)), g
        assert tw.update_iters(den, num, 0, 2000) == 2000 and tw.update_iters(den, num, n, 2000) == 0
        g = max(n // 2, 1)
        want = num / den[g]
        assert tw.update_iters(den, num, g, 2000) == (2000 if want >= 2000 else round(want))


@pytest.mark.parametrize("n", [8, 9])
def test_the_jacobi_routine_gives_eigenpairs(n):
    tw = hc.twin()
    rng = np.random.default_rng(n)
    for trial in range(20):
        B = rng.standard_normal((n + (trial % 3) - 1, n))   # one trial in three is rank-deficient, as LtL of exact data is
        A = B.T @ B
        w, V = tw.jacobi(A)
        scale = np.abs(w).max()
        assert np.all(np.diff(w) <= 0)
        assert np.abs(A @ V.T - V.T * w).max() <= 1e-13 * scale            # A v = lambda v
        assert np.abs(V @ V.T - np.eye(n)).max() <= 1e-13
        assert np.abs(w - np.linalg.eigh(A)[0][::-1]).max() <= 1e-13 * scale
    for a, b in ((3.0, 4.0), (-4.0, 3.0), (0.0, 0.0), (1e200, 1e200), (0.0, -2.5)):
        assert tw.hypot(a, b) == pytest.approx(math.hypot(a, b), rel=4e-16)


def test_four_point_solve_and_errors():
    tw = hc.twin()
    H = hc.geometry("plane", 1)
    s1 = np.array([[100, 50], [900, 60], [1000, 300], [200, 330]], np.float64)
    s2 = hc._proj(H, s1)
    got = tw.four_point(s1, s2)
    assert got[2, 2] == 1.0 and np.linalg.norm(got - H) / np.linalg.norm(H) < 1e-4   # (the points are cast to float32)
    p1, p2 = hc.points("plane", 1, 63, 0.3)
    err = tw.errors(got, p1, p2)
    Hf = got.astype(np.float32)
    x, y = p1[:, 0], p1[:, 1]
    ww = np.float32(1) / (Hf[2, 0] * x + Hf[2, 1] * y + np.float32(1))
    dx, dy = (Hf[0, 0] * x + Hf[0, 1] * y + Hf[0, 2]) * ww - p2[:, 0], (Hf[1, 0] * x + Hf[1, 1] * y + Hf[1, 2]) * ww - p2[:, 1]
    assert err.dtype == np.float32 and np.array_equal(err, dx * dx + dy * dy)


# The refined H of the noise-free, outlier-free plane scenes (integer-rounded like every scene) against the H built from the scene's plane and
# poses, in relative Frobenius norm. Measured on the twin over the ten cases below: worst 3.144e-02 (n = 5; 2.4e-02 at n = 63, <= 1.2e-02 for
# the others - the rounding to integer pixels is what is left). The bound allows 10 x the worst for other seeds.
REFINED_H_BOUND = 0.3144


def test_the_refined_h_is_the_scenes():
    worst = 0.0
    for n, seed in ((5, 1), (63, 1), (64, 2), (65, 3), (300, 1)):
        Ht = hc.geometry("plane", seed)
        for thr in (1.0, 3.0):
            r = hc.twin().find(*hc.points("plane", seed, n, 0.0, 0.0), thr)
            e = np.linalg.norm(r["H"] - Ht) / np.linalg.norm(Ht)
            print(f"n={n} seed={seed} thr={thr}: inliers {int(r['mask'].sum())}, relative Frobenius error {e:.3e}")
            assert r["found"] and r["H"][2, 2] == 1.0
            worst = max(worst, e)
    print(f"worst {worst:.3e} (bound {REFINED_H_BOUND})")
    assert worst <= REFINED_H_BOUND


def test_refit_stages():
    """the DLT on the inliers is a least-squares fit of all of them; the LM stage never increases the sum of squared reprojection errors over
    the inliers, in the whole call and iteration by iteration"""
    tw = hc.twin()
    for key, thr in hc.CASES:
        r = hc.found(key, thr)
        if not r["found"] or len(r["mask"]) == 4:
            continue
        S0, S1 = r["S2"]
        assert S1 <= S0, (key, thr, S0, S1)
        p1, p2 = hc.points(*key)
        inl = r["mask"].astype(bool)
        q = hc._proj(r["H"], p1[inl].astype(np.float64)) - p2[inl]
        assert (q * q).sum() == pytest.approx(S1, rel=1e-9, abs=1e-18)
    key = ("plane", 2, 64, 0.3)
    r = hc.found(key, 3.0)
    p1, p2 = hc.points(*key)
    H = tw.refit_dlt(p1, p2, r["mask"])
    assert H is not None and H[2, 2] == 1.0
    S_prev = None
    for it in range(1, 6):
        Hn, made, S0, S1 = tw.lm(p1, p2, r["mask"], H, it)
        assert made <= it and S1 <= S0 and (S_prev is None or S1 <= S_prev)
        S_prev = S1
    Hn, made, S0, S1 = tw.lm(p1, p2, r["mask"], H, 10)
    assert np.array_equal(hc.bits(Hn), hc.bits(r["H"])) and r["S2"][0] == S0 and r["S2"][1] == S1   # the whole call is these stages
    # a mask with one point in it: the deviation sums are 0, runKernel has no model
    one = np.zeros(len(p1), np.uint8)
    one[7] = 1
    assert tw.refit_dlt(p1, p2, one) is None
