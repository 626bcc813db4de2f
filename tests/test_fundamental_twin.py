"""The CPU twin of pmv_find_fundamental_mat (tests/twin/fundamental_twin.cpp) against independent restatements, without a GPU: the subset
stream against cv::RNG / getSubset / the collinearity rule written out in numpy; the seven-point solver against numpy's SVD null space and
np.roots; the libm-free cubic against cv's trigonometric form on glibc; the RANSAC's properties on the scenes the GPU test compares bits on,
each asserted so that a scene which stops exercising its branch fails here.

Measured on these inputs (the bounds below are 10 x the worst case seen; the margin covers other seeds - the two null-space constructions and
the two root formulas differ by conditioning, not by design):
  seven-point models against the SVD / np.roots solver, unit Frobenius norm and sign: worst 1.6e-9 over 4800 subsets; subsets whose model
  counts differ (near-double roots): 0 of 4800 (cap 1 %).
  cubic roots against acos / cos / pow on glibc, 3002 cubics with a leading coefficient: the counts and the order agree on every one; values:
  median 2 ulps, worst 2.0e-8 of the largest root's magnitude (cubics with two nearly equal roots, where acos near +-1 loses digits; in ulps of
  a root near 0 that worst case is 1.5e13, which is why the bound is relative to the largest root). The quadratic, linear and double-root
  cases are cv's own arithmetic and agree exactly.
  the true F of the noise-free scenes among the models: NOT to the solver bound. The points are float32 (a relative error of 6e-8 on pixel
  coordinates of up to 1200), and a minimal subset amplifies that by its conditioning, which has no worst case: over the 2400 noise-free
  subsets the distance to the true F has median 2.8e-7, 99th percentile 5.8e-5, and 3 subsets (0.125 %) lie beyond 1e-3 (largest 0.094).
  Asserted: 10 x each of the three figures."""
import math

import numpy as np
import pytest

import fundamental_common as fc
from test_twoview_host import CvRNG, K, _scene, _skew, update_num_iters

SOLVER_BOUND = 1.6e-8    # 10 x the worst difference measured (see above)
CUBIC_BOUND = 2.0e-7     # 10 x the worst relative difference measured
TRUE_F_MEDIAN, TRUE_F_P99, TRUE_F_FAR_LIMIT, TRUE_F_FAR_SHARE = 2.8e-6, 5.8e-4, 1e-3, 0.0125   # 10 x the measured median, 99th percentile, share beyond the limit
FLT_EPSILON = float(np.finfo(np.float32).eps)


# ---- RNG and subsets ---------------------------------------------------------------------------------------------------------------------
def _collinear(p, idx):
    """haveCollinearPoints on the subset's last point: float subtractions widened to double"""
    q = p[idx]
    d = (q[:-1] - q[-1]).astype(np.float64)   # float32 - float32, then widened
    for j in range(len(d)):
        for k in range(j):
            dx1, dy1, dx2, dy2 = d[j, 0], d[j, 1], d[k, 0], d[k, 1]
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def _subsets(p1, p2, count, max_attempts=10000):
    rng, out, refused = CvRNG(), [], 0
    for _ in range(count):
        for attempt in range(max_attempts):
            idx = []
            while len(idx) < 7:
                v = rng.uniform(0, len(p1))
                if v not in idx:
                    idx.append(v)
            if _collinear(p1, idx) or _collinear(p2, idx):
                refused += 1
                continue
            break
        else:
            return out, refused
        out.append(idx)
    return out, refused


@pytest.mark.parametrize("key", [("scene", 1, 15, 0.0), ("scene", 2, 65, 0.3), ("scene", 1, 300, 0.5), ("col40", 1, 100, 0.0)], ids=fc.scene_id)
def test_the_subset_stream_equals_the_numpy_restatement(key):
    p1, p2 = fc.points(*key)
    got, refused = fc.twin().subsets(p1, p2, 60)
    want, wrefused = _subsets(p1, p2, 60)
    assert got.tolist() == want and refused == wrefused
    if key[0] == "col40":
        print("subsets refused by checkSubset among the first 60 + refused:", refused)
        assert refused >= 1, "the scene is there for the refusal branch"
    assert got[0].tolist() == _subsets(p1, p2, 1)[0][0]


def test_all_points_on_one_line_give_no_model_and_no_sample():
    p1, p2 = fc.points("colall", 1, 100, 0.0)
    got, refused = fc.twin().subsets(p1, p2, 3)
    assert len(got) == 0 and refused == 10000
    found, F, mask, drawn, _ = fc.found(("colall", 1, 100, 0.0))
    assert not found and drawn == 0 and not mask.any() and not F.any()


# ---- the seven-point solver against an independent one -------------------------------------------------------------------------------------
def _unit(F):
    return F / np.linalg.norm(F)


def _dist(Fa, Fb):
    return min(np.abs(Fa - Fb).max(), np.abs(Fa + Fb).max())


def _numpy_seven_point(s1, s2):
    x1, y1, x2, y2 = (v.astype(np.float64) for v in (s1[:, 0], s1[:, 1], s2[:, 0], s2[:, 1]))
    A = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(7)], 1)
    Vt = np.linalg.svd(A)[2]
    f1, f2 = Vt[7].reshape(3, 3), Vt[8].reshape(3, 3)
    ls = np.array([-1.0, 0.0, 1.0, 2.0])   # the cubic det(l f1 + (1 - l) f2) through four of its values
    c = np.linalg.solve(np.vander(ls, 4), [np.linalg.det(l * f1 + (1 - l) * f2) for l in ls])
    return [_unit(r.real * f1 + (1 - r.real) * f2) for r in np.roots(c) if abs(r.imag) < 1e-12 * max(1.0, abs(r))]


def test_the_seven_point_solver_equals_an_svd_and_np_roots_solver():
    tw = fc.twin()
    rng = np.random.default_rng(0)
    Kinv = np.linalg.inv(K.reshape(3, 3))
    worst, differ, total, true_d = 0.0, 0, 0, []
    for seed in range(1, 9):
        for noise in (0.0, 0.3):
            S = _scene(seed, 200, noise_px=noise)
            p1, p2 = S["p1"].astype(np.float32), S["p2"].astype(np.float32)
            Ft = _unit(Kinv.T @ _skew(S["t"]) @ S["R"] @ Kinv)
            for _ in range(300):
                idx = rng.choice(200, 7, replace=False)
                a, b = tw.seven_point(p1[idx], p2[idx]), _numpy_seven_point(p1[idx], p2[idx])
                total += 1
                if len(a) != len(b):
                    differ += 1
                    continue
                assert 1 <= len(a) <= 3
                worst = max([worst] + [min(_dist(_unit(Fa), Fb) for Fb in b) for Fa in a])
                if noise == 0.0:   # float32 points of an exact scene: the true F is among the models, to what the subset's conditioning leaves
                    true_d.append(min(_dist(_unit(Fa), Ft) for Fa in a))
    print(f"seven-point: worst difference {worst:.3g} over {total} subsets, model counts differ on {differ} ({100.0 * differ / total:.2f} %)")
    assert differ <= 0.01 * total
    assert worst <= SOLVER_BOUND
    true_d = np.array(true_d)
    far = float((true_d > TRUE_F_FAR_LIMIT).mean())
    print(f"true F among the models of {len(true_d)} noise-free subsets: median {np.median(true_d):.3g}, 99th percentile {np.percentile(true_d, 99):.3g}, "
          f"{100 * far:.3f} % beyond {TRUE_F_FAR_LIMIT:g} (largest {true_d.max():.3g})")
    assert len(true_d) >= 2000
    assert np.median(true_d) <= TRUE_F_MEDIAN and np.percentile(true_d, 99) <= TRUE_F_P99 and far <= TRUE_F_FAR_SHARE


# ---- the cubic against cv's trigonometric form on glibc ----------------------------------------------------------------------------------------
def _cv_cubic(c):
    """cv::solveCubic (3.4) with the host's libm: (n, roots)"""
    a0, a1, a2, a3 = (float(v) for v in c)
    x0 = x1 = x2 = 0.0
    n = 0
    if a0 == 0:
        if a1 == 0:
            if a2 == 0:
                n = -1 if a3 == 0 else 0
            else:
                x0, n = -a3 / a2, 1
        else:
            d = a2 * a2 - 4 * a1 * a3
            if d >= 0:
                d = math.sqrt(d)
                q1, q2 = (-a2 + d) * 0.5, (a2 + d) * -0.5
                if abs(q1) > abs(q2):
                    x0, x1 = q1 / a1, a3 / q1
                else:
                    x0, x1 = q2 / a1, a3 / q2
                n = 2 if d > 0 else 1
    else:
        a0 = 1.0 / a0
        a1, a2, a3 = a1 * a0, a2 * a0, a3 * a0
        Q = (a1 * a1 - 3 * a2) * (1.0 / 9)
        R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1.0 / 54)
        Qc = Q * Q * Q
        d = Qc - R * R
        if d > 0:
            theta = math.acos(R / math.sqrt(Qc))
            t0, t1, t2 = -2 * math.sqrt(Q), theta * (1.0 / 3), a1 * (1.0 / 3)
            x0, x1, x2 = t0 * math.cos(t1) - t2, t0 * math.cos(t1 + 2.0 * math.pi / 3) - t2, t0 * math.cos(t1 + 4.0 * math.pi / 3) - t2
            n = 3
        elif d == 0:
            e = math.pow(abs(R), 1.0 / 3) * (1 if R >= 0 else -1)
            x0, x1 = -2 * e - a1 / 3, e - a1 / 3
            n = 1 if x0 == x1 else 2
        else:
            e = math.pow(math.sqrt(-d) + abs(R), 1.0 / 3)
            if R > 0:
                e = -e
            x0, n = (e + Q / e) - a1 * (1.0 / 3), 1
    return n, [x0, x1, x2][:max(n, 0)]


def _ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64))) if (a < 0) == (b < 0) else 2 ** 62


def test_the_cubic_without_libm_equals_cvs_trigonometric_form():
    tw = fc.twin()
    rng = np.random.default_rng(5)
    cubics = [rng.normal(0, 1, 4) * 10.0 ** rng.integers(-2, 3, 4) for _ in range(1500)]          # mostly one real root
    cubics += [np.poly(rng.normal(0, 3, 3)) * rng.normal() for _ in range(1500)]                   # three real roots
    cubics += [np.concatenate([[0.0], rng.normal(0, 1, 3)]) for _ in range(200)]                   # quadratic
    cubics += [np.array([0.0, 0.0, 2.0, -3.0]), np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(4), np.array([0.0, 1.0, 2.0, 1.0]), np.array([0.0, 1.0, 0.0, 1.0]),
               np.array([1.0, -3.0, 3.0, -1.0]), np.array([1.0, 0.0, 0.0, 0.0]), np.array([2.0, 0.0, -6.0, 4.0]), np.array([1.0, 0.0, -3.0, -2.0])]
    worst_rel, ul, three, one = 0.0, [], 0, 0
    for c in cubics:
        n, r = tw.cubic(c)
        wn, wr = _cv_cubic(c)
        assert n == wn, (c, n, wn)
        three += n == 3
        one += n == 1 and c[0] != 0
        if n == 3:
            assert r[0] <= r[2] <= r[1], "smallest, largest, middle"
        scale = max([1e-300] + [abs(v) for v in wr])
        for a, b in zip(r[:max(n, 0)], wr):
            if c[0] == 0 or n == 2:
                assert a == b, (c, r, wr)   # cv's own arithmetic (and the exact double root)
            else:
                worst_rel = max(worst_rel, abs(a - b) / scale)
                ul.append(_ulps(a, b))
    print(f"cubic: {three} with three roots, {one} with one; worst |difference| / largest root {worst_rel:.3g}; ulps: median {int(np.median(ul))}, "
          f"99 % {int(np.percentile(ul, 99))}, worst {max(ul)}")
    assert three > 1000 and one > 800
    assert worst_rel <= CUBIC_BOUND


# ---- RANSAC properties -------------------------------------------------------------------------------------------------------------------------
def test_ransac_properties_of_the_scenes():
    tw = fc.twin()
    R = fc.DEFAULT_R
    f15 = fc.found(("scene", 1, 15, 0.0))
    assert f15[0] and 0 < f15[3] < R and f15[2].sum() >= 7, "n = 15 works and ends inside the first round"
    # outlier fraction 0.3 ends within the first few rounds (3 px: see fundamental_common.CASES)
    f03 = fc.found(("scene", 1, 65, 0.3), 3.0)
    assert f03[0] and f03[3] <= 3 * R and f03[4] > 1
    # outlier fraction 0.5 at n = 300: several hundred samples, more than one niters update, not the cap
    f05 = fc.found(("scene", 1, 300, 0.5), 3.0)
    assert f05[0] and 300 < f05[3] < 1000 and f05[4] > 1
    # ... and at 1 px the same scene and the two-image noise scenes run into the 1000 cap
    for key in [("scene", 1, 300, 0.5), ("noise", 5, 40, 0.0), ("noise", 5, 200, 0.0)]:
        assert fc.found(key)[3] == 1000, key
    # a refused subset inside a call that goes on, and a later-iteration count that is not a multiple of anything special
    assert 0 < fc.found(("col40", 1, 100, 0.0))[3] < 1000
    for key, thr in fc.CASES:
        found, F, mask, drawn, _ = fc.found(key, thr)
        p1, p2 = fc.points(*key)
        if not found:
            assert not mask.any()
            continue
        assert np.array_equal(mask, (tw.errors(F, p1, p2) <= np.float32(thr * thr)).astype(np.uint8)), key
        assert mask.sum() >= 7
        if key[0] == "scene" and key[3] <= 0.3 and key[2] >= 63:
            S = fc.scene(*key[1:])
            true_in = ~S["outliers"]
            kept = (mask.astype(bool) & true_in).sum() / true_in.sum()
            print(f"{fc.case_id((key, thr))}: {100 * kept:.1f} % of the true inliers in the consensus set")
            # The pixel error of a coordinate is the 0.3 px noise plus the rounding (sigma 0.29): 0.42 px, in both images, so the epipolar
            # distance under the TRUE F has sigma 0.59 px. At 3 px that is five sigma: the issue's 90 %. At 1 px the true F would keep
            # erf(1 / (0.59 sqrt 2)) = 91 %; the F of a minimal sample carries the same noise itself, and one that doubles the sigma (1.18 px)
            # still keeps erf(1 / (1.18 sqrt 2)) = 60 %: that is asserted at 1 px (measured: 63.5 - 85.7 %).
            assert kept >= (0.9 if thr >= 3.0 else 0.6), (key, thr)
            assert (mask.astype(bool) & S["outliers"]).sum() <= 0.1 * key[2], (key, thr)


@pytest.mark.parametrize("seed,n,f", [(1, 65, 0.0), (2, 64, 0.3), (3, 63, 0.3), (1, 150, 0.1), (1, 300, 0.3)])
def test_the_inliers_contain_the_true_inliers(seed, n, f):
    """3 px against 0.3 px noise on integer pixels: at least 90 % of the scene's true inliers are in the consensus set, and F explains them"""
    found, F, mask, drawn, _ = fc.found(("scene", seed, n, f), 3.0)
    S = fc.scene(seed, n, f)
    true_in = ~S["outliers"]
    assert found and (mask.astype(bool) & true_in).sum() >= 0.9 * true_in.sum()


@pytest.mark.parametrize("n", [15, 64, 300, 1024])
def test_the_iteration_table_equals_update_num_iters(n):
    tw = fc.twin()
    for p in (0.99, 0.5, 0.999999):
        den, num = tw.iters_table(n, p)
        assert den[n] == -np.inf and num == math.log(1 - p)
        for max_iters in (1000, 37, 1):
            got = [tw.update_iters(den, num, g, max_iters) for g in range(n + 1)]
            want = [update_num_iters(p, (n - g) / n, 7, max_iters) for g in range(n + 1)]
            assert got == want, (p, max_iters)
