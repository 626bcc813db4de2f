"""The CPU twin of pmv_triangulate_tracks (tests/twin/tri_tracks_twin.cpp) without a GPU: its DLT against numpy's SVD, against the oracle's
two-view triangulation bit for bit, its refinement, its gates and the order rule of its lists. The GPU tests compare the device with this
twin bit for bit (tests/test_tri_tracks_gpu.py)."""
import numpy as np
import pytest

import orc_binding
import tri_tracks_common as tc

NCS = [2, 3, 5, 12]
ACCURACY = [(nc, noise, pixel) for nc in NCS for noise in (0.0, 0.5) for pixel in (False, True)]


def _acc_scene(nc, noise, pixel):
    return tc.scene(nc, 60, 100 + nc, noise_px=noise, pixel=pixel, min_v=2)


@pytest.mark.parametrize("nc,noise,pixel", ACCURACY, ids=["nc%d-noise%g-%s" % (a, b, "px" if c else "norm") for a, b, c in ACCURACY])
def test_the_dlt_agrees_with_numpys_svd(nc, noise, pixel):
    """The bar is numpy's, not the code's: X of the smallest right singular vector of A (np.linalg.svd, float64), 1e-8 relative. A numpy port
    of the same Jacobi differs from the SVD by at most 1.1e-10 on scenes of this kind (8.5e-12 from the truth without noise); the bar is that
    with a factor of about 100."""
    sc = _acc_scene(nc, noise, pixel)
    got = tc.run(sc, tc.NO_GATES)
    want = tc.svd_points(sc)
    assert got["rc"] == 0 and not got["status"].any() and got["good"] == sc["n_pts"]
    rel = np.linalg.norm(got["xyz"] - want, axis=1) / np.linalg.norm(want, axis=1)
    print(f"nc={nc} noise={noise} pixel={pixel}: worst relative difference to the SVD {rel.max():.3e}")
    assert rel.max() <= 1e-8
    if noise == 0:
        true = np.linalg.norm(got["xyz"] - sc["X"], axis=1) / np.linalg.norm(sc["X"], axis=1)
        print(f"   worst relative difference to the truth {true.max():.3e}")
        assert true.max() <= 1e-8


def test_two_views_with_the_first_camera_at_the_origin_have_the_oracles_bits():
    """nc = 2, first camera [I|0]: the twin's homogeneous vector is orc_binding.triangulate_candidates', candidate by candidate"""
    n = 40
    scs = [tc.scene(2, n, 20 + k, noise_px=0.5, first_identity=True, min_v=2) for k in range(4)]
    q1, q2 = np.zeros((n, 2)), np.zeros((n, 2))
    for i in range(len(scs[0]["pt"])):   # every candidate sees the same observations: scene 0's (the candidates differ in the second camera)
        (q1 if scs[0]["cam"][i] == 0 else q2)[scs[0]["pt"][i]] = scs[0]["obs"][i]
    P1x4 = np.array([s["P"][1] for s in scs])
    Q, _, _ = orc_binding.triangulate_candidates(q1, q2, P1x4, np.ones(n, np.uint8))
    pt = np.repeat(np.arange(n, dtype=np.int32), 2)
    cam = np.tile(np.array([0, 1], np.int32), n)
    obs = np.stack([q1, q2], axis=1).reshape(-1, 2)
    for c in range(4):
        P = np.array([np.c_[np.eye(3), np.zeros(3)], P1x4[c]])
        got = tc.twin().run(P, obs, cam, pt, n, tc.NO_GATES)
        assert np.array_equal(tc.bits(got["Qh"]), tc.bits(Q[c].T)), c
        ok = got["status"] == 0
        assert ok.sum() >= n - 2 and np.array_equal(tc.bits(got["xyz"][ok]), tc.bits((Q[c][:3] / Q[c][3]).T[ok]))


@pytest.mark.parametrize("nc,pixel", [(nc, px) for nc in NCS for px in (False, True)])
def test_every_accepted_step_lowers_the_cost_and_the_refined_error_is_not_above_the_dlts(nc, pixel):
    sc = _acc_scene(nc, 0.5, pixel)
    dlt = tc.run(sc, tc.NO_GATES)
    ref = tc.run(sc, dict(tc.NO_GATES, refine_iters=5))
    assert not ref["status"].any()
    taken = 0
    for j in range(sc["n_pts"]):
        k = ref["steps"][j]
        costs = ref["costs"][j]
        assert np.isfinite(costs[:k + 1]).all() and np.isnan(costs[k + 1:]).all()
        assert (np.diff(costs[:k + 1]) < 0).all(), (j, costs)
        taken += k
    assert taken > 0
    print(f"nc={nc} pixel={pixel}: {taken} accepted steps over {sc['n_pts']} landmarks; rms {dlt['err'].mean():.4g} -> {ref['err'].mean():.4g}")
    assert (ref["err"] <= dlt["err"]).all()
    assert (ref["err"] < dlt["err"]).any()
    # rms^2 * views is the cost the refinement saw last
    m = np.bincount(sc["pt"], minlength=sc["n_pts"])
    last = np.array([ref["costs"][j][ref["steps"][j]] for j in range(sc["n_pts"])])
    assert np.allclose(ref["err"] ** 2 * m, last, rtol=1e-12, atol=0)


def test_refine_iters_zero_is_the_dlt_and_more_iterations_never_raise_the_cost():
    sc = _acc_scene(5, 0.5, True)
    prev = tc.run(sc, tc.NO_GATES)["err"]
    for it in (1, 2, 20):
        cur = tc.twin().run(sc["P"], sc["obs"], sc["cam"], sc["pt"], sc["n_pts"], dict(tc.NO_GATES, refine_iters=it))["err"]
        assert (cur <= prev).all()
        prev = cur


def test_the_gate_scene_produces_every_bit_and_two_at_once():
    sc = tc.gate_scene()
    for it in (0, 5):
        r = tc.run(sc, dict(tc.GATE_PARAMS, refine_iters=it))
        st = dict(zip(tc.GATE_NAMES, r["status"].tolist()))
        print(it, st, r["err"])
        assert r["rc"] == 0
        assert st["good"] == 0 and r["good"] == 1
        assert st["behind"] == tc.DEPTH
        assert st["outlier"] == tc.REPROJ
        assert st["baseline"] == tc.PARALLAX
        assert st["no-obs"] == tc.FEW_VIEWS and st["one-obs"] == tc.FEW_VIEWS
        assert st["behind+outlier"] == tc.DEPTH | tc.REPROJ
        assert st["twice-degenerate"] == tc.DEGENERATE
        assert st["at-centre"] & tc.DEPTH
        assert np.bitwise_or.reduce(r["status"]) == 31
        assert any(bin(s).count("1") >= 2 for s in r["status"])
        for name in ("no-obs", "one-obs", "twice-degenerate"):   # the short circuits: xyz = 0, err = +inf
            j = tc.GATE_NAMES.index(name)
            assert not r["xyz"][j].any() and r["err"][j] == np.inf
        assert np.allclose(r["xyz"][0], sc["X"][0], rtol=1e-10) and r["err"][0] < 1e-12
    # gates off: the same landmarks are accepted wherever the DLT has a point
    off = tc.run(sc, tc.NO_GATES)
    assert [int(s) for s in off["status"]] == [0, 0, 0, 0, tc.FEW_VIEWS, tc.FEW_VIEWS, 0, 0, tc.DEGENERATE]
    # min_views = 3 turns the two-view landmark into FEW_VIEWS
    r3 = tc.twin().run(sc["P"], sc["obs"], sc["cam"], sc["pt"], sc["n_pts"], dict(tc.GATE_PARAMS, min_views=3))
    assert r3["status"][tc.GATE_NAMES.index("baseline")] == tc.FEW_VIEWS


def test_a_singular_camera_is_named_only_with_the_parallax_gate_on():
    sc = tc.gate_scene()
    P = sc["P"].copy()
    P[3, :, :3] = np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]])
    assert tc.twin().run(P, sc["obs"], sc["cam"], sc["pt"], sc["n_pts"], tc.GATE_PARAMS)["rc"] == -(1 + 3)
    assert tc.twin().run(P, sc["obs"], sc["cam"], sc["pt"], sc["n_pts"], dict(tc.GATE_PARAMS, min_parallax_deg=0.0))["rc"] == 0
    bad, Cn = tc.twin().centres(sc["P"])
    assert bad == -1 and np.allclose(Cn, [[0, 0, 0.8 * i] for i in range(4)] + [[0.01, 0, 0]], atol=1e-15)


@pytest.mark.parametrize("nc", [3, 12])
def test_only_the_order_within_a_landmarks_list_matters(nc):
    sc = tc.scene(nc, 70, 7 + nc, noise_px=0.5, pixel=True)
    p = tc.gates_on(True, refine_iters=5)
    want = tc.run(sc, p)
    for seed in (1, 2):
        sh = tc.order_preserving_shuffle(sc, seed)
        assert not np.array_equal(sh["pt"], sc["pt"])
        got = tc.twin().run(sh["P"], sh["obs"], sh["cam"], sh["pt"], sh["n_pts"], p)
        for k in ("xyz", "err"):
            assert np.array_equal(tc.bits(got[k]), tc.bits(want[k])), k
        assert np.array_equal(got["status"], want["status"]) and got["good"] == want["good"]
    # sorted by landmark (stable) is one such permutation
    o = np.argsort(sc["pt"], kind="stable")
    got = tc.twin().run(sc["P"], sc["obs"][o], sc["cam"][o], sc["pt"][o], sc["n_pts"], p)
    assert np.array_equal(tc.bits(got["xyz"]), tc.bits(want["xyz"])) and np.array_equal(got["status"], want["status"])
    # reversing the lists is not: some bits move (the sums are ordered), the points stay close
    rev = tc.twin().run(sc["P"], sc["obs"][::-1].copy(), sc["cam"][::-1].copy(), sc["pt"][::-1].copy(), sc["n_pts"], p)
    ok = (want["status"] & 3) == 0
    assert not np.array_equal(tc.bits(rev["xyz"]), tc.bits(want["xyz"]))
    assert np.allclose(rev["xyz"][ok], want["xyz"][ok], rtol=1e-6)


def test_the_same_camera_listed_twice_is_accepted():
    sc = tc.scene(3, 30, 5, noise_px=0.5, min_v=2)
    obs = np.r_[sc["obs"], sc["obs"][:10] + 1e-4]
    cam, pt = np.r_[sc["cam"], sc["cam"][:10]], np.r_[sc["pt"], sc["pt"][:10]]
    r = tc.twin().run(sc["P"], obs, cam, pt, sc["n_pts"], tc.DEFAULTS)
    base = tc.run(sc, tc.DEFAULTS)
    assert r["rc"] == 0 and not r["status"].any()
    touched = np.unique(sc["pt"][:10])
    same = np.setdiff1d(np.arange(sc["n_pts"]), touched)
    assert np.array_equal(tc.bits(r["xyz"][same]), tc.bits(base["xyz"][same]))
    assert not np.array_equal(tc.bits(r["xyz"][touched]), tc.bits(base["xyz"][touched]))
    assert (r["err"][touched] < 3.0 / 718.0).all()   # still a fit of all its rows: 0.5 px of noise per coordinate, 6 sigma
