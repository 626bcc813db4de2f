"""The bundle-adjustment launch chain (pmv_ba_solve, multi-kernel form) computes what it computed before its launches were fused: bit for
bit the cameras, points and summaries recorded in tests/golden/ba_chain_parent.npz (made by tests/golden/make_ba_chain_golden.py on the commit
named inside the file, before the change), and the CPU oracle's results at the tolerance of test_backend_gpu.test_ba_solve_matches_oracle.
The problems sit at the structural edges of the chain: smallest problem, one K-slice / several / all eight with a short last one, 3 np a
multiple of 16 and not, a point whose three rows straddle a slice boundary (with and without duplicate observations), a camera that sees no
point of a slice, rejected steps, a point block that is not positive definite (every step invalid), early termination (step tolerance,
gradient tolerance in the first iteration), 1 and 50 iterations, more than 2 x 2 tiles, K-slices around and above what a block's LDS holds.

What the recorded commit itself does against the oracle (print-out of the maker script on that commit): iterations, accepted steps and
termination are equal on every problem; cameras and points are within the tolerance on every problem. Two comparisons need a word:
 * final cost: a cost that the solve has driven to ~1e-16 (one camera and one point; the noiseless scene) has no relative accuracy - the
   parameters are compared at 1e-6 relative, and moving them by that much moves the cost by ~1e-12 of its starting value. So the cost is
   compared with rtol 1e-8 plus an absolute term of 1e-12 x the initial cost. (Recorded commit: 2.1e-19 against the oracle's, initial 15.5.)
 * more than 5 iterations: as in test_ba_solve_matches_oracle, only the iteration count and the reached cost level (rtol 1e-3) are compared
   with the oracle's. The recorded bits are compared in full."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_ba_chain_golden", os.path.join(HERE, "golden", "make_ba_chain_golden.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

PROBLEMS = {p[0]: p for p in maker.problems()}
NAMES = list(PROBLEMS)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "ba_chain_parent.npz"))
    assert len(str(g["commit"])) == 40
    return g


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(64, 64, n_slots=1)


@pytest.fixture(scope="module")
def oracle():
    """name -> (cams, pts, summary) of the CPU oracle, computed once"""
    with np.errstate(all="ignore"):
        return {name: maker.oracle_solve(p) for name, p in PROBLEMS.items()}


def test_fixture_covers_the_problems(golden):
    assert sorted(k[:-8] for k in golden.files if k.endswith("_summary")) == sorted(NAMES)


def test_problems_exercise_what_they_are_meant_to(golden):
    """the recorded summaries show the paths: rejected steps, invalid steps, early termination, the iteration-count edges"""
    s = {n: golden[n + "_summary"] for n in NAMES}   # [initial cost, final cost, iterations, accepted steps, termination]
    for n in ("nc5_np60", "nc5_np120_far_start", "nc5_np700", "nc5_np100_it50"):
        assert s[n][3] < s[n][2], n                               # at least one rejected step (the LM diagonal is reused)
    assert tuple(s["nc5_np40_degenerate_ray"][2:]) == (5, 0, 4)   # five invalid steps: "no convergence"
    assert s["nc5_np100_noiseless"][2] < 50 and s["nc5_np100_noiseless"][4] == 3
    assert tuple(s["nc5_np100_at_the_optimum"][2:]) == (1, 0, 3)
    assert s["nc5_np100_it1"][2] == 1 and 5 < s["nc5_np100_it50"][2] < 50
    # the straddling point of the np = 60 problems and the blind camera
    _, _, pts, _, ci, pi, _ = PROBLEMS["nc5_np60_dup_straddle"]
    krows = (3 * len(pts) + 15) // 16 * 16
    kper = ((krows + 7) // 8 + 15) // 16 * 16
    assert 3 * maker.STRADDLER < kper < 3 * maker.STRADDLER + 3 and (krows + kper - 1) // kper < 8
    pairs = [(c, p) for c, p in zip(ci, pi) if p == maker.STRADDLER]
    assert pairs.count((1, maker.STRADDLER)) == 3 and pairs.count((3, maker.STRADDLER)) == 2
    _, _, pts, _, ci, pi, _ = PROBLEMS["nc5_np60_cam_blind_in_slice"]
    assert not np.any((ci == 2) & (3 * pi < 2 * kper)) and np.any(ci == 2) and len(np.unique(pi)) == len(pts)
    krows = (3 * 390 + 15) // 16 * 16
    kper = ((krows + 7) // 8 + 15) // 16 * 16
    assert (krows + kper - 1) // kper == 8 and krows - 7 * kper < kper   # the metric shape: 8 slices, the last one short


@pytest.mark.parametrize("name", NAMES)
def test_ba_chain_same_bits_as_recorded(ctx, golden, oracle, name):
    prob = PROBLEMS[name]
    cams, pts, s = maker.solve(ctx, prob)
    oc, op, os_ = oracle[name]
    with np.errstate(all="ignore"):
        print(f"{name}: summary {s.tolist()} recorded {golden[name + '_summary'].tolist()} oracle {os_.tolist()}; "
              f"|cams - oracle| {np.abs(cams - oc).max():.3g} |pts - oracle| {np.abs(pts - op).max():.3g}")
    # 1. the recorded bits
    assert s.tobytes() == golden[name + "_summary"].tobytes(), f"summary {s} differs from the recorded {golden[name + '_summary']}"
    bad = np.nonzero((cams.view(np.uint64) != golden[name + "_cams"].view(np.uint64)).any(1))[0]
    assert bad.size == 0, f"cameras {bad.tolist()} differ from the recorded bits"
    bad = np.nonzero((pts.view(np.uint64) != golden[name + "_pts"].view(np.uint64)).any(1))[0]
    assert bad.size == 0, f"{bad.size} points (first {bad[:8].tolist()}) differ from the recorded bits"
    # 2. the oracle, at the tolerance of test_backend_gpu.test_ba_solve_matches_oracle (see the module docstring)
    if np.isfinite(os_[0]):
        np.testing.assert_allclose(s[0], os_[0], rtol=1e-12)
    else:
        assert s[0] == os_[0]
    if prob[6] > 5:
        assert s[2] == os_[2]
        np.testing.assert_allclose(s[1], os_[1], rtol=1e-3)
    else:
        assert np.array_equal(s[2:], os_[2:]), f"iterations / accepted steps / termination {s[2:]} vs the oracle's {os_[2:]}"
        if np.isfinite(os_[1]):
            np.testing.assert_allclose(s[1], os_[1], rtol=1e-8, atol=1e-12 * os_[0])
        else:
            assert s[1] == os_[1]
        np.testing.assert_allclose(cams, oc, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(pts, op, rtol=1e-6, atol=1e-6)
    # 3. a second call on the same context
    again = maker.solve(ctx, prob)
    for a, b in zip((cams, pts, s), again):
        assert a.tobytes() == b.tobytes(), "a second call on the same context returns other bits"
