"""The solve / back-substitution launch of the bundle-adjustment chain (k_bam_solveback: load front, tmp3 in LDS, look-ahead Cholesky)
computes what it computed before its schedule changed: bit for bit the cameras, points and summaries recorded in
tests/golden/ba_solveback_parent.npz (made by tests/golden/make_ba_solveback_golden.py on the commit named inside the file, before the change),
and the CPU oracle's results at the tolerance of tests/test_ba_chain_gpu.py (see that module's docstring for the two comparisons that need a
word). The problems sit at the edges the schedule creates - the maker's docstring lists them - and a round of three of them, of different
nc, through the batched entry (k_bamB_solve, k_bamB_backsub: the same role code) must equal their single runs bit for bit.

What the recorded commit does against the oracle (print-out of the maker on that commit): iterations, accepted steps and termination are equal
on every problem; cameras within 4.6e-9 and points within 3.4e-7 of the oracle's.

Which way a block takes tmp3 is asserted from maker.tmp3_lds_rows(), the Python statement of bam_tmp3_lds_rows() in backend_ba.hip: the recorded
commit has no LDS path, so nothing on the device can say it there; PMV_BA_STAMPS=1 counts block 0's choice (scripts/dbg_ba_solve_stamps.py)."""
import importlib.util
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_ba_solveback_golden", os.path.join(HERE, "golden", "make_ba_solveback_golden.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)
chain = maker.chain

PROBLEMS = {p[0]: p for p in maker.problems()}
NAMES = list(PROBLEMS)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "ba_solveback_parent.npz"))
    assert len(str(g["commit"])) == 40
    return g


@pytest.fixture(scope="module", autouse=True)
def _lingering_rounds():
    """read by the batch engine when it is made (the first batch_open of this module's context): the three requests of the round below wait
    for each other"""
    old = os.environ.get("PMV_BATCH_LINGER_US")
    os.environ["PMV_BATCH_LINGER_US"] = "50000"
    yield
    if old is None:
        del os.environ["PMV_BATCH_LINGER_US"]
    else:
        os.environ["PMV_BATCH_LINGER_US"] = old


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(64, 64, n_slots=1)


@pytest.fixture(scope="module")
def oracle():
    """name -> (cams, pts, summary) of the CPU oracle, computed once"""
    with np.errstate(all="ignore"):
        return {name: chain.oracle_solve(p) for name, p in PROBLEMS.items()}


@pytest.fixture(scope="module")
def single(ctx):
    """name -> (cams, pts, summary) of the single call, computed once"""
    return {name: chain.solve(ctx, p) for name, p in PROBLEMS.items()}


def test_fixture_covers_the_problems(golden):
    assert sorted(k[:-8] for k in golden.files if k.endswith("_summary")) == sorted(NAMES)


def test_problems_take_the_paths_they_are_meant_to(golden):
    """from the shapes and the recorded summaries [initial cost, final cost, iterations, accepted steps, termination]"""
    s = {n: golden[n + "_summary"] for n in NAMES}
    dims = {n: (len(PROBLEMS[n][1]), len(PROBLEMS[n][2])) for n in NAMES}
    assert dims["nc1_np20"][0] == 1 and dims["nc2_np30"][0] == 2
    assert maker.block_rows(PROBLEMS["nc5_np64"]) == [len(PROBLEMS["nc5_np64"][4])]                      # one back-substitution block
    rows = maker.block_rows(PROBLEMS["nc5_np65"])
    assert len(rows) == 2 and dims["nc5_np65"][1] == 65 and 1 <= rows[1] <= 5                            # ... and two, the second with one point
    _, _, pts, _, ci, pi, _ = PROBLEMS["nc5_np70_dup_last_block"]
    pairs = list(zip(ci.tolist(), pi.tolist()))
    assert pairs.count((maker.DUP_CAM, maker.DUP_POINT)) == 2 and maker.DUP_POINT // maker.BM_PB == 1 and len(pts) == 70
    nc, npts = dims["nc6_np130"]
    assert ((6 * nc + 1 + 15) // 16) * ((6 * nc + 15) // 16) > 4                                          # more than 2 x 2 tiles: C, G, S|B
    # tmp3: which way each block takes it
    assert maker.tmp3_paths(PROBLEMS["nc22_np66_full"]) == ["global", "lds"] and maker.block_rows(PROBLEMS["nc22_np66_full"]) == [1408, 44]
    assert maker.tmp3_paths(PROBLEMS["nc12_np66_full"]) == ["lds", "lds"] and maker.block_rows(PROBLEMS["nc12_np66_full"]) == [768, 24]
    for n in NAMES:
        if n != "nc22_np66_full":
            assert set(maker.tmp3_paths(PROBLEMS[n])) == {"lds"}, n
    # the first step of the far start is rejected (its one-iteration twin accepts nothing), so iteration 2 re-reads the LM diagonal
    assert tuple(s["nc5_np40_far_start_it1"][2:4]) == (1, 0) and s["nc5_np40_far_start"][3] < s["nc5_np40_far_start"][2] == 5
    assert np.array_equal(PROBLEMS["nc5_np40_far_start_it1"][1], PROBLEMS["nc5_np40_far_start"][1])
    assert tuple(s["nc5_np20_degenerate_ray"][2:]) == (5, 0, 4)    # five invalid steps: every S|B launch leaves on the flag
    assert tuple(s["nc5_np30_at_the_optimum"][2:]) == (1, 0, 3)    # terminates in iteration 1: the later S|B launches find `done`
    assert len({dims[n][0] for n in maker.BATCH_ROUND}) == 3


@pytest.mark.parametrize("name", NAMES)
def test_ba_solveback_same_bits_as_recorded(ctx, golden, oracle, single, name):
    prob = PROBLEMS[name]
    cams, pts, s = single[name]
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
    # 2. the oracle, at the tolerance of test_ba_chain_gpu.py
    if np.isfinite(os_[0]):
        np.testing.assert_allclose(s[0], os_[0], rtol=1e-12)
    else:
        assert s[0] == os_[0]
    assert np.array_equal(s[2:], os_[2:]), f"iterations / accepted steps / termination {s[2:]} vs the oracle's {os_[2:]}"
    if np.isfinite(os_[1]):
        np.testing.assert_allclose(s[1], os_[1], rtol=1e-8, atol=1e-12 * os_[0])
    else:
        assert s[1] == os_[1]
    np.testing.assert_allclose(cams, oc, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(pts, op, rtol=1e-6, atol=1e-6)
    # 3. a second call on the same context
    again = chain.solve(ctx, prob)
    for a, b in zip((cams, pts, s), again):
        assert a.tobytes() == b.tobytes(), "a second call on the same context returns other bits"


def test_batched_round_of_three_equals_the_single_runs(ctx, single):
    """nc = 1, 5 and 12 in one round of the batched chain"""
    import scenes
    names = maker.BATCH_ROUND
    n = len(names)
    res, errors = [None] * n, []
    start = threading.Barrier(n)

    def run(j):
        try:
            _, cams, pts, obs, ci, pi, iters = PROBLEMS[names[j]]
            start.wait()
            c, p, s = ctx.batch_ba_solve(j, cams, pts, obs, ci, pi, scenes.K, 1.0, iters)
            res[j] = (c, p, np.array([s.initial_cost, s.final_cost, s.iterations, s.successful_steps, s.termination], np.float64))
        except Exception as e:   # noqa: BLE001 - reported by the main thread
            errors.append((j, repr(e)))

    ctx.set_ba_mode(0)
    with ctx.batch_session(n, [(64, 64)]):
        before = ctx.batch_stats()["ba"]
        th = [threading.Thread(target=run, args=(j,)) for j in range(n)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        after = ctx.batch_stats()["ba"]
    assert not errors, errors
    assert after["requests"] - before["requests"] == n and after["launches"] - before["launches"] == 1, "the three requests did not form one round"
    for j, name in enumerate(names):
        for what, a, b in zip(("cameras", "points", "summary"), res[j], single[name]):
            assert a.tobytes() == b.tobytes(), f"{name}: the batched {what} differ from the single run's bits"
