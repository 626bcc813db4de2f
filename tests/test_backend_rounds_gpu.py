"""The batched forms of the back-end solvers in rounds of DIFFERENT problems: the edge problems of tests/golden/make_ba_chain_golden.py and
make_pnp_chain_golden.py, which tests/test_ba_chain_gpu.py and tests/test_pnp_chain_gpu.py run through the single calls only, and DLT
problems of unequal n, eight to a round of the batch engine (tests/backend_rounds_common.py holds the plans, tests/test_backend_rounds_plan.py
shows on the CPU what each plan reaches).

 * pmv_batch_ba_solve, launch chain (k_bamB_*): cameras, points and summary of every problem of every round equal the bits recorded in
   tests/golden/ba_chain_parent.npz - the rounds have one iteration cap and eight shapes (the maxima of the launch grids come from
   different problems), three caps (three chains on one record array), a small problem after a large one on every sequence's workspaces,
   and two of them run again with the sequences in the opposite order;
 * pmv_set_ba_mode(1), one workgroup per solve: the single call (k_ba_lm) against the CPU oracle at the bars of test_ba_chain_gpu.py's
   section 2, on all 21 problems - K-slice settings 8, 2 and 1, where every earlier test had nc = 5 and so 2 - and the batched form
   (k_ba_lm_batch) bit for bit against the single call;
 * pmv_batch_pnp_ransac: the recorded bits of tests/golden/pnp_chain_parent.npz at the default arguments; rounds of different iteration
   counts (1, 8, 16, 17, 100, 1024: both sides of the split of the hypotheses into two launches), confidences and thresholds against the
   single call bit for bit and against the oracle as test_capacity_edge_gpu.py::test_pnp_ransac compares;
 * pmv_batch_triangulate_candidates: n = 1 .. 1500 in one round, bit-equal to the single call and to the oracle.

A round is made to form as in tests/test_capacity_edge_gpu.py: the engine of this module's context is created under
PMV_BATCH_LINGER_US = 50 ms, the eight threads of a volley start behind a barrier, and pmv_batch_stats must show that the class served the
eight requests in exactly one round - a volley that split says nothing about mixed rounds and fails with that message.

Relaxed problems of the one-workgroup mode (RELAXED below): none."""
import os
import threading

import numpy as np
import pytest

import backend_rounds_common as rc
import orc_binding as ob
import scenes

pytestmark = pytest.mark.gpu

N = rc.N_SEQ
SIZE = (64, 64)
BA_NAMES = sorted(set().union(*rc.BA_VOLLEYS.values()))
# name -> evidence: a problem of the one-workgroup mode held to "iterations equal, cost level rtol 1e-3" only, because the oracle's own
# numbers show an accept / reject decision within rounding of its threshold. At most two, none of rc.BA_NEVER_RELAXED.
RELAXED = {}
_state = {}


@pytest.fixture(scope="module", autouse=True)
def _lingering_rounds():
    """read by the engine when it is made (the first batch_open of this module's context)"""
    old = os.environ.get("PMV_BATCH_LINGER_US")
    os.environ["PMV_BATCH_LINGER_US"] = "50000"
    yield
    if old is None:
        del os.environ["PMV_BATCH_LINGER_US"]
    else:
        os.environ["PMV_BATCH_LINGER_US"] = old


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(*SIZE, n_slots=1, max_tracks=4096)


@pytest.fixture(scope="module")
def ba_golden():
    g = np.load(os.path.join(rc.HERE, "golden", "ba_chain_parent.npz"))
    assert len(str(g["commit"])) == 40
    return g


@pytest.fixture(scope="module")
def pnp_golden():
    g = np.load(os.path.join(rc.HERE, "golden", "pnp_chain_parent.npz"))
    assert len(str(g["commit"])) == 40
    return g


@pytest.fixture(scope="module")
def ba_oracle():
    """name -> (cams, pts, summary) of the CPU oracle, computed once"""
    with np.errstate(all="ignore"):
        return {name: rc.ba_maker.oracle_solve(p) for name, p in rc.ba_problems().items()}


def _threads(fn):
    res, errors = [None] * N, []
    start = threading.Barrier(N)

    def run(j):
        try:
            start.wait()
            res[j] = fn(j)
        except Exception as e:   # noqa: BLE001 - reported by the main thread
            errors.append((j, repr(e)))
    th = [threading.Thread(target=run, args=(j,)) for j in range(N)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    return res


def _volley(ctx, role, fn, what):
    """fn(seq) from N threads at once; the class `role` of the engine must have served exactly these N requests, in ONE round"""
    before = ctx.batch_stats()[role]
    res = _threads(fn)
    after = ctx.batch_stats()[role]
    rounds, requests = after["launches"] - before["launches"], after["requests"] - before["requests"]
    assert requests == N, f"{what}: the {role} class served {requests} requests, not the volley's {N}"
    assert rounds == 1, f"{what}: the volley split into {rounds} rounds - it shows nothing about a round of {N} different problems"
    return res


# ---- BA ------------------------------------------------------------------------------------------------------------------------------
def _summary(s):
    return np.array([s.initial_cost, s.final_cost, s.iterations, s.successful_steps, s.termination], np.float64)


def _all_ba_problems():
    return {**rc.ba_problems(), **rc.ba_eight_slice_problems()}


def _batch_ba(ctx, seq, prob):
    _, cams, pts, obs, ci, pi, iters = prob
    c, p, s = ctx.batch_ba_solve(seq, cams, pts, obs, ci, pi, scenes.K, 1.0, iters)
    return c, p, _summary(s)


def _differences(got, want, what, whose):
    """the comparison of test_ba_chain_same_bits_as_recorded, as a list of messages"""
    (cams, pts, s), (wc, wp, ws) = got, want
    out = []
    if s.tobytes() != ws.tobytes():
        out.append(f"{what}: summary {s} differs from {whose} {ws}")
    bad = np.nonzero((cams.view(np.uint64) != wc.view(np.uint64)).any(1))[0]
    if bad.size:
        out.append(f"{what}: cameras {bad.tolist()} differ from {whose} bits")
    bad = np.nonzero((pts.view(np.uint64) != wp.view(np.uint64)).any(1))[0]
    if bad.size:
        out.append(f"{what}: {bad.size} points (first {bad[:8].tolist()}) differ from {whose} bits")
    return out


def _recorded(golden, name):
    return golden[name + "_cams"], golden[name + "_pts"], golden[name + "_summary"]


def _ba_volleys(ctx, run, want, whose, volleys=rc.BA_VOLLEYS):
    """the volleys named in `run`, in that order, in one session; want(name) -> (cams, pts, summary)"""
    wrong = []
    problems = _all_ba_problems()   # made before the threads start: a thread that builds its problem behind the barrier arrives late
    with ctx.batch_session(N, [SIZE]):
        for vname in run:
            names = volleys[vname]
            got = _volley(ctx, "ba", lambda j: _batch_ba(ctx, j, problems[names[j]]), f"BA volley '{vname}'")
            diff = [d for j, name in enumerate(names) for d in _differences(got[j], want(name), f"volley '{vname}', seq {j}, {name}", whose)]
            print(f"BA volley '{vname}': one round of {N}; {rc.describe(names) if volleys is rc.BA_VOLLEYS else names}; {len(diff)} differences")
            wrong += diff
    return wrong


def test_ba_chain_rounds_same_bits_as_recorded(ctx, ba_golden):
    """k_bamB_*: 40 solves in five rounds, every one equal to the recorded bits of its problem"""
    ctx.set_ba_mode(0)
    wrong = _ba_volleys(ctx, rc.BA_RUN, lambda name: _recorded(ba_golden, name), "the recorded")
    assert not wrong, "\n".join(wrong)


def _one_workgroup_single(ctx, name):
    """the single call in mode 1 (k_ba_lm), once per problem; called with the mode set and no session open"""
    key = ("single1", name)
    if key not in _state:
        c, p, s = rc.ba_maker.solve(ctx, _all_ba_problems()[name])
        again = rc.ba_maker.solve(ctx, _all_ba_problems()[name])
        assert all(a.tobytes() == b.tobytes() for a, b in zip((c, p, s), again)), f"{name}: a second call in mode 1 returns other bits"
        _state[key] = (c, p, s)
    return _state[key]


def _distances(got, oracle):
    (cams, pts, s), (oc, op, os_) = got, oracle
    with np.errstate(all="ignore"):
        return (f"summary {s.tolist()} oracle {os_.tolist()}; cost rel {abs(s[1] - os_[1]) / max(abs(os_[1]), 1e-300):.3g}, "
                f"|cams - oracle| {np.abs(cams - oc).max():.3g} |pts - oracle| {np.abs(pts - op).max():.3g}")


@pytest.mark.parametrize("name", BA_NAMES)
def test_ba_one_workgroup_single_call_meets_the_oracle_bars(ctx, ba_oracle, name):
    """k_ba_lm against the CPU oracle, at the bars of test_ba_chain_gpu.py's section 2 (see that module's docstring)"""
    assert len(RELAXED) <= 2 and not set(RELAXED) & set(rc.BA_NEVER_RELAXED)
    prob = rc.ba_problems()[name]
    d = rc.ba_dims(prob)
    ctx.set_ba_mode(1)
    try:
        cams, pts, s = _one_workgroup_single(ctx, name)
    finally:
        ctx.set_ba_mode(0)
    oc, op, os_ = ba_oracle[name]
    print(f"{name}: ks {d['ks_mode1']} ({d['kslices_mode1']} slices of {d['krows']} rows, {d['tiles']} tiles); {_distances((cams, pts, s), ba_oracle[name])}")
    if np.isfinite(os_[0]):
        np.testing.assert_allclose(s[0], os_[0], rtol=1e-12)
    else:
        assert s[0] == os_[0]
    if prob[6] > 5 or name in RELAXED:
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


def test_ba_one_workgroup_rounds_equal_the_single_call(ctx, ba_golden, ba_oracle):
    """k_ba_lm_batch: the same five rounds in mode 1, every solve equal to the single call's bits in that mode (the same body; LDS sized by
    the round's largest m); back in mode 0 the round of eight shapes returns the recorded bits again"""
    ctx.set_ba_mode(1)
    try:
        for name in BA_NAMES:
            _one_workgroup_single(ctx, name)
        wrong = _ba_volleys(ctx, rc.BA_RUN, lambda name: _state[("single1", name)], "the single call's")
    finally:
        ctx.set_ba_mode(0)
    for name in BA_NAMES:
        print(f"{name}: {_distances(_state[('single1', name)], ba_oracle[name])}")
    assert not wrong, "\n".join(wrong)
    wrong = _ba_volleys(ctx, ["shapes"], lambda name: _recorded(ba_golden, name), "the recorded")
    assert not wrong, "after mode 1:\n" + "\n".join(wrong)


def test_ba_one_workgroup_eight_slices(ctx):
    """ks = 8 with more rows than one slice holds (the golden problems of one and two cameras have 16 rows): two problems of two cameras,
    seven slices with a short last one and eight full ones - the single call against the oracle at the same bars, then in a round with
    ks = 1 and ks = 2 problems against the single call's bits"""
    extra = rc.ba_eight_slice_problems()
    ctx.set_ba_mode(1)
    try:
        for name in rc.BA_EIGHT_SLICES_VOLLEY:
            _one_workgroup_single(ctx, name)
        wrong = _ba_volleys(ctx, ["eight_slices"], lambda name: _state[("single1", name)], "the single call's", {"eight_slices": rc.BA_EIGHT_SLICES_VOLLEY})
    finally:
        ctx.set_ba_mode(0)
    assert not wrong, "\n".join(wrong)
    for name, prob in extra.items():
        cams, pts, s = _state[("single1", name)]
        with np.errstate(all="ignore"):
            oracle = rc.ba_maker.oracle_solve(prob)
        d = rc.ba_dims(prob)
        print(f"{name}: ks {d['ks_mode1']} ({d['kslices_mode1']} slices of {d['krows']} rows, {d['tiles']} tiles); {_distances((cams, pts, s), oracle)}")
        oc, op, os_ = oracle
        np.testing.assert_allclose(s[0], os_[0], rtol=1e-12)
        assert np.array_equal(s[2:], os_[2:]), f"iterations / accepted steps / termination {s[2:]} vs the oracle's {os_[2:]}"
        np.testing.assert_allclose(s[1], os_[1], rtol=1e-8, atol=1e-12 * os_[0])
        np.testing.assert_allclose(cams, oc, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(pts, op, rtol=1e-6, atol=1e-6)


# ---- PnP -----------------------------------------------------------------------------------------------------------------------------
def _pnp_args(req):
    name, iterations, reproj_err, confidence = req
    obj, img, gr, gt = rc.pnp_problems()[name]
    return (obj, img, scenes.K, gr, gt), dict(iterations=iterations, reproj_err=reproj_err, confidence=confidence)


def _pnp_volley(ctx, vname, volley):
    args = [_pnp_args(req) for req in volley]   # (before the threads start, as the BA problems)
    got = _volley(ctx, "pnp", lambda j: ctx.batch_pnp_ransac(j, *args[j][0], **args[j][1]), f"PnP volley '{vname}'")
    print(f"PnP volley '{vname}': one round of {N}; iterations {[r[1] for r in volley]} (split at {rc.kernel_constants()['PNP_H0']}), "
          f"inliers {[len(g[2]) for g in got]}")
    return got


def _same_pose_bits(got, want, what, whose):
    (rv, tv, inl), (wr, wt, winl) = got, want
    assert np.array_equal(inl, winl), f"{what}: inlier list differs from {whose}"
    assert np.array_equal(rv.view(np.uint64), np.asarray(wr).view(np.uint64)), f"{what}: rvec {rv} vs {whose} {wr}"
    assert np.array_equal(tv.view(np.uint64), np.asarray(wt).view(np.uint64)), f"{what}: tvec {tv} vs {whose} {wt}"


@pytest.mark.parametrize("vname", list(rc.PNP_GOLDEN_VOLLEYS))
def test_pnp_rounds_same_bits_as_recorded(ctx, pnp_golden, vname):
    """the nine golden problems at the default arguments, eight different ones in one round and the ninth among repeats in another: early
    RANSAC exit after one hypothesis, none at all, more than 512 inliers, and the no-model pose (hypothesis 99, from the second launch)"""
    volley = rc.PNP_GOLDEN_VOLLEYS[vname]
    with ctx.batch_session(N, [SIZE]):
        got = _pnp_volley(ctx, vname, volley)
    for j, (name, *_) in enumerate(volley):
        _same_pose_bits(got[j], (pnp_golden[name + "_rvec"], pnp_golden[name + "_tvec"], pnp_golden[name + "_inliers"]), f"seq {j}, {name}", "the recorded")
    assert len(got[[r[0] for r in volley].index(rc.PNP_NO_MODEL)][2]) == 0


@pytest.mark.parametrize("vname", list(rc.PNP_MIXED_VOLLEYS))
def test_pnp_round_of_mixed_arguments(ctx, vname):
    """different iteration counts, confidences and thresholds in one round: each request equals the single call at its arguments bit for bit,
    and the oracle as test_capacity_edge_gpu.py::test_pnp_ransac compares (no model: the oracle's last hypothesis, as test_pnp_chain_gpu.py)"""
    volley = rc.PNP_MIXED_VOLLEYS[vname]
    single = []
    for req in volley:
        a, kw = _pnp_args(req)
        single.append(ctx.pnp_ransac(*a, **kw))
    with ctx.batch_session(N, [SIZE]):
        got = _pnp_volley(ctx, vname, volley)
    for j, req in enumerate(volley):
        _same_pose_bits(got[j], single[j], f"seq {j}, {req}", "the single call's")
    for j, req in enumerate(volley):
        (obj, img, K, gr, gt), kw = _pnp_args(req)
        orv, otv, oinl, used = ob.pnp_ransac(obj, img, K, gr, gt, **kw)
        rv, tv, inl = got[j]
        if req[0] == rc.PNP_NO_MODEL:
            assert len(oinl) == 0, f"{req}: the oracle finds a model"
            models, _ = ob.pnp_hypotheses(obj, img, K, req[1], req[2])
            orv, otv = models[req[1] - 1, :3], models[req[1] - 1, 3:]
        print(f"seq {j}, {req}: {len(oinl)} inliers and {used} hypotheses in the oracle, {len(inl)} inliers on the device, "
              f"pose - oracle {max(np.abs(rv - orv).max(), np.abs(tv - otv).max()):.3g}")
        assert np.array_equal(inl, oinl), f"seq {j}, {req}: inlier index list differs from the oracle's"
        np.testing.assert_allclose(rv, orv, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(tv, otv, rtol=1e-6, atol=1e-8)


# ---- DLT -----------------------------------------------------------------------------------------------------------------------------
def test_dlt_round_of_unequal_n(ctx):
    """launch_tri_dlt_batch takes its grid from the round's largest n: n = 1, 63, 64, 65, 400, 1500 and two repeats in one round, each bit-equal
    to the single call and to the oracle (the rule of test_triangulate_candidates_bit_exact)"""
    probs = [scenes.two_view_problem(seed, n=n) for seed, n in rc.DLT_VOLLEY]
    args = [(P["q1"], P["q2"], P["P1x4"], P["mask"]) for P in probs]
    single = [ctx.triangulate_candidates(*a) for a in args]
    with ctx.batch_session(N, [SIZE]):
        got = _volley(ctx, "dlt", lambda j: ctx.batch_triangulate_candidates(j, *args[j]), "DLT volley")
    print(f"DLT volley: one round of {N}; n {[n for _, n in rc.DLT_VOLLEY]}; good {[g[2].tolist() for g in got]}")
    for j, a in enumerate(args):
        want = ob.triangulate_candidates(*a)
        for k, what in enumerate(("Q", "mask", "good")):
            assert got[j][k].shape == single[j][k].shape and got[j][k].tobytes() == single[j][k].tobytes(), f"seq {j}, n = {rc.DLT_VOLLEY[j][1]}: {what} differs from the single call's"
            assert np.array_equal(got[j][k], want[k]), f"seq {j}, n = {rc.DLT_VOLLEY[j][1]}: {what} differs from the oracle's"
