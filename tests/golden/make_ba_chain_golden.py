"""Golden results of the bundle-adjustment launch chain (pmv_ba_solve, multi-kernel form) as the commit named in the file computed them on
an MI355X: for each problem of problems() the cameras, the points and the 5-slot summary, bit for bit. tests/test_ba_chain_gpu.py holds
every later form of the chain to these bits.

The file is recorded ONCE, on the commit BEFORE a change to the chain, and is not re-recorded with the change:
    python tests/golden/make_ba_chain_golden.py --commit $(git rev-parse HEAD) [--out FILE]
(needs the built library, the oracle and a gfx950 device; the commit id is passed in because the tree may be run from a copy without .git).
It also prints, per problem, what the solve did (iterations, accepted steps, termination) and how far it is from the CPU oracle - what the
test's docstring says about the recorded commit comes from that print-out."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ba_chain_parent.npz")

# The Schur product cuts K = round_up(3 np, 16) rows into slices of kper = round_up(ceil(K / 8), 16) rows: a point straddles a slice
# boundary when 3 p < s kper < 3 p + 3.  np = 60: K = 192, kper = 32, 6 slices, point 10 holds rows 30..32 and straddles row 32.
STRADDLER = 10   # of the np = 60 problems


def _scene(seed, nc, npts, **kw):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scenes
    kw.setdefault("vis", 1.0)
    for k in range(50):   # (ba_problem drops a point that no camera happens to see: take the first seed that keeps them all)
        P = scenes.ba_problem(seed + 1000 * k, nc=nc, npts=npts, **kw)
        if P["pts"].shape[0] == npts:
            return P
    raise AssertionError("no seed keeps every point")


def _exact_obs(P):
    import scenes
    return np.array([scenes.project_ref(P["cams_true"][c], P["pts_true"][p]) for c, p in zip(P["cam_idx"], P["pt_idx"])])


def problems():
    """[(name, cams, pts, obs, cam_idx, pt_idx, max_iterations)] at the structural edges of the chain"""
    out = []

    def add(name, P, iters=5, **over):
        d = dict(P)
        d.update(over)
        out.append((name, d["cams"], d["pts"], d["obs"], d["cam_idx"], d["pt_idx"], iters))

    add("nc1_np1", _scene(31, 1, 1, outlier_every=0))                       # smallest problem
    add("nc2_np5", _scene(32, 2, 5, outlier_every=0))                       # one slice, one tile row
    add("nc5_np16", _scene(33, 5, 16))                                      # 3 np = 48: a multiple of 16
    add("nc5_np17", _scene(34, 5, 17))                                      # ... and not
    add("nc5_np60", _scene(35, 5, 60, vis=0.8))                             # 6 slices, point 10 straddles rows 30..32
    add("nc5_np390", _scene(36, 5, 390, vis=0.8))                           # the metric shape: 8 slices, the last one short
    P = _scene(37, 5, 60)
    # duplicate (point, camera) observations on the straddling point: camera 1 sees it three times, camera 3 twice
    rng = np.random.default_rng(370)
    ci, pi, obs = list(P["cam_idx"]), list(P["pt_idx"]), list(P["obs"])
    for c in (1, 3, 1):
        e = next(i for i in range(len(ci)) if ci[i] == c and pi[i] == STRADDLER)
        ci.append(c); pi.append(STRADDLER); obs.append(obs[e] + np.floor(rng.normal(0, 1.5, 2)))
    add("nc5_np60_dup_straddle", P, cam_idx=np.array(ci, np.int32), pt_idx=np.array(pi, np.int32), obs=np.array(obs))
    P = _scene(38, 5, 60)
    keep = ~((P["cam_idx"] == 2) & (P["pt_idx"] < 22))                       # camera 2 sees no point of slices 0 and 1 (rows 0..63)
    add("nc5_np60_cam_blind_in_slice", P, cam_idx=P["cam_idx"][keep], pt_idx=P["pt_idx"][keep], obs=P["obs"][keep])
    P = _scene(39, 5, 120, vis=0.8)
    rng = np.random.default_rng(390)
    add("nc5_np120_far_start", P, cams=P["cams"] + rng.normal(0, 0.1, P["cams"].shape), pts=P["pts"] + rng.normal(0, 8.0, P["pts"].shape))   # 2 of 5 steps rejected
    # point 7 lies in the focal plane of camera 0 (identity rotation, zero translation): its ray is degenerate, the point's 3x3 block is not
    # positive definite, every step is invalid
    P = _scene(40, 5, 40, perturb=False)
    cams = P["cams"].copy(); pts = P["pts"].copy()
    cams[0] = 0.0
    pts[7] = [1.0, 1.0, 0.0]
    add("nc5_np40_degenerate_ray", P, cams=cams, pts=pts)
    P = _scene(41, 5, 100, vis=0.8, noise=0.0, outlier_every=0)
    add("nc5_np100_noiseless", P, iters=50, obs=_exact_obs(P))               # early termination
    P = _scene(42, 5, 100, vis=0.8, noise=0.0, outlier_every=0, perturb=False)
    add("nc5_np100_at_the_optimum", P, obs=_exact_obs(P))                    # terminates on the gradient in the first iteration
    P = _scene(43, 5, 100, vis=0.8)
    add("nc5_np100_it1", P, iters=1)
    add("nc5_np100_it50", P, iters=50)
    add("nc6_np80", _scene(44, 6, 80, vis=0.8))                             # 3 x 3 tiles
    add("nc3_np200", _scene(45, 3, 200, vis=0.8))                           # 2 x 2 tiles
    for npts in (700, 760, 800, 1000):                                      # around and above the largest K-slice that fits a block's LDS
        add(f"nc5_np{npts}", _scene(46, 5, npts, vis=0.8))
    add("nc10_np300", _scene(47, 10, 300, vis=0.6))
    return out


def solve(ctx, prob):
    import scenes
    _, cams, pts, obs, ci, pi, iters = prob
    c, p, s = ctx.ba_solve(cams, pts, obs, ci, pi, scenes.K, 1.0, iters)
    return c, p, np.array([s.initial_cost, s.final_cost, s.iterations, s.successful_steps, s.termination], np.float64)


def oracle_solve(prob):
    import orc_binding as ob
    import scenes
    _, cams, pts, obs, ci, pi, iters = prob
    c, p, s = ob.ba_solve(cams, pts, obs, ci, pi, scenes.K, 1.0, iters)
    return c, p, np.array([s["initial_cost"], s["final_cost"], s["iterations"], s["successful_steps"], s["termination"]], np.float64)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    pmv = importlib.import_module("practical-multi-view_amd")
    ctx = pmv.Context(64, 64, n_slots=1)
    rec = {"commit": np.array(a.commit)}
    for prob in problems():
        name = prob[0]
        c, p, s = solve(ctx, prob)
        rec[name + "_cams"], rec[name + "_pts"], rec[name + "_summary"] = c, p, s
        oc, op, os_ = oracle_solve(prob)
        with np.errstate(all="ignore"):
            print(f"{name}: nobs {len(prob[4])}, cost {s[0]:.6g} -> {s[1]:.6g}, iterations {int(s[2])}, accepted {int(s[3])}, termination {int(s[4])}; "
                  f"oracle: iterations/accepted/termination {'equal' if np.array_equal(s[2:], os_[2:]) else 'DIFFERENT ' + str(os_[2:])}, "
                  f"cost rel {abs(s[1] - os_[1]) / max(abs(os_[1]), 1e-300):.3g}, |cams - oracle| {np.abs(c - oc).max():.3g}, "
                  f"|pts - oracle| {np.abs(p - op).max():.3g}")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print("->", a.out, os.path.getsize(a.out), "bytes")
