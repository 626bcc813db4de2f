"""Golden results of pmv_ba_solve (launch chain) for the problems at the edges of the solve / back-substitution launch k_bam_solveback, as
the commit named in the file computed them on an MI355X: cameras, points and the 5-slot summary, bit for bit. tests/test_ba_solveback_gpu.py
holds every later schedule of that launch to these bits. The pattern is make_ba_chain_golden.py's: recorded ONCE, on the commit BEFORE the change,
    python tests/golden/make_ba_solveback_golden.py --commit $(git rev-parse HEAD) [--out FILE]
(needs the built library, the oracle and a gfx950 device). It prints per problem what the solve did, how far it is from the CPU oracle, and
for every back-substitution block the rows of `tmp3` it holds against the rows the launch's LDS has room for.

The edges: one camera block (no look-ahead in the blocked Cholesky, the trailing part is the right-hand side alone); two (the first block is
the last but one); one and two back-substitution blocks of BM_PB = 64 points, the second with a single point; duplicate (point, camera)
records in the last block; more than 2 x 2 tiles (C, G, S|B launches); the largest system the kernel's LDS takes, where the 1408 rows of block
0 do not fit beside it and go through global memory; 768 rows that stay in LDS at nc = 12; a rejected first step (the LM diagonal is re-read);
a point block that is not positive definite (every block leaves early); termination in iteration 1 (the later S|B launches find `done`)."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ba_solveback_parent.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_ba_chain_golden as chain   # noqa: E402 - _scene, _exact_obs, solve, oracle_solve

BM_PB = 64               # points per back-substitution block (backend_ba.hip)
LDS_BYTES = 150 * 1024   # dynamic LDS a block of k_bam_solveback may ask for
DUP_POINT, DUP_CAM = 67, 1


def tmp3_lds_rows(nc, nobs):
    """rows of tmp3 (3 doubles each) that k_bam_solveback keeps in LDS: what [S (m+1) x m | dg m | candrot 16 nc] leaves of the 150 KB, at
    most one row per observation - bam_tmp3_lds_rows() of backend_ba.hip"""
    m = 6 * nc
    base = ((m + 1) * m + m + 16 * nc) * 8
    return max(0, min(nobs, (LDS_BYTES - base) // 24))


def block_rows(prob):
    """observation records per back-substitution block (block b holds the points [64 b, 64 b + 64))"""
    pts, pi = prob[2], prob[5]
    return np.bincount(np.asarray(pi) // BM_PB, minlength=(len(pts) + BM_PB - 1) // BM_PB).tolist()


def tmp3_paths(prob):
    """per block: 'lds' or 'global'"""
    cap = tmp3_lds_rows(len(prob[1]), len(prob[4]))
    return ["lds" if r <= cap else "global" for r in block_rows(prob)]


def problems():
    """[(name, cams, pts, obs, cam_idx, pt_idx, max_iterations)]"""
    out = []

    def add(name, P, iters=5, **over):
        d = dict(P)
        d.update(over)
        out.append((name, d["cams"], d["pts"], d["obs"], d["cam_idx"], d["pt_idx"], iters))

    add("nc1_np20", chain._scene(51, 1, 20, outlier_every=0))
    add("nc2_np30", chain._scene(52, 2, 30, outlier_every=0))
    add("nc5_np64", chain._scene(53, 5, 64, vis=0.8))
    add("nc5_np65", chain._scene(54, 5, 65, vis=0.8))
    P = chain._scene(55, 5, 70, vis=0.8)
    ci, pi, obs = list(P["cam_idx"]), list(P["pt_idx"]), list(P["obs"])
    if not any(c == DUP_CAM and p == DUP_POINT for c, p in zip(ci, pi)):   # the camera must see the point once before it sees it twice
        ci.append(DUP_CAM); pi.append(DUP_POINT); obs.append(np.floor(chain_project(P, DUP_CAM, DUP_POINT)))
    e = next(i for i in range(len(ci)) if ci[i] == DUP_CAM and pi[i] == DUP_POINT)
    ci.append(DUP_CAM); pi.append(DUP_POINT); obs.append(obs[e] + np.array([1.0, -2.0]))
    add("nc5_np70_dup_last_block", P, cam_idx=np.array(ci, np.int32), pt_idx=np.array(pi, np.int32), obs=np.array(obs))
    add("nc6_np130", chain._scene(56, 6, 130, vis=0.8))
    add("nc22_np66_full", chain._scene(57, 22, 66))
    add("nc12_np66_full", chain._scene(58, 12, 66))
    P = chain._scene(59, 5, 40, vis=0.8)
    rng = np.random.default_rng(591)   # (the CPU oracle rejects the first step from this start; from seed 590 it accepts it)
    far = dict(cams=P["cams"] + rng.normal(0, 0.1, P["cams"].shape), pts=P["pts"] + rng.normal(0, 8.0, P["pts"].shape))
    add("nc5_np40_far_start_it1", P, iters=1, **far)   # the same start: its one step is the five-iteration problem's first
    add("nc5_np40_far_start", P, **far)
    P = chain._scene(60, 5, 20, perturb=False)
    cams = P["cams"].copy(); pts = P["pts"].copy()
    cams[0] = 0.0
    pts[7] = [1.0, 1.0, 0.0]   # in the focal plane of camera 0: the point's 3x3 block is not positive definite
    add("nc5_np20_degenerate_ray", P, cams=cams, pts=pts)
    P = chain._scene(61, 5, 30, vis=0.8, noise=0.0, outlier_every=0, perturb=False)
    add("nc5_np30_at_the_optimum", P, obs=chain._exact_obs(P))
    return out


def chain_project(P, c, p):
    import scenes
    return scenes.project_ref(P["cams_true"][c], P["pts_true"][p])


BATCH_ROUND = ("nc1_np20", "nc5_np65", "nc12_np66_full")   # three problems of different nc in one batched round

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--oracle-only", action="store_true", help="print what the CPU oracle does on each problem; needs no device, writes nothing")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    ctx = None
    if not a.oracle_only:
        pmv = importlib.import_module("practical-multi-view_amd")
        ctx = pmv.Context(64, 64, n_slots=1)
    rec = {"commit": np.array(a.commit)}
    for prob in problems():
        name = prob[0]
        with np.errstate(all="ignore"):
            oc, op, os_ = chain.oracle_solve(prob)
        cap = tmp3_lds_rows(len(prob[1]), len(prob[4]))
        where = f"tmp3 rows per block {block_rows(prob)} against {cap} in LDS: {tmp3_paths(prob)}"
        if ctx is None:
            print(f"{name}: nobs {len(prob[4])}, oracle summary {os_.tolist()}; {where}")
            continue
        c, p, s = chain.solve(ctx, prob)
        rec[name + "_cams"], rec[name + "_pts"], rec[name + "_summary"] = c, p, s
        with np.errstate(all="ignore"):
            print(f"{name}: nobs {len(prob[4])}, cost {s[0]:.6g} -> {s[1]:.6g}, iterations {int(s[2])}, accepted {int(s[3])}, termination {int(s[4])}; "
                  f"oracle: iterations/accepted/termination {'equal' if np.array_equal(s[2:], os_[2:]) else 'DIFFERENT ' + str(os_[2:])}, "
                  f"cost rel {abs(s[1] - os_[1]) / max(abs(os_[1]), 1e-300):.3g}, |cams - oracle| {np.abs(c - oc).max():.3g}, "
                  f"|pts - oracle| {np.abs(p - op).max():.3g}; {where}")
    if ctx is not None:
        ctx.close()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        np.savez_compressed(a.out, **rec)
        print("->", a.out, os.path.getsize(a.out), "bytes")
