"""Golden results of the PnP chain (k_pnp_hyp + k_pnp_select_refit) as the commit named in the file computed them on an MI355X:
for each problem of problems() the pose and inlier list of Context.pnp_ransac and the 100 hypothesis models and inlier counts behind it,
bit for bit. tests/test_pnp_chain_gpu.py holds every later form of the two kernels to these bits.

The file is recorded ONCE, on the commit BEFORE a change to the kernels, and is not re-recorded with the change:
    python tests/golden/make_pnp_chain_golden.py --commit $(git rev-parse HEAD) [--out FILE]
(needs the built library, the oracle and a gfx950 device; the commit id is passed in because the tree may be run from a copy without .git).
It also prints, per problem, whether the hypotheses are bit-equal to the CPU oracle's and how far the pose is from the oracle's - the
lists ORACLE_BITEQUAL_HYP of the test come from that print-out."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pnp_chain_parent.npz")

# (seed, m, outlier_frac, noise) of scenes.pnp_problem, and what each exercises (behaviour of the CPU oracle)
SEEDED = [
    (26, 6, 0.0, 0.5),     # smallest legal m; RANSAC stops after 1 hypothesis; 2 rejected LM steps
    (24, 12, 0.0, 0.5),    # 5 rejected steps on 12 inliers
    (22, 40, 0.0, 0.0),    # noiseless; no rejected step; shortest LM
    (12, 64, 0.2, 0.5),    # one full wavefront of points; 11 hypotheses used
    (13, 65, 0.3, 0.5),    # 65 points; all 100 hypotheses used, refit starts from hypothesis 99
    (4, 217, 0.02, 0.3),   # the workload's size; 10 rejected steps
    (25, 300, 0.5, 0.5),   # no early RANSAC exit; LM runs into the 20-iteration cap with 22 rejects
    (21, 700, 0.05, 0.5),  # 662 inliers (> 512): the third-point-per-thread path of the refit
]
N_HYP = 100


def problems():
    """[(name, obj, img, rvec_guess, tvec_guess)]: the seeded problems, then the all-outlier one (no model with more than 4 inliers)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scenes
    out = []
    for seed, m, frac, noise in SEEDED:
        P = scenes.pnp_problem(seed, m=m, outlier_frac=frac, noise=noise)
        out.append((f"s{seed}_m{m}", P["obj"], P["img"], np.array([0.3, -0.2, 0.1]), np.array([1.0, 2.0, -30.0])))
    rng = np.random.default_rng(0)
    obj = rng.uniform(-5, 5, (50, 3)).astype(np.float32) + [0, 0, 20]
    img = rng.uniform(0, 1200, (50, 2)).astype(np.float32)
    out.append(("all_outliers_m50", obj.astype(np.float32), img, np.zeros(3), np.zeros(3)))
    return out


def solve(ctx, obj, img, K, gr, gt):
    rv, tv, inl = ctx.pnp_ransac(obj, img, K, gr, gt)
    models, counts = ctx.pnp_hypotheses(N_HYP)
    return rv, tv, inl, models, counts


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orc_binding as ob
    import scenes
    pmv = importlib.import_module("practical-multi-view_amd")
    ctx = pmv.Context(64, 64, n_slots=1)
    rec = {"commit": np.array(a.commit)}
    for name, obj, img, gr, gt in problems():
        rv, tv, inl, models, counts = solve(ctx, obj, img, scenes.K, gr, gt)
        rec[name + "_rvec"], rec[name + "_tvec"], rec[name + "_inliers"] = rv, tv, inl
        rec[name + "_models"], rec[name + "_counts"] = models, counts
        om, oc = ob.pnp_hypotheses(obj, img, scenes.K, N_HYP)
        orv, otv, oinl, used = ob.pnp_ransac(obj, img, scenes.K, gr, gt)
        dm = np.abs(models - om)
        print(f"{name}: {len(inl)} inliers ({'equal to' if np.array_equal(inl, oinl) else 'DIFFERENT from'} the oracle's), oracle used {used} hypotheses; "
              f"models bit-equal to the oracle {np.array_equal(models, om)} ({int((models != om).any(1).sum())} rows differ, worst {np.nanmax(dm):.3g}), "
              f"counts equal {np.array_equal(counts, oc)}; pose - oracle: {max(np.abs(rv - orv).max(), np.abs(tv - otv).max()):.3g}, finite {np.isfinite(models).all()}")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print("->", a.out, os.path.getsize(a.out), "bytes")
