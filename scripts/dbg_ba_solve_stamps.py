"""Phase timers (shader clock) of the S|B launch k_bam_solveback, block 0, per LM iteration:
  solve role   prologue (state trip, loop-top tests) / assemble (S from Ublk, Gpart, diag) / cholesky / backward substitution / candidate cameras
  backsub role phase A (Jp^T Jc y_c per observation) / phase B (point steps) / phase C (cost terms, candidate r and J) / reduce
and of the point role of the launch before it.   python scripts/dbg_ba_solve_stamps.py [--json FILE] [--label NAME]"""
import sys, os, importlib, json, ctypes as C, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
os.environ["PMV_BA_STAMPS"] = "1"
import scenes
pmv = importlib.import_module("practical-multi-view_amd")
ctx = pmv.Context(64, 64, n_slots=1)
solve_names = ["prologue", "assemble", "cholesky", "backward", "candrot"]      # stamps 16..20
back_names = ["phaseA", "phaseB", "phaseC", "reduce"]                          # stamps 10..13
point_names = ["phase1", "wait", "rescale_first", "phase2"]                    # stamps 4..7
# stamps 21..23: parts carved out of the phases above (the phase's own figure is what is left of it: add them for the phase total);
# 24, 25: counters
detail_names = ["state_trip(of prologue)", "chol_first_factor+panels(of cholesky)", "chol_lookahead_factor|trailing(of cholesky)",
                "launches_with_a_valid_step", "of_them_tmp3_in_LDS"]
rows = []
for nc, npts in ((5, 400), (5, 600), (10, 1000), (20, 1500)):
    P = scenes.ba_problem(4, nc=nc, npts=npts)
    st0 = np.zeros(32, np.uint64)
    ctx.lib.pmv_debug_ba_stamps(ctx.h, st0.ctypes.data_as(C.POINTER(C.c_uint64)))
    _, _, s = ctx.ba_solve(P["cams"], P["pts"], P["obs"], P["cam_idx"], P["pt_idx"], scenes.K, 1.0, 5)
    st = np.zeros(32, np.uint64)
    ctx.lib.pmv_debug_ba_stamps(ctx.h, st.ctypes.data_as(C.POINTER(C.c_uint64)))
    it = max(1, s.iterations)
    d = [(int(st[16 + i]) - int(st0[16 + i])) / it for i in range(5)]
    db = [(int(st[10 + i]) - int(st0[10 + i])) / it for i in range(4)]
    dp = [(int(st[4 + i]) - int(st0[4 + i])) / it for i in range(4)]
    print("nc", nc, "np", P["pts"].shape[0], "nobs", len(P["cam_idx"]), "iterations", s.iterations, "(cycles per iteration, shader clock)")
    print("   solve role (block 0):  ", " ".join("%s=%d" % (n, v) for n, v in zip(solve_names, d)), " sum=%d" % sum(d))
    print("   backsub role (block 0):", " ".join("%s=%d" % (n, v) for n, v in zip(back_names, db)), " sum=%d" % sum(db))
    print("   point role (block 0):  ", " ".join("%s=%d" % (n, v) for n, v in zip(point_names, dp)))
    dx = [(int(st[21 + i]) - int(st0[21 + i])) / it for i in range(5)]
    print("   detail (where the build stamps them): ", " ".join("%s=%d" % (n, v) for n, v in zip(detail_names, dx)))
    rows.append({"nc": nc, "np": int(P["pts"].shape[0]), "nobs": int(len(P["cam_idx"])), "iterations": int(s.iterations),
                 "solve": dict(zip(solve_names, [round(v) for v in d])), "backsub": dict(zip(back_names, [round(v) for v in db])),
                 "detail": dict(zip(detail_names, [round(v) for v in dx])), "solveback_sum": round(sum(d) + sum(db) + sum(dx[:3]))})
if "--json" in sys.argv:
    out = sys.argv[sys.argv.index("--json") + 1]
    label = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else "run"
    os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump({"label": label, "unit": "shader-clock cycles per LM iteration, block 0", "shapes": rows}, f, indent=1)
ctx.close()
