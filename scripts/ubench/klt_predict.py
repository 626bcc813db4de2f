"""What a prediction saves in the tracker step (pmv_klt_set_prediction: LK from projected guesses on capped pyramid levels): path PLAIN is
pmv_klt_step, path PRED pmv_klt_set_prediction(top_level 1, back_top_level 1, min_succ 10) followed by the step, with a point for every
track that PLAIN's own step tracks, projected to within 1.5 px of where PLAIN finds it; path FALLBACK is the same with every point far
outside the frame - the wasted predicted pass, the gate and the full pass. One line per case and one JSON line at the end (kept as
profiles/klt_predict_ubench.json; --out names the file).

Frames 1241x376 and 752x480 (synthetic, consecutive), target 150 (radius = min_dist = 30) and 1000 (radius = min_dist = 10), rejectWithF on,
forward-backward 0.5 px, border 1, under the LK settings (win 21, max_level 3) and (32, 4); the camera is the scene's pinhole with k1 = -0.1
and 20 iterations. A PLAIN pass from an empty list over the frames gives the states; every timed step of every path then starts from
PLAIN's state in front of that frame (pmv_klt_set_tracks, not timed), so the three paths track the same list. Before anything is timed, a
FALLBACK step with back_top_level -1 must return PLAIN's bytes for every frame, and PRED must consume its prediction without falling back.
Each figure is the median over `--repeats` passes of the per-step host clock around the calls (every path ends in its waits), with the
smallest and the largest step. The paths alternate pass by pass and the order flips from repeat to repeat. The profiler is off. All paths
run through the Python binding. The LK work of stage 1 is read from pmv_lk_counters around pmv_lk_track_fb_levels on the same inputs (the
step's own launches do not count): iterations and (track, level) passes per track, plain and predicted.

Without --case the script only starts one child process per frame size, each under a time limit of its own, one after the other; the first
child that fails or runs out of time ends the script with its status, and nothing more is started.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = [(1241, 376), (752, 480)]
TARGETS = [(150, 30), (1000, 10)]   # (target, radius = min_dist)
LKS = [(21, 3), (32, 4)]
SETTING = dict(top_level=1, back_top_level=1, min_succ=10)
FAR = (3.0, 3.0, 1.0)
CASE_LIMIT_S = 300


def _mls(v):
    return dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))


def run_case(args, w, h):
    pmv = importlib.import_module("practical-multi-view_amd")
    import klt_common as kc
    nf = args.frames
    frames = pmv.synth_sequence(1007, 10, nf, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=8)[0]
    rows = []
    for win, max_level in LKS:
        ctx = pmv.Context(w, h, n_slots=nf, max_tracks=1024)
        ctx.set_lk_params(win=win, max_level=max_level)
        kc.upload(ctx, frames)
        cam = ctx.camera_create(fx=0.58 * w, fy=0.58 * w, cx=w / 2, cy=h / 2, dist=(-0.1,), iters=20)
        rng = np.random.default_rng(5)
        for target, dist in TARGETS:
            p = kc.params(target=target, radius=dist, min_dist=float(dist), reject_f=True)
            trk = ctx.klt_create(**p)
            # the PLAIN pass: the state in front of every frame, its outputs, and the predictions made from them
            states, outs, next_id = [], [], 0
            for i in range(nf):
                states.append(trk.get_tracks() + (next_id,))
                outs.append(trk.step(max(i - 1, 0), i))
                next_id += int(outs[-1][4][4])
            good, far, lk_work = [None], [None], []
            for i in range(1, nf):
                ids0, _, xy0, _ = states[i]
                fwd = ctx.lk_track_ex(i - 1, i, xy0)
                tracked = fwd[1] == 1
                px = (fwd[0][tracked] + rng.uniform(-1.5, 1.5, (int(tracked.sum()), 2))).astype(np.float32)
                un, ok = ctx.undistort_points(cam, px)
                assert ok.all()
                z = rng.uniform(2.0, 30.0, len(un))
                good.append((ids0[tracked], np.stack([un[:, 0] * z, un[:, 1] * z, z], axis=1).astype(np.float64)))
                far.append((ids0, np.tile(FAR, (len(ids0), 1)).astype(np.float64)))
                guess = xy0.copy()
                guess[tracked] = ctx.project_points(cam, good[i][1])[0]
                ctx.lk_counters(reset=True)
                ctx.lk_track_fb_levels(i - 1, i, xy0)
                c_plain = ctx.lk_counters(reset=True)
                ctx.lk_track_fb_levels(i - 1, i, xy0, init_xy=guess, fwd_top_level=SETTING["top_level"], back_top_level=SETTING["back_top_level"])
                c_pred = ctx.lk_counters(reset=True)
                lk_work.append((c_plain, c_pred))

            def run(path, times=None, keep=None, setting=SETTING):
                for i in range(1, nf):
                    trk.set_tracks(*states[i])
                    t0 = time.perf_counter()
                    if path != "plain":
                        ids, xyz = (good if path == "pred" else far)[i]
                        trk.set_prediction(cam, ids, xyz, **setting)
                    out = trk.step(i - 1, i)
                    if times is not None:
                        times.append((time.perf_counter() - t0) * 1e6)
                    if keep is not None:
                        keep.append((out, trk.get_prediction_result()))

            kept = {name: [] for name in ("plain", "pred", "fallback")}
            run("plain", keep=kept["plain"])
            run("pred", keep=kept["pred"])
            run("fallback", keep=kept["fallback"], setting=dict(SETTING, back_top_level=-1))
            for i, ((a, ra), (b, rb), (c, rc)) in enumerate(zip(kept["plain"], kept["pred"], kept["fallback"])):
                kc.same(a, outs[i + 1])   # (a step from the restored state is the pass's own step)
                kc.same(c, a)             # the fall-back with every level in the backward pass returns PLAIN's bytes: else nothing to time
                assert ra["consumed"] == 0 and rc["consumed"] == 1 and rc["fell_back"] == 1 and rc["succ"] == 0, (ra, rc)
                assert rb["consumed"] == 1 and rb["fell_back"] == 0 and rb["joined"] == len(good[i + 1][0]), rb
            paths = ("plain", "pred", "fallback")
            for _ in range(args.warmup):
                for name in paths:
                    run(name)
            s0 = ctx.debug_klt_stats()
            times = {name: [] for name in paths}
            for rep in range(args.repeats):
                for name in (paths if rep % 2 == 0 else paths[::-1]):
                    run(name, times=times[name])
            s1 = ctx.debug_klt_stats()
            us = {name: _mls(v) for name, v in times.items()}
            n_tracks = sum(c[0][2] for c in lk_work)
            work = dict(plain_iters_per_track=round(sum(c[0][0] for c in lk_work) / n_tracks, 2), plain_levels_per_track=round(sum(c[0][1] for c in lk_work) / n_tracks, 2),
                        pred_iters_per_track=round(sum(c[1][0] for c in lk_work) / n_tracks, 2), pred_levels_per_track=round(sum(c[1][1] for c in lk_work) / n_tracks, 2))
            row = dict(w=w, h=h, win=win, max_level=max_level, levels_built=ctx.num_levels(0) + 1, target=target, radius=dist, reject_f=1, plain_us=us["plain"], pred_us=us["pred"],
                       fallback_us=us["fallback"], saved_us=round(us["plain"]["median"] - us["pred"]["median"], 1),
                       wasted_us=round(us["fallback"]["median"] - us["plain"]["median"], 1), ratio_pred_plain=round(us["pred"]["median"] / us["plain"]["median"], 3),
                       launches_per_step=round((s1[2] - s0[2]) / (s1[0] - s0[0]), 2), lk_work=work,
                       plain_counts=[[int(v) for v in o[4][:7]] for o, _ in kept["plain"]], pred_counts=[[int(v) for v in o[4][:7]] for o, _ in kept["pred"]],
                       pred_results=[[r["joined"], r["succ"]] for _, r in kept["pred"]])
            rows.append(row)
            print(f"{w}x{h}, win {win}, {row['levels_built']} levels, target {target}: plain {us['plain']['median']:8.1f} us [{us['plain']['min']:.1f} .. {us['plain']['max']:.1f}] | "
                  f"predicted {us['pred']['median']:8.1f} us [{us['pred']['min']:.1f} .. {us['pred']['max']:.1f}] | fall-back {us['fallback']['median']:8.1f} us "
                  f"[{us['fallback']['min']:.1f} .. {us['fallback']['max']:.1f}] | saved {row['saved_us']:.1f} us, wasted {row['wasted_us']:.1f} us | LK per track: "
                  f"{work['plain_iters_per_track']} iterations on {work['plain_levels_per_track']} levels plain, {work['pred_iters_per_track']} on "
                  f"{work['pred_levels_per_track']} predicted", flush=True)
            trk.close()
        ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", type=int, nargs=2, metavar=("W", "H"), help="run this frame size in this process and print its rows as one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_predict_ubench.json"))
    args = ap.parse_args()
    if args.case:
        print("ROWS " + json.dumps(run_case(args, *args.case)), flush=True)
        return 0
    rows = []
    for w, h in FRAMES:   # one child per frame size, each under its own limit; a failure ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(w), str(h), "--frames", str(args.frames), "--repeats", str(args.repeats), "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=CASE_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{w}x{h}: no result within {CASE_LIMIT_S} s; nothing more is started", file=sys.stderr)
            return 124
        lines = r.stdout.splitlines()
        print("\n".join(ln for ln in lines if not ln.startswith("ROWS ")), flush=True)
        if r.returncode != 0:
            print(f"{w}x{h}: the child ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        rows += json.loads(next(ln for ln in lines if ln.startswith("ROWS "))[5:])
    doc = dict(bench="klt_predict", frames=args.frames, repeats=args.repeats, warmup=args.warmup, setting=SETTING, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
