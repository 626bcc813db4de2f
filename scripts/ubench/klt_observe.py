"""What the observation stage costs inside the tracker step (pmv_klt_set_observe: normalised positions and velocities as stage 9): path ON is
pmv_klt_step with the setting on followed by pmv_klt_get_observations, path OFF the same step with the setting off, path CALLS pmv_klt_step
with the setting off followed by two pmv_undistort_points calls from Python (the list and its previous positions) and the velocity rule in
numpy. One line per case and one JSON line at the end (kept as profiles/klt_observe_ubench.json; --out names the file).

Frames 1241x376 and 752x480 (synthetic, consecutive), target 150 (radius = min_dist = 30) and 1000 (radius = min_dist = 10), rejectWithF
on, forward-backward 0.5 px, border 1; the camera is the scene's pinhole with k1 = -0.3 and 8 iterations, dt = 0.05 s. A fourth path, F-LIFT,
is path ON with undistorted_f = 1 (f_focal 460): its lists differ from the other paths', so only its time is reported. A pass runs a path
from an empty list over the frames; the first step of a pass only detects and is not timed. Before anything is timed one pass of ON, OFF
and CALLS is compared: every step must return the same bytes, and ON's observations must equal CALLS'. Each figure is the median over
`--repeats` passes of the per-step host clock around the calls (every path ends in its waits), with the smallest and the largest step. The
paths alternate pass by pass and the order flips from repeat to repeat. The profiler is off. All paths run through the Python binding.

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
DT, F_FOCAL = 0.05, 460.0
CASE_LIMIT_S = 240


def _mls(v):
    return dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))


def run_case(args, w, h):
    pmv = importlib.import_module("practical-multi-view_amd")
    import klt_common as kc
    nf = args.frames
    frames = pmv.synth_sequence(1007, 10, nf, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=8)[0]
    ctx = pmv.Context(w, h, n_slots=nf, max_tracks=1024)
    kc.upload(ctx, frames)
    cam = ctx.camera_create(fx=0.58 * w, fy=0.58 * w, cx=w / 2, cy=h / 2, dist=(-0.3,), iters=8)
    rows = []
    for target, dist in TARGETS:
        p = kc.params(target=target, radius=dist, min_dist=float(dist), reject_f=True)
        trk = ctx.klt_create(**p)

        def run(setting, after, times=None, keep=None):
            trk.set_observe(*setting) if setting else trk.set_observe(None)
            trk.set_tracks([], [], [], 0)
            for i in range(nf):
                t0 = time.perf_counter()
                out = trk.step(max(i - 1, 0), i)
                obs = after(out)
                if times is not None and i > 0:
                    times.append((time.perf_counter() - t0) * 1e6)
                if keep is not None:
                    keep.append((out, obs))

        def two_calls(out):
            """the observations through the single call, the rule of stage 9 in numpy"""
            _, ages, xy, prev, _ = out
            if not len(xy):
                return np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)
            un, ok = ctx.undistort_points(cam, xy)
            pun, pok = ctx.undistort_points(cam, prev)
            vel = ((un - pun).astype(np.float64) / DT).astype(np.float32)
            vel[~((ages > 1) & (ok == 1) & (pok == 1))] = 0
            return un, vel, ok

        paths = dict(on=((cam, -1, DT), lambda out: trk.get_observations()[:3]), off=(None, lambda out: None), calls=(None, two_calls),
                     f_lift=((cam, -1, DT, True, F_FOCAL), lambda out: trk.get_observations()[:3]))
        kept = {name: [] for name in ("on", "off", "calls")}
        for name in kept:
            run(*paths[name], keep=kept[name])
        for (a, oa), (b, _), (c, oc) in zip(kept["on"], kept["off"], kept["calls"]):
            kc.same(a, b)   # the paths differ: nothing to time
            kc.same(a, c)
            for x, y in zip(oa, oc):
                assert x.tobytes() == y.tobytes(), "the step's observations differ from the single calls'"
        for _ in range(args.warmup):
            for name in paths:
                run(*paths[name])
        s0, o0 = ctx.debug_klt_stats(), ctx.debug_klt_observe_stats()
        times = {name: [] for name in paths}
        order = list(paths)
        for rep in range(args.repeats):
            for name in (order if rep % 2 == 0 else order[::-1]):
                run(*paths[name], times=times[name])
        s1, o1 = ctx.debug_klt_stats(), ctx.debug_klt_observe_stats()
        us = {name: _mls(v) for name, v in times.items()}
        row = dict(w=w, h=h, target=target, radius=dist, reject_f=1, on_us=us["on"], off_us=us["off"], calls_us=us["calls"], f_lift_us=us["f_lift"],
                   stage_us=round(us["on"]["median"] - us["off"]["median"], 1), saved_us=round(us["calls"]["median"] - us["on"]["median"], 1),
                   ratio_on_calls=round(us["on"]["median"] / us["calls"]["median"], 3),
                   launches_per_step=round((s1[2] - s0[2]) / (s1[0] - s0[0]), 2), observe_launches_per_on_step=round((o1[1] - o0[1]) / (o1[0] - o0[0]), 2),
                   lift_launches=o1[2] - o0[2], counts=[[int(v) for v in o[4][:7]] for o, _ in kept["on"]])
        rows.append(row)
        print(f"{w}x{h}, target {target}, radius {dist}: off {us['off']['median']:8.1f} us [{us['off']['min']:.1f} .. {us['off']['max']:.1f}] | "
              f"on {us['on']['median']:8.1f} us [{us['on']['min']:.1f} .. {us['on']['max']:.1f}] | step + 2 undistort_points {us['calls']['median']:8.1f} us "
              f"[{us['calls']['min']:.1f} .. {us['calls']['max']:.1f}] | on with undistorted_f {us['f_lift']['median']:8.1f} us | stage 9 {row['stage_us']:.1f} us, "
              f"{row['saved_us']:.1f} us saved over the calls", flush=True)
        trk.close()
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", type=int, nargs=2, metavar=("W", "H"), help="run this frame size in this process and print its rows as one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_observe_ubench.json"))
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
    doc = dict(bench="klt_observe", frames=args.frames, repeats=args.repeats, warmup=args.warmup, dt=DT, f_focal=F_FOCAL, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
