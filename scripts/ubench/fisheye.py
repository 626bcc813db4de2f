"""What a camera of the equidistant (cv::fisheye) model costs next to a radial-tangential one: pmv_undistort_points and pmv_project_points at
n = 256 and 2048 through a radial-tangential camera (k1 = -0.3, 5 iterations) and through a fisheye camera, and pmv_klt_step with
observations and undistorted_f through either camera. One line per leg and one JSON line at the end (kept as
profiles/fisheye_ubench.json; --out names the file).

The radial-tangential legs use only calls that exist without the fisheye model, so the script also runs on a tree from before it (--root
names the tree whose package is loaded; the fisheye legs are then left out and "fisheye": false is recorded). Those legs are to be compared
between the two trees; the fisheye legs with the radial-tangential legs of the same run.

Method: the host clock around the call, which ends in its wait. The legs alternate call by call (points) or pass by pass (tracker) and the
order flips from repeat to repeat, so that drift hits all legs alike; `--warmup` rounds run first and are not timed; each figure is the
median over `--repeats` rounds with the quartiles, and `spread_us` = (q3 - q1) is the run-to-run spread a difference has to exceed before
it means anything. The tracker legs run 752 x 480 synthetic frames, target 150 (radius = min_dist = 30), rejectWithF on lifted points,
forward-backward 0.5 px; a pass runs from an empty list over the frames, and its first step, which only detects, is not timed. The lists of
the two cameras differ (F sees different points), so the tracker legs compare times only. The profiler is off.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H = 752, 480
DT, F_FOCAL = 0.05, 460.0
POINT_NS = (256, 2048)
RADTAN = dict(fx=0.58 * W, fy=0.58 * W, cx=W / 2, cy=H / 2, dist=(-0.3,), iters=5)
FISHEYE = dict(fx=0.58 * W, fy=0.58 * W, cx=W / 2, cy=H / 2, k=(-0.02, 0.004, -0.001, 0.0002))


def _stat(v):
    q = statistics.quantiles(v, n=4)
    return dict(median_us=round(statistics.median(v), 2), q1_us=round(q[0], 2), q3_us=round(q[2], 2), spread_us=round(q[2] - q[0], 2), min_us=round(min(v), 2), samples=len(v))


def _alternate(legs, repeats, warmup):
    """legs: name -> callable returning the microseconds of one round (or a list of them); rounds alternate, the order flips"""
    times = {name: [] for name in legs}
    order = list(legs)
    for rep in range(warmup + repeats):
        for name in (order if rep % 2 == 0 else order[::-1]):
            t = legs[name]()
            if rep >= warmup:
                times[name] += t if isinstance(t, list) else [t]
    return {name: _stat(v) for name, v in times.items()}


def _timed(fn, *a):
    t0 = time.perf_counter()
    fn(*a)
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE_ROOT, help="the tree whose package and tests/klt_common.py are loaded")
    ap.add_argument("--repeats", type=int, default=200, help="timed rounds of every point leg")
    ap.add_argument("--passes", type=int, default=15, help="timed passes of every tracker leg")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(HERE_ROOT, "profiles", "fisheye_ubench.json"))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, "tests"))
    pmv = importlib.import_module("practical-multi-view_amd")
    import klt_common as kc
    frames = pmv.synth_sequence(1007, 10, args.frames, W, H, 0.58 * W, 0.58 * W, W / 2, H / 2, nthreads=8)[0]
    ctx = pmv.Context(W, H, n_slots=args.frames, max_tracks=2048)
    kc.upload(ctx, frames)
    has_fisheye = hasattr(ctx, "camera_create_fisheye")
    cams = dict(radtan=ctx.camera_create(**RADTAN))
    if has_fisheye:
        cams["fisheye"] = ctx.camera_create_fisheye(**FISHEYE)
    rng = np.random.default_rng(1)
    rows = []
    for n in POINT_NS:
        xy = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1).astype(np.float32)
        ang, az, z = rng.uniform(0, 0.9, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(1, 30, n)
        xyz = np.stack([z * np.tan(ang) * np.cos(az), z * np.tan(ang) * np.sin(az), z], axis=1)
        for call, fn, arg in (("undistort_points", ctx.undistort_points, xy), ("project_points", ctx.project_points, xyz)):
            legs = {name: (lambda c=c: _timed(fn, c, arg)) for name, c in cams.items()}
            for name, st in _alternate(legs, args.repeats, args.warmup).items():
                rows.append(dict(leg=call, n=n, camera=name, ok=int(fn(cams[name], arg)[1].sum()), **st))
                print(f"{call:17s} n {n:5d} {name:8s}: {st['median_us']:8.2f} us  [q1 {st['q1_us']:.2f} .. q3 {st['q3_us']:.2f}]  spread {st['spread_us']:.2f} us", flush=True)
    p = kc.params(target=150, radius=30, min_dist=30.0, reject_f=True)
    trk = ctx.klt_create(**p)

    def one_pass(cam):
        trk.set_observe(cam, -1, DT, True, F_FOCAL)
        trk.set_tracks([], [], [], 0)
        out = []
        for i in range(args.frames):
            t0 = time.perf_counter()
            trk.step(max(i - 1, 0), i)
            trk.get_observations()
            if i > 0:
                out.append((time.perf_counter() - t0) * 1e6)
        return out

    s0 = ctx.debug_klt_stats()
    legs = {name: (lambda c=c: one_pass(c)) for name, c in cams.items()}
    res = _alternate(legs, args.passes, max(2, args.warmup // 10))
    s1 = ctx.debug_klt_stats()
    for name, st in res.items():
        rows.append(dict(leg="klt_step + observations, undistorted_f", n=150, camera=name, **st))
        print(f"klt_step observe+F target 150 {name:8s}: {st['median_us']:8.2f} us  [q1 {st['q1_us']:.2f} .. q3 {st['q3_us']:.2f}]  spread {st['spread_us']:.2f} us", flush=True)
    trk.close()
    ctx.close()
    doc = dict(bench="fisheye", fisheye=has_fisheye, w=W, h=H, repeats=args.repeats, passes=args.passes, warmup=args.warmup, frames=args.frames,
               launches_per_step=round((s1[2] - s0[2]) / max(1, s1[0] - s0[0]), 2), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
