"""What one frame of a caller's KLT loop costs through the device-resident tracker (pmv_klt_step) next to the same frames driven through the
chain of single calls with the policy in numpy (tests/klt_common.py: calls_step), one line per case and one JSON line at the end (kept as
profiles/klt_step_ubench.json; --out names the file).

Frames 1241x376 and 752x480 (synthetic, consecutive), target 150 (radius = min_dist = 30) and 1000 (radius = min_dist = 10), rejectWithF on
and off, forward-backward 0.5 px, border 1. A pass runs both paths from an empty list over the frames; the first step of a pass only detects
and is not timed. Before anything is timed one pass of each path is compared: every step must return the same bytes. Each figure is the
median over `--repeats` passes of the per-step host clock around the call (both paths end in their waits), with the smallest and the largest
step. The two paths alternate pass by pass and the order flips from repeat to repeat. The profiler is off. Both paths run through the
Python binding: calls_step's policy (boolean indexing of a few hundred tracks) is part of what a caller of the single calls pays.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = [(1241, 376), (752, 480)]
TARGETS = [(150, 30), (1000, 10)]   # (target, radius = min_dist)


def _mls(v):
    return dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_step_ubench.json"))
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    import klt_common as kc
    rows = []
    for w, h in FRAMES:
        frames = pmv.synth_sequence(1007, 10, args.frames, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=8)[0]
        ctx = pmv.Context(w, h, n_slots=args.frames, max_tracks=1024)
        kc.upload(ctx, frames)
        for target, dist in TARGETS:
            for reject_f in (True, False):
                p = kc.params(target=target, radius=dist, min_dist=float(dist), reject_f=reject_f)
                trk = ctx.klt_create(**p)

                def tracker_pass(times=None, keep=None):
                    trk.set_tracks([], [], [], 0)
                    for i in range(args.frames):
                        t0 = time.perf_counter()
                        out = trk.step(max(i - 1, 0), i)
                        if times is not None and i > 0:
                            times.append((time.perf_counter() - t0) * 1e6)
                        if keep is not None:
                            keep.append(out)

                def calls_pass(times=None, keep=None):
                    state = kc.empty_state()
                    for i in range(args.frames):
                        t0 = time.perf_counter()
                        state, out = kc.calls_step(ctx, state, max(i - 1, 0), i, p)
                        if times is not None and i > 0:
                            times.append((time.perf_counter() - t0) * 1e6)
                        if keep is not None:
                            keep.append(out)

                a, b = [], []
                tracker_pass(keep=a)
                calls_pass(keep=b)
                for x, y in zip(a, b):
                    kc.same(x, y)   # the two paths differ: nothing to time
                for _ in range(args.warmup):
                    tracker_pass()
                    calls_pass()
                s0 = ctx.debug_klt_stats()
                t_trk, t_calls = [], []
                for rep in range(args.repeats):
                    pair = [(tracker_pass, t_trk), (calls_pass, t_calls)]
                    for fn, out in (pair if rep % 2 == 0 else pair[::-1]):
                        fn(times=out)
                s1 = ctx.debug_klt_stats()
                steps = s1[0] - s0[0]
                counts = [[int(v) for v in o[4][:7]] for o in a]
                row = dict(w=w, h=h, target=target, radius=dist, reject_f=int(reject_f), step_us=_mls(t_trk), calls_us=_mls(t_calls),
                           waits_per_step=round((s1[1] - s0[1]) / steps, 2), launches_per_step=round((s1[2] - s0[2]) / steps, 2), counts=counts)
                rows.append(row)
                print(f"{w}x{h}, target {target}, radius {dist}, F {'on ' if reject_f else 'off'}: tracker step {row['step_us']['median']:8.1f} us "
                      f"[{row['step_us']['min']:.1f} .. {row['step_us']['max']:.1f}] | single calls {row['calls_us']['median']:8.1f} us "
                      f"[{row['calls_us']['min']:.1f} .. {row['calls_us']['max']:.1f}] | {row['waits_per_step']} waits, {row['launches_per_step']} launches a step", flush=True)
                trk.close()
        ctx.close()
    doc = dict(bench="klt_step", frames=args.frames, repeats=args.repeats, warmup=args.warmup, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
