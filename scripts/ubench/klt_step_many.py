"""What one frame of a group of KLT trackers costs: path A steps the group one tracker after the other (pmv_klt_step, what a caller with
several cameras had before), path B is one pmv_klt_step_many. One line per case and one JSON line at the end (kept as
profiles/klt_step_many_ubench.json; --out names the file).

Frames 752x480 and 1241x376 (synthetic, consecutive; `--seeds` different sequences, dealt out to the trackers in turn), target 150 with
radius = min_dist = 30, rejectWithF on and off, forward-backward 0.5 px, border 1, groups of 1, 2, 4, 8 and 16 trackers, every tracker on
slots of its own. A pass runs a path from empty lists over the frames; the first step of a pass only detects and is not timed. Before
anything is timed one pass of each path is compared: every tracker must return the same bytes at every step. Each figure is the median over
`--repeats` passes of the host clock around one frame of the whole group (both paths end in their waits), with the smallest and the largest
frame. The two paths alternate pass by pass and the order flips from repeat to repeat. The profiler is off.
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

FRAMES = [(752, 480), (1241, 376)]
GROUPS = [1, 2, 4, 8, 16]
TARGET, DIST = 150, 30


def _mls(v):
    return dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_step_many_ubench.json"))
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    import klt_common as kc
    rows = []
    nf = args.frames
    for w, h in FRAMES:
        seqs = [pmv.synth_sequence(1007 + k, 10, nf, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=8)[0] for k in range(args.seeds)]
        ctx = pmv.Context(w, h, n_slots=nf * max(GROUPS), max_tracks=1024)
        for j in range(max(GROUPS)):
            kc.upload(ctx, seqs[j % args.seeds], first_slot=j * nf)
        for reject_f in (True, False):
            p = kc.params(target=TARGET, radius=DIST, min_dist=float(DIST), reject_f=reject_f)
            for n_trk in GROUPS:
                trackers = [ctx.klt_create(**p) for _ in range(n_trk)]

                def slots(i):
                    return [j * nf + max(i - 1, 0) for j in range(n_trk)], [j * nf + i for j in range(n_trk)]

                def reset():
                    for t in trackers:
                        t.set_tracks([], [], [], 0)

                def single_pass(times=None, keep=None):
                    reset()
                    for i in range(nf):
                        ps, cs = slots(i)
                        t0 = time.perf_counter()
                        out = [t.step(ps[j], cs[j]) for j, t in enumerate(trackers)]
                        if times is not None and i > 0:
                            times.append((time.perf_counter() - t0) * 1e6)
                        if keep is not None:
                            keep.append(out)

                def many_pass(times=None, keep=None):
                    reset()
                    for i in range(nf):
                        ps, cs = slots(i)
                        t0 = time.perf_counter()
                        out = ctx.klt_step_many(trackers, ps, cs)
                        if times is not None and i > 0:
                            times.append((time.perf_counter() - t0) * 1e6)
                        if keep is not None:
                            keep.append(out)

                a, b = [], []
                single_pass(keep=a)
                many_pass(keep=b)
                for fa, fb in zip(a, b):
                    for x, y in zip(fa, fb):
                        kc.same(x, y)   # the two paths differ: nothing to time
                for _ in range(args.warmup):
                    single_pass()
                    many_pass()
                s0, m0 = ctx.debug_klt_stats(), ctx.debug_klt_many_stats()
                t_a, t_b = [], []
                for rep in range(args.repeats):
                    pair = [(single_pass, t_a), (many_pass, t_b)]
                    for fn, out in (pair if rep % 2 == 0 else pair[::-1]):
                        fn(times=out)
                s1, m1 = ctx.debug_klt_stats(), ctx.debug_klt_many_stats()
                steps, calls = s1[0] - s0[0], m1[0] - m0[0]
                ua, ub = _mls(t_a), _mls(t_b)
                row = dict(w=w, h=h, target=TARGET, radius=DIST, reject_f=int(reject_f), n_trk=n_trk, single_us=ua, many_us=ub,
                           single_us_per_tracker=round(ua["median"] / n_trk, 1), many_us_per_tracker=round(ub["median"] / n_trk, 1),
                           ratio=round(ub["median"] / ua["median"], 3),
                           single_waits_per_frame=round((s1[1] - s0[1]) / steps * n_trk, 2), single_launches_per_frame=round((s1[2] - s0[2]) / steps * n_trk, 2),
                           many_waits_per_call=round((m1[2] - m0[2]) / calls, 2), many_launches_per_call=round((m1[3] - m0[3]) / calls, 2),
                           counts=[[int(v) for v in o[4][:7]] for o in b[-1]])
                rows.append(row)
                print(f"{w}x{h}, F {'on ' if reject_f else 'off'}, {n_trk:2d} trackers: one after the other {ua['median']:8.1f} us [{ua['min']:.1f} .. {ua['max']:.1f}] | "
                      f"one call {ub['median']:8.1f} us [{ub['min']:.1f} .. {ub['max']:.1f}] | {row['many_us_per_tracker']:.1f} us a tracker, B/A {row['ratio']:.3f} | "
                      f"{row['many_waits_per_call']} waits, {row['many_launches_per_call']} launches a call (A: {row['single_waits_per_frame']}, "
                      f"{row['single_launches_per_frame']} a frame)", flush=True)
                for t in trackers:
                    t.close()
        ctx.close()
    doc = dict(bench="klt_step_many", frames=nf, repeats=args.repeats, warmup=args.warmup, seeds=args.seeds, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
