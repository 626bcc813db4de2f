"""What pmv_corner_subpix costs, one line per case and one JSON line at the end (also written to --out).

A synthetic 1241x376 frame; the points are the detector's corners of the whole grid (no limit), shifted by (+0.3, -0.2) and repeated to n.
Criteria 30 iterations, eps 0.01. Cases: n = 256 and 2048, windows (5, 5) and (15, 15); each as the single call and through a batch
session with 16 caller threads, every caller on its own slot with the same frame.
  single:  `call` = microseconds per call by the host clock (records, launch, synchronise, copy-out): the median of `--passes` repetitions
           after a warm-up, with minimum and maximum; `kernel` = mean microseconds per launch by HIP events (the detector's selection
           class, which only this call uses here), over a second run with the profiler on.
  session: `call` = the median latency of one pmv_batch_corner_subpix as a caller sees it; `per_call` = wall time of the whole run divided
           by the number of calls (16 x passes): what one refinement costs when 16 callers share launches; rounds and launches made.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

W, H, CALLERS = 1241, 376, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    frames, _ = pmv.synth_sequence(1007, 10, 1, W, H, 718.856, 718.856, 607.1928, 185.2157, nthreads=8)
    ctx = pmv.Context(W, H, n_slots=CALLERS, max_tracks=2048)
    for s in range(CALLERS):
        ctx.frame_upload(s, frames[0])
    cells = pmv.grid_cells(W, H)
    corners = np.concatenate([d + c[:2] for c, d in zip(cells, ctx.detect_gftt(0, cells, 0))]).astype(np.float32) + np.asarray([0.3, -0.2], np.float32)
    rows = []
    for n in (256, 2048):
        pts = corners[np.arange(n) % len(corners)].copy()
        for win in ((5, 5), (15, 15)):
            kw = dict(win=win, max_iter=30, eps=0.01)
            _, it, fl = ctx.corner_subpix(0, pts, return_info=True, **kw)
            t = []
            for k in range(args.warmup + args.passes):
                t0 = time.perf_counter()
                ctx.corner_subpix(0, pts, **kw)
                if k >= args.warmup:
                    t.append((time.perf_counter() - t0) * 1e6)
            ctx.prof_enable(True)
            for _ in range(args.passes):
                ctx.corner_subpix(0, pts, **kw)
            prof = ctx.prof_read()
            ctx.prof_enable(False)
            assert set(prof) == {"k_gftt_pick"} and prof["k_gftt_pick"][0] == args.passes, prof
            row = dict(form="single", n=n, win=list(win), distinct_points=int(min(n, len(corners))), mean_updates=round(float(it.mean()), 2),
                       reverted=int(((fl & 8) != 0).sum()), call_us=round(statistics.median(t), 1), call_min=round(min(t), 1), call_max=round(max(t), 1),
                       kernel_us=round(prof["k_gftt_pick"][1] * 1e3 / args.passes, 2))
            rows.append(row)
            print(f"single  n {n:5d} win {win}: call {row['call_us']:8.1f} us ({row['call_min']:.1f} .. {row['call_max']:.1f}) | kernel {row['kernel_us']:8.2f} us | "
                  f"{row['mean_updates']} updates per point", flush=True)
            lat = [[] for _ in range(CALLERS)]
            with ctx.batch_session(CALLERS, [(W, H)]):
                c0 = ctx.debug_subpix_launches()
                start = threading.Barrier(CALLERS + 1)

                def run(j):
                    start.wait()
                    for k in range(args.warmup + args.passes):
                        t0 = time.perf_counter()
                        ctx.batch_corner_subpix(j, pts, **kw)
                        if k >= args.warmup:
                            lat[j].append((time.perf_counter() - t0) * 1e6)
                th = [threading.Thread(target=run, args=(j,)) for j in range(CALLERS)]
                for x in th:
                    x.start()
                start.wait()
                t0 = time.perf_counter()
                for x in th:
                    x.join()
                wall = (time.perf_counter() - t0) * 1e6
                c1 = ctx.debug_subpix_launches()
            calls = CALLERS * (args.warmup + args.passes)
            all_lat = [v for l in lat for v in l]
            row = dict(form="session16", n=n, win=list(win), call_us=round(statistics.median(all_lat), 1), call_min=round(min(all_lat), 1), call_max=round(max(all_lat), 1),
                       per_call_us=round(wall / calls, 1), rounds=c1[1] - c0[1], launches=c1[2] - c0[2], calls=calls)
            rows.append(row)
            print(f"session n {n:5d} win {win}: call {row['call_us']:8.1f} us ({row['call_min']:.1f} .. {row['call_max']:.1f}) | {row['per_call_us']:8.1f} us per call over "
                  f"{calls} calls in {row['rounds']} rounds, {row['launches']} launches", flush=True)
    ctx.close()
    line = json.dumps(dict(bench="corner_subpix", w=W, h=H, callers=CALLERS, passes=args.passes, max_iter=30, eps=0.01, rows=rows))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
