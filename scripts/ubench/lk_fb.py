"""What the extended Lucas-Kanade calls cost next to pmv_lk_track, one line per window and one JSON line at the end.

300 tracks (GFTT corners of frame 0, topped up with uniform points if the detector finds fewer) on a 1241x376 synthetic pair, maxLevel 4,
windows 21 (general kernels) and 32 (tuned kernels). Four ways to call, each as single calls and as 64 session requests:
  lk_track     pmv_lk_track: the plain kernels;
  ex           pmv_lk_track_ex with flags 0: the same arithmetic through the extended kernels;
  fb           pmv_lk_track_fb: forward and back in one launch;
  2 x ex       the same back check composed by the caller: pmv_lk_track_ex forward, the tracked points selected on the host,
               pmv_lk_track_ex back with the original positions as initial flow.
single   microseconds per call (or per pair of calls), the host's copy-in and the synchronise included;
batched  microseconds for 64 threads that each make the call (or the pair of calls) on the same two slots at once through a session: wall
         time from the common start until the last thread has returned, and the number of LK combiner rounds that served them. The
         callers are Python threads, which take turns entering the library (see lk_window.py).
Every figure is the median of `--passes` timed repetitions after a warm-up; minimum and maximum are printed with it.
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

W, H, N_TRACKS, REQUESTS = 1241, 376, 300, 64
WINDOWS = [21, 32]


def _stats(v):
    return dict(us=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    frames, _ = pmv.synth_sequence(1007, 10, 2, W, H, 718.856, 718.856, 607.1928, 185.2157, nthreads=8)
    ctx = pmv.Context(W, H, n_slots=2, max_tracks=REQUESTS * N_TRACKS)   # a round's result blocks hold n_seq * max_tracks tracks
    ctx.frame_upload(0, frames[0])
    cells = pmv.grid_cells(W, H)
    pts = np.concatenate([d + c[:2] for c, d in zip(cells, ctx.detect_gftt(0, cells, 40))]).astype(np.float32)
    rng = np.random.default_rng(3)
    fill = np.stack([rng.uniform(8, W - 8, N_TRACKS), rng.uniform(8, H - 8, N_TRACKS)], axis=1).astype(np.float32)
    pts = np.concatenate([pts, fill])[:N_TRACKS]

    def two_calls(ex):
        xy, st, _ = ex(0, 1, pts)
        ok = st > 0
        return ex(1, 0, xy[ok], init_xy=pts[ok])

    out = []
    for win in WINDOWS:
        ctx.set_lk_params(win=win, max_level=4)
        ctx.frame_upload(0, frames[0])
        ctx.frame_upload(1, frames[1])
        forms = [("lk_track", lambda: ctx.lk_track(0, 1, pts), lambda: ctx.batch_lk_track(0, 1, pts)),
                 ("ex", lambda: ctx.lk_track_ex(0, 1, pts), lambda: ctx.batch_lk_track_ex(0, 1, pts)),
                 ("fb", lambda: ctx.lk_track_fb(0, 1, pts), lambda: ctx.batch_lk_track_fb(0, 1, pts)),
                 ("2 x ex", lambda: two_calls(ctx.lk_track_ex), lambda: two_calls(ctx.batch_lk_track_ex))]
        st = ctx.lk_track_fb(0, 1, pts)
        row = dict(win=win, levels=ctx.num_levels(0) + 1, tracked=int(st[1].sum()), tracked_back=int(st[4].sum()))
        for name, single, batched in forms:
            t_single = []
            for k in range(args.warmup + args.passes):
                t0 = time.perf_counter()
                single()
                if k >= args.warmup:
                    t_single.append((time.perf_counter() - t0) * 1e6)
            t_batch, rounds = [], []
            with ctx.batch_session(1, [(W, H)]):
                for k in range(args.warmup + args.passes):
                    start = threading.Barrier(REQUESTS + 1)

                    def call():
                        start.wait()
                        batched()
                    th = [threading.Thread(target=call) for _ in range(REQUESTS)]
                    for t in th:
                        t.start()
                    r0 = ctx.batch_stats()["lk"]["launches"]
                    start.wait()
                    t0 = time.perf_counter()
                    for t in th:
                        t.join()
                    dt = (time.perf_counter() - t0) * 1e6
                    if k >= args.warmup:
                        t_batch.append(dt)
                        rounds.append(max(ctx.batch_stats()["lk"]["launches"] - r0, 1))
            row[name] = dict(single=_stats(t_single), batched_64=_stats(t_batch), rounds_per_64=statistics.median(rounds))
            s, b = row[name]["single"], row[name]["batched_64"]
            print(f"win {win} {name:>8}: single {s['us']:8.1f} us ({s['min']:.1f} .. {s['max']:.1f}) | {REQUESTS} session callers {b['us']:9.1f} us "
                  f"({b['min']:.1f} .. {b['max']:.1f}) in {row[name]['rounds_per_64']} round(s)", flush=True)
        out.append(row)
    ctx.close()
    print(json.dumps(dict(bench="lk_fb", w=W, h=H, tracks=N_TRACKS, requests=REQUESTS, passes=args.passes, rows=out)))


if __name__ == "__main__":
    main()
