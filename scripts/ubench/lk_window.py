"""What a Lucas-Kanade call costs by window (pmv_set_lk_params), one line per window and one JSON line at the end.

300 tracks (GFTT corners of frame 0, topped up with uniform points if the detector finds fewer) on a 1241x376 synthetic pair, maxLevel 4:
  single   microseconds per pmv_lk_track call (one launch of four wavefronts per track, the host's copy-in and the synchronise included);
  batched  microseconds for a round of 64 such requests: 64 threads call pmv_batch_lk_track on the same two slots at once, so the requests
           meet in the LK combiners' launches (one wavefront per track); wall time from the common start until the last call has returned.
           The callers are Python threads, which take turns entering the library, so the 64 requests are served by as many launches as
           the two LK combiners need while they arrive (one launch takes whatever has queued up): that count is printed next to the figure,
           and the figure is the time for all 64 requests, not for one launch.
Windows: 15, 21, 32 through the tuned kernels, 32 through the general ones (pmv_debug_lk_general), 41, 63. Every figure is the median of
`--passes` timed repetitions after a warm-up; minimum and maximum are printed with it.
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
CASES = [(15, False, "15"), (21, False, "21"), (32, False, "32 tuned"), (32, True, "32 general"), (41, False, "41"), (63, False, "63")]


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
    out = []
    for win, general, name in CASES:
        ctx.set_lk_params(win=win, max_level=4)
        ctx.debug_lk_general(general)
        ctx.frame_upload(0, frames[0])
        ctx.frame_upload(1, frames[1])
        single = []
        for k in range(args.warmup + args.passes):
            t0 = time.perf_counter()
            _, st, _ = ctx.lk_track(0, 1, pts)
            if k >= args.warmup:
                single.append((time.perf_counter() - t0) * 1e6)
        batched, rounds = [], []
        with ctx.batch_session(1, [(W, H)]):
            for k in range(args.warmup + args.passes):
                start = threading.Barrier(REQUESTS + 1)

                def call():
                    start.wait()
                    ctx.batch_lk_track(0, 1, pts)
                th = [threading.Thread(target=call) for _ in range(REQUESTS)]
                for t in th:
                    t.start()
                r0 = ctx.batch_stats()["lk"]["launches"]
                start.wait()
                t0 = time.perf_counter()
                for t in th:
                    t.join()
                dt = (time.perf_counter() - t0) * 1e6
                r = max(ctx.batch_stats()["lk"]["launches"] - r0, 1)
                if k >= args.warmup:
                    batched.append(dt)
                    rounds.append(r)
        row = dict(win=name, levels=ctx.num_levels(0) + 1, tracked=int(st.sum()), single_us=round(statistics.median(single), 1), single_min=round(min(single), 1),
                   single_max=round(max(single), 1), batched_64_us=round(statistics.median(batched), 1), batched_min=round(min(batched), 1),
                   batched_max=round(max(batched), 1), launches_per_64=statistics.median(rounds))
        out.append(row)
        print(f"win {name:>10}: {row['levels']} levels, {row['tracked']:3d}/{N_TRACKS} tracked | lk_track {row['single_us']:8.1f} us ({row['single_min']:.1f} .. {row['single_max']:.1f}) | "
              f"{REQUESTS} batched requests {row['batched_64_us']:9.1f} us ({row['batched_min']:.1f} .. {row['batched_max']:.1f}) in {row['launches_per_64']} launch(es)")
    ctx.debug_lk_general(False)
    ctx.close()
    print(json.dumps(dict(bench="lk_window", w=W, h=H, tracks=N_TRACKS, requests=REQUESTS, passes=args.passes, rows=out)))


if __name__ == "__main__":
    main()
