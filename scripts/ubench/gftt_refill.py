"""What pmv_detect_gftt_refill costs next to the path a caller has without it, one line per case and one JSON document at the end (kept as
profiles/gftt_refill_ubench.json; --out names the file).

Frames 1241x376 and 752x480 (synthetic), 150 and 1000 tracks with random ages, radius 30, (max_corners, quality, min_dist) = (150, 0.01, 30).
  host    today's path: the mask built on one host core by tests/twin/refill_twin.cpp (sort, walk, cv::circle's loop), then
          pmv_detect_gftt_frame with that host mask (packed into pinned memory and copied by the call);
          mask_us = the twin alone, call_us = mask + frame call;
  refill  pmv_detect_gftt_refill with the same tracks: call_us by the host clock around the call (it ends in its wait).
Each figure is the median of `--repeats` runs of `--passes` calls, with the smallest and the largest run. The two paths alternate run by
run, and the order within a pair flips from repeat to repeat, so a drift of the machine lands on both. Before anything is timed the two
paths' corners and keep bytes are compared: they must be the same bytes. The profiler is off.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = [(1241, 376), (752, 480)]
TRACKS = [150, 1000]
RADIUS = 30
SETTING = (150, 0.01, 30.0)


def _mls(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def _run(fn, passes):
    t0 = time.perf_counter()
    for _ in range(passes):
        fn()
    return (time.perf_counter() - t0) * 1e6 / passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gftt_refill_ubench.json"))
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    import refill_common as rc
    twin = rc.twin()
    mc, q, d = SETTING
    rows = []
    for w, h in FRAMES:
        img = pmv.synth_sequence(1007, 10, 1, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=8)[0][0]
        ctx = pmv.Context(w, h, n_slots=1, max_tracks=1024)
        ctx.frame_upload(0, img)
        for n in TRACKS:
            xy, prio = rc.tracks(w, h, n, seed=11)
            kw = dict(quality=q, min_dist=d)
            host_mask = lambda: twin.mask(w, h, xy, RADIUS, prio)   # noqa: E731
            host = lambda: ctx.detect_gftt_frame(0, mc, mask=host_mask()[1], **kw)   # noqa: E731
            refill = lambda: ctx.detect_gftt_refill(0, mc, xy, RADIUS, priorities=prio, **kw)   # noqa: E731
            keep_h, mask_h = host_mask()
            corners_h = ctx.detect_gftt_frame(0, mc, mask=mask_h, **kw)
            keep_r, corners_r = refill()
            assert np.array_equal(keep_h, keep_r) and np.array_equal(corners_h, corners_r), "the two paths differ: nothing to time"
            for _ in range(args.warmup):
                host()
                refill()
            t_host, t_refill, t_mask = [], [], []
            for rep in range(args.repeats):
                pair = [("host", host, t_host), ("refill", refill, t_refill)]
                for _, fn, out in (pair if rep % 2 == 0 else pair[::-1]):
                    out.append(_run(fn, args.passes))
                t_mask.append(_run(host_mask, args.passes))
            row = dict(w=w, h=h, tracks=n, radius=RADIUS, kept=int(keep_r.sum()), corners=len(corners_r), max_corners=mc, min_dist=d,
                       host_mask_us=_mls(t_mask), host_call_us=_mls(t_host), refill_call_us=_mls(t_refill), mask_bytes=w * h,
                       copied_bytes_refill=ctx.debug_refill_stats()[3])
            rows.append(row)
            print(f"{w}x{h}, {n} tracks (kept {row['kept']}), radius {RADIUS}: host mask {row['host_mask_us']['median']:8.1f} us, host path "
                  f"{row['host_call_us']['median']:8.1f} us [{row['host_call_us']['min']:.1f} .. {row['host_call_us']['max']:.1f}] | refill "
                  f"{row['refill_call_us']['median']:8.1f} us [{row['refill_call_us']['min']:.1f} .. {row['refill_call_us']['max']:.1f}] | {row['corners']} corners", flush=True)
        ctx.close()
    doc = dict(bench="gftt_refill", passes=args.passes, repeats=args.repeats, warmup=args.warmup, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
