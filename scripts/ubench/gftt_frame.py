"""What pmv_detect_gftt_frame costs, one line per case and one JSON line at the end (kept as profiles/gftt_frame_ubench.json).

Frames 752x480 and 1241x376 (synthetic), settings (max_corners, quality, min_dist) = (150, 0.01, 30) and (500, 0.01, 7), with and without
a mask of discs of radius 10 around 300 points, block sizes 3 and 7.
Per case, each figure the median of `--repeats` runs of `--passes` calls, with the smallest and the largest run (the spread):
  frame  cand / pick = mean microseconds per launch of the two profiling classes (HIP events, pmv_prof_read) for the frame call;
         call = microseconds per call by the host clock, profiler off;
  grid   the same three figures for pmv_detect_gftt_ex over the 255-grid of the same slot with max_per_cell = max_corners (its pass 1 does
         the same per-tile work, its pass 2 is split over the cells, one workgroup each - the launch ends with its slowest cell);
  twin   tests/twin/gftt_twin.cpp on one host core, milliseconds per call (median of 5).
records = records above the threshold of the frame call (pmv_debug_gftt_frame_stats), off_chip = those kept in HBM.
The grid's corners are NOT the frame call's (threshold, order, cut and min_dist are per cell there): it is a yardstick for time only.
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

FRAMES = [(752, 480), (1241, 376)]
SETTINGS = [(150, 0.01, 30.0), (500, 0.01, 7.0)]
MASK_POINTS, MASK_RADIUS = 300, 10


def _disc_mask(w, h, points, radius):
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.full((h, w), 255, np.uint8)
    for x, y in points:
        y0, y1, x0, x1 = max(y - radius, 0), min(y + radius + 1, h), max(x - radius, 0), min(x + radius + 1, w)
        sub = (xx[y0:y1, x0:x1] - x) ** 2 + (yy[y0:y1, x0:x1] - y) ** 2 <= radius * radius
        m[y0:y1, x0:x1][sub] = 0
    return m


def _mls(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def _measure(ctx, call, passes, warmup, repeats):
    """({class: per-launch us per repeat}, [per-call us per repeat])"""
    prof_runs, call_runs = {"k_gftt_cand": [], "k_gftt_pick": []}, []
    for _ in range(warmup):
        call()
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(passes):
            call()
        call_runs.append((time.perf_counter() - t0) * 1e6 / passes)
        ctx.prof_enable(True)
        for _ in range(passes):
            call()
        prof = ctx.prof_read()
        ctx.prof_enable(False)
        assert set(prof) == set(prof_runs) and all(v[0] == passes for v in prof.values()), prof
        for k in prof_runs:
            prof_runs[k].append(prof[k][1] * 1e3 / passes)
    return prof_runs, call_runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    import gftt_common as gc
    twin = gc.twin()
    rows = []
    for w, h in FRAMES:
        img = pmv.synth_sequence(1007, 10, 1, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=8)[0][0]
        ctx = pmv.Context(w, h, n_slots=1, max_tracks=1024)
        ctx.frame_upload(0, img)
        cells = pmv.grid_cells(w, h)
        rng = np.random.default_rng(5)
        discs = _disc_mask(w, h, np.stack([rng.integers(0, w, MASK_POINTS), rng.integers(0, h, MASK_POINTS)], axis=1), MASK_RADIUS)
        for mc, q, d in SETTINGS:
            for mask in (None, discs):
                for b in (3, 7):
                    kw = dict(quality=q, min_dist=d, mask=mask, block_size=b)
                    corners = len(ctx.detect_gftt_frame(0, mc, **kw))
                    stats = ctx.debug_gftt_frame_stats()
                    fp, fc = _measure(ctx, lambda: ctx.detect_gftt_frame(0, mc, **kw), args.passes, args.warmup, args.repeats)
                    gp, gcall = _measure(ctx, lambda: ctx.detect_gftt_ex(0, cells, mc, **kw), args.passes, args.warmup, args.repeats)
                    tw = []
                    for _ in range(5):
                        t0 = time.perf_counter()
                        twin.corners(img, (0, 0, w, h), mc, **kw)
                        tw.append((time.perf_counter() - t0) * 1e3)
                    row = dict(w=w, h=h, max_corners=mc, min_dist=d, mask=mask is not None, block=b, corners=corners, records=stats[3], off_chip=stats[4],
                               cells=len(cells), frame_cand_us=_mls(fp["k_gftt_cand"]), frame_pick_us=_mls(fp["k_gftt_pick"]), frame_call_us=_mls(fc),
                               grid_cand_us=_mls(gp["k_gftt_cand"]), grid_pick_us=_mls(gp["k_gftt_pick"]), grid_call_us=_mls(gcall), twin_ms=_mls(tw))
                    rows.append(row)
                    print(f"{w}x{h} ({mc}, {d:g}) mask {int(mask is not None)} b={b}: frame cand {row['frame_cand_us']['median']:7.2f} pick {row['frame_pick_us']['median']:7.2f} "
                          f"call {row['frame_call_us']['median']:7.1f} us | grid cand {row['grid_cand_us']['median']:7.2f} pick {row['grid_pick_us']['median']:7.2f} "
                          f"call {row['grid_call_us']['median']:7.1f} us | twin {row['twin_ms']['median']:6.2f} ms | {corners} corners, {stats[3]} records", flush=True)
        ctx.close()
    print(json.dumps(dict(bench="gftt_frame", passes=args.passes, repeats=args.repeats, mask_points=MASK_POINTS, mask_radius=MASK_RADIUS, rows=rows)))


if __name__ == "__main__":
    main()
