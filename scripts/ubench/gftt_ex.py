"""What pmv_detect_gftt_ex costs next to pmv_detect_gftt, one line per case and one JSON line at the end.

The grid of the metric frame (1241x376: 5 x 2 cells of at most 255x255) on a synthetic frame, max_per_cell 40, quality 0.01, min_dist 5.
Cases:
  tuned      pmv_detect_gftt: k_gftt_cand + k_gftt_pick;
  b=3 gen    the same arguments through k_gftt_cand_general (pmv_debug_gftt_general): what the general form costs by itself;
  b=5, 7, 15 larger blocks (the b*b-term double sum);
  harris     block 3, the Harris response with k = 0.04;
  mask       block 3, a mask of discs of radius 10 around 500 points (what a KLT loop hands the detector on a refill).
Per case: `call` = microseconds per call by the host clock (copy-in, launches, copy-out and the synchronise included): the median of
`--passes` timed repetitions after a warm-up, with minimum and maximum; `cand` and `pick` = mean microseconds per launch of the two
profiling classes by HIP events, over a second run of the same `--passes` calls with the profiler on (events cost host time); and the
corners found. ratio_general_over_tuned_b3 = cand(b=3 gen) / cand(tuned).
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

W, H, MAX_PER_CELL, MASK_POINTS, MASK_RADIUS = 1241, 376, 40, 500, 10


def _disc_mask(points, radius):
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.full((H, W), 255, np.uint8)
    for x, y in points:
        y0, y1, x0, x1 = max(y - radius, 0), min(y + radius + 1, H), max(x - radius, 0), min(x + radius + 1, W)
        sub = (xx[y0:y1, x0:x1] - x) ** 2 + (yy[y0:y1, x0:x1] - y) ** 2 <= radius * radius
        m[y0:y1, x0:x1][sub] = 0
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    frames, _ = pmv.synth_sequence(1007, 10, 1, W, H, 718.856, 718.856, 607.1928, 185.2157, nthreads=8)
    ctx = pmv.Context(W, H, n_slots=1, max_tracks=1024)
    ctx.frame_upload(0, frames[0])
    cells = pmv.grid_cells(W, H)
    rng = np.random.default_rng(5)
    mask = _disc_mask(np.stack([rng.integers(0, W, MASK_POINTS), rng.integers(0, H, MASK_POINTS)], axis=1), MASK_RADIUS)
    ex = ctx.detect_gftt_ex
    cases = [("tuned", False, lambda: ctx.detect_gftt(0, cells, MAX_PER_CELL)),
             ("b=3 gen", True, lambda: ex(0, cells, MAX_PER_CELL)),
             ("b=5", False, lambda: ex(0, cells, MAX_PER_CELL, block_size=5)),
             ("b=7", False, lambda: ex(0, cells, MAX_PER_CELL, block_size=7)),
             ("b=15", False, lambda: ex(0, cells, MAX_PER_CELL, block_size=15)),
             ("harris", False, lambda: ex(0, cells, MAX_PER_CELL, use_harris=True, k=0.04)),
             ("mask", False, lambda: ex(0, cells, MAX_PER_CELL, mask=mask))]
    rows = []
    for name, general, call in cases:
        ctx.debug_gftt_general(general)
        corners = sum(len(c) for c in call())
        t = []
        for k in range(args.warmup + args.passes):
            t0 = time.perf_counter()
            call()
            if k >= args.warmup:
                t.append((time.perf_counter() - t0) * 1e6)
        for _ in range(args.warmup):
            call()
        ctx.prof_enable(True)
        for _ in range(args.passes):
            call()
        prof = ctx.prof_read()
        ctx.prof_enable(False)
        assert set(prof) == {"k_gftt_cand", "k_gftt_pick"} and all(v[0] == args.passes for v in prof.values()), prof
        row = dict(case=name, corners=corners, call_us=round(statistics.median(t), 1), call_min=round(min(t), 1), call_max=round(max(t), 1),
                   cand_us=round(prof["k_gftt_cand"][1] * 1e3 / args.passes, 2), pick_us=round(prof["k_gftt_pick"][1] * 1e3 / args.passes, 2))
        rows.append(row)
        print(f"{name:>8}: call {row['call_us']:7.1f} us ({row['call_min']:.1f} .. {row['call_max']:.1f}) | k_gftt_cand {row['cand_us']:7.2f} us, "
              f"k_gftt_pick {row['pick_us']:7.2f} us per launch | {corners} corners", flush=True)
    ctx.debug_gftt_general(False)
    ctx.close()
    ratio = round(rows[1]["cand_us"] / rows[0]["cand_us"], 3)
    print(json.dumps(dict(bench="gftt_ex", w=W, h=H, cells=len(cells), max_per_cell=MAX_PER_CELL, passes=args.passes, mask_points=MASK_POINTS,
                          mask_radius=MASK_RADIUS, ratio_general_over_tuned_b3=ratio, rows=rows)))


if __name__ == "__main__":
    main()
