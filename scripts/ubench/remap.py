"""What pmv_frames_remap costs against the pyramid build it contains, one line per figure and one JSON line at the end (also written to --out).

64 synthetic 1241x376 frames, staged before every repetition (staging is not timed; a second remap would see another image), the map of
undistort_map with the coefficients of the test table scaled to that size (f = 0.75 w, fy = 1.02 f, c = ((w - 1) / 2 + 1.3, (h - 1) / 2 -
0.8), dist = (-0.35, 0.12, 0.001, -0.0005, -0.02), new_K = K), border value 0. Two calls are timed in the same run, each the median of
`--passes` repetitions after a warm-up:
  build: pmv_frames_build alone - code that exists without this call, the yardstick;
  remap: pmv_frames_remap, which contains the same build (its list form) behind k_remap.
  `*_kernel_us` = the sum of the call's launches by HIP events (the level-0 and pyrDown profiling classes; k_remap is booked under level 0),
                  from repetitions with the profiler on;
  `*_call_us`   = the host clock around the call and a synchronise, from repetitions with the profiler off.
The difference per frame and the bytes per second it implies are derived from the kernel figures, at 12 bytes per pixel: 6 of the packed
map, 4 tap bytes, the scratch frame written once by k_remap and read once by the level-0 launch behind it (the build alone reads the slot's
own interior instead, so the last term is no extra traffic; it is kept in the count because it is what the plan moves).
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

W, H, N = 1241, 376, 64
DIST = (-0.35, 0.12, 0.001, -0.0005, -0.02, 0.0, 0.0, 0.0)
BYTES_PER_PIXEL = 12.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.passes >= 20, "the median of at least 20 repetitions"
    pmv = importlib.import_module("practical-multi-view_amd")
    frames, _ = pmv.synth_sequence(1007, 10, N, W, H, 718.856, 718.856, 607.1928, 185.2157, nthreads=8)
    f = 0.75 * W
    K = np.array([[f, 0.0, (W - 1) / 2 + 1.3], [0.0, 1.02 * f, (H - 1) / 2 - 0.8], [0.0, 0.0, 1.0]])
    ctx = pmv.Context(W, H, n_slots=N, max_tracks=64)
    map_id = ctx.remap_map_create(*pmv.undistort_map(K, DIST, (W, H), new_K=K))
    calls = {"build": lambda: ctx.frames_build(0, N), "remap": lambda: ctx.frames_remap(0, N, map_id, 0)}
    res = {}
    for name, call in calls.items():
        kern, wall, classes = [], [], None
        for k in range(args.warmup + args.passes):
            ctx.frames_stage(0, frames)
            ctx.prof_enable(True)
            call()
            ctx.sync()
            prof = ctx.prof_read()
            ctx.prof_enable(False)
            assert set(prof) == {"k_pad_level0", "k_pyrdown"}, prof
            classes = {c: prof[c][0] for c in prof}
            if k >= args.warmup:
                kern.append(sum(v[1] for v in prof.values()) * 1e3)
        for k in range(args.warmup + args.passes):
            ctx.frames_stage(0, frames)
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if k >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e6)
        res[name] = dict(kernel_us=round(statistics.median(kern), 1), kernel_min=round(min(kern), 1), kernel_max=round(max(kern), 1),
                         call_us=round(statistics.median(wall), 1), call_min=round(min(wall), 1), call_max=round(max(wall), 1), launches=classes)
        r = res[name]
        print(f"{name:5s}: kernels {r['kernel_us']:9.1f} us ({r['kernel_min']:.1f} .. {r['kernel_max']:.1f}) | call {r['call_us']:9.1f} us "
              f"({r['call_min']:.1f} .. {r['call_max']:.1f}) | launches {classes}", flush=True)
    extra = res["remap"]["kernel_us"] - res["build"]["kernel_us"]
    per_frame = extra / N
    gbs = BYTES_PER_PIXEL * W * H / (per_frame * 1e-6) / 1e9 if per_frame > 0 else None
    print(f"remap: {extra:.1f} us on top of the build for {N} frames = {per_frame:.2f} us per frame, {gbs and round(gbs, 1)} GB/s at {BYTES_PER_PIXEL:g} bytes per pixel; "
          f"the build alone {res['build']['kernel_us'] / N:.2f} us per frame")
    ctx.close()
    line = json.dumps(dict(bench="remap", w=W, h=H, frames=N, dist=list(DIST), border_value=0, passes=args.passes, build=res["build"], remap=res["remap"],
                           remap_us_per_frame=round(per_frame, 3), build_us_per_frame=round(res["build"]["kernel_us"] / N, 3),
                           bytes_per_pixel=BYTES_PER_PIXEL, remap_gb_per_s=gbs and round(gbs, 1)))
    print(line)
    if args.out:
        with open(args.out, "w") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
