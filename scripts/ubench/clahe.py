"""What pmv_frames_clahe costs against the pyramid build it contains, one line per figure and one JSON line at the end (also written to --out).

64 synthetic 1241x376 frames, staged before every repetition (staging is not timed; a second equalisation would see another image), cv's
default parameters (clip 40, tiles 8x8). Two calls are timed, each the median of `--passes` repetitions after a warm-up:
  build: pmv_frames_build alone - code that exists without this call, the yardstick;
  clahe: pmv_frames_clahe, which contains the same build behind its two kernels.
  `*_kernel_us` = the sum of the call's launches by HIP events (the level-0 and pyrDown profiling classes; the equalisation's two kernels are
                  booked under level 0), from repetitions with the profiler on;
  `*_call_us`   = the host clock around the call and a synchronise, from repetitions with the profiler off.
The difference per frame and the bytes per second it implies (3 w h per frame: the histogram pass reads the image, the second pass reads and
writes it) are derived from the kernel figures.
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

W, H, N = 1241, 376, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.passes >= 20, "the median of at least 20 repetitions"
    pmv = importlib.import_module("practical-multi-view_amd")
    frames, _ = pmv.synth_sequence(1007, 10, N, W, H, 718.856, 718.856, 607.1928, 185.2157, nthreads=8)
    ctx = pmv.Context(W, H, n_slots=N, max_tracks=64)
    calls = {"build": lambda: ctx.frames_build(0, N), "clahe": lambda: ctx.frames_clahe(0, N)}
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
    extra = res["clahe"]["kernel_us"] - res["build"]["kernel_us"]
    per_frame = extra / N
    gbs = 3.0 * W * H / (per_frame * 1e-6) / 1e9 if per_frame > 0 else None
    print(f"equalisation: {extra:.1f} us on top of the build for {N} frames = {per_frame:.2f} us per frame, {gbs and round(gbs, 1)} GB/s at 3 w h bytes per frame; "
          f"the build alone {res['build']['kernel_us'] / N:.2f} us per frame")
    ctx.close()
    line = json.dumps(dict(bench="clahe", w=W, h=H, frames=N, clip_limit=40.0, tiles=[8, 8], passes=args.passes, build=res["build"], clahe=res["clahe"],
                           equalisation_us_per_frame=round(per_frame, 3), build_us_per_frame=round(res["build"]["kernel_us"] / N, 3),
                           equalisation_gb_per_s=gbs and round(gbs, 1)))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
