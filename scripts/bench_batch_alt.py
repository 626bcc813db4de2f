"""The plugin pairs on the batch engine: (extractor, matcher) = (0,0) GFTT + LK (the control), (2,0) FAST + LK, (2,1) kNN over FAST. One JSON
line, kept as profiles/batch_alt_bench.json.

bench.py's distinct sequences (4 seeds x start offsets 0/40/80/120 of config 1: 400 tracks, bundle 5), cycled over B staged slots. Per B
(one context per B: the engine's round-forming threshold follows the B it was created for) and per pair:
  batched     frames/s of pmv_pipeline_run_batch, `--passes` passes alternated between the pairs, every value and the median;
  sequential  the same B sequences one after another through pmv_pipeline_run on one context (all a user had for (2,0) and (2,1) before the
              batch engine served them), timed once over the distinct sequences and scaled by their share of the B slots;
every batched result is compared bitwise (poses) with its single run. pmv_batch_stats of the last pass: requests per round and us per
round of the lk and det combiners (the kNN requests are served by the lk combiners).
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K00 = dict(w=1241, h=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)
PAIRS = {"gftt_lk": (0, 0), "fast_lk": (2, 0), "fast_knn": (2, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 192])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_alt_bench.json"))
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    w, h, n = K00["w"], K00["h"], args.frames
    K = np.array([K00["fx"], 0, K00["cx"], 0, K00["fy"], K00["cy"], 0, 0, 1.0])
    kw = dict(min_tracked=400, tol=150, init_frames=5, bundle_size=5, ba_iterations=5, threaded=1, want_features=False)
    ctx_kw = dict(max_tracks=2048, max_ba_cams=8, max_ba_points=4096, max_ba_obs=32768)   # (the kNN matcher carries up to ~1400 features)
    ncpu = int(os.environ.get("OMP_NUM_THREADS", "16"))
    D, OFF = args.distinct, 40
    distinct = []
    for k in range((D + 3) // 4):
        fr, gt = pmv.synth_sequence(1007 + 64 + k, 0, n + 3 * OFF, w, h, K00["fx"], K00["fy"], K00["cx"], K00["cy"], nthreads=ncpu)
        distinct += [(fr[OFF * d: OFF * d + n], gt[OFF * d: OFF * d + n]) for d in range(4)]
    distinct = distinct[:D]

    def count(res):
        return sum(n - int(r.stats["init_offset"]) for r in res)

    out = dict(metric="plugin pairs on the batch engine, batched vs one sequence after another", n_frames=n, distinct_sequences=D, passes=args.passes,
               unit="frames/s", pairs={k: list(v) for k, v in PAIRS.items()}, results={})
    # the single runs: one context, one sequence after another
    single, seq_rate = {}, {}
    sc = pmv.Context(w, h, n_slots=n, **ctx_kw)
    for name, (ex, ma) in PAIRS.items():
        frames_done, dt = 0, 0.0
        for d, (fr, gt) in enumerate(distinct):
            sc.frames_stage(0, fr)
            sc.sync()
            t0 = time.perf_counter()
            r = sc.pipeline_run(n, w, h, K, gt, extractor=ex, matcher=ma, **kw)
            dt += time.perf_counter() - t0
            frames_done += n - int(r.stats["init_offset"])
            single[(name, d)] = r.poses.copy()
        seq_rate[name] = round(frames_done / dt, 1)
        print(f"sequential {name}: {seq_rate[name]} frames/s", file=sys.stderr, flush=True)
    sc.close()
    for B in args.batch:
        ctx = pmv.Context(w, h, n_slots=B * n, **ctx_kw)
        for b in range(B):
            ctx.frames_stage(b * n, distinct[b % D][0])
        seqs = [(b * n, n, distinct[b % D][1]) for b in range(B)]
        legs, identical, stats = {}, {}, {}
        for name, (ex, ma) in PAIRS.items():   # warm-up pass and the bitwise check
            res = ctx.pipeline_run_batch(seqs, w, h, K, extractor=ex, matcher=ma, **kw)
            identical[name] = all(np.array_equal(r.poses, single[(name, b % D)]) for b, r in enumerate(res))
            del res
        for p in range(args.passes):
            for name, (ex, ma) in PAIRS.items():
                ctx.sync()
                s0 = ctx.batch_stats()
                t0 = time.perf_counter()
                res = ctx.pipeline_run_batch(seqs, w, h, K, extractor=ex, matcher=ma, **kw)
                dt = time.perf_counter() - t0
                s1 = ctx.batch_stats()
                legs.setdefault(name, []).append(round(count(res) / dt, 1))
                stats[name] = {role: dict(requests_per_round=round((s1[role]["requests"] - s0[role]["requests"]) / max(1, s1[role]["launches"] - s0[role]["launches"]), 2),
                                          us_per_round=round(1e6 * (s1[role]["work_s"] - s0[role]["work_s"]) / max(1, s1[role]["launches"] - s0[role]["launches"]), 1),
                                          rounds=s1[role]["launches"] - s0[role]["launches"]) for role in ("lk", "det")}
                print(f"B={B} pass {p} {name}: {legs[name][-1]} frames/s", file=sys.stderr, flush=True)
                del res
        ctx.close()
        out["results"][str(B)] = {name: dict(batched=v, batched_median=statistics.median(v), sequential=seq_rate[name],
                                             ratio=round(statistics.median(v) / seq_rate[name], 2), identical_to_single_runs=identical[name],
                                             combiners=stats[name]) for name, v in legs.items()}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
