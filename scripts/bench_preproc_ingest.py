"""Remap and CLAHE inside the feeder (pmv_set_frame_preproc) against the streamed batch without them and against what a caller had to do
before, one JSON line (kept as profiles/preproc_ingest_bench.json when --out says so).

bench_colour_ingest.py's layout: distinct sequences (seeds x start offsets 0/40/80/120) of config 1 (1101 frames, 400 tracks, bundle 5)
cycled over B slots, streamed from pinned host memory on rings of `--ring` slots. The camera is a mild radial distortion (k1 = -0.05,
k2 = 0.01, new_K = K: every tap inside the frame), the equalisation cv's CLAHE(2.0, (8, 8)). In one process, each leg timed `--passes` times,
the legs alternated, every value and the median printed (frames = sum of n - init_offset):
  off / remap / clahe / both   pmv_pipeline_run_batch_streamed with the setting off, with the map, with CLAHE, with both;
  staged_<same>                what a caller has to do without the setting: frames_stage -> frames_remap -> frames_clahe ->
                               pipeline_run_batch on the same sequences in B x n slots, the preprocessing calls INSIDE the timed region,
                               the staging itself (a copy the streamed legs make too, inside theirs) reported beside it.
The legs track different images, so their results differ by design; what is compared bitwise is each streamed leg with its staged twin.
The script sets no threshold. `--batch` is for smaller boxes (the staged context holds B x n frames of device memory).
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
CFG1 = dict(min_tracked=400, tol=150, bundle_size=5, seed=1007)
DIST = (-0.05, 0.01)
CLAHE = (2.0, (8, 8))
LEGS = {"off": dict(), "remap": dict(remap=True), "clahe": dict(clahe=CLAHE), "both": dict(remap=True, clahe=CLAHE)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--frames", type=int, default=1101)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--ring", type=int, default=16)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--no-staged", action="store_true", help="skip the staged legs (B x n slots of device memory)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch   # page-locked host memory
    pmv = importlib.import_module("practical-multi-view_amd")
    w, h, n, B = K00["w"], K00["h"], args.frames, args.batch
    K = np.array([K00["fx"], 0, K00["cx"], 0, K00["fy"], K00["cy"], 0, 0, 1.0])
    kw = dict(min_tracked=CFG1["min_tracked"], tol=CFG1["tol"], init_frames=5, bundle_size=CFG1["bundle_size"], ba_iterations=5, threaded=1,
              want_features=False)
    ctx_kw = dict(max_tracks=1024, max_ba_cams=8, max_ba_points=4096, max_ba_obs=32768)
    ncpu = int(os.environ.get("OMP_NUM_THREADS", "16"))
    maps = pmv.undistort_map(K.reshape(3, 3), DIST, (w, h), new_K=K.reshape(3, 3))

    # bench.py's distinct sequences: seeds cfg.seed + 64 + k, start offsets 0/40/80/120; a sequence is a view of its seed's buffer
    D, OFF = max(1, min(args.distinct, B)), 40
    bufs, gts = [], []
    for k in range((D + 3) // 4):
        fr, gt = pmv.synth_sequence(CFG1["seed"] + 64 + k, 0, n + OFF * (min(4, D - 4 * k) - 1), w, h, K00["fx"], K00["fy"], K00["cx"], K00["cy"], nthreads=ncpu)
        t = torch.empty(fr.shape, dtype=torch.uint8).pin_memory()
        t.numpy()[:] = fr
        bufs.append(t)
        gts.append(gt)
    views = [(d // 4, OFF * (d % 4)) for d in range(D)]
    seqs = [(bufs[k].numpy()[o:o + n], gts[k][o:o + n]) for k, o in views]

    def count(res):
        return sum(n - int(r.stats["init_offset"]) for r in res)

    out = dict(metric="remap / CLAHE inside the feeder vs the streamed batch without them and vs stage -> remap -> clahe -> run", B=B, n_frames=n,
               distinct_sequences=D, ring=args.ring, config="configs[1] (metric)", passes=args.passes, unit="frames/s", dist=DIST, clahe=[CLAHE[0], list(CLAHE[1])])
    rc = pmv.Context(w, h, n_slots=B * args.ring, **ctx_kw)
    rc_map = rc.remap_map_create(*maps)
    runs, prepare, prep_s = {}, {}, {}
    for name, leg in LEGS.items():
        def run(leg=leg):
            rc.set_frame_preproc(remap=rc_map if leg.get("remap") else None, clahe=leg.get("clahe"))
            try:
                return rc.pipeline_run_batch_streamed([seqs[b % D] for b in range(B)], w, h, K, ring=args.ring, **kw)
            finally:
                rc.set_frame_preproc()
        runs[name] = (rc, run)
    sc = None
    if not args.no_staged:
        sc = pmv.Context(w, h, n_slots=B * n, **ctx_kw)
        sc_map = sc.remap_map_create(*maps)
        bseqs = [(b * n, n, seqs[b % D][1]) for b in range(B)]
        for name, leg in LEGS.items():
            def stage(name=name):
                t0 = time.perf_counter()
                for b in range(B):
                    sc.frames_stage(b * n, seqs[b % D][0])
                prep_s.setdefault(name, []).append(round(time.perf_counter() - t0, 3))
            prepare["staged_" + name] = stage

            def run(leg=leg):
                if leg.get("remap"):
                    sc.frames_remap(0, B * n, sc_map, 0)
                if leg.get("clahe"):
                    sc.frames_clahe(0, B * n, *leg["clahe"])
                # (a preprocessing call leaves built pyramids; the plain leg builds them in the run, as its callers do)
                return sc.pipeline_run_batch(bseqs, w, h, K, build_pyramids=0 if leg else 1, **kw)
            runs["staged_" + name] = (sc, run)
    identical, ingest, legs, launches = {}, {}, {}, {}
    want = {}
    for name, (c, fn) in runs.items():   # warm-up pass of every leg (engine, staging buffers, scratches) and the bitwise check
        if name in prepare:
            prepare[name]()
        before = c.debug_preproc_launches()
        res = fn()
        print(f"warm-up {name}", file=sys.stderr, flush=True)
        launches[name] = [a - b for a, b in zip(c.debug_preproc_launches(), before)]
        key = name[len("staged_"):] if name.startswith("staged_") else name
        if key not in want:
            want[key] = [r.poses.copy() for r in res]
        else:
            identical[name] = all(np.array_equal(r.poses, want[key][b]) for b, r in enumerate(res))
        del res
    for p in range(args.passes):
        for name, (c, fn) in runs.items():
            if name in prepare:
                prepare[name]()
            c.sync()
            t0 = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t0
            legs.setdefault(name, []).append(round(count(res) / dt, 1))
            print(f"pass {p} {name}: {legs[name][-1]} frames/s", file=sys.stderr, flush=True)
            if not name.startswith("staged_"):
                ingest[name] = c.batch_ingest_stats()
                ingest[name]["seconds"] = round(dt, 3)
            del res
    out["legs"] = {k: dict(values=v, median=statistics.median(v), spread=round((max(v) - min(v)) / statistics.median(v), 4)) for k, v in legs.items()}
    out["over_off"] = {k: round(statistics.median(v) / statistics.median(legs["off"]), 4) for k, v in legs.items() if k in LEGS and k != "off"}
    out["streamed_over_staged"] = {k: round(statistics.median(legs[k]) / statistics.median(legs["staged_" + k]), 4) for k in LEGS if "staged_" + k in legs}
    out["staged_identical_to_streamed"] = identical
    out["ingest"] = ingest
    out["preproc_launches_of_a_pass"] = launches
    out["staging_seconds_untimed"] = prep_s
    if sc is not None:
        sc.close()
    rc.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
