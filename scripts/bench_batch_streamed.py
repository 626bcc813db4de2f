"""Streamed batched path against the staged one (pmv_pipeline_run_batch_streamed vs pmv_pipeline_run_batch), one JSON line.

bench.py's distinct-sequence layout: 16 distinct sequences (4 seeds x start offsets 0/40/80/120) of config 1 (1101 frames, 400 tracks,
bundle 5) cycled over B slots. In one process, at the same B:
  staged    frames staged in B x n slots first, then the batched run (what bench.py's batched leg times);
  pinned    the same frames streamed from page-locked host memory (torch pin_memory) through rings of `--ring` slots;
  pageable  the same from ordinary numpy arrays;
each timed `--passes` times, the legs alternated, every value and the median printed (frames = sum of n - init_offset, as bench.py counts).
Streamed legs run under each ingest form of `--modes` (PMV_BATCH_INGEST). Every streamed result is compared bitwise with the staged one.
Device memory of each context: hipMemGetInfo (torch.cuda.mem_get_info) before and after its creation. Finally one streamed run at
B = `--big` with full-length sequences, which staged storage cannot hold (256 x 1101 slots = 313 GB).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--frames", type=int, default=1101)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--ring", type=int, default=16)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--modes", default="mapped,copy", help="ingest forms of the streamed legs (PMV_BATCH_INGEST), comma-separated")
    ap.add_argument("--big", type=int, default=256, help="B of the final streamed-only run (0 = skip)")
    ap.add_argument("--no-staged", action="store_true", help="skip the staged leg (and the bitwise check)")
    args = ap.parse_args()
    import torch   # page-locked host memory and hipMemGetInfo
    pmv = importlib.import_module("practical-multi-view_amd")
    w, h, n, B = K00["w"], K00["h"], args.frames, args.batch
    K = np.array([K00["fx"], 0, K00["cx"], 0, K00["fy"], K00["cy"], 0, 0, 1.0])
    kw = dict(min_tracked=CFG1["min_tracked"], tol=CFG1["tol"], init_frames=5, bundle_size=CFG1["bundle_size"], ba_iterations=5, threaded=1,
              want_features=False)
    ctx_kw = dict(max_tracks=1024, max_ba_cams=8, max_ba_points=4096, max_ba_obs=32768)
    ncpu = int(os.environ.get("OMP_NUM_THREADS", "16"))

    # bench.py's distinct sequences: seeds cfg.seed + 64 + k, start offsets 0/40/80/120; a sequence is a view of its seed's buffer
    D, OFF = max(1, min(args.distinct, B)), 40
    n_seed = (D + 3) // 4
    gen = [pmv.synth_sequence(CFG1["seed"] + 64 + k, 0, n + OFF * (min(4, D - 4 * k) - 1), w, h, K00["fx"], K00["fy"], K00["cx"], K00["cy"],
                              nthreads=ncpu) for k in range(n_seed)]
    pinned_gen = []
    for fr, _ in gen:
        t = torch.empty(fr.shape, dtype=torch.uint8).pin_memory()
        t.numpy()[:] = fr
        pinned_gen.append(t)
    views = [(d // 4, OFF * (d % 4)) for d in range(D)]
    pageable = [(gen[k][0][o:o + n], gen[k][1][o:o + n]) for k, o in views]
    pinned = [(pinned_gen[k].numpy()[o:o + n], gen[k][1][o:o + n]) for k, o in views]

    def mem_free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    def count(res):
        return sum(n - int(r.stats["init_offset"]) for r in res)

    out = dict(metric="streamed batched path vs staged", B=B, n_frames=n, distinct_sequences=D, ring=args.ring, config="configs[1] (metric)",
               passes=args.passes, modes=args.modes.split(","), unit="frames/s")
    legs, runs = {}, {}
    staged_res = None
    mem = {}
    if not args.no_staged:
        f0 = mem_free()
        sc = pmv.Context(w, h, n_slots=B * n, **ctx_kw)
        mem["staged_ctx_bytes"] = f0 - mem_free()
        for b in range(B):
            sc.frames_stage(b * n, pageable[b % D][0])
        bseqs = [(b * n, n, pageable[b % D][1]) for b in range(B)]
        runs["staged"] = lambda: sc.pipeline_run_batch(bseqs, w, h, K, **kw)
    f0 = mem_free()
    rc = pmv.Context(w, h, n_slots=B * args.ring, **ctx_kw)
    mem["streamed_ctx_bytes_before_first_run"] = f0 - mem_free()
    for mode in out["modes"]:
        for kind, src in (("pinned", pinned), ("pageable", pageable)):
            seqs = [src[b % D] for b in range(B)]

            def run(seqs=seqs, mode=mode):
                os.environ["PMV_BATCH_INGEST"] = mode
                try:
                    return rc.pipeline_run_batch_streamed(seqs, w, h, K, ring=args.ring, **kw)
                finally:
                    del os.environ["PMV_BATCH_INGEST"]
            runs[f"{kind}_{mode}"] = run
    identical = {}
    ingest = {}
    for name, fn in runs.items():   # warm-up pass of every leg (engine, staging buffers), and the bitwise check
        res = fn()
        if name == "staged":
            staged_res = [r.poses.copy() for r in res]
        elif staged_res is not None:
            identical[name] = all(np.array_equal(r.poses, staged_res[b]) for b, r in enumerate(res))
        del res
    mem["streamed_ctx_bytes"] = f0 - mem_free()   # after its staging buffers exist
    for p in range(args.passes):
        for name, fn in runs.items():
            rc.sync()
            t0 = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t0
            legs.setdefault(name, []).append(round(count(res) / dt, 1))
            if name != "staged":
                ingest[name] = rc.batch_ingest_stats()
                ingest[name]["seconds"] = round(dt, 3)
            del res
    out["legs"] = {k: dict(values=v, median=statistics.median(v)) for k, v in legs.items()}
    if "staged" in legs:
        out["ratio_to_staged"] = {k: round(statistics.median(v) / statistics.median(legs["staged"]), 4) for k, v in legs.items() if k != "staged"}
    out["identical_to_staged"] = identical
    out["ingest"] = ingest
    out["device_memory"] = mem
    if not args.no_staged:
        del runs["staged"]
        sc.close()
    rc.close()
    if args.big:
        Bb = args.big
        f0 = mem_free()
        bc = pmv.Context(w, h, n_slots=Bb * args.ring, **ctx_kw)
        t0 = time.perf_counter()
        res = bc.pipeline_run_batch_streamed([pinned[b % D] for b in range(Bb)], w, h, K, ring=args.ring, **kw)
        dt = time.perf_counter() - t0
        mem_per_slot = None
        if "staged_ctx_bytes" in mem:
            mem_per_slot = mem["staged_ctx_bytes"] / (B * n)
        out["big"] = dict(B=Bb, n_frames=n, value=round(count(res) / dt, 1), seconds=round(dt, 3), source="pinned", mode=os.environ.get("PMV_BATCH_INGEST", "default"),
                          device_bytes=f0 - mem_free(), staged_bytes_would_be=None if mem_per_slot is None else round(mem_per_slot * Bb * n),
                          ingest=bc.batch_ingest_stats(), poses_per_sequence=[min(len(r.poses) for r in res), max(len(r.poses) for r in res)])
        bc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
