"""What a batch of mixed frame sizes buys (pmv_pipeline_run_batch_streamed with sizes per sequence), one JSON line.

B sequences, a third each of the three KITTI odometry sizes (A 1241x376: sequences 00-02, B 1242x375: 03, C 1226x370: 04-10), config 1
(400 tracks, bundle 5), streamed from page-locked host memory through rings of `--ring` slots, on ONE context, two ways:
  mixed     ONE batch of all B sequences (rounds hold all three sizes);
  by_size   three consecutive batches of B/3, one per size - the only way to run them before sizes were per sequence;
each timed `--passes` times after a warm-up, the legs alternated, every value and the median printed. frames/s = all frames (sum of
n - init_offset, as bench.py counts) / total wall time of the leg. The results of the two legs are compared bitwise.
With KITTI_ROOT set the sequences are read with kitti.load_sequence instead (00, 03, 04, cut to `--frames`); otherwise the synthetic corridor.
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

SIZES = [dict(name="A", kitti="00", w=1241, h=376, f=718.856, cx=607.1928, cy=185.2157),
         dict(name="B", kitti="03", w=1242, h=375, f=721.5377, cx=609.5593, cy=172.854),
         dict(name="C", kitti="04", w=1226, h=370, f=707.0912, cx=601.8873, cy=183.1104)]
CFG1 = dict(min_tracked=400, tol=150, bundle_size=5, seed=1007)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192, help="sequences in all (a multiple of 3)")
    ap.add_argument("--frames", type=int, default=1101)
    ap.add_argument("--distinct", type=int, default=4, help="distinct sequences per size (start offsets 0, 40, .. of one generated run)")
    ap.add_argument("--ring", type=int, default=16)
    ap.add_argument("--passes", type=int, default=5)
    args = ap.parse_args()
    if args.batch % 3 or args.batch < 3:
        ap.error("--batch must be a multiple of 3")
    import torch   # page-locked host memory
    pmv = importlib.import_module("practical-multi-view_amd")
    n, B, D, OFF = args.frames, args.batch, max(1, args.distinct), 40
    kw = dict(min_tracked=CFG1["min_tracked"], tol=CFG1["tol"], init_frames=5, bundle_size=CFG1["bundle_size"], ba_iterations=5, threaded=1,
              want_features=False)
    ncpu = int(os.environ.get("OMP_NUM_THREADS", "16"))
    kitti_root = os.environ.get("KITTI_ROOT")
    per_size, keep = [], []
    for k, S in enumerate(SIZES):
        if kitti_root:
            kitti = importlib.import_module("practical-multi-view_amd.kitti")
            frames, gt, Kk = kitti.load_sequence(kitti_root, S["kitti"], n=n + OFF * (D - 1))
            frames = np.ascontiguousarray(frames)
            Kk = np.asarray(Kk, np.float64).reshape(9)
        else:
            frames, gt = pmv.synth_sequence(CFG1["seed"] + 64 + k, 0, n + OFF * (D - 1), S["w"], S["h"], S["f"], S["f"], S["cx"], S["cy"], nthreads=ncpu)
            Kk = np.array([S["f"], 0, S["cx"], 0, S["f"], S["cy"], 0, 0, 1.0])
        t = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()
        t.numpy()[:] = frames
        keep.append(t)
        per_size.append(([(t.numpy()[OFF * d:OFF * d + n], gt[OFF * d:OFF * d + n]) for d in range(D)], Kk))
    third = B // 3
    # sequence b of the mixed batch: size b % 3 (the sizes interleaved, as the pieces of one rank would be), distinct sequence (b // 3) % D
    mixed = [per_size[b % 3][0][(b // 3) % D] for b in range(B)]
    mixed_K = np.stack([per_size[b % 3][1] for b in range(B)])
    by_size = [([per_size[k][0][j % D] for j in range(third)], per_size[k][1]) for k in range(3)]
    ctx = pmv.Context(max(S["w"] for S in SIZES), max(S["h"] for S in SIZES), n_slots=B * args.ring, max_tracks=1024, max_ba_cams=8, max_ba_points=4096,
                      max_ba_obs=32768)

    def run_mixed():
        return ctx.pipeline_run_batch_streamed(mixed, K=mixed_K, ring=args.ring, **kw)

    def run_by_size():
        res = [ctx.pipeline_run_batch_streamed(seqs, K=Kk, ring=args.ring, **kw) for seqs, Kk in by_size]
        return [res[b % 3][b // 3] for b in range(B)]   # in the mixed batch's order

    def count(res):
        return sum(n - int(r.stats["init_offset"]) for r in res)

    runs = dict(mixed=run_mixed, by_size=run_by_size)
    poses = {name: [r.poses.copy() for r in fn()] for name, fn in runs.items()}   # warm-up pass of each leg, and the bitwise check
    identical = all(np.array_equal(a, b) for a, b in zip(poses["mixed"], poses["by_size"]))
    legs, ingest = {}, {}
    for _ in range(args.passes):
        for name, fn in runs.items():
            ctx.sync()
            t0 = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t0
            legs.setdefault(name, []).append(round(count(res) / dt, 1))
            if name == "mixed":
                ingest = ctx.batch_ingest_stats()
            del res
    out = dict(metric="one batch of mixed frame sizes vs one batch per size", B=B, n_frames=n, sizes=[f"{S['w']}x{S['h']}" for S in SIZES],
               distinct_per_size=D, ring=args.ring, config="configs[1] (metric)", passes=args.passes, unit="frames/s",
               source="kitti" if kitti_root else "synthetic corridor",
               legs={k: dict(values=v, median=statistics.median(v), spread=round(max(v) - min(v), 1)) for k, v in legs.items()},
               mixed_over_by_size=round(statistics.median(legs["mixed"]) / statistics.median(legs["by_size"]), 4),
               identical=identical, ingest_mixed=ingest, launches=ctx.batch_launches(), combiners=ctx.batch_stats())
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
