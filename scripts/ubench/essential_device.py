"""What a whole findEssentialMat costs on the device (pmv_find_essential_mat: one k_essential_ransac launch) against the host code
(orc_host_find_essential, one thread), and what per-request completion gives a session. One line per scene, one JSON line at the end.

Scenes: those of tests/test_essential_gpu.py - two views of a point cloud with 0.3 px noise, integer pixels, an outlier fraction f, and two
pure-noise scenes that run into the 1000-iteration cap. Per scene: the samples the RANSAC draws, microseconds per call on the device and on
the host (median of `--passes` calls after a warm-up; the device figure includes the copy-in and the wait for the completion word), and
whether the two agree in found / E / mask / samples.

Session: `--callers` threads (64) call pmv_batch_find_essential_mat at once, each on its own seq; caller 0 holds the n = 40 noise scene (the
full 1000 iterations), the others a fast scene. Every caller notes when its call returned. The slow request's return marks the end of its
round's launch (a round ends with its slowest workgroup); reported: how many callers returned before that, how long before (median), and
the time of the slow call itself. PMV_BATCH_LANES_FP=2 gives the class a second combiner; PMV_ESSENTIAL_R sets the hypotheses per in-kernel round.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENES = [("scene", 1, 8, 0.3), ("scene", 2, 65, 0.0), ("scene", 1, 64, 0.3), ("scene", 3, 64, 0.6), ("scene", 1, 300, 0.0), ("scene", 1, 300, 0.3),
          ("scene", 1, 300, 0.6), ("noise", 5, 40, 0.0), ("noise", 5, 200, 0.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--callers", type=int, default=64)
    ap.add_argument("--session-passes", type=int, default=5)
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    import orc_binding
    from test_twoview_host import K, _find_essential
    from test_essential_gpu import _points
    orc = orc_binding.load()
    ctx = pmv.Context(640, 200, n_slots=2, max_tracks=1024)
    rows = []
    for key in SCENES:
        p1, p2 = _points(*key)
        dev, host = [], []
        for k in range(args.warmup + args.passes):
            t0 = time.perf_counter()
            got = ctx.find_essential_mat(p1, p2, K)
            t1 = time.perf_counter()
            want = _find_essential(orc, p1, p2)
            t2 = time.perf_counter()
            if k >= args.warmup:
                dev.append((t1 - t0) * 1e6)
                host.append((t2 - t1) * 1e6)
        same = got[0] == want[0] and got[3] == want[3] and np.array_equal(got[2], want[2]) and (not want[0] or got[1].tobytes() == want[1].tobytes())
        row = dict(scene="%s seed %d n %d f %g" % key, samples=want[3], inliers=int(want[2].sum()), device_us=round(statistics.median(dev), 1), device_min=round(min(dev), 1),
                   host_us=round(statistics.median(host), 1), host_min=round(min(host), 1), same=bool(same))
        rows.append(row)
        print(f"{row['scene']:>28}: {row['samples']:4d} samples | device {row['device_us']:10.1f} us (min {row['device_min']:.1f}) | host {row['host_us']:9.1f} us (min {row['host_min']:.1f}) | "
              f"same bits: {same}", flush=True)
    # ---- 64 callers, one of them slow
    slow = _points("noise", 5, 40, 0.0)
    fast = _points("scene", 2, 65, 0.0)
    sess = []
    with ctx.batch_session(args.callers, [(640, 200)]):
        for k in range(1 + args.session_passes):
            start = threading.Barrier(args.callers + 1)
            done = [0.0] * args.callers

            def call(j):
                p1, p2 = slow if j == 0 else fast
                start.wait()
                ctx.batch_find_essential_mat(j, p1, p2, K)
                done[j] = time.perf_counter()
            th = [threading.Thread(target=call, args=(j,)) for j in range(args.callers)]
            for t in th:
                t.start()
            start.wait()
            t0 = time.perf_counter()
            for t in th:
                t.join()
            if k == 0:
                continue   # warm-up
            early = [done[0] - d for d in done[1:] if d < done[0]]
            sess.append(dict(returned_before_the_slow_request=len(early), of=args.callers - 1, median_lead_us=round(statistics.median(early) * 1e6, 1) if early else 0.0,
                             slow_call_us=round((done[0] - t0) * 1e6, 1), last_fast_call_us=round((max(done[1:]) - t0) * 1e6, 1)))
            print(f"session pass {k}: {sess[-1]}", flush=True)
    ctx.close()
    print(json.dumps(dict(bench="essential_device", R=os.environ.get("PMV_ESSENTIAL_R", "default"), lanes_fp=os.environ.get("PMV_BATCH_LANES_FP", "default"),
                          passes=args.passes, rows=rows, session=sess)))


if __name__ == "__main__":
    main()
