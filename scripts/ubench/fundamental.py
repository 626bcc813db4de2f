"""What a whole findFundamentalMat costs on the device (pmv_find_fundamental_mat: one k_fundamental_ransac launch) against its CPU twin on
one host core (tests/twin/fundamental_twin.cpp: what a KLT loop pays today is such a CPU call), per round width R, and what a session of B
callers pays per call. One line per row, one JSON line at the end, also written to `--out` (profiles/fundamental_ubench.json).

Scenes: tests/fundamental_common.py - two views of a point cloud with 0.3 px noise, integer pixels, float32, an outlier fraction f;
n in {150, 300, 1000}, f in {0.1, 0.3, 0.5}, threshold 1 px, confidence 0.99. Per scene and R in {8, 16, 32, 64}: microseconds per call
(median of `--passes` calls after a warm-up; the figure includes the copy-in and the wait for the completion word); per scene the twin's
microseconds and whether device and twin agree in found / F / mask / samples.

Session: B in {1, 16, 64} threads call pmv_batch_find_fundamental_mat at once, each on its own seq with its own scene (the nine scenes in
turn), `--session-passes` times; reported: the wall time of a pass over B (microseconds per call) and the median of the callers' own call times.
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

SCENES = [("scene", 1, n, f) for n in (150, 300, 1000) for f in (0.1, 0.3, 0.5)]
WIDTHS = (8, 16, 32, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--session-passes", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fundamental_ubench.json"))
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    import fundamental_common as fc
    tw = fc.twin()
    ctx = pmv.Context(640, 200, n_slots=2, max_tracks=1024)
    rows = []
    for key in SCENES:
        p1, p2 = fc.points(*key)
        host = []
        for k in range(args.warmup + args.passes):
            t0 = time.perf_counter()
            want = tw.find(p1, p2)
            if k >= args.warmup:
                host.append((time.perf_counter() - t0) * 1e6)
        row = dict(scene="n %d f %g" % key[2:], samples=want[3], inliers=int(want[2].sum()), twin_us=round(statistics.median(host), 1), device_us={}, same=True)
        for R in WIDTHS:
            assert ctx.lib.pmv_debug_set_fundamental_r(R) == 0
            dev = []
            for k in range(args.warmup + args.passes):
                t0 = time.perf_counter()
                got = ctx.find_fundamental_mat(p1, p2)
                if k >= args.warmup:
                    dev.append((time.perf_counter() - t0) * 1e6)
            row["device_us"][str(R)] = round(statistics.median(dev), 1)
            row["same"] = bool(row["same"] and got[0] == want[0] and got[3] == want[3] and np.array_equal(got[2], want[2]) and
                               (not want[0] or got[1].tobytes() == want[1].tobytes()))
        rows.append(row)
        print(f"{row['scene']:>12}: {row['samples']:4d} samples | twin {row['twin_us']:9.1f} us | device " +
              " ".join(f"R={R}: {row['device_us'][str(R)]:8.1f}" for R in WIDTHS) + f" us | same bits: {row['same']}", flush=True)
    assert ctx.lib.pmv_debug_set_fundamental_r(0) == 0
    session_R = ctx.lib.pmv_debug_fundamental_r()   # the default, or PMV_FUNDAMENTAL_R
    sess = []
    for B in (1, 16, 64):
        pts = [fc.points(*SCENES[j % len(SCENES)]) for j in range(B)]
        twin_us = sum(rows[j % len(SCENES)]["twin_us"] for j in range(B)) / B
        with ctx.batch_session(B, [(640, 200)]):
            walls, calls = [], []
            for k in range(1 + args.session_passes):
                start = threading.Barrier(B + 1)
                took = [0.0] * B

                def call(j):
                    start.wait()
                    t0 = time.perf_counter()
                    ctx.batch_find_fundamental_mat(j, *pts[j])
                    took[j] = time.perf_counter() - t0
                th = [threading.Thread(target=call, args=(j,)) for j in range(B)]
                for t in th:
                    t.start()
                start.wait()
                t0 = time.perf_counter()
                for t in th:
                    t.join()
                if k:   # (pass 0 warms up)
                    walls.append((time.perf_counter() - t0) * 1e6)
                    calls.append(statistics.median(took) * 1e6)
        sess.append(dict(callers=B, R=session_R, wall_us_per_call=round(statistics.median(walls) / B, 1), median_call_us=round(statistics.median(calls), 1),
                         twin_us_per_call=round(twin_us, 1)))
        print(f"session B={B}: {sess[-1]}", flush=True)
    ctx.close()
    line = json.dumps(dict(bench="fundamental", session_R=session_R, passes=args.passes, rows=rows, session=sess))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
