"""What an N-view triangulation of a window's landmarks costs on the device (pmv_triangulate_tracks: one k_tri_tracks launch, one lane per
landmark) against its CPU twin on one host core (tests/twin/tri_tracks_twin.cpp), and what a session of 16 callers pays per call against 16
single calls one after the other. One line per row, one JSON line at the end, also written to `--out` (profiles/tri_tracks_ubench.json).

Scenes: tests/tri_tracks_common.py - a corridor of cameras 0.8 apart, pixel observations with 0.5 px noise; (landmarks, mean views) =
(200, 4), (1000, 6), (4000, 10), each with refine_iters 0 and 5, every gate on. Per row: microseconds per call (median of `--passes` calls
after a warm-up; the device figure includes the host's counting sort, the copy-in and the wait for the completion word; both go through the
same ctypes marshalling), and whether device and twin agree in every output bit.

Session: 16 threads call pmv_batch_triangulate_tracks at once, each on its own seq, on the (1000, 6) scene with refine_iters 5,
`--session-passes` times; reported: the wall time of a pass over 16 (microseconds per call), the median of the callers' own call times,
and the same 16 calls as single calls in a row.
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

SCENES = [(200, 6, 2), (1000, 10, 2), (4000, 12, 8)]   # (landmarks, cameras, fewest views): views uniform in fewest..cameras
SESSION_CALLERS = 16


def _median_us(fn, warmup, passes):
    took, out = [], None
    for k in range(warmup + passes):
        t0 = time.perf_counter()
        out = fn()
        if k >= warmup:
            took.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(took), 1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--session-passes", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tri_tracks_ubench.json"))
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    import tri_tracks_common as tc
    tw = tc.twin()
    ctx = pmv.Context(640, 200, n_slots=2, max_tracks=1024, max_ba_cams=12, max_ba_points=4096, max_ba_obs=49152)
    rows, scenes = [], {}
    for n_pts, nc, min_v in SCENES:
        sc = scenes[n_pts] = tc.scene(nc, n_pts, 9000 + n_pts, noise_px=0.5, pixel=True, min_v=min_v)
        for it in (0, 5):
            p = tc.gates_on(True, refine_iters=it)
            twin_us, want = _median_us(lambda: tw.run(sc["P"], sc["obs"], sc["cam"], sc["pt"], n_pts, p), args.warmup, args.passes)
            device_us, got = _median_us(lambda: ctx.triangulate_tracks(sc["P"], sc["obs"], sc["cam"], sc["pt"], n_pts, p), args.warmup, args.passes)
            same = bool(got[0].tobytes() == want["xyz"].tobytes() and np.array_equal(got[1], want["status"]) and got[2].tobytes() == want["err"].tobytes() and
                        got[3] == want["good"])
            rows.append(dict(landmarks=n_pts, observations=len(sc["obs"]), mean_views=round(len(sc["obs"]) / n_pts, 2), refine_iters=it, good=want["good"],
                             twin_us=twin_us, device_us=device_us, same=same))
            r = rows[-1]
            print(f"np {n_pts:5d} views {r['mean_views']:5.2f} refine {it}: twin {twin_us:9.1f} us | device {device_us:8.1f} us | good {r['good']} | same bits: {same}", flush=True)
    B = SESSION_CALLERS
    sc, p = scenes[1000], tc.gates_on(True, refine_iters=5)
    a = (sc["P"], sc["obs"], sc["cam"], sc["pt"], 1000, p)
    seq_us, _ = _median_us(lambda: [ctx.triangulate_tracks(*a) for _ in range(B)], 1, args.session_passes)
    with ctx.batch_session(B, [(640, 200)]):
        walls, calls = [], []
        for k in range(1 + args.session_passes):
            start = threading.Barrier(B + 1)
            took = [0.0] * B

            def call(j):
                start.wait()
                t0 = time.perf_counter()
                ctx.batch_triangulate_tracks(j, *a)
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
    launches, requests = ctx.tri_tracks_launches()
    twin_us = next(r["twin_us"] for r in rows if r["landmarks"] == 1000 and r["refine_iters"] == 5)
    sess = dict(callers=B, wall_us_per_call=round(statistics.median(walls) / B, 1), median_call_us=round(statistics.median(calls), 1),
                sequential_single_us_per_call=round(seq_us / B, 1), twin_us_per_call=twin_us)
    print(f"session B={B}: {sess}", flush=True)
    ctx.close()
    line = json.dumps(dict(bench="tri_tracks", passes=args.passes, rows=rows, session=sess, launches=launches, requests=requests))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
