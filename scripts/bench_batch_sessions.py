"""What B plugin-level callers reach through a batch session (pmv_batch_open .. pmv_batch_close), one JSON line.

B sequences run the front-end chain of tests/test_batch_session_gpu.py - upload frame k into a ring of 3 slots, GFTT (20 corners per grid
cell) on frame 0 and again every `--redetect` frames, pyramidal LK from frame k - 1 to k on the truncated survivors - two ways on ONE context:
  session  B ctypes threads (ctypes releases the GIL during a call), every call a pmv_batch_* session call: the uploads meet in the upload
           class's rounds, the LK and detector requests in the combiners' launches;
  single   the same B chains through pmv_frame_upload / pmv_detect_gftt / pmv_lk_track, one after the other on one thread - the
           single-sequence calls allow one call per role at a time, so this is what B such callers get without a session. These calls are
           the parent commit's, unchanged.
Each leg is timed `--passes` times after a warm-up, alternated; frames/s = B * frames / wall time of the leg, every value and the median
printed. The tracked points of the two legs are compared bitwise. The callers are Python threads: their share of interpreter time between
two calls (argument packing, np.trunc of the survivors) is serialised by the GIL in the session leg and is part of both figures.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Chain:
    """one sequence's front-end loop on buffers of its own; `session` picks the pmv_batch_* calls"""

    def __init__(self, pmv, ctx, frames, ring, redetect, session):
        self.lib, self.h, self.frames, self.ring, self.redetect, self.session = ctx.lib, ctx.h, frames, ring, redetect, session
        h, w = frames[0].shape
        self.w, self.hh = w, h
        self.cells = np.ascontiguousarray(pmv.grid_cells(w, h))
        nc = len(self.cells)
        self.xy = np.zeros((nc, 20, 2), np.int32)
        self.cnt = np.zeros(nc, np.int32)
        n = 20 * nc
        self.out, self.st, self.err = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
        self.trace = []

    def _ck(self, rc):
        if rc != 0:
            raise RuntimeError(f"pmv error {rc}: {self.lib.pmv_last_error(self.h).decode()}")

    def _detect(self, slot):
        f = self.lib.pmv_batch_detect_gftt if self.session else self.lib.pmv_detect_gftt
        self._ck(f(self.h, slot, _p(self.cells, C.c_int), len(self.cells), 20, C.c_double(0.01), C.c_double(5.0), _p(self.xy, C.c_int), _p(self.cnt, C.c_int)))
        return np.concatenate([self.xy[i, : self.cnt[i]] + self.cells[i, :2] for i in range(len(self.cells))]).astype(np.float32)

    def run(self):
        lib, h = self.lib, self.h
        pts = None
        self.trace = []
        for k, f in enumerate(self.frames):
            slot = self.ring[k % 3]
            if self.session:
                self._ck(lib.pmv_batch_frame_upload(h, slot, _p(f, C.c_uint8), self.w, self.hh, self.w, 0))
            else:
                self._ck(lib.pmv_frame_upload(h, slot, _p(f, C.c_uint8), self.w, self.hh, self.w))
            if k % self.redetect == 0:
                pts = self._detect(slot)
                continue
            n = len(pts)
            pts = np.ascontiguousarray(pts)
            lk = lib.pmv_batch_lk_track if self.session else lib.pmv_lk_track
            self._ck(lk(h, self.ring[(k - 1) % 3], slot, _p(pts, C.c_float), n, _p(self.out, C.c_float), _p(self.st, C.c_uint8), _p(self.err, C.c_float)))
            pts = np.trunc(self.out[:n][self.st[:n] > 0])
            self.trace.append(pts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64, help="B: sequences = caller threads of the session leg")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--size", default="1241x376")
    ap.add_argument("--distinct", type=int, default=4, help="distinct sequences (start offsets 0, 10, .. of one generated run) cycled over the B callers")
    ap.add_argument("--redetect", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    pmv = importlib.import_module("practical-multi-view_amd")
    w, h = (int(v) for v in args.size.split("x"))
    B, n = args.batch, args.frames
    allf, _ = pmv.synth_sequence(1000, 0, n + 10 * (args.distinct - 1), w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=16)
    seqs = [np.ascontiguousarray(allf[10 * (b % args.distinct): 10 * (b % args.distinct) + n]) for b in range(B)]
    ctx = pmv.Context(w, h, n_slots=3 * B, max_tracks=1024)
    single = [Chain(pmv, ctx, seqs[b], [3 * b, 3 * b + 1, 3 * b + 2], args.redetect, False) for b in range(B)]
    session = [Chain(pmv, ctx, seqs[b], [3 * b, 3 * b + 1, 3 * b + 2], args.redetect, True) for b in range(B)]

    def leg_single():
        t0 = time.perf_counter()
        for c in single:
            c.run()
        return time.perf_counter() - t0

    def leg_session():
        errors = []

        def run(c):
            try:
                c.run()
            except Exception as e:   # noqa: BLE001
                errors.append(repr(e))
        ctx.batch_open(B, [(w, h)])
        try:
            th = [threading.Thread(target=run, args=(c,)) for c in session]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            dt = time.perf_counter() - t0
            up = ctx.batch_upload_stats()
        finally:
            ctx.batch_close()
        if errors:
            raise RuntimeError(errors[0])
        return dt, up
    s0 = ctx.batch_stats()
    leg_single(); leg_session()   # warm-up
    t_single, t_session, up = [], [], None
    for _ in range(args.passes):
        t_single.append(leg_single())
        dt, up = leg_session()
        t_session.append(dt)
    s1 = ctx.batch_stats()
    same = all(len(a.trace) == len(b.trace) and all(np.array_equal(x, y) for x, y in zip(a.trace, b.trace)) for a, b in zip(single, session))
    tracked = int(np.mean([len(c.trace[-1]) for c in single]))

    def fps(ts):
        return [round(B * n / t, 1) for t in ts]

    def med(ts):
        return round(B * n / statistics.median(ts), 1)
    print(json.dumps({
        "bench": "batch_sessions", "B": B, "frames": n, "size": [w, h], "passes": args.passes, "bitwise_equal": bool(same), "tracked_at_end": tracked,
        "session_frames_per_s": fps(t_session), "single_frames_per_s": fps(t_single),
        "session_median": med(t_session), "single_median": med(t_single), "ratio": round(med(t_session) / med(t_single), 2),
        "uploads_last_pass": up,
        "lk_requests_per_round": round((s1["lk"]["requests"] - s0["lk"]["requests"]) / max(1, s1["lk"]["launches"] - s0["lk"]["launches"]), 2),
        "det_requests_per_round": round((s1["det"]["requests"] - s0["det"]["requests"]) / max(1, s1["det"]["launches"] - s0["det"]["launches"]), 2),
    }))
    ctx.close()
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
