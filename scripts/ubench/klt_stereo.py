"""What the stereo stage costs inside the tracker step (pmv_klt_step_stereo, pmv_klt_step_many_stereo) next to the same work through the
calls that existed before it: path A is pmv_klt_step followed by pmv_lk_track_fb(cur, right) on the returned list (for a group:
pmv_klt_step_many followed by one pmv_lk_track_fb per tracker) with the stereo rule in numpy, path B is the one stereo call. One line per
case and one JSON line at the end (kept as profiles/klt_stereo_ubench.json; --out names the file).

Frames 640x480 and 1241x376 (synthetic, consecutive; `--seeds` different sequences, dealt out to the trackers in turn); the right frame of
a left frame is tests/klt_stereo_common.py's (two disparities and an occluder). Target 150 with radius = min_dist = 30, rejectWithF on,
forward-backward 0.5 px and border 1 in both the tracker and the stereo setting. One tracker through the single form, then groups of 2, 4
and 16 through the many form. A pass runs a path from empty lists over the frames; the first step of a pass only detects and is not timed.
Before anything is timed one pass of each path is compared: every tracker must return the same bytes at every step, right outputs
included. Each figure is the median over `--repeats` passes of the host clock around one frame of the whole group (both paths end in their
waits), with the smallest and the largest frame. The two paths alternate pass by pass and the order flips from repeat to repeat. The
profiler is off. Both paths run through the Python binding: the rule of path A (a few boolean operations on 150 tracks) is part of what a
caller of the two calls pays.

Without --case the script only starts one child process per frame size, each under a time limit of its own, one after the other; the first
child that fails or runs out of time ends the script with its status, and nothing more is started.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = [(640, 480), (1241, 376)]
GROUPS = [2, 4, 16]
TARGET, DIST = 150, 30
CASE_LIMIT_S = 240


def _mls(v):
    return dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))


def run_case(args, w, h):
    pmv = importlib.import_module("practical-multi-view_amd")
    import klt_common as kc
    import klt_stereo_common as ks
    nf, st = args.frames, ks.STEREO["fb"]
    lefts = [pmv.synth_sequence(1007 + k, 10, nf, w, h, 0.58 * w, 0.58 * w, w / 2, h / 2, nthreads=8)[0] for k in range(args.seeds)]
    rts = [[ks.right_of(f) for f in seq] for seq in lefts]
    ctx = pmv.Context(w, h, n_slots=2 * nf * max(GROUPS), max_tracks=1024)
    for j in range(max(GROUPS)):   # tracker j: left frame i in slot 2 nf j + i, right frame i in slot 2 nf j + nf + i
        kc.upload(ctx, lefts[j % args.seeds], first_slot=2 * nf * j)
        kc.upload(ctx, rts[j % args.seeds], first_slot=2 * nf * j + nf)
    p = kc.params(target=TARGET, radius=DIST, min_dist=float(DIST), reject_f=True)
    rows = []
    for n_trk in [1] + GROUPS:
        many = n_trk > 1
        trackers = [ctx.klt_create(**p) for _ in range(n_trk)]
        for t in trackers:
            t.set_stereo(**st)

        def slots(i):
            base = [2 * nf * j for j in range(n_trk)]
            return [b + max(i - 1, 0) for b in base], [b + i for b in base], [b + nf + i for b in base]

        def reset():
            for t in trackers:
                t.set_tracks([], [], [], 0)

        def two_call_pass(times=None, keep=None):
            reset()
            for i in range(nf):
                ps, cs, rs = slots(i)
                t0 = time.perf_counter()
                left = ctx.klt_step_many(trackers, ps, cs) if many else [trackers[0].step(ps[0], cs[0])]
                out = []
                for j, o in enumerate(left):
                    rxy, rst = ks.rule(o[2], ctx.lk_track_fb(cs[j], rs[j], o[2]), st, w, h) if len(o[2]) else ks.rule(o[2], None, st, w, h)
                    out.append(ks.with_matched(o, rst) + (rxy, rst))
                if times is not None and i > 0:
                    times.append((time.perf_counter() - t0) * 1e6)
                if keep is not None:
                    keep.append(out)

        def stereo_pass(times=None, keep=None):
            reset()
            for i in range(nf):
                ps, cs, rs = slots(i)
                t0 = time.perf_counter()
                out = ctx.klt_step_many_stereo(trackers, ps, cs, rs) if many else [trackers[0].step_stereo(ps[0], cs[0], rs[0])]
                if times is not None and i > 0:
                    times.append((time.perf_counter() - t0) * 1e6)
                if keep is not None:
                    keep.append(out)

        a, b = [], []
        two_call_pass(keep=a)
        stereo_pass(keep=b)
        for fa, fb in zip(a, b):
            for x, y in zip(fa, fb):
                kc.same(x[:5], y[:5])   # the two paths differ: nothing to time
                ks.same_right(x[5:], y[5:])
        for _ in range(args.warmup):
            two_call_pass()
            stereo_pass()
        s0 = ctx.debug_klt_stereo_stats()
        t_a, t_b = [], []
        for rep in range(args.repeats):
            pair = [(two_call_pass, t_a), (stereo_pass, t_b)]
            for fn, out in (pair if rep % 2 == 0 else pair[::-1]):
                fn(times=out)
        s1 = ctx.debug_klt_stereo_stats()
        calls = (s1[1] - s0[1]) if many else (s1[0] - s0[0])
        ua, ub = _mls(t_a), _mls(t_b)
        row = dict(w=w, h=h, target=TARGET, radius=DIST, reject_f=1, n_trk=n_trk, form="many" if many else "single", two_calls_us=ua, stereo_us=ub,
                   saved_us=round(ua["median"] - ub["median"], 1), ratio=round(ub["median"] / ua["median"], 3),
                   stereo_waits_per_call=round((s1[2] - s0[2]) / calls, 2), stereo_launches_per_call=round((s1[3] - s0[3]) / calls, 2),
                   counts=[[int(v) for v in o[4]] for o in b[-1]])
        rows.append(row)
        print(f"{w}x{h}, {n_trk:2d} tracker(s), {row['form']:6s}: step + lk_track_fb {ua['median']:8.1f} us [{ua['min']:.1f} .. {ua['max']:.1f}] | "
              f"stereo step {ub['median']:8.1f} us [{ub['min']:.1f} .. {ub['max']:.1f}] | B/A {row['ratio']:.3f}, {row['saved_us']:.1f} us saved | "
              f"{row['stereo_waits_per_call']} waits, {row['stereo_launches_per_call']} launches a call", flush=True)
        for t in trackers:
            t.close()
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--case", type=int, nargs=2, metavar=("W", "H"), help="run this frame size in this process and print its rows as one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_stereo_ubench.json"))
    args = ap.parse_args()
    if args.case:
        print("ROWS " + json.dumps(run_case(args, *args.case)), flush=True)
        return 0
    rows = []
    for w, h in FRAMES:   # one child per frame size, each under its own limit; a failure ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(w), str(h), "--frames", str(args.frames), "--repeats", str(args.repeats), "--warmup", str(args.warmup),
               "--seeds", str(args.seeds)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=CASE_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{w}x{h}: no result within {CASE_LIMIT_S} s; nothing more is started", file=sys.stderr)
            return 124
        lines = r.stdout.splitlines()
        print("\n".join(ln for ln in lines if not ln.startswith("ROWS ")), flush=True)
        if r.returncode != 0:
            print(f"{w}x{h}: the child ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        rows += json.loads(next(ln for ln in lines if ln.startswith("ROWS "))[5:])
    doc = dict(bench="klt_stereo", frames=args.frames, repeats=args.repeats, warmup=args.warmup, seeds=args.seeds, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
