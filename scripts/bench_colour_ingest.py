"""Colour (BGR) host frames against gray ones on the batched paths (pmv_set_frame_format), one JSON line, kept as
profiles/colour_ingest_bench.json.

bench_batch_streamed.py's layout: 16 distinct sequences (4 seeds x start offsets 0/40/80/120) of config 1 (1101 frames, 400 tracks,
bundle 5) cycled over B slots. The colour frames are the gray ones plus three smooth per-channel offset fields; the GRAY legs run on the
BGR2GRAY of those colour frames (numpy twin of the 14-bit formula), so both formats do the same tracking work. In one process, at the same B
and ring, each leg timed `--passes` times, the legs alternated, every value and the median printed (frames = sum of n - init_offset):
  gray_staged / bgr_staged        frames staged in B x n slots first (not timed; one context, re-staged in the leg's format before each
                                  pass: two staged contexts of 234 GB do not fit), then the batched run over the staged slots;
  gray_<src>_<mode> / bgr_...     streamed from pinned (torch pin_memory) or pageable host memory under each ingest form of `--modes`
                                  (PMV_BATCH_INGEST). The B slots share the 16 distinct source buffers, so the pinned footprint is
                                  16 x (n + 120) x w x h x (1 + 3) bytes whatever B.
Every result is compared bitwise with the gray staged one. Then the level-0 kernels: per-launch time and achieved bytes/s of k_pad_level0_bgr
next to k_pad_level0 from pmv_prof, staging the same 63 frames from the HBM landing area in both formats (per slot: w h or 3 w h read,
(w + 128)(h + 128) written), and the per-launch times of one streamed run of each format under each form.
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


def bgr2gray(bgr):
    """numpy twin of cv::cvtColor(BGR2GRAY) for 8-bit images (tests/test_oracle_frontend.py pins the oracle and the kernels to it)"""
    out = np.empty(bgr.shape[:-1], np.uint8)
    for i in range(bgr.shape[0]):   # frame by frame: the int32 temporaries stay small
        f = bgr[i].astype(np.int32)
        out[i] = (f[..., 0] * 1868 + f[..., 1] * 9617 + f[..., 2] * 4899 + 8192) >> 14
    return out


def colourise(gray, out):
    n, h, w = gray.shape
    yy, xx = np.mgrid[0:h, 0:w]
    fields = (25 + 20 * np.sin(2 * np.pi * xx / w * 1.5), -20 + 15 * np.cos(2 * np.pi * yy / h), 10 + 25 * np.sin(2 * np.pi * (xx + yy) / (w + h) * 2))
    for c, f in enumerate(fields):
        o = np.rint(f).astype(np.int16)
        for i in range(n):
            out[i, :, :, c] = np.clip(gray[i].astype(np.int16) + o, 0, 255)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--frames", type=int, default=1101)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--ring", type=int, default=16)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--modes", default="mapped,copy", help="ingest forms of the streamed legs (PMV_BATCH_INGEST), comma-separated")
    ap.add_argument("--no-staged", action="store_true", help="skip the staged legs (B x n slots of device memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_ingest_bench.json"))
    args = ap.parse_args()
    import torch   # page-locked host memory
    pmv = importlib.import_module("practical-multi-view_amd")
    w, h, n, B = K00["w"], K00["h"], args.frames, args.batch
    K = np.array([K00["fx"], 0, K00["cx"], 0, K00["fy"], K00["cy"], 0, 0, 1.0])
    kw = dict(min_tracked=CFG1["min_tracked"], tol=CFG1["tol"], init_frames=5, bundle_size=CFG1["bundle_size"], ba_iterations=5, threaded=1,
              want_features=False)
    ctx_kw = dict(max_tracks=1024, max_ba_cams=8, max_ba_points=4096, max_ba_obs=32768)
    ncpu = int(os.environ.get("OMP_NUM_THREADS", "16"))
    modes = args.modes.split(",")

    # bench.py's distinct sequences: seeds cfg.seed + 64 + k, start offsets 0/40/80/120; a sequence is a view of its seed's buffer
    D, OFF = max(1, min(args.distinct, B)), 40
    n_seed = (D + 3) // 4
    src = {"gray": {"pinned": [], "pageable": []}, "bgr": {"pinned": [], "pageable": []}}
    gts = []
    for k in range(n_seed):
        fr, gt = pmv.synth_sequence(CFG1["seed"] + 64 + k, 0, n + OFF * (min(4, D - 4 * k) - 1), w, h, K00["fx"], K00["fy"], K00["cx"], K00["cy"], nthreads=ncpu)
        gts.append(gt)
        tb = torch.empty(fr.shape + (3,), dtype=torch.uint8).pin_memory()
        colourise(fr, tb.numpy())
        tg = torch.empty(fr.shape, dtype=torch.uint8).pin_memory()
        tg.numpy()[:] = bgr2gray(tb.numpy())
        src["bgr"]["pinned"].append(tb)
        src["gray"]["pinned"].append(tg)
        src["bgr"]["pageable"].append(tb.numpy().copy())
        src["gray"]["pageable"].append(tg.numpy().copy())
    views = [(d // 4, OFF * (d % 4)) for d in range(D)]

    def seqs_of(fmt, kind):
        bufs = [t.numpy() if kind == "pinned" else t for t in src[fmt][kind]]
        return [(bufs[k][o:o + n], gts[k][o:o + n]) for k, o in views]

    def count(res):
        return sum(n - int(r.stats["init_offset"]) for r in res)

    out = dict(metric="colour (BGR) host frames vs gray on the batched paths", B=B, n_frames=n, distinct_sequences=D, ring=args.ring,
               config="configs[1] (metric)", passes=args.passes, modes=modes, unit="frames/s",
               pinned_source_bytes=sum(t.numel() for f in src.values() for t in f["pinned"]))
    runs, prepare, staging_s = {}, {}, {}
    sc = None
    if not args.no_staged:
        sc = pmv.Context(w, h, n_slots=B * n, **ctx_kw)
        for fmt in ("gray", "bgr"):
            sq = seqs_of(fmt, "pinned")
            bseqs = [(b * n, n, sq[b % D][1]) for b in range(B)]

            def stage(fmt=fmt, sq=sq):
                sc.set_frame_format(fmt)
                t0 = time.perf_counter()
                for b in range(B):
                    sc.frames_stage(b * n, sq[b % D][0])
                staging_s.setdefault(fmt, []).append(round(time.perf_counter() - t0, 3))
            prepare[f"{fmt}_staged"] = stage
            runs[f"{fmt}_staged"] = (sc, lambda bseqs=bseqs: sc.pipeline_run_batch(bseqs, w, h, K, **kw))
    rc = pmv.Context(w, h, n_slots=B * args.ring, **ctx_kw)
    for mode in modes:
        for kind in ("pinned", "pageable"):
            for fmt in ("gray", "bgr"):
                sq = seqs_of(fmt, kind)
                seqs = [sq[b % D] for b in range(B)]

                def run(seqs=seqs, mode=mode, fmt=fmt):
                    os.environ["PMV_BATCH_INGEST"] = mode
                    rc.set_frame_format(fmt)
                    try:
                        return rc.pipeline_run_batch_streamed(seqs, w, h, K, ring=args.ring, **kw)
                    finally:
                        del os.environ["PMV_BATCH_INGEST"]
                runs[f"{fmt}_{kind}_{mode}"] = (rc, run)
    identical, ingest, legs, kernels = {}, {}, {}, {}
    want = None
    for name, (c, fn) in runs.items():   # warm-up pass of every leg (engine, staging buffers), the bitwise check, and the kernels' times
        streamed = not name.endswith("_staged")
        if name in prepare:
            prepare[name]()
        if streamed:
            c.prof_enable(True)
            c.prof_select(["k_pad_level0", "k_pad_level0_bgr", "k_pyrdown"])
        res = fn()
        print(f"warm-up {name}", file=sys.stderr, flush=True)
        if streamed:
            c.sync()
            kernels[name] = {k: dict(launches=v[0], mean_us=round(1e3 * v[1] / v[0], 2), max_us=round(1e3 * v[2], 2)) for k, v in c.prof_read().items()}
            c.prof_enable(False)
        if want is None:
            want = [r.poses.copy() for r in res]
        else:
            identical[name] = all(np.array_equal(r.poses, want[b]) for b, r in enumerate(res))
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
            if not name.endswith("_staged"):
                ingest[name] = c.batch_ingest_stats()
                ingest[name]["seconds"] = round(dt, 3)
            del res
    out["legs"] = {k: dict(values=v, median=statistics.median(v), spread=round((max(v) - min(v)) / statistics.median(v), 4)) for k, v in legs.items()}
    out["bgr_over_gray"] = {k[4:]: round(statistics.median(v) / statistics.median(legs["gray_" + k[4:]]), 4) for k, v in legs.items() if k.startswith("bgr_")}
    out["identical_to_first_leg"] = identical
    out["ingest"] = ingest
    out["level0_kernels_streamed"] = kernels
    if sc is not None:
        out["staging_seconds_untimed"] = staging_s   # B x n frames from pinned memory through the landing area, per pass
        sc.close()
    rc.close()
    print(json.dumps(out), file=sys.stderr, flush=True)   # (kept if the kernel part below fails)

    # the level-0 kernels from the HBM landing area: 63 frames = one gray chunk / three BGR chunks of 21, every launch timed by pmv_prof
    kc = pmv.Context(w, h, n_slots=64, **ctx_kw)
    pad = {}
    for fmt, name, bpp in (("gray", "k_pad_level0", 1), ("bgr", "k_pad_level0_bgr", 3)):
        frames = src[fmt]["pinned"][0].numpy()[:63]
        kc.set_frame_format(fmt)
        kc.frames_stage(0, frames)   # warm-up
        per = []
        for p in range(max(args.passes, 5)):
            kc.prof_enable(True)
            kc.prof_select([name])
            kc.frames_stage(0, frames)
            launches, total_ms, _ = kc.prof_read()[name]
            kc.prof_enable(False)
            per.append(1e3 * total_ms / 63)   # us per slot
        us = statistics.median(per)
        pad[name] = dict(us_per_slot=[round(v, 3) for v in per], median_us_per_slot=round(us, 3), launches_per_63_frames=launches,
                         bytes_per_slot=bpp * w * h + (w + 128) * (h + 128), GB_per_s=round((bpp * w * h + (w + 128) * (h + 128)) / us * 1e-3, 1))
    kc.close()
    out["level0_from_hbm"] = pad
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
