"""N x pmv_knn_match with n = 900 source features against m = 1000 candidates on two frames of the synthetic corridor: a small target
for `rocprofv3 --kernel-trace --stats -- python scripts/ubench/knn_only.py` (the kNN kernel's mean time). Writes the results of the last
call to $OUT (an .npz) so that two builds can be compared on the same inputs."""
import importlib, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
pmv = importlib.import_module("practical-multi-view_amd")
W, H = 1241, 376
fr, _ = pmv.synth_sequence(1007, 0, 2, W, H, 718.856, 718.856, 607.1928, 185.2157, nthreads=16)
ctx = pmv.Context(W, H, n_slots=2, max_tracks=2048)
ctx.frame_upload(0, fr[0]); ctx.frame_upload(1, fr[1])
whole = np.asarray([[0, 0, W, H]], np.int32)
src = ctx.detect_fast(0, whole, 900)[0][0]      # what the matcher is given: FAST keypoints of both frames
cmp_xy = ctx.detect_fast(1, whole, 1000)[0][0]
assert len(src) == 900 and len(cmp_xy) == 1000, (len(src), len(cmp_xy))
N = int(os.environ.get("N", "200"))
ctx.knn_match(0, 1, src, cmp_xy)
t0 = time.perf_counter()
for _ in range(N):
    best, err = ctx.knn_match(0, 1, src, cmp_xy)
print("%.1f us per call (host clock around the synchronous call), n=%d m=%d" % ((time.perf_counter() - t0) / N * 1e6, len(src), len(cmp_xy)))
if os.environ.get("OUT"):
    np.savez(os.environ["OUT"], best=best, err=err)
ctx.close()
