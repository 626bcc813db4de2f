"""A bad argument is refused alike by every form of a plugin call: the single call (pmv_*) and the session call (pmv_batch_*) return the same
status code and a message with the same words, nothing is queued for a combiner, and the session goes on serving.

Set-up: a context of 96x64 with 3 slots and max_tracks = 64; slots 0 and 1 hold built 96x64 frames of noise, slot 2 a built 64x48 frame; a
session with both sizes declared and n_seq = 1. The calls are made through the raw library entry points, so that no argument is stopped by
the binding first. The table's codes and words are those of the library's check functions (lk_check, lkx_check, knn_check, detect_check,
gftt_ex_check, gftt_mask_check, fast_check, subpix_check and the entry points' own first lines); the `who` column is the call whose name the
message carries, which for some calls is the single call's name in both forms."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, CAPACITY = 0, -2, -3
W, H, MAX_TRACKS = 96, 64, 64


class _GfttParams(C.Structure):   # pmv_gftt_params
    _fields_ = [("quality", C.c_double), ("min_dist", C.c_double), ("block_size", C.c_int), ("use_harris", C.c_int), ("k", C.c_double)]


class _SubpixParams(C.Structure):   # pmv_subpix_params
    _fields_ = [("win_w", C.c_int), ("win_h", C.c_int), ("zero_w", C.c_int), ("zero_h", C.c_int), ("max_iter", C.c_int), ("eps", C.c_double)]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Calls:
    """the raw calls with good default arguments; form = "single" (pmv_*) or "session" (pmv_batch_*). Each returns (status, counts or None)."""

    def __init__(self, ctx, form):
        self.ctx, self.lib, self.pre = ctx, ctx.lib, "pmv_" if form == "single" else "pmv_batch_"

    def fn(self, name):
        f = getattr(self.lib, self.pre + name)
        f.argtypes = None   # (the binding declares some of them on first use: the raw arguments below are complete ctypes values)
        return f

    def lk(self, name="lk_track", prev=0, nxt=1, n=4, flags=None, init=None, null_out=False, null_back=False):
        xy = np.full((MAX_TRACKS + 1, 2), 20.0, np.float32)
        out = np.zeros((MAX_TRACKS + 1, 2), np.float32) if init is None else init
        st, err = np.zeros(MAX_TRACKS + 1, np.uint8), np.zeros(MAX_TRACKS + 1, np.float32)
        args = [self.ctx.h, prev, nxt, _ptr(xy), n, _ptr(out)] + ([] if flags is None else [flags]) + [_ptr(None if null_out else st), _ptr(err)]
        if name == "lk_track_fb":
            bxy, bst, berr = np.zeros((MAX_TRACKS + 1, 2), np.float32), np.zeros(MAX_TRACKS + 1, np.uint8), np.zeros(MAX_TRACKS + 1, np.float32)
            args += [_ptr(bxy), _ptr(None if null_back else bst), _ptr(berr)]
        return self.fn(name)(*args), None

    def knn(self, n=4, m=4, neighbours=7, window=15):
        src, cmp_ = np.full((MAX_TRACKS + 1, 2), 20, np.int32), np.full((MAX_TRACKS + 1, 2), 22, np.int32)
        best, err = np.zeros(MAX_TRACKS + 1, np.int32), np.zeros(MAX_TRACKS + 1, np.float32)
        return self.fn("knn_match")(self.ctx.h, 0, 1, _ptr(src), n, _ptr(cmp_), m, neighbours, window, _ptr(best), _ptr(err)), None

    @staticmethod
    def _cells(cell, n_cells):
        return np.ascontiguousarray(np.tile(np.asarray(cell, np.int32), (max(n_cells, 1), 1)))

    def detect(self, name, slot=0, cell=(0, 0, 32, 32), n_cells=1, max_per_cell=5, null_response=False):
        """detect_gftt, detect_shitomasi or detect_fast over n_cells copies of `cell`"""
        cells = self._cells(cell, n_cells)
        per = max(n_cells, 1) * max(max_per_cell, 1)
        xy, cnt = np.zeros((per, 2), np.int32), np.full(max(n_cells, 1), 7, np.int32)
        if name == "detect_gftt":
            rc = self.fn(name)(self.ctx.h, slot, _ptr(cells), n_cells, max_per_cell, C.c_double(0.01), C.c_double(5.0), _ptr(xy), _ptr(cnt))
        elif name == "detect_shitomasi":
            rc = self.fn(name)(self.ctx.h, slot, _ptr(cells), n_cells, max_per_cell, C.c_double(0.4), _ptr(xy), _ptr(np.zeros(per, np.float64)), _ptr(cnt))
        else:
            rc = self.fn(name)(self.ctx.h, slot, _ptr(cells), n_cells, max_per_cell, 10, 1, _ptr(xy), _ptr(None if null_response else np.zeros(per, np.float32)), _ptr(cnt))
        return rc, cnt

    def gftt_ex(self, block_size=3, quality=0.01, min_dist=5.0, mask_stride=None):
        cells = self._cells((0, 0, 32, 32), 1)
        xy, cnt = np.zeros((5, 2), np.int32), np.zeros(1, np.int32)
        p = _GfttParams(quality, min_dist, block_size, 0, 0.04)
        mask = None if mask_stride is None else np.full((H, W), 255, np.uint8)
        return self.fn("detect_gftt_ex")(self.ctx.h, 0, _ptr(cells), 1, 5, C.byref(p), _ptr(mask), mask_stride or 0, _ptr(xy), _ptr(cnt)), None

    def subpix(self, win=5, max_iter=30, eps=0.01, n=4, point=20.0):
        xy = np.full((MAX_TRACKS + 1, 2), 20.0, np.float32)
        xy[0, 0] = point
        p = _SubpixParams(win, win, -1, -1, max_iter, eps)
        return self.fn("corner_subpix")(self.ctx.h, 0, _ptr(xy), n, C.byref(p), None, None), None


def _inf_flow():
    a = np.full((MAX_TRACKS + 1, 2), 20.0, np.float32)
    a[1, 1] = np.inf
    return a


# (what, the call, status, words of the message, the call the message names: in the single form / in the session form)
ROWS = [
    ("LK: n = 65", lambda c: c.lk(n=65), CAPACITY, ("max_tracks", "n=65"), ("pmv_lk_track:", "pmv_lk_track:")),
    ("LK: slot 3", lambda c: c.lk(nxt=3), CAPACITY, ("slot out of range",), ("pmv_lk_track:", "pmv_lk_track:")),
    ("LK: slots 0 and 2", lambda c: c.lk(nxt=2), INVALID, ("sizes differ",), ("pmv_lk_track:", "pmv_lk_track:")),
    ("LK: a null output with n > 0", lambda c: c.lk(null_out=True), INVALID, ("null argument",), ("pmv_lk_track:", "pmv_lk_track:")),
    ("LK-ex: flag bit 1", lambda c: c.lk("lk_track_ex", flags=1), INVALID, ("flags = 0x1",), ("pmv_lk_track_ex:", "pmv_batch_lk_track_ex:")),
    ("LK-ex: an infinite initial flow", lambda c: c.lk("lk_track_ex", flags=4, init=_inf_flow()), INVALID, ("initial flow of point 1",),
     ("pmv_lk_track_ex:", "pmv_batch_lk_track_ex:")),
    ("LK-fb: a null back output", lambda c: c.lk("lk_track_fb", flags=0, null_back=True), INVALID, ("null argument",), ("pmv_lk_track_fb:", "pmv_batch_lk_track_fb:")),
    ("kNN: 9 neighbours", lambda c: c.knn(neighbours=9), INVALID, ("n_neighbours 1..8",), ("pmv_knn_match:", "pmv_knn_match:")),
    ("kNN: window 64", lambda c: c.knn(window=64), INVALID, ("window 1..63",), ("pmv_knn_match:", "pmv_knn_match:")),
    ("kNN: m = 65", lambda c: c.knn(m=65), CAPACITY, ("max_tracks", "m=65"), ("pmv_knn_match:", "pmv_knn_match:")),
]
for _name in ("detect_gftt", "detect_shitomasi"):
    ROWS += [
        (f"{_name}: n_cells = 65", lambda c, f=_name: c.detect(f, n_cells=65), CAPACITY, ("n_cells=65",), ("detect:", "detect:")),
        (f"{_name}: max_per_cell = 4097", lambda c, f=_name: c.detect(f, max_per_cell=4097), CAPACITY, ("max_per_cell=4097",), ("detect:", "detect:")),
        (f"{_name}: a 2x2 cell", lambda c, f=_name: c.detect(f, cell=(0, 0, 2, 2)), INVALID, ("cell 0 (0,0,2,2) invalid",), ("detect:", "detect:")),
        (f"{_name}: a cell past the frame edge", lambda c, f=_name: c.detect(f, cell=(90, 0, 10, 10)), INVALID, ("cell 0 (90,0,10,10) invalid for 96x64",),
         ("detect:", "detect:")),
        (f"{_name}: slot 3", lambda c, f=_name: c.detect(f, slot=3), CAPACITY, ("slot out of range",), ("detect:", "detect:")),
    ]
ROWS += [
    ("detect_shitomasi: max_per_cell = 0 with n_cells = 0", lambda c: c.detect("detect_shitomasi", n_cells=0, max_per_cell=0), INVALID, ("bad argument",),
     ("pmv_detect_shitomasi:", "pmv_detect_shitomasi:")),
    ("detect_fast: max_per_cell = 0 with n_cells = 0", lambda c: c.detect("detect_fast", n_cells=0, max_per_cell=0), INVALID, ("bad argument",),
     ("pmv_detect_fast:", "pmv_detect_fast:")),
    ("GFTT-ex: block_size = 16", lambda c: c.gftt_ex(block_size=16), INVALID, ("block_size = 16",), ("pmv_detect_gftt_ex:", "pmv_batch_detect_gftt_ex:")),
    ("GFTT-ex: quality = 0", lambda c: c.gftt_ex(quality=0.0), INVALID, ("quality = 0",), ("pmv_detect_gftt_ex:", "pmv_batch_detect_gftt_ex:")),
    ("GFTT-ex: min_dist = -1", lambda c: c.gftt_ex(min_dist=-1.0), INVALID, ("min_dist = -1",), ("pmv_detect_gftt_ex:", "pmv_batch_detect_gftt_ex:")),
    ("GFTT-ex: a mask stride of 95", lambda c: c.gftt_ex(mask_stride=95), CAPACITY, ("mask_stride = 95", "frame width 96"),
     ("pmv_detect_gftt_ex:", "pmv_batch_detect_gftt_ex:")),
    ("FAST: a null response", lambda c: c.detect("detect_fast", null_response=True), INVALID, ("null output",), ("pmv_detect_fast:", "pmv_detect_fast:")),
    ("FAST: a 0x5 cell", lambda c: c.detect("detect_fast", cell=(0, 0, 0, 5)), INVALID, ("cell 0 (0,0,0,5) invalid",), ("pmv_detect_fast:", "pmv_detect_fast:")),
    ("cornerSubPix: win = 0", lambda c: c.subpix(win=0), INVALID, ("win = (0, 0)",), ("pmv_corner_subpix:", "pmv_batch_corner_subpix:")),
    ("cornerSubPix: max_iter = 0", lambda c: c.subpix(max_iter=0), INVALID, ("max_iter = 0",), ("pmv_corner_subpix:", "pmv_batch_corner_subpix:")),
    ("cornerSubPix: eps = NaN", lambda c: c.subpix(eps=float("nan")), INVALID, ("eps =", "negative or not finite"), ("pmv_corner_subpix:", "pmv_batch_corner_subpix:")),
    ("cornerSubPix: a NaN point", lambda c: c.subpix(point=float("nan")), INVALID, ("point 0", "not finite"), ("pmv_corner_subpix:", "pmv_batch_corner_subpix:")),
    ("cornerSubPix: n = 65", lambda c: c.subpix(n=65), CAPACITY, ("n=65", "max_tracks=64"), ("pmv_corner_subpix:", "pmv_batch_corner_subpix:")),
]


def _counters(ctx):
    """what the combiners have been handed and have launched so far"""
    st = ctx.batch_stats()
    return ({k: (v["launches"], v["requests"]) for k, v in st.items()}, ctx.batch_launches(), ctx.debug_subpix_launches()[1:])


def test_every_form_refuses_alike_and_queues_nothing(pmv, gpu_ctx_factory):
    rng = np.random.default_rng(11)
    ctx = gpu_ctx_factory(W, H, n_slots=3, max_tracks=MAX_TRACKS)
    with ctx.batch_session(1, [(W, H), (64, 48)]):
        ctx.batch_frame_upload(0, rng.integers(0, 256, (H, W), dtype=np.uint8))
        ctx.batch_frame_upload(1, rng.integers(0, 256, (H, W), dtype=np.uint8))
        ctx.batch_frame_upload(2, rng.integers(0, 256, (48, 64), dtype=np.uint8))
        before = _counters(ctx)
        failures = []
        for form, who in (("single", 0), ("session", 1)):
            calls = _Calls(ctx, form)
            for what, call, code, words, names in ROWS:
                rc, _ = call(calls)
                msg = ctx.lib.pmv_last_error(ctx.h).decode()
                if rc != code or not all(s in msg for s in words) or names[who] not in msg:
                    failures.append(f"{form} {what}: status {rc} (expected {code}), message {msg!r} (expected {names[who]!r} and {words})")
            # the legal short cut: max_per_cell = 0 with valid cells is no error, every count is 0 and nothing is launched
            for name in ("detect_shitomasi", "detect_fast"):
                rc, cnt = calls.detect(name, n_cells=3, max_per_cell=0)
                if rc != OK or cnt.tolist() != [0, 0, 0]:
                    failures.append(f"{form} {name} with max_per_cell = 0: status {rc}, counts {cnt.tolist()}")
        assert not failures, "\n".join(failures)
        assert _counters(ctx) == before, "a refused call or a max_per_cell = 0 call reached a combiner"
        # the session still serves, with the single calls' bits
        cells = pmv.grid_cells(W, H)
        det = ctx.batch_detect_gftt(0, cells, 20)
        p0 = np.concatenate([d + c[:2] for c, d in zip(cells, det)]).astype(np.float32)
        got = ctx.batch_lk_track(0, 1, p0)
        after = _counters(ctx)
        assert after[0]["det"] == (before[0]["det"][0] + 1, before[0]["det"][1] + 1) and after[0]["lk"][1] == before[0]["lk"][1] + 1
        want_det = ctx.detect_gftt(0, cells, 20)
        want = ctx.lk_track(0, 1, p0)
    assert len(p0) > 0 and all(np.array_equal(a, b) for a, b in zip(det, want_det))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
