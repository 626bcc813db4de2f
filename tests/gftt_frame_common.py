"""Shared by the tests of pmv_detect_gftt_frame, next to tests/gftt_common.py (the twin, the synthetic scenes, the masks): the frames that a
whole-frame call needs - more than 8 tiles a side, ragged last tiles, x above 255, pixel indices above 65 535 -, an independent numpy
selection, and the raw ctypes call. Everything handed out is computed once and shared; callers must not modify it."""
import ctypes as C

import numpy as np

import gftt_common as gc

W1, H1 = 517, 261      # 17 x 9 tiles, ragged right and bottom, width no multiple of 4
W2, H2 = 768, 512      # the context's capacity: 24 x 16 tiles
MAX_CORNERS = 16384    # PMV_GFTT_FRAME_MAX_CORNERS
INVALID, CAPACITY, OVERFLOW = -2, -3, -6
_i32p = C.POINTER(C.c_int32)


def rect_frame(pmv, w=W1, h=H1):
    """the synthetic scene of the other detector tests (high-contrast rectangles seen by a moving camera) at this size"""
    return gc.frame(pmv, w, h)


def plateau_frame(w=W1, h=H1):
    """isolated single bright pixels on a 16-pixel lattice ([::16, ::16] = 255): every one off the border gives the same response, so 512
    records tie in value and are ordered by address alone - with x > 255 and y * w + x > 65 535"""
    def make():
        img = np.zeros((h, w), np.uint8)
        img[::16, ::16] = 255
        return img
    return gc.cached(("plateau", w, h), make)


def noise(w, h):
    return gc.noise_frame(w, h)


def whole(img):
    return np.asarray([0, 0, img.shape[1], img.shape[0]], np.int32)


def twin_region(img, roi, max_corners, **kw):
    """(corners, records above the threshold) of the twin with the region as its cell, computed once per case"""
    key = ("frame-twin", id(img), tuple(int(v) for v in roi), int(max_corners), tuple(sorted((k, id(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items())))
    r = gc.cached(key, lambda: gc.twin().cell(img, roi, max_corners, **kw))
    return r[0], r[3]


def numpy_selection(resp, max_corners, quality, min_dist, mask=None):
    """cv::goodFeaturesToTrack's selection on a response map, written independently of the twin: masked maximum, threshold, 3x3 test on the
    thresholded map, stable sort by (value, address) descending, O(n^2) greedy. Returns ((n, 2) int32 corners, records above the threshold)."""
    h, w = resp.shape
    allowed = np.ones((h, w), bool) if mask is None else mask != 0
    vals = resp[allowed & ~np.isnan(resp)]
    mx = float(vals.max()) if vals.size else 0.0
    thr = np.float32(mx * quality)
    t = np.where(resp > thr, resp, np.float32(0))
    pad = np.pad(t, 1, mode="constant", constant_values=0)
    nb = np.max(np.stack([pad[j:j + h, i:i + w] for j in range(3) for i in range(3)]), axis=0)
    cand = (t != 0) & (t == nb) & allowed
    cand[0, :] = cand[-1, :] = False
    cand[:, 0] = cand[:, -1] = False
    ys, xs = np.nonzero(cand)
    idx = ys.astype(np.int64) * w + xs
    v = t[ys, xs]
    order = np.lexsort((-idx, -v.astype(np.float64)))   # value descending, then address descending
    out = []
    md2 = min_dist * min_dist
    for o in order:
        x, y = int(xs[o]), int(ys[o])
        if min_dist >= 1 and out:
            a = np.asarray(out)
            if (((a[:, 0] - x) ** 2 + (a[:, 1] - y) ** 2) < md2).any():
                continue
        out.append((x, y))
        if max_corners > 0 and len(out) == max_corners:
            break
    return np.asarray(out, np.int32).reshape(-1, 2), len(order)


def grid_union(pmv, img, max_corners_per_cell_total, **kw):
    """what the 255-grid gives: the twin per cell of pmv.grid_cells, frame coordinates; the per-cell limit is the frame's limit shared out"""
    h, w = img.shape
    cells = pmv.grid_cells(w, h)
    per = max(max_corners_per_cell_total // len(cells), 1)
    return np.concatenate([gc.twin().corners(img, c, per, **kw) + np.asarray(c[:2]) for c in cells])


def raw_frame_call(ctx, fn, slot, roi, max_corners, params, mask, stride, xy, out_cap, cnt):
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    roi = None if roi is None else np.ascontiguousarray(roi, np.int32)
    return fn(ctx.h, slot, None if roi is None else roi.ctypes.data, max_corners, None if params is None else C.cast(C.pointer(params), C.c_void_p),
              None if mask is None else mask.ctypes.data, stride, None if xy is None else xy.ctypes.data, out_cap, None if cnt is None else cnt.ctypes.data)
