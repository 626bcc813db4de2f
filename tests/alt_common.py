"""Shared by the tests that take ShiTomasi, FAST and the kNN matcher off their default arguments (tests/test_alt_plugins_gpu.py and the CPU
cases of tests/test_oracle_alt.py / tests/test_oracle_frontend.py): the frame sizes, the seeded images and the candidate lists.

Every frame is small and none is a multiple of 4 wide. Everything handed out is computed once and shared; callers must not modify it."""
import numpy as np

SMALL, MID, WIDE, TALL = (97, 67), (224, 131), (333, 121), (300, 260)   # (w, h); TALL only where a 255x255 cell is needed
KNN_LDS_M, KNN_WAVES, ST_CAP, MAX_CELLS = 1024, 4, 8192, 64            # csrc/frontend_alt.hip, csrc/frontend.hip, csrc/pmv_ctx.h

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _rng(kind, w, h):
    return np.random.default_rng([{"noise": 1, "binary": 2, "periodic": 3}[kind], w, h])


def noise(w, h):
    """uniform uint8"""
    return cached(("noise", w, h), lambda: _rng("noise", w, h).integers(0, 256, (h, w), dtype=np.uint8))


def binary(w, h):
    """0 or 255 per pixel"""
    return cached(("binary", w, h), lambda: (_rng("binary", w, h).integers(0, 2, (h, w)) * 255).astype(np.uint8))


def flat(w, h):
    return cached(("flat", w, h), lambda: np.full((h, w), 128, np.uint8))


def periodic(w, h):
    """a 16x16 noise tile repeated over the frame: every response value occurs once per period"""
    def make():
        tile = _rng("periodic", w, h).integers(0, 256, (16, 16), dtype=np.uint8)
        return np.ascontiguousarray(np.tile(tile, (h // 16 + 1, w // 16 + 1))[:h, :w])
    return cached(("periodic", w, h), make)


def shifted(w, h):
    """the noise image rolled by (1, 2): one row down, two columns right - the second frame of the kNN pairs"""
    return cached(("shifted", w, h), lambda: np.ascontiguousarray(np.roll(noise(w, h), (1, 2), (0, 1))))


def points(seed, w, h, n, margin=0):
    """n (x, y) int32 rows drawn uniformly, NOT made unique; margin > 0 lets them leave the frame by up to that many pixels on every side"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(-margin, w + margin, n), rng.integers(-margin, h + margin, n)], 1).astype(np.int32)


def knn_sweep_lists(w, h):
    """the parameter sweep's lists: 9 sources with (0, 0), (w - 1, h - 1) and (3, h - 2) among them; 300 candidates, not unique, with five
    duplicated rows and one row at a source's own coordinates"""
    def make():
        src = points(11, w, h, 9)
        src[0] = (0, 0); src[1] = (w - 1, h - 1); src[2] = (3, h - 2)
        src[3] = (w // 2, h // 2)                      # a window of 65x65 that lies inside the smallest frame almost whole
        cand = points(12, w, h, 300)
        cand[10] = src[3] + (3, -2)                    # near that source, so that at least one large window is compared
        cand[100:105] = cand[40:45]                    # five duplicated rows
        cand[7] = src[4]                               # a candidate at a source's own coordinates
        cand[200] = cand[10]                           # and a duplicate of a near neighbour
        return src, cand
    return cached(("knn_sweep", w, h), make)


def knn_length_lists(w, h, m, n_nn):
    """21 sources and m candidates (not unique) for the list lengths on both sides of KNN_LDS_M. From m = 1023 on the first 20 candidates
    are the first 20 sources plus a small random offset. From m = 1025 on the LAST candidate is the true match of source 20: the shifted
    frame is the noise frame rolled by (2, 1) in (x, y), so the window at source + (2, 1) is the source's own and its error is 0. Under the
    `_err < err || err == 0` rule a zero error survives only in the last neighbour compared, so n_nn - 1 candidates at Chebyshev distance 1
    (indices 20 ..) come before it and no other candidate is as near as its distance of 2: the best fit of source 20 is index m - 1 >= 1024."""
    def make():
        rng = np.random.default_rng(13)
        src = np.concatenate([points(14, w - 60, h - 40, 20) + (40, 20), [[12, 60]]]).astype(np.int32)
        cand = points(15 + m, w, h, m)
        if m >= 1023:
            cand[:20] = src[:20] + rng.integers(-2, 3, (20, 2))
        if m >= 1025:
            near = np.abs(cand - src[20]).max(1) <= 2
            cand[near] = (w - 1, 0)                   # nothing else within the true match's distance
            ring = np.array([(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)])
            cand[20:20 + n_nn - 1] = src[20] + ring[:n_nn - 1]
            cand[m - 1] = src[20] + (2, 1)
        return src, cand
    return cached(("knn_length", w, h, m, n_nn), make)


def window_totals(a, b, src_xy, cmp_xy, best, window):
    """the integer totals of the windows compareFeatures walked for (source i, its best candidate): sum of squared differences over the pixel
    pairs inside both images (-1 = the default Feature at (0, 0))"""
    h, w = a.shape
    win = -(-window // 2)
    out = []
    for (sx, sy), j in zip(src_xy, best):
        cx, cy = (0, 0) if j < 0 else cmp_xy[j]
        ys, xs = np.mgrid[-win:win + 1, -win:win + 1]
        ok = (sx + xs >= 0) & (sy + ys >= 0) & (cx + xs >= 0) & (cy + ys >= 0) & (sx + xs < w) & (sy + ys < h) & (cx + xs < w) & (cy + ys < h)
        d = a[(sy + ys)[ok], (sx + xs)[ok]].astype(np.int64) - b[(cy + ys)[ok], (cx + xs)[ok]].astype(np.int64)
        out.append(int((d * d).sum()))
    return np.array(out, np.int64)
