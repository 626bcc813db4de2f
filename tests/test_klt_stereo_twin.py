"""What the stereo scene of tests/klt_stereo_common.py is there for, asserted on the CPU twins alone: most tracks of the left list find
their right observation, the occluder and the frame's edge leave some without one, the back check is what rejects most of those, and the
matched tracks carry the disparity the right frame was made with."""
import numpy as np
import pytest

import klt_common as kc
import klt_stereo_common as ks


def _runs(pmv, w, h):
    lefts, rts = kc.scene(pmv, w, h), ks.scene_rights(pmv, w, h)
    _, run = kc.scene_run(pmv, w, h, "default")
    return lefts, run, {name: ks.twin_stereo_run(lefts, rts, run, st, (w, h, "default", name)) for name, st in ks.STEREO.items()}


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_scene_has_matched_and_unmatched_tracks_in_every_frame(pmv, size):
    w, h = size
    lefts, run, st = _runs(pmv, w, h)
    assert len(run) == kc.N_FRAMES
    for i in range(kc.N_FRAMES):
        n = len(run[i][1][0])
        with_fb, without = int(st["fb"][i][1].sum()), int(st["fb_off"][i][1].sum())
        print(f"{w}x{h} frame {i}: {n} tracks, {with_fb} matched with the back check, {without} without")
        assert 2 * with_fb >= n and n - with_fb >= 5
        assert without > with_fb


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_upper_half_has_disparity_4(pmv, size):
    w, h = size
    lefts, run, st = _runs(pmv, w, h)
    for i in range(kc.N_FRAMES):
        xy = run[i][1][2]
        rxy, ok = st["fb"][i]
        up =(ok == 1) & (xy[:, 1] < h // 2)
        assert up.sum() >= 5
        d = np.median(xy[up, 0].astype(np.float64) - rxy[up, 0].astype(np.float64))
        print(f"{w}x{h} frame {i}: median disparity of the upper half {d:.3f} over {int(up.sum())} tracks")
        assert abs(d - 4.0) <= 0.5


def test_the_40x40_pair_has_matches(pmv):
    lefts, rts = ks.small_pair(pmv)
    p = kc.params(**ks.SMALL)
    run = kc.twin_run(lefts, p, "40x40")
    got = ks.twin_stereo_run(lefts, rts, run, ks.STEREO["fb"], "40x40")
    for i in range(2):
        n, matched = len(run[i][1][0]), int(got[i][1].sum())
        print(f"40x40 frame {i}: {n} tracks, {matched} matched")
        assert n > 0 and matched > 0
