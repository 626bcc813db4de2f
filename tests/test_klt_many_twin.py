"""What the groups of tests/test_klt_many_gpu.py are there for, asserted on the CPU twin alone (klt_common.twin_run): the preconditions the
GPU cases rely on."""
import pytest

import klt_common as kc
import klt_many_common as mc

W, H = kc.SIZES[0]


def test_target_1_never_runs_f_and_has_nothing_to_refill(pmv):
    c = mc.counts(kc.scene_run(pmv, W, H, "default", target=1)[1])
    assert (c[:, 5] == -1).all()
    assert (c[1:, 3] == 1).all() and (c[1:, 4] == 0).all()


def test_target_14_skips_f_drops_and_refills(pmv):
    c = mc.counts(kc.scene_run(pmv, W, H, "default", target=14)[1])
    assert (c[:, 5] == -1).all()
    assert c[1:, 1].tolist() == [12, 14, 14, 12, 10]
    assert [i for i in range(1, 6) if c[i, 0] > c[i, 1]] == [1, 4, 5], "stage 2"
    assert [i for i in range(1, 6) if c[i, 2] > c[i, 3]] == [1], "stage 4"
    assert [i for i in range(1, 6) if c[i, 4] > 0] == [1, 4, 5], "the refill"


@pytest.mark.parametrize("target", [63, 150])
def test_the_larger_targets_find_f_in_every_tracking_step(pmv, target):
    c = mc.counts(kc.scene_run(pmv, W, H, "default", target=target)[1])
    assert (c[1:, 5] == 1).all()


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["default", "fb_off", "f_off"])
def test_the_reversed_frames_drop_at_every_stage(pmv, size, name):
    w, h = size
    c = mc.counts(mc.reversed_run(pmv, w, h, name)[1])
    assert (c[0, :4] == 0).all() and c[0, 4] > 0
    drops2 = int((c[1:, 0] > c[1:, 1]).sum())
    if name == "fb_off" and size == kc.SIZES[0]:
        assert drops2 == 1
    else:
        assert drops2 > 0, "stage 2 drops nothing"
    if name != "f_off":
        assert (c[1:, 1] > c[1:, 2]).any(), "stage 3 drops nothing"
    else:
        assert (c[:, 5] == -1).all()
    assert (c[1:, 2] > c[1:, 3]).any(), "stage 4 drops nothing"
    assert (c[1:, 4] > 0).any(), "the refill adds nothing"


@pytest.mark.parametrize("size", kc.SIZES, ids=lambda s: "%dx%d" % s)
def test_no_model_over_all_six_frames(pmv, size):
    w, h = size
    c = mc.counts(mc.no_model_run(pmv, w, h)[1])
    assert (c[1:, 1] >= 15).all() and (c[1:, 5] == 0).all() and (c[1:, 2] == 0).all() and (c[1:, 3] == 0).all() and (c[1:, 4] > 0).all()


def test_a_late_joiner_tracks_and_rejects_in_both_later_steps(pmv):
    c = mc.counts(mc.late_run(pmv, W, H, "subpix")[1])
    assert len(c) == 3 and (c[0, :4] == 0).all() and c[0, 4] > 0
    assert (c[1:, 0] > 0).all() and (c[1:, 5] == 1).all()
    assert (c[1:, 0] > c[1:, 3]).all(), "nothing is rejected"
