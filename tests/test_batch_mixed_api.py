"""Sequences of different frame sizes in one batch, without a GPU: the binding takes the size per sequence (one int, B ints, or - streamed -
each array's own shape), checks it before anything reaches the device, and the header states the rule at both batched entry points."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.eye(3).reshape(9)


class _NoDevice:
    """stands in for the library: any use means the binding reached the device (so every argument check has passed)"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} called before the arguments were checked")


def _offline_ctx(pmv):
    ctx = object.__new__(pmv.Context)
    ctx.lib = _NoDevice()
    ctx.h = None
    return ctx


def _seq(n, w, h):
    return np.zeros((n, h, w), np.uint8), np.zeros((n, 12))


def test_sizes_default_to_each_array_s_own_shape(pmv):
    a, b = _seq(8, 640, 200), _seq(9, 1241, 376)
    frames, gts, first = pmv._batch_streamed_args([a, b], None, None, 6, None)
    assert frames[0].ctypes.data == a[0].ctypes.data and frames[1].ctypes.data == b[0].ctypes.data, "contiguous uint8 arrays are read in place"
    assert [f.shape for f in frames] == [(8, 200, 640), (9, 376, 1241)]
    assert [g.shape for g in gts] == [(8, 12), (9, 12)] and first == [0, 6]
    # per sequence, stated: the same arrays
    frames2, _, _ = pmv._batch_streamed_args([a, b], [640, 1241], [200, 376], 6, None)
    assert frames2[0].ctypes.data == a[0].ctypes.data and frames2[1].ctypes.data == b[0].ctypes.data


@pytest.mark.parametrize("w, h", [
    ([640], [200, 376]),                # w: one entry for two sequences
    ([640, 1241], [200]),               # h
    ([640, 1241, 640], [200, 376, 200]),
    ([640, 1241], [200, 375]),          # the right length, but sequence 1 is 1241 x 376
    (640, 200),                         # one size for all: sequence 1 does not match (as before)
    (None, 200),                        # w and h go together
])
def test_sizes_that_do_not_fit_the_arrays_are_refused_before_any_library_call(pmv, w, h):
    a, b = _seq(8, 640, 200), _seq(9, 1241, 376)
    with pytest.raises(ValueError):
        pmv._batch_streamed_args([a, b], w, h, 6, None)
    with pytest.raises(ValueError):
        _offline_ctx(pmv).pipeline_run_batch_streamed([a, b], w, h, K, ring=6)


@pytest.mark.parametrize("w, h", [([640], [200, 376]), ([640, 1241, 640], [200, 376, 200]), ([], [])])
def test_staged_sizes_of_the_wrong_length_are_refused_before_any_library_call(pmv, w, h):
    gt = np.zeros((8, 12))
    with pytest.raises(ValueError):
        _offline_ctx(pmv).pipeline_run_batch([(0, 8, gt), (8, 8, gt)], w, h, K)


def test_a_mixed_size_call_reaches_the_library(pmv):
    """(the stand-in library refuses every call: getting that far means no argument check stood in the way)"""
    a, b = _seq(8, 640, 200), _seq(9, 1241, 376)
    for kw in (dict(), dict(w=[640, 1241], h=[200, 376])):
        with pytest.raises(AssertionError, match="pmv_pipeline_run_batch_streamed"):
            _offline_ctx(pmv).pipeline_run_batch_streamed([a, b], K=K, ring=6, **kw)
    with pytest.raises(AssertionError, match="pmv_pipeline_run_batch"):
        _offline_ctx(pmv).pipeline_run_batch([(0, 8, a[1]), (8, 9, b[1])], [640, 1241], [200, 376], K)
    # one size for all, as before
    with pytest.raises(AssertionError, match="pmv_pipeline_run_batch_streamed"):
        _offline_ctx(pmv).pipeline_run_batch_streamed([a, a], 640, 200, K, ring=6)


def test_header_states_the_size_rule_at_both_batched_entry_points():
    src = open(os.path.join(ROOT, "include", "pmv_hip.h")).read()
    assert "one frame size for all" not in src
    staged = src[src.index("B independent sequences through batched launches"):src.index("int pmv_pipeline_run_batch(")]
    streamed = src[src.index("The same B sequences streamed from HOST memory"):src.index("int pmv_pipeline_run_batch_streamed(")]
    for doc in (staged, streamed):
        flat = " ".join(doc.replace("*", " ").split())
        assert "Frame sizes: per sequence, from params[b].w / params[b].h" in flat
        assert "Frame.cpp:31-42" in flat and "capacity" in flat and "PMV_ERR_CAPACITY" in flat
    flat = " ".join(staged.replace("*", " ").split())
    assert "overlapping ranges must agree on the size of every shared slot" in flat and "PMV_ERR_INVALID" in flat
    assert "every slot of sequence b's ring holds that size" in " ".join(streamed.replace("*", " ").split())


def test_the_launch_counter_is_declared_exported_and_bound(pmv):
    assert "pmv_debug_batch_launches" in pmv.ABI_SYMBOLS and hasattr(pmv.load_library(), "pmv_debug_batch_launches")
    assert callable(pmv.Context.batch_launches)
