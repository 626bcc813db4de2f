"""The alternative plugins (FAST extractor, kNN matcher) on the batched entry points, without a GPU: the binding takes `matcher` and
per-sequence plugin options on both batched methods and checks them before anything reaches the library; the header states the plugin
rule next to both entry points and no longer restricts the batch engine to the default plugins."""
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def test_both_batched_methods_take_matcher_and_share_their_keywords(pmv):
    staged = inspect.signature(pmv.Context.pipeline_run_batch).parameters
    streamed = inspect.signature(pmv.Context.pipeline_run_batch_streamed).parameters
    for sig in (staged, streamed):
        assert sig["matcher"].default == 0 and sig["extractor"].default == 0
    assert set(staged) - {"self", "seqs"} == set(streamed) - {"self", "seqs", "ring", "first_slot"}


def test_scalar_and_per_sequence_plugin_options(pmv):
    assert pmv._per_sequence("who", "extractor", 2, 3) == [2, 2, 2]
    assert pmv._per_sequence("who", "matcher", np.int32(1), 2) == [1, 1]
    assert pmv._per_sequence("who", "extractor", [0, 1, 2], 3) == [0, 1, 2]
    assert pmv._per_sequence("who", "matcher", np.array([0, 1]), 2) == [0, 1]
    assert pmv._per_sequence("who", "matcher", (1,), 1) == [1]
    for bad in ([0, 1], [], np.zeros(4, int)):
        with pytest.raises(ValueError, match="extractor"):
            pmv._per_sequence("who", "extractor", bad, 3)


class _NoDevice:
    """stands in for the library: any use means the binding reached the device before checking its arguments"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} called before the arguments were checked")


def _offline_ctx(pmv):
    ctx = object.__new__(pmv.Context)
    ctx.lib = _NoDevice()
    ctx.h = None
    return ctx


W, H = 64, 48
K = np.eye(3).reshape(9)


@pytest.mark.parametrize("kw", [dict(extractor=[2]), dict(matcher=[1, 1, 1]), dict(extractor=[2, 2], matcher=[1]), dict(extractor=[])])
def test_a_list_of_the_wrong_length_is_refused_before_any_library_call(pmv, kw):
    gt = np.zeros((8, 12))
    with pytest.raises(ValueError):
        _offline_ctx(pmv).pipeline_run_batch([(0, 8, gt), (8, 8, gt)], W, H, K, **kw)
    frames = np.zeros((8, H, W), np.uint8)
    with pytest.raises(ValueError):
        _offline_ctx(pmv).pipeline_run_batch_streamed([(frames, gt), (frames, gt)], W, H, K, ring=6, **kw)


def test_lists_of_the_right_length_reach_the_library(pmv):
    """(the stand-in library refuses every call: getting that far means the argument checks passed)"""
    gt = np.zeros((8, 12))
    frames = np.zeros((8, H, W), np.uint8)
    with pytest.raises(AssertionError, match="pmv_pipeline_run_batch"):
        _offline_ctx(pmv).pipeline_run_batch([(0, 8, gt), (8, 8, gt)], W, H, K, extractor=[2, 0], matcher=[1, 0])
    with pytest.raises(AssertionError, match="pmv_pipeline_run_batch_streamed"):
        _offline_ctx(pmv).pipeline_run_batch_streamed([(frames, gt), (frames, gt)], W, H, K, ring=6, extractor=2, matcher=[1, 0])


def test_header_states_the_plugin_rule_at_both_batched_entry_points():
    src = _header()
    assert "LK with GFTT or ShiTomasi" not in src and "default plugins" not in src
    staged = src[src.index("B independent sequences through batched launches"):src.index("int pmv_pipeline_run_batch(")]
    streamed = src[src.index("The same B sequences streamed from HOST memory"):src.index("int pmv_pipeline_run_batch_streamed(")]
    for doc in (staged, streamed):
        flat = " ".join(doc.replace("*", " ").split())
        assert "matcher = 1 (kNN) with extractor = 2 (FAST)" in flat, "the kNN matcher's rule"
        assert "extractor 0, 1 or 2" in flat
    assert "PMV_ERR_INVALID" in staged and "kNNFeatureMatcher.cpp:11" in staged
    assert "release rule" in streamed and "minimum ring" in streamed   # the streamed rules hold for the new plugins, and the header says so
