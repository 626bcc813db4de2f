"""The streamed batched entry point without a GPU: the header documents it and its ingest counters, the library exports them, the binding
exposes them, and the binding checks argument shapes before anything reaches the device."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def test_header_documents_the_streamed_batch():
    src = _header()
    assert re.search(r"int pmv_pipeline_run_batch_streamed\(pmv_ctx\* ctx, int B, const pmv_pipeline_params\* params, const double\* K9,\s*"
                     r"const double\* const\* gt_poses12,\s*const uint8_t\* const\* host_frames, const int\* first_slot, int ring, "
                     r"pmv_pipeline_result\*\* out\);", src)
    doc = src[src.index("The same B sequences streamed from HOST memory"):src.index("int pmv_pipeline_run_batch_streamed(")]
    for must in ("first_slot[b] + f % ring", "ring >= init_frames + 1", "PMV_ERR_INVALID", "PMV_ERR_CAPACITY", "pmv_frames_stream_begin",
                 "Release rule", "bit-identical", "pinned", "pageable", "Frame.cpp:31-42", "OdometryPipeline.cpp:329-374"):
        assert must in doc, must


def test_header_documents_the_ingest_counters(pmv):
    src = _header()
    doc = src[src.index("Ingest counters of the last"):src.index("int pmv_batch_ingest_stats(")]
    n = int(re.search(r"#define PMV_BATCH_INGEST_STATS (\d+)", src).group(1))
    assert f"(= {n})" in doc
    assert [int(k) for k in re.findall(r"\[(\d+)\]", doc)] == list(range(n)), "every counter documented once, in order"
    assert len(pmv.BATCH_INGEST_KEYS) == n
    lib = pmv.load_library()
    assert lib.pmv_batch_ingest_stats(None, None) == n   # the library reports the same count without a context


def test_binding_exposes_the_streamed_batch(pmv):
    for sym in ("pmv_pipeline_run_batch_streamed", "pmv_batch_ingest_stats"):
        assert sym in pmv.ABI_SYMBOLS
        assert hasattr(pmv.load_library(), sym)
    assert callable(pmv.Context.pipeline_run_batch_streamed) and callable(pmv.Context.batch_ingest_stats)
    import inspect
    sig = inspect.signature(pmv.Context.pipeline_run_batch_streamed)
    assert sig.parameters["ring"].default == 16 and sig.parameters["first_slot"].default is None
    # the same keyword arguments as pipeline_run_batch
    staged = set(inspect.signature(pmv.Context.pipeline_run_batch).parameters) - {"self", "seqs"}
    assert staged <= set(sig.parameters)


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


def _seq(n=8, w=W, h=H, dtype=np.uint8, rows=None):
    return np.zeros((n, h, w), dtype), np.zeros((n if rows is None else rows, 12))


@pytest.mark.parametrize("seqs, kw", [
    ([], {}),                                                     # no sequence
    ([_seq(dtype=np.int16)], {}),                                 # not 8-bit
    ([_seq(w=W + 1)], {}),                                        # another frame size
    ([(np.zeros((8, H * W), np.uint8), np.zeros((8, 12)))], {}),  # not (n, h, w)
    ([_seq(rows=7)], {}),                                         # pose rows != frames
    ([_seq()], dict(ring=0)),
    ([_seq(), _seq()], dict(first_slot=[0])),                     # one first slot per sequence
    ([(np.zeros((8, H, W), np.uint8),)], {}),                     # not (frames, poses)
])
def test_argument_shapes_are_checked_before_any_device_call(pmv, seqs, kw):
    with pytest.raises(ValueError):
        _offline_ctx(pmv).pipeline_run_batch_streamed(seqs, W, H, K, **kw)


def test_argument_defaults(pmv):
    a, b = _seq(10), _seq(12)
    frames, gts, first = pmv._batch_streamed_args([a, b, a], W, H, 6, None)
    assert first == [0, 6, 12]
    assert frames[0].ctypes.data == frames[2].ctypes.data == a[0].ctypes.data   # aliased sources stay one buffer, read in place
    assert [g.shape for g in gts] == [(10, 12), (12, 12), (10, 12)]
    assert pmv._batch_streamed_args([a], W, H, 6, [5])[2] == [5]
