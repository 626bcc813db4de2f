"""Colour (BGR) host frames without a GPU: the header declares the frame format and its error rules, the library exports the setter, the
binding lists it and checks formats and frame shapes before anything reaches the device, and the KITTI loader returns BGR channel order."""
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "pmv_hip.h")).read()


def test_header_declares_the_frame_format():
    src = _header()
    assert re.search(r"enum pmv_frame_format \{ PMV_FRAMES_GRAY = 0, PMV_FRAMES_BGR = 1 \};", src)
    assert re.search(r"int pmv_set_frame_format\(pmv_ctx\* ctx, int format\);", src)
    doc = src[src.index("The format of the host frames"):src.index("enum pmv_frame_format")]
    for must in ("pmv_frames_stage", "pmv_frames_stream_begin", "pmv_pipeline_run_streamed", "pmv_pipeline_run_batch_streamed", "pmv_frame_upload_bgr",
                 "Frame.cpp:33,40-41", "PMV_ERR_INVALID", "bracket", "batched run", "1868", "9617", "4899", "8192", ">> 14", "3 * w * h"):
        assert must in doc, must
    # the parameter struct stays as it was: the format is a context setting
    body = src[src.index("typedef struct pmv_pipeline_params {"):src.index("} pmv_pipeline_params;")]
    assert "format" not in body


def test_library_exports_and_binding_lists_the_setter(pmv):
    assert "pmv_set_frame_format" in pmv.ABI_SYMBOLS
    assert hasattr(pmv.load_library(), "pmv_set_frame_format")
    assert callable(pmv.Context.set_frame_format)
    assert pmv.FRAME_FORMATS == {"gray": 0, "bgr": 1}
    # without a context the library refuses instead of touching anything
    assert pmv.load_library().pmv_set_frame_format(None, 1) == -2


def test_profiler_lists_the_colour_kernel_after_the_existing_classes(pmv):
    import ctypes as C
    lib = pmv.load_library()
    lib.pmv_prof_kernel_name.restype = C.c_char_p
    names = [lib.pmv_prof_kernel_name(i).decode() for i in range(lib.pmv_prof_kernel_count())]
    assert names[:2] == ["k_pad_level0", "k_pyrdown"] and names[-1] == "k_pad_level0_bgr" and names.count("k_pad_level0_bgr") == 1
    assert names[18] == "k_fivepoint_hyp+score"   # the ids that existed keep their meaning


class _OnlyTheSetter:
    """stands in for the library: the format setter succeeds, any other use means the binding reached the device before checking its arguments"""

    def __init__(self):
        self.formats = []

    def pmv_set_frame_format(self, handle, fmt):
        self.formats.append(fmt)
        return 0

    def __getattr__(self, name):
        raise AssertionError(f"{name} called before the arguments were checked")


def _offline_ctx(pmv, fmt=None):
    ctx = object.__new__(pmv.Context)
    ctx.lib = _OnlyTheSetter()
    ctx.h = None
    if fmt is not None:
        ctx.set_frame_format(fmt)
    return ctx


def test_set_frame_format_argument_checks(pmv):
    ctx = _offline_ctx(pmv)
    assert ctx.frame_format == "gray"
    for bad in ("rgb", "BGR", "", 1, None, b"bgr"):
        with pytest.raises(ValueError):
            ctx.set_frame_format(bad)
    assert ctx.lib.formats == [] and ctx.frame_format == "gray"   # nothing reached the library
    ctx.set_frame_format("bgr")
    assert ctx.frame_format == "bgr"
    ctx.set_frame_format("gray")
    assert ctx.frame_format == "gray" and ctx.lib.formats == [1, 0]


W, H, N = 64, 48, 8
K = np.eye(3).reshape(9)
GT = np.zeros((N, 12))
BAD_BGR = [
    np.zeros((N, H, W), np.uint8),            # gray frames
    np.zeros((N, H, W, 4), np.uint8),         # four channels
    np.zeros((N, H, W, 1), np.uint8),
    np.zeros((N, 3, H, W), np.uint8),         # planar
    np.zeros((H, W, 3), np.uint8),            # one image, not a sequence
    np.zeros((N, H, W, 3), np.int16),         # not 8-bit
    np.zeros((N, H, W, 3), np.float32),
    np.zeros((N * H * W * 3,), np.uint8),     # flat
]


@pytest.mark.parametrize("frames", BAD_BGR, ids=lambda f: f"{f.shape}-{f.dtype}")
def test_bgr_shapes_are_checked_before_any_device_call(pmv, frames):
    ctx = _offline_ctx(pmv, "bgr")
    with pytest.raises(ValueError):
        ctx.frames_stage(0, frames)
    with pytest.raises(ValueError):
        ctx.frames_stream_begin(0, frames)
    with pytest.raises(ValueError):
        ctx.pipeline_run(N, W, H, K, GT, host_frames=frames)
    with pytest.raises(ValueError):
        ctx.pipeline_run_batch_streamed([(frames, GT)], W, H, K, ring=6)


def test_bgr_frame_size_and_count_must_match_the_run(pmv):
    ctx = _offline_ctx(pmv, "bgr")
    with pytest.raises(ValueError):
        ctx.pipeline_run(N, W, H, K, GT, host_frames=np.zeros((N, H, W + 1, 3), np.uint8))
    with pytest.raises(ValueError):
        ctx.pipeline_run(N, W, H, K, GT, host_frames=np.zeros((N - 1, H, W, 3), np.uint8))
    with pytest.raises(ValueError):
        ctx.pipeline_run_batch_streamed([(np.zeros((N, H + 2, W, 3), np.uint8), GT)], W, H, K, ring=6)
    with pytest.raises(ValueError):
        ctx.pipeline_run_batch_streamed([(np.zeros((N, H, W, 3), np.uint8), GT[:-1])], W, H, K, ring=6)   # pose rows != frames


def test_bgr_arguments_that_pass_are_read_in_place(pmv):
    a = np.zeros((10, H, W, 3), np.uint8)
    odd = np.zeros(12 * H * W * 3 + 1, np.uint8)[1:].reshape(12, H, W, 3)   # a source that starts at an odd byte
    frames, gts, first = pmv._batch_streamed_args([(a, np.zeros((10, 12))), (odd, np.zeros((12, 12))), (a, np.zeros((10, 12)))], W, H, 6, None, "bgr")
    assert first == [0, 6, 12]
    assert frames[0].ctypes.data == frames[2].ctypes.data == a.ctypes.data and frames[1].ctypes.data == odd.ctypes.data
    assert frames[1].ctypes.data % 2 == 1
    assert [f.shape for f in frames] == [(10, H, W, 3), (12, H, W, 3), (10, H, W, 3)]
    # a gray context keeps refusing colour arrays in the batched call, as before
    with pytest.raises(ValueError):
        pmv._batch_streamed_args([(a, np.zeros((10, 12)))], W, H, 6, None)


def test_kitti_loader_returns_bgr_channel_order(tmp_path):
    from PIL import Image
    kitti = importlib.import_module("practical-multi-view_amd.kitti")
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 256, (3, 40, 56, 3), dtype=np.uint8)
    rgb[:, :, :, 0] |= 1    # no channel equals another anywhere near by chance: red odd ...
    rgb[:, :, :, 2] &= 254  # ... blue even
    for cam, imgs in (("image_2", rgb), ("image_3", rgb[::-1])):
        os.makedirs(tmp_path / "sequences" / "03" / cam)
        for i, im in enumerate(imgs):
            Image.fromarray(im, "RGB").save(tmp_path / "sequences" / "03" / cam / ("%06d.png" % i))
    os.makedirs(tmp_path / "poses")
    (tmp_path / "sequences" / "03" / "calib.txt").write_text("P0: 120 0 28 0 0 120 20 0 0 0 1 0\n")
    gt = np.arange(36, dtype=np.float64).reshape(3, 12)
    np.savetxt(tmp_path / "poses" / "03.txt", gt)
    frames, poses, Km = kitti.load_sequence(str(tmp_path), "03", colour=True)
    assert frames.shape == (3, 40, 56, 3) and frames.dtype == np.uint8
    assert np.array_equal(frames[..., 0], rgb[..., 2]) and np.array_equal(frames[..., 1], rgb[..., 1]) and np.array_equal(frames[..., 2], rgb[..., 0])
    np.testing.assert_allclose(poses, gt)
    np.testing.assert_allclose(Km, [[120, 0, 28], [0, 120, 20], [0, 0, 1]])
    right, _, _ = kitti.load_sequence(str(tmp_path), "03", n=2, camera="image_3", colour=True)
    assert np.array_equal(right, rgb[::-1][:2][..., ::-1])
    # the gray loader is what it was: one channel, image_0 by default
    with pytest.raises(FileNotFoundError):
        kitti.load_sequence(str(tmp_path), "03")
    gray, _, _ = kitti.load_sequence(str(tmp_path), "03", camera="image_2")
    assert gray.shape == (3, 40, 56)


def test_a_gray_context_refuses_colour_arrays(pmv):
    """the likely mistake once colour exists: (n, h, w, 3) frames without set_frame_format("bgr") must not be read as gray bytes"""
    ctx = _offline_ctx(pmv)
    bgr = np.zeros((N, H, W, 3), np.uint8)
    with pytest.raises(ValueError):
        ctx.frames_stage(0, bgr)
    with pytest.raises(ValueError):
        ctx.frames_stream_begin(0, bgr)
    with pytest.raises(ValueError):
        ctx.pipeline_run(N, W, H, K, GT, host_frames=bgr)
    with pytest.raises(ValueError):
        ctx.pipeline_run(N, W, H, K, GT, host_frames=np.zeros((N, H, W + 1), np.uint8))
    with pytest.raises(ValueError):
        ctx.pipeline_run_batch_streamed([(bgr, GT)], W, H, K, ring=6)
