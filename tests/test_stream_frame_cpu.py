"""Raw sensor frames for the event stream, on the CPU: the closed form ``dagr_stream_frame`` computes
(``frame_closed_form``) against the definition (``frame_definition``: ``DSEC.preprocess_image`` + ``format_data``), and the
definition against those two functions themselves."""
import types

import numpy as np
import pytest
import torch

from dagr_amd.data.dsec_data import DSEC
from dagr_amd.streaming import STATUS_BITS, frame_closed_form, frame_definition

CASES = [(2, 2, 40, 27), (2, 2, 320, 215), (3, 2, 17, 9), (1, 3, 8, 5), (4, 4, 11, 7), (2, 2, 1, 1)]


def _frames(fx, fy, W, H, seed):
    """A uniform random frame and a frame of only 0 and 255, both a little larger than the crop."""
    rng = np.random.default_rng(seed)
    shape = (fy * H + 3, fx * W + 5, 3)
    return rng.integers(0, 256, shape, dtype=np.uint8), (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8)


@pytest.mark.parametrize("fx,fy,W,H", CASES)
@pytest.mark.parametrize("bgr", [False, True])
def test_closed_form_equals_the_definition(fx, fy, W, H, bgr):
    for k, raw in enumerate(_frames(fx, fy, W, H, 100 * fx + fy)):
        want = frame_definition(raw, fx, fy, W, H, bgr)
        got, _ = frame_closed_form(raw, fx, fy, W, H, bgr)
        assert want.dtype == torch.float32 and tuple(want.shape) == (3, H, W)
        assert np.array_equal(got, want.numpy()), (k, np.abs(got - want.numpy()).max())


def test_taps_are_clamped_to_the_crop_not_to_the_frame():
    """Pixels right of / below the crop must not be read: changing them changes nothing."""
    fx, fy, W, H = 2, 2, 40, 27
    raw = np.random.default_rng(3).integers(0, 256, (104, 86, 3), dtype=np.uint8)
    other = raw.copy()
    other[fy * H:] = 255 - other[fy * H:]
    other[:, fx * W:] = 255 - other[:, fx * W:]
    for f in (frame_definition, lambda *a: torch.from_numpy(frame_closed_form(*a)[0])):
        assert torch.equal(f(raw, fx, fy, W, H), f(other, fx, fy, W, H))


def test_division_by_255_agrees_for_every_value():
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(u.astype(np.float32) / np.float32(255.0), (torch.from_numpy(u).float() / 255.0).numpy())


def test_definition_is_preprocess_image_then_format_data():
    """``DSEC.preprocess_image`` (rows [0, scale * height), every column, shrunk to width x height) on a stand-in frame,
    then ``format_data``'s ``image.float() / 255.0``."""
    scale, width, height = 2, 44, 31
    raw = np.random.default_rng(5).integers(0, 256, (scale * height + 10, scale * width, 3), dtype=np.uint8)
    from dagr_amd.data.dsec_data import _resize_area_free
    ds = types.SimpleNamespace(scale=scale, width=width, height=height, _resize=_resize_area_free)
    image = DSEC.preprocess_image(ds, raw)                               # uint8 [1, 3, height, width]
    want = image.float() / 255.0                                         # utils/buffers.py: format_data
    got = frame_definition(raw, scale, scale, width, height)
    assert torch.equal(got, want[0])
    assert torch.equal(frame_definition(raw, scale, scale, width, height, bgr=True), want[0].flip(0))


def test_definition_refuses_what_is_not_a_frame():
    with pytest.raises(ValueError, match="smaller than the crop"):
        frame_definition(np.zeros((53, 80, 3), np.uint8), 2, 2, 40, 27)
    with pytest.raises(ValueError, match="uint8"):
        frame_definition(np.zeros((54, 80, 3), np.float32), 2, 2, 40, 27)


def test_status_bit_32_names_the_lane():
    assert "lane" in dict(STATUS_BITS)[32]


def test_the_binding_declares_dagr_stream_frame():
    import ctypes
    from dagr_amd import _lib
    res, args = _lib.SIGNATURES["dagr_stream_frame"]
    assert res is ctypes.c_int and len(args) == 20
    L = _lib.lib()
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    one = ctypes.c_void_p(8)
    # a frame smaller than the crop, strides smaller than the frame, NULL pointers: refused before any launch
    assert L.dagr_stream_frame(one, 0, 3 * 79, 1, one, 79, 54, 2, 2, 40, 27, 0, one, 1, 1, 1, 1, 1, one, None) == bad
    assert L.dagr_stream_frame(one, 0, 3 * 80 - 1, 1, one, 80, 54, 2, 2, 40, 27, 0, one, 1, 1, 1, 1, 1, one, None) == bad
    assert L.dagr_stream_frame(None, 0, 3 * 80, 1, one, 80, 54, 2, 2, 40, 27, 0, one, 1, 1, 1, 1, 1, one, None) == bad
    assert L.dagr_stream_frame(None, 0, 3 * 80, 0, None, 80, 54, 2, 2, 40, 27, 0, None, 1, 1, 1, 1, 1, None, None) == 0
