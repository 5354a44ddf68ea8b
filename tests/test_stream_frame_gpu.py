"""dagr_stream_frame on the GPU against ``frame_definition`` (dagr_amd/streaming.py), bit for bit: crops inside larger
frames, padded rows, mixed and odd factors, the identity, a single pixel, overshoot on 0 / 255 frames, both channel orders,
round-half-to-even on a frame that is checked to hold ties of both parities, and lanes (a lane that keeps its contents, a
lane outside the batch that writes nothing and is flagged)."""
import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.streaming import STATUS_BITS, _flag_names, frame_closed_form, frame_definition

pytestmark = pytest.mark.gpu


def _run(frames, lanes, fx, fy, W, H, bgr, out, status):
    """frames: uint8 [n, H_f, W_f, 3] on the device (a view with padded rows passes its own strides)."""
    n, h_f, w_f = frames.shape[:3]
    lanes = torch.as_tensor(lanes, dtype=torch.int32).cuda()
    rc = _lib.lib().dagr_stream_frame(_lib.ptr(frames), frames.stride(0), frames.stride(1), n, _lib.ptr(lanes),
                                      w_f, h_f, fx, fy, W, H, 1 if bgr else 0, _lib.ptr(out), out.shape[0], out.stride(0),
                                      out.stride(1), out.stride(2), out.stride(3), _lib.ptr(status),
                                      _lib.cur_stream(out.device))
    _lib.check(rc, "stream_frame")
    torch.cuda.synchronize()


def _one(raw, fx, fy, W, H, bgr, pad=0):
    """One frame through the kernel into a one-lane output; ``pad``: extra bytes at the end of every frame row."""
    h_f, w_f = raw.shape[:2]
    if pad:
        rows = np.full((h_f, 3 * w_f + pad), 0xA5, np.uint8)
        rows[:, :3 * w_f] = raw.reshape(h_f, 3 * w_f)
        dev = torch.from_numpy(rows).cuda()
        frames = dev.as_strided((1, h_f, w_f, 3), (h_f * (3 * w_f + pad), 3 * w_f + pad, 3, 1))
    else:
        frames = torch.from_numpy(np.ascontiguousarray(raw)).cuda()[None]
    out = torch.full((1, 3, H, W), -1.0, device="cuda")
    status = torch.zeros((1,), dtype=torch.int32, device="cuda")
    _run(frames, [0], fx, fy, W, H, bgr, out, status)
    assert int(status) == 0
    return out[0].cpu()


def _random(shape, seed, binary=False):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8) if binary else \
        rng.integers(0, 256, shape, dtype=np.uint8)


# (fx, fy, W, H, frame W_f x H_f, row padding in bytes, 0 / 255 frame)
CASES = {"crop_inside_a_larger_frame": (2, 2, 40, 27, 86, 104, 0, False),
         "padded_rows": (2, 2, 40, 27, 86, 104, 13, False),
         "mixed_factors": (3, 2, 17, 9, 51, 18, 0, False),
         "identity": (1, 1, 33, 5, 33, 5, 0, False),
         "single_pixel": (2, 2, 1, 1, 2, 2, 0, False),
         "factor_four": (4, 4, 11, 7, 47, 30, 0, False),
         "zeros_and_255": (2, 2, 40, 27, 86, 104, 0, True)}


@pytest.mark.parametrize("bgr", [False, True], ids=["rgb", "bgr"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_equals_the_definition(case, bgr):
    fx, fy, W, H, w_f, h_f, pad, binary = CASES[case]
    raw = _random((h_f, w_f, 3), 40 + len(case), binary)
    want = frame_definition(raw, fx, fy, W, H, bgr)
    got = _one(raw, fx, fy, W, H, bgr, pad)
    assert torch.equal(got, want), (got - want).abs().max()
    if case == "identity":
        assert torch.equal(got, torch.from_numpy(raw[..., ::-1].copy() if bgr else raw).permute(2, 0, 1).float() / 255.0)
    if binary:                                  # overshoot and undershoot are clamped, and both occur
        sums = frame_closed_form(raw, fx, fy, W, H)[1]
        assert (sums < 0).any() and (sums > 255 * 1024).any()
        assert float(got.min()) == 0.0 and float(got.max()) == 1.0


def test_rounding_is_half_to_even():
    """(2, 2, 320, 215) on a uniform random frame that holds ties with an odd and with an even quotient and sums below 0
    and above 255 -- asserted on the CPU first, so the comparison cannot pass for want of such pixels."""
    fx, fy, W, H = 2, 2, 320, 215
    raw = np.random.default_rng(11).integers(0, 256, (fy * H, fx * W, 3), dtype=np.uint8)
    closed, sums = frame_closed_form(raw, fx, fy, W, H)
    tie = (sums & 1023) == 512
    odd, even = int((tie & ((sums >> 10) & 1 == 1)).sum()), int((tie & ((sums >> 10) & 1 == 0)).sum())
    below, above = int((sums < 0).sum()), int((sums > 255 * 1024).sum())
    print("ties with an odd quotient", odd, "with an even one", even, "sums below 0", below, "above 255", above)
    assert odd >= 1 and even >= 1 and below >= 1 and above >= 1
    want = frame_definition(raw, fx, fy, W, H)
    assert np.array_equal(closed, want.numpy())
    assert torch.equal(_one(raw, fx, fy, W, H, False), want)


def test_lanes_are_written_where_named_and_nowhere_else():
    fx, fy, W, H, B = 2, 2, 40, 27, 3
    raw = _random((2, 60, 90, 3), 77)
    frames = torch.from_numpy(raw).cuda()
    before = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(1)).cuda()
    out = before.clone()
    status = torch.zeros((1,), dtype=torch.int32, device="cuda")
    _run(frames, [2, 0], fx, fy, W, H, True, out, status)
    assert int(status) == 0
    assert torch.equal(out[2].cpu(), frame_definition(raw[0], fx, fy, W, H, True))
    assert torch.equal(out[0].cpu(), frame_definition(raw[1], fx, fy, W, H, True))
    assert torch.equal(out[1], before[1])                      # lane 1 keeps its contents, bit for bit
    # a lane outside the batch: nothing is written, and the stream's status word says so
    kept = out.clone()
    _run(frames, [3, 1], fx, fy, W, H, False, out, status)
    assert int(status) == 32
    assert torch.equal(out[0], kept[0]) and torch.equal(out[2], kept[2])
    assert torch.equal(out[1].cpu(), frame_definition(raw[1], fx, fy, W, H, False))
    assert dict(STATUS_BITS)[32] in _flag_names(32)


def test_stream_state_flags_a_lane_outside_the_batch():
    """StreamState.write_frames with a lane 3 of B = 3: nothing written, bit 32 in the stream's status word, named as
    EventStream.check_status names it (tests/test_stream_hold_gpu.py raises it through a step)."""
    from dagr_amd.engine import StreamState
    st = StreamState(3, 50000, torch.device("cuda:0"))
    frames = torch.from_numpy(_random((1, 54, 80, 3), 5)).cuda()
    st.write_frames(frames, torch.tensor([3], dtype=torch.int32, device="cuda"), 2, 2, 40, 27, False)
    torch.cuda.synchronize()
    flag = int(st.status)
    assert flag == 32 and "lane is outside [0, batch_size)" in _flag_names(flag)
    assert float(st.image.abs().max()) == 0.0 and st.frame_new
