"""``dagr.visualization.event_viz`` (reference: src/dagr/visualization/event_viz.py:3-10), drawn on the device.

Same result as the reference's loop, bit for bit: every pixel hit by at least one event becomes ``alpha * img`` on all
channels (float64, truncated), then the channel ``int(p) - 1`` (Python's negative-index wrap: p = 0 -> red, p = 1 ->
blue on a BGR image, p = -1 -> green) of the LAST event on it gets ``+ 255 * (1 - alpha)`` (truncated).

Out-of-range input: rows with ``y >= H`` are skipped as in the reference; so are ``x >= W`` (which the reference's
numba loop does not check: undefined there) and negative coordinates.  A polarity whose ``p - 1`` lies outside
``[-3, 2]`` raises ``ValueError``, and so does an ``alpha`` outside ``[0, 1]``.
"""
import numpy as np
import torch

from .frames import render_frames


def draw_events_on_image(img, x, y, p, alpha=0.5):
    """Blend the events into ``img`` (uint8 ``[H, W, 3]``), in place, and return it.  ``img`` is a numpy array (uploaded,
    drawn, written back) or a device tensor (drawn where it is); ``x``, ``y``, ``p`` are numpy arrays or tensors."""
    n = len(x)
    if torch.is_tensor(img):
        if img.dim() != 3 or img.shape[-1] != 3 or img.dtype != torch.uint8 or not img.is_cuda or not img.is_contiguous():
            raise ValueError("img must be a contiguous uint8 [H, W, 3] device tensor (or a numpy array)")
        render_frames(img, [0], x, y, p, [0, n], alpha, out=img.unsqueeze(0), device=img.device)
        return img
    if not isinstance(img, np.ndarray) or img.ndim != 3 or img.shape[-1] != 3 or img.dtype != np.uint8:
        raise ValueError("img must be a uint8 [H, W, 3] array")
    out = render_frames(img, [0], x, y, p, [0, n], alpha)
    img[...] = out[0].cpu().numpy()
    return img
