"""Batched visualisation frames on the device (``dagr_viz_render``, csrc/viz.hip).

Every frame is a base image, an event segment drawn as ``event_viz.draw_events_on_image`` does, and optionally a list of
box outlines (``bbox_viz``'s outline rule).  Frame metadata (which image, which events, which boxes) is small and lives on
the host; images, events and the output live on the device.
"""
import numpy as np
import torch

from .. import _lib

_STATUS = ((1, ValueError, "an event's polarity p gives a channel p - 1 outside [-3, 2]"),
           (2, IndexError, "a box's class id has no colour"),
           (4, IndexError, "a frame's image index is out of range"),
           (8, ValueError, "alpha must lie in [0, 1]"))


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("dagr visualisation renders on the GPU; no device is available")
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _upload(a, dtype, dev):
    if torch.is_tensor(a):
        return a.to(dev, dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=torch.empty((), dtype=dtype).numpy().dtype)).to(dev)


def _coords(a, dev):
    """Event coordinates as int32; values beyond int32 (never inside an image) are clamped, not wrapped."""
    if torch.is_tensor(a):
        return a.to(dev, torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()
    a = np.asarray(a)
    if a.dtype.itemsize > 4 or a.dtype == np.uint32:
        a = np.clip(a, -1, 2 ** 31 - 1)
    return _upload(a, torch.int32, dev)


def _polarity(p, dev):
    """int8 polarities.  A value whose p - 1 is no channel index (outside [-2, 3]) becomes 127, which the kernel reports:
    an unchecked int8 cast could turn e.g. a uint8 255 into a valid -1."""
    if torch.is_tensor(p):
        p = p.to(dev)
        p = torch.trunc(p) if p.is_floating_point() else p.to(torch.int64)
        return torch.where((p >= -2) & (p <= 3), p, torch.full_like(p, 127)).to(torch.int8).contiguous()
    p = np.asarray(p)
    if p.dtype.kind == "f":
        p = np.trunc(p)
    ok = (p >= -2) & (p <= 3)
    return _upload(np.where(ok, p, 127).astype(np.int8), torch.int8, dev)


def _host_i64(a, name):
    a = np.asarray(a.cpu() if torch.is_tensor(a) else a)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError(f"{name} must be a 1-D integer array")
    return a.astype(np.int64)


def _check_ptr(ptr, n_frames, total, name):
    if len(ptr) != n_frames + 1 or ptr[0] != 0 or ptr[-1] != total or np.any(np.diff(ptr) < 0):
        raise ValueError(f"{name} must be non-decreasing, of length F + 1 = {n_frames + 1}, from 0 to {total}")


def render_frames(images, frame_image, x, y, p, ev_ptr, alpha=0.5, boxes=None, box_ptr=None, linewidth=2, colors=None,
                  out=None, device=None):
    """Render F frames in one device call and return ``out``, uint8 ``[F, H, W, 3]`` on the device.

    images       uint8 BGR ``[n_images, H, W, 3]`` (numpy, uploaded, or a device tensor)
    frame_image  ``[F]`` host ints: the base image of every frame (frames may share one)
    x, y, p      the events of all frames, concatenated (numpy or tensors); frame f owns ``[ev_ptr[f], ev_ptr[f+1])``
    alpha        a float or ``[F]`` floats in [0, 1]
    boxes        optional ``[n_boxes, 5]`` int rows ``(x0, y0, x1, y1, class id)``; frame f owns ``[box_ptr[f], box_ptr[f+1])``
    colors       uint8 ``[n_classes, 3]`` outline colours (default: ``bbox_viz``'s per-class colours)

    ``out`` may be given (a contiguous uint8 device tensor of the right shape); it may be ``images`` itself when
    ``frame_image[f] == f`` for every f.
    """
    dev = _device(device)
    images_t = _upload(images, torch.uint8, dev)
    if images_t.dim() == 3:
        images_t = images_t.unsqueeze(0)
    if images_t.dim() != 4 or images_t.shape[-1] != 3:
        raise ValueError(f"images must be [n, H, W, 3] uint8, got {tuple(images_t.shape)}")
    n_img, H, W = (int(s) for s in images_t.shape[:3])
    fi = _host_i64(frame_image, "frame_image")
    F = len(fi)
    if F < 1 or F > 65535:
        raise ValueError(f"render_frames: 1 <= F <= 65535 frames per call, got {F}")
    if np.any((fi < 0) | (fi >= n_img)):
        raise IndexError(f"frame_image entries must lie in [0, {n_img})")
    xt, yt, pt = _coords(x, dev), _coords(y, dev), _polarity(p, dev)
    n_ev = int(xt.numel())
    if int(yt.numel()) != n_ev or int(pt.numel()) != n_ev:
        raise ValueError("x, y and p must have the same length")
    if n_ev >= 2 ** 31:
        raise ValueError("render_frames: fewer than 2**31 events per call")
    ep = _host_i64(ev_ptr, "ev_ptr")
    _check_ptr(ep, F, n_ev, "ev_ptr")
    a = np.array(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (F,)))
    if not np.all((a >= 0) & (a <= 1)):
        raise ValueError("alpha must lie in [0, 1]")
    box_t = bp_t = col_t = None
    n_boxes = n_col = 0
    if boxes is not None:
        if int(linewidth) < 1:
            raise ValueError("linewidth must be >= 1 (outlines only)")
        rows = np.asarray(boxes, dtype=np.int64).reshape(-1, 5)
        n_boxes = len(rows)
        bp = _host_i64(box_ptr, "box_ptr")
        _check_ptr(bp, F, n_boxes, "box_ptr")
        if colors is None:
            from .bbox_viz import outline_colors
            colors = outline_colors()
        col = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
        n_col = len(col)
        if n_boxes and (rows[:, 4].min() < 0 or rows[:, 4].max() >= n_col):
            raise IndexError(f"class ids must lie in [0, {n_col})")
        rows = np.clip(rows, -2 ** 30, 2 ** 30)     # far outside any image either way: no int32 wrap
        box_t = _upload(rows.astype(np.int32), torch.int32, dev)
        bp_t = _upload(bp.astype(np.int32), torch.int32, dev)
        col_t = _upload(col, torch.uint8, dev)
    if out is None:
        out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != (F, H, W, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous uint8 [F, H, W, 3] tensor on the rendering device")
    fi_t = _upload(fi.astype(np.int32), torch.int32, dev)
    ep_t = _upload(ep.astype(np.int32), torch.int32, dev)
    a_t = _upload(a, torch.float64, dev)
    L = _lib.lib()
    ws_bytes = L.dagr_viz_workspace_bytes(F, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.dagr_viz_render(_lib.ptr(images_t), n_img, H, W, _lib.ptr(fi_t), F,
                                     _lib.ptr(xt), _lib.ptr(yt), _lib.ptr(pt), _lib.ptr(ep_t), n_ev, _lib.ptr(a_t),
                                     _lib.ptr(box_t), _lib.ptr(bp_t), n_boxes, int(linewidth), _lib.ptr(col_t), n_col,
                                     _lib.ptr(out), _lib.ptr(status), _lib.ptr(ws), ws_bytes, _lib.cur_stream(dev)),
                   "viz_render")
    st = int(status.item())
    for bit, exc, msg in _STATUS:
        if st & bit:
            raise exc(f"render_frames: {msg}")
    return out
