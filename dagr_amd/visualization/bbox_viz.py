"""``dagr.visualization.bbox_viz`` (reference: src/dagr/visualization/bbox_viz.py), filter and outlines on the device.

* ``filter_boxes``: ``scores > conf`` (strict) AND class-wise NMS over ALL the boxes (not only the confident ones), as
  the reference composes them; the NMS is ``dagr_nms_batched`` with torchvision ``batched_nms``'s class-offset trick
  (offset = largest coordinate + 1, in float32).  At most 1024 boxes per image (the kernel's limit): more raise.
  Boxes are taken in float32 (the records' type); ties in score are broken by the lower index.
* ``draw_bbox_on_img``: the outlines are drawn by ``dagr_viz_render`` under this project's own rule (OpenCV's thick-line
  rasteriser is not reproduced): a pixel is on a box's outline when its Chebyshev distance to the border of the box's
  rectangle is <= ``linewidth // 2``, clipped to the image, later boxes over earlier ones.  Corners are
  ``int(x)``, ``int(y)``, ``int(x + w)``, ``int(y + h)`` (truncation, the sum in the inputs' dtype) and colours are the
  reference's.  The label backgrounds (the reference's rectangle geometry, with PIL's text size in place of
  ``cv2.getTextSize``) and texts are drawn afterwards, on the host, with PIL's default font: text pixels are not
  OpenCV's Hershey font.  ``text=False`` draws outlines only.
* Class ids outside the colour table raise ``IndexError`` (negative ids wrap, as the reference's ``_COLORS[cls_id]``).
"""
import numpy as np
import torch

from .. import _lib
from .frames import _device, render_frames

_COLORS = np.array([[0.000, 0.8, 0.1], [1, 0.67, 0.00]])
class_names = ["car", "pedestrian"]
MAX_BOXES = 1024      # dagr_nms_batched's A <= 1024


def outline_colors():
    """``(_COLORS[c] * 255).astype(uint8)`` per class, the outline colours (bbox_viz.py:32)."""
    return (_COLORS * 255).astype(np.uint8)


def label_colors(cls_id):
    """Label background and text colours of a class (bbox_viz.py:37, :43)."""
    bk = tuple((_COLORS[cls_id] * 255 * 0.7).astype(np.uint8).tolist())
    txt = (0, 0, 0) if np.mean(_COLORS[cls_id]) > 0.5 else (255, 255, 255)
    return bk, txt


def filter_boxes(x, y, w, h, labels, scores, conf, nms):
    """Boolean mask of the boxes to draw: ``scores > conf`` and kept by class-wise NMS (IoU > ``nms`` suppressed)."""
    x, y, w, h = (np.asarray(v, dtype=np.float32) for v in (x, y, w, h))
    scores = np.asarray(scores, dtype=np.float32)
    labels = np.asarray(labels)
    A = len(x)
    if A > MAX_BOXES:
        raise ValueError(f"filter_boxes: at most {MAX_BOXES} boxes per image (dagr_nms_batched), got {A}")
    if A == 0:
        return np.zeros(0, dtype=bool)
    coords = np.stack([x, y, x + w, y + h], axis=-1)
    offset = np.float32(coords.max()) + np.float32(1)               # batched_nms: max_coordinate + 1
    dev = _device(None)
    boxes_t = torch.from_numpy(np.ascontiguousarray(coords)).to(dev)
    scores_t = torch.from_numpy(np.ascontiguousarray(scores)).to(dev)
    cls_t = torch.from_numpy(labels.astype(np.int32)).to(dev)
    valid = torch.ones(A, dtype=torch.uint8, device=dev)
    order = torch.empty(A, dtype=torch.int32, device=dev)
    keep = torch.empty(A, dtype=torch.int32, device=dev)
    n_keep = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dagr_nms_batched(_lib.ptr(boxes_t), _lib.ptr(scores_t), _lib.ptr(cls_t), _lib.ptr(valid),
                                               1, A, float(nms), float(offset), _lib.ptr(order), _lib.ptr(keep),
                                               _lib.ptr(n_keep), _lib.cur_stream(dev)), "nms_batched")
    nms_mask = torch.zeros(A, dtype=torch.bool, device=dev)
    nms_mask[order[keep != 0].long()] = True
    return ((scores_t > conf) & nms_mask).cpu().numpy()


def select_boxes(x, y, w, h, labels, scores=None, conf=0.5, nms=0.45):
    """The boxes ``draw_bbox_on_img`` draws, in list order: ``(corners int64 [n, 4] (x0, y0, x1, y1), class ids [n],
    scores [n] or None)``."""
    x, y, w, h = (np.asarray(v) for v in (x, y, w, h))
    labels = np.asarray(labels)
    if scores is not None:
        scores = np.asarray(scores)
        mask = filter_boxes(x, y, w, h, labels, scores, conf, nms)
        mask &= ~(scores < conf)                                         # bbox_viz.py:22-23
        x, y, w, h, labels, scores = x[mask], y[mask], w[mask], h[mask], labels[mask], scores[mask]
    corners = np.stack([x, y, x + w, y + h], axis=-1) if len(x) else np.zeros((0, 4), dtype=np.float32)
    if not np.all(np.isfinite(corners)):
        raise ValueError("box coordinates must be finite")
    n_cls = len(_COLORS)
    cls = labels.astype(np.int64)
    if len(cls) and (cls.min() < -n_cls or cls.max() >= n_cls):
        raise IndexError(f"class ids must lie in [0, {n_cls})")
    return np.trunc(corners).astype(np.int64), np.where(cls < 0, cls + n_cls, cls), scores


def box_rows(corners, cls):
    """``[n, 5]`` rows ``(x0, y0, x1, y1, class id)`` for ``render_frames``."""
    return np.concatenate([np.asarray(corners, dtype=np.int64).reshape(-1, 4),
                           np.asarray(cls, dtype=np.int64).reshape(-1, 1)], axis=1)


def _font():
    from PIL import ImageFont
    return ImageFont.load_default()


def label_text(cls_id, score=None, label=""):
    text = f"{label}-{class_names[cls_id]}"
    if score is not None:
        text += f":{score * 100: .1f}"
    return text


def label_rect(x0, y0, text, font=None):
    """The label background of a box with top-left corner (x0, y0), inclusive ``(xa, ya, xb, yb)`` (bbox_viz.py:41-49:
    ``(x0, y0 - int(1.5 * text_h))`` to ``(x0 + text_w + 1, y0 + 1)``), and the text's top-left position inside it."""
    font = font or _font()
    _, _, tw, th = (int(v) for v in font.getbbox(text))
    txt_height = int(1.5 * th)
    rect = (int(x0), int(y0) - txt_height, int(x0) + tw + 1, int(y0) + 1)
    return rect, (int(x0), int(y0) - txt_height + (txt_height + 1 - th) // 2)


def draw_labels(img, corners, cls, scores=None, label=""):
    """Label backgrounds and texts of the boxes, in list order, on a host image (numpy uint8 ``[H, W, 3]``, in place)."""
    if len(corners) == 0:
        return img
    from PIL import Image, ImageDraw
    font = _font()
    H, W = img.shape[:2]
    pil = Image.fromarray(img)                     # channel order kept as is: the colours below are BGR like the image
    draw = ImageDraw.Draw(pil)
    for i in range(len(corners)):
        c = int(cls[i])
        text = label_text(c, None if scores is None else scores[i], label)
        (xa, ya, xb, yb), pos = label_rect(corners[i][0], corners[i][1], text, font)
        bk, txt = label_colors(c)
        if xa < W and ya < H and xb >= 0 and yb >= 0:
            draw.rectangle([max(xa, 0), max(ya, 0), min(xb, W - 1), min(yb, H - 1)], fill=bk)
        draw.text(pos, text, fill=txt, font=font)
    img[...] = np.asarray(pil)
    return img


def draw_bbox_on_img(img, x, y, w, h, labels, scores=None, conf=0.5, nms=0.45, label="", linewidth=2, text=True):
    """Draw the boxes on ``img`` (uint8 BGR ``[H, W, 3]``: numpy, or a device tensor) in place and return it: outlines on
    the device, then (``text=True``) the label backgrounds and texts on the host."""
    corners, cls, scores = select_boxes(x, y, w, h, labels, scores, conf, nms)
    is_tensor = torch.is_tensor(img)
    if is_tensor and (img.dim() != 3 or img.shape[-1] != 3 or img.dtype != torch.uint8 or not img.is_cuda
                      or not img.is_contiguous()):
        raise ValueError("img must be a contiguous uint8 [H, W, 3] device tensor (or a numpy array)")
    if not is_tensor and (not isinstance(img, np.ndarray) or img.ndim != 3 or img.shape[-1] != 3 or img.dtype != np.uint8):
        raise ValueError("img must be a uint8 [H, W, 3] array")
    if len(corners) == 0:
        return img
    rows = box_rows(corners, cls)
    empty = np.zeros(0, dtype=np.int32)
    if is_tensor:
        render_frames(img, [0], empty, empty, empty, [0, 0], boxes=rows, box_ptr=[0, len(rows)], linewidth=linewidth,
                      out=img.unsqueeze(0), device=img.device)
        if text:
            host = img.cpu().numpy()
            img.copy_(torch.from_numpy(draw_labels(host, corners, cls, scores, label)))
        return img
    out = render_frames(img, [0], empty, empty, empty, [0, 0], boxes=rows, box_ptr=[0, len(rows)], linewidth=linewidth)
    img[...] = out[0].cpu().numpy()
    if text:
        draw_labels(img, corners, cls, scores, label)
    return img
