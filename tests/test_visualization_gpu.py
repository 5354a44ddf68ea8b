"""dagr.visualization on the device (csrc/viz.hip, dagr_viz_render; dagr_nms_batched for the box filter).

* ``draw_events_on_image`` equals the reference's own function bit for bit (tests/golden/ref_py_viz.npz <-
  tests/make_golden_refpy_viz.py), numpy or device tensors in, and draws in place;
* ``render_frames`` over 40 frames with overlapping windows equals a per-frame loop of the numpy restatement below;
* ``filter_boxes`` equals the reference's masks; the outlines equal the numpy restatement of this project's outline rule;
* ``scripts/visualize_detections.py`` end to end over an in-memory sequence: PNG count and contents."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_refpy_viz as G  # noqa: E402  (input builders; the generator's main() is not run)

from dagr_amd.utils import synthetic as syn  # noqa: E402
from dagr_amd.utils.buffers import detections_to_records  # noqa: E402
from dagr_amd.visualization import bbox_viz as B  # noqa: E402
from dagr_amd.visualization import event_viz as EV  # noqa: E402
from dagr_amd.visualization import render_frames  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "ref_py_viz.npz"))
DEV = torch.device("cuda:0")


# ---- numpy restatements (test-only) ------------------------------------------------------------------------------------
def events_np(img, x, y, p, alpha):
    """event_viz.py:4-10: the last event (array order) on a pixel decides it; rows outside the image are skipped."""
    out = img.copy()
    H, W = img.shape[:2]
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    idx = np.nonzero((x >= 0) & (x < W) & (y >= 0) & (y < H))[0]
    last = np.full(H * W, -1, np.int64)
    np.maximum.at(last, y[idx] * W + x[idx], idx)
    hit = np.nonzero(last >= 0)[0]
    flat = out.reshape(-1, 3)
    v = (alpha * flat[hit].astype(np.float64)).astype(np.uint8)
    ch = (np.asarray(p, np.int64)[last[hit]] - 1) % 3
    r = np.arange(len(hit))
    v[r, ch] = (v[r, ch] + 255 * (1 - alpha)).astype(np.uint8)
    flat[hit] = v
    return out


def outlines_np(img, rows, linewidth, colors=None):
    """The outline rule: Chebyshev distance to the rectangle's border <= linewidth // 2, later boxes on top."""
    colors = B.outline_colors() if colors is None else colors
    out = img.copy()
    H, W = img.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    for x0, y0, x1, y1, c in np.asarray(rows, np.int64).reshape(-1, 5):
        xa, xb, ya, yb = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        inside = (xx >= xa) & (xx <= xb) & (yy >= ya) & (yy <= yb)
        d_in = np.minimum(np.minimum(xx - xa, xb - xx), np.minimum(yy - ya, yb - yy))
        d_out = np.maximum(np.maximum(np.maximum(xa - xx, xx - xb), 0), np.maximum(np.maximum(ya - yy, yy - yb), 0))
        out[np.where(inside, d_in, d_out) <= linewidth // 2] = colors[c]
    return out


def label_mask(shape, corners, cls, scores, label=""):
    m = np.zeros(shape[:2], bool)
    for i in range(len(corners)):
        (xa, ya, xb, yb), _ = B.label_rect(corners[i][0], corners[i][1],
                                           B.label_text(int(cls[i]), None if scores is None else scores[i], label))
        m[max(ya, 0):max(yb + 1, 0), max(xa, 0):max(xb + 1, 0)] = True
    return m


# ---- events ------------------------------------------------------------------------------------------------------------
def _small_cases():
    names = sorted({k[3:-4] for k in GOLD.files if k.startswith("ev_") and k.endswith("_out")})
    assert len(names) == 6
    return names


@pytest.mark.parametrize("name", _small_cases())
def test_draw_events_equals_the_reference(name):
    img, x, y, p = (GOLD[f"ev_{name}_{k}"] for k in ("img", "x", "y", "p"))
    alpha, want = float(GOLD[f"ev_{name}_alpha"]), GOLD[f"ev_{name}_out"]
    assert np.array_equal(events_np(img, x, y, p, alpha), want)          # the restatement itself, against the reference
    a = img.copy()
    r = EV.draw_events_on_image(a, x, y, p, alpha)
    assert r is a and np.array_equal(a, want)
    t = torch.from_numpy(img.copy()).to(DEV)
    xt, yt, pt = (torch.from_numpy(v.astype(np.int64)).to(DEV) for v in (x, y, p))
    r = EV.draw_events_on_image(t, xt, yt, pt, alpha)
    assert r is t and np.array_equal(t.cpu().numpy(), want)


def test_draw_events_full_frame_digest():
    import hashlib
    img, x, y, p, alpha = G.full_case()
    a = img.copy()
    EV.draw_events_on_image(a, x, y, p, alpha)
    assert int((a != img).any(-1).sum()) == int(GOLD["ev_full_changed"])
    assert hashlib.sha256(a.tobytes()).digest() == GOLD["ev_full_sha256"].tobytes()


def test_bad_polarity_and_alpha_are_errors():
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="polarity"):
        EV.draw_events_on_image(img, np.array([1]), np.array([1]), np.array([5]))
    with pytest.raises(ValueError, match="polarity"):
        EV.draw_events_on_image(img, np.array([1]), np.array([1]), np.array([255], np.uint8))
    with pytest.raises(ValueError, match="alpha"):
        EV.draw_events_on_image(img, np.array([1]), np.array([1]), np.array([1]), alpha=1.5)
    assert not img.any()
    a = img.copy()      # x >= W and negative rows are skipped
    EV.draw_events_on_image(a, np.array([8, 3, 100]), np.array([1, -2, 2]), np.array([1, 1, 0]))
    assert not a.any()


def _stream(W=640, H=480, span=60000, n=120000, seed=5):
    x, y, t, p = syn.edges_window(n // 2, W, H, seed, window_us=span, time_window=span)
    x2, y2, t2, p2 = syn.uniform_window(n // 2, W, H, seed + 1, window_us=span, time_window=span)
    order = np.argsort(np.concatenate([t, t2]), kind="stable")
    cat = lambda a, b: np.concatenate([a, b])[order]
    return cat(x, x2), cat(y, y2), cat(t, t2), cat(p, p2)


def test_render_frames_equals_a_per_frame_loop():
    W, H = 640, 480
    x, y, t, p = _stream(W, H)
    g = np.random.default_rng(2)
    images = g.integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    F = 40
    stamps = 5000 + 1000 * np.arange(F)            # overlapping 5 ms windows ...
    stamps[-4:] = 80000 + 7000 * np.arange(4)      # ... and empty ones after the stream ends
    frame_image = np.array([0] * 12 + [1] * 20 + [2] * 8)
    frame_image[5] = 2                             # frames 5 and 32 share image 2 with others
    segs = [np.nonzero((t >= s - 5000) & (t <= s))[0] for s in stamps]
    assert sum(len(s) == 0 for s in segs) == 4 and min(len(s) for s in segs[:-4]) > 1000
    ev = np.concatenate(segs)
    ev_ptr = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    alpha = np.where(np.arange(F) % 3 == 0, 0.3, 0.5)
    rows, box_ptr = [], [0]
    for f in range(F):                              # boxes on every other frame (the fused outline pass)
        n = 0 if f % 2 else int(g.integers(1, 6))
        c = g.integers(-30, 660, (n, 2))
        rows.append(np.concatenate([c, c + g.integers(-40, 200, (n, 2)), g.integers(0, 2, (n, 1))], 1))
        box_ptr.append(box_ptr[-1] + n)
    out = render_frames(images, frame_image, x[ev], y[ev], p[ev], ev_ptr, alpha, boxes=np.concatenate(rows),
                        box_ptr=box_ptr, linewidth=2).cpu().numpy()
    for f in range(F):
        s = segs[f]
        want = outlines_np(events_np(images[frame_image[f]], x[s], y[s], p[s], alpha[f]), rows[f], 2)
        assert np.array_equal(out[f], want), f
    assert np.array_equal(out[-1], outlines_np(images[frame_image[-1]], rows[-1], 2))     # empty window: image + boxes


# ---- boxes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["boxes0", "boxes1", "boxes2", "boxes3", "boxes_empty"])
def test_filter_boxes_equals_the_reference(name):
    args = [GOLD[f"{name}_{k}"] for k in ("x", "y", "w", "h", "labels", "scores")]
    conf, nms = float(GOLD[f"{name}_conf"]), float(GOLD[f"{name}_nms"])
    got = B.filter_boxes(*args, conf, nms)
    want = GOLD[f"{name}_mask"]
    assert got.dtype == bool and np.array_equal(got, want)


def _box_scene():
    """Boxes partly and wholly outside the image, negative corners, swapped corners, overlaps of both classes."""
    x = np.array([-10.7, 20.2, 30.0, 200.0, -80.0, 5.5, 40.0, 45.0, 60.9, 10.0, 90.0], np.float32)
    y = np.array([-3.2, 10.0, 15.5, 20.0, -60.0, 70.0, 30.0, 35.0, 41.0, 50.0, 5.0], np.float32)
    w = np.array([40.0, 50.0, 30.0, 40.0, 30.0, 110.0, 30.0, 20.0, 8.0, -6.0, 0.0], np.float32)
    h = np.array([20.0, 40.0, 20.0, 30.0, 20.0, 30.0, 20.0, 30.0, 6.0, 9.0, 0.0], np.float32)
    labels = np.array([0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1], np.uint8)
    return x, y, w, h, labels


@pytest.mark.parametrize("linewidth", [1, 2, 3])
def test_outlines_equal_the_restated_rule(linewidth):
    g = np.random.default_rng(linewidth)
    img = g.integers(0, 256, (80, 120, 3)).astype(np.uint8)
    x, y, w, h, labels = _box_scene()
    corners, cls, _ = B.select_boxes(x, y, w, h, labels)
    want = outlines_np(img, B.box_rows(corners, cls), linewidth)
    a = img.copy()
    assert B.draw_bbox_on_img(a, x, y, w, h, labels, linewidth=linewidth, text=False) is a
    assert np.array_equal(a, want)
    t = torch.from_numpy(img.copy()).to(DEV)
    assert B.draw_bbox_on_img(t, x, y, w, h, labels, linewidth=linewidth, text=False) is t
    assert np.array_equal(t.cpu().numpy(), want)


def test_scored_boxes_are_filtered_before_drawing():
    name = "boxes0"
    args = [GOLD[f"{name}_{k}"] for k in ("x", "y", "w", "h", "labels", "scores")]
    conf, nms = float(GOLD[f"{name}_conf"]), float(GOLD[f"{name}_nms"])
    img = np.zeros((480, 640, 3), np.uint8)
    m = GOLD[f"{name}_mask"]
    corners, cls, _ = B.select_boxes(*(a[m] for a in args[:5]))
    a = B.draw_bbox_on_img(img.copy(), *args, conf=conf, nms=nms, text=False)
    assert np.array_equal(a, outlines_np(img, B.box_rows(corners, cls), 2))


def test_label_text_stays_inside_the_label_backgrounds():
    pytest.importorskip("PIL")
    g = np.random.default_rng(4)
    img = g.integers(0, 256, (120, 160, 3)).astype(np.uint8)
    x, y, w, h, labels = _box_scene()
    scores = np.linspace(0.99, 0.6, len(x)).astype(np.float32)
    plain = B.draw_bbox_on_img(img.copy(), x, y, w, h, labels, scores, conf=0.3, nms=0.99, text=False)
    text = B.draw_bbox_on_img(img.copy(), x, y, w, h, labels, scores, conf=0.3, nms=0.99, label="L")
    corners, cls, sc = B.select_boxes(x, y, w, h, labels, scores, conf=0.3, nms=0.99)
    inside = label_mask(img.shape, corners, cls, sc, "L")
    diff = (plain != text).any(-1)
    assert diff.any() and not (diff & ~inside).any()


def test_more_than_1024_boxes_is_the_documented_error():
    n = 1025
    v = np.arange(n, dtype=np.float32)
    with pytest.raises(ValueError, match="1024"):
        B.filter_boxes(v, v, v + 1, v + 1, np.zeros(n, np.uint8), np.ones(n, np.float32), 0.3, 0.65)
    B.filter_boxes(v[:1024], v[:1024], v[:1024] + 1, v[:1024] + 1, np.zeros(1024, np.uint8), np.ones(1024, np.float32),
                   0.3, 0.65)


# ---- the script, end to end --------------------------------------------------------------------------------------------
class MemorySource:
    """300 ms of events, an image every 50 ms (BGR), t_range / image_timestamps / image(i) / events(t0, t1)."""
    T0, SPAN, W, H = 7_000_000, 300_000, 640, 480

    def __init__(self):
        x, y, t, p = _stream(self.W, self.H, span=self.SPAN, n=90000, seed=9)
        self.x, self.y, self.t = x.astype(np.uint16), y.astype(np.uint16), t.astype(np.int64) + self.T0
        self.p = (p > 0).astype(np.uint8)                  # DSEC's {0, 1}
        self.image_timestamps = self.T0 + np.arange(0, self.SPAN, 50_000)
        yy, xx = np.mgrid[0:self.H, 0:self.W]          # smooth frames: the PNGs stay small
        self.images = np.stack([np.stack([(xx // 3 + 40 * i) % 256, (yy // 2 + 25 * i) % 256, (xx + yy) // 5 % 256], -1)
                                for i in range(len(self.image_timestamps))]).astype(np.uint8)

    def t_range(self):
        return self.T0, self.T0 + self.SPAN

    def image(self, i):
        return self.images[i].copy()

    def events(self, t0, t1):
        m = (self.t >= t0) & (self.t <= t1)
        return {"x": self.x[m], "y": self.y[m], "p": self.p[m], "t": self.t[m]}


def _detections():
    g = np.random.default_rng(3)
    recs = []
    for k in range(12):                                   # every 20 ms from 40 ms on: early frames clip to the first
        n = int(g.integers(3, 14))
        c = g.uniform(0, 320, (n, 2)).astype(np.float32)
        wh = g.uniform(8, 60, (n, 2)).astype(np.float32)
        boxes = np.concatenate([c, c + wh], 1)
        recs.append(detections_to_records(dict(boxes=boxes, labels=g.integers(0, 2, n), scores=g.uniform(0.1, 1, n)
                                               .astype(np.float32)), MemorySource.T0 + 40_000 + 20_000 * k))
    return np.concatenate(recs)


def _expected(src, s, t, dets=None):
    import visualize_detections as V
    img = src.image(int(V.compute_index(src.image_timestamps, [t])[0]))
    ev = src.events(t - 5000, t)
    frame = events_np(img, ev["x"], ev["y"], ev["p"], 0.5)
    if dets is None:
        return frame, None
    ts = np.unique(dets["t"])
    b = dets[dets["t"] == ts[V.compute_index(ts, [t])[0]]]
    corners, cls, sc = B.select_boxes(2 * b["x"], 2 * b["y"], 2 * b["w"], 2 * b["h"], b["class_id"], b["class_confidence"],
                                      conf=0.3, nms=0.65)
    return outlines_np(frame, B.box_rows(corners, cls), 2), label_mask(frame.shape, corners, cls, sc)


def test_script_end_to_end(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    import visualize_detections as V
    src, dets = MemorySource(), _detections()
    folder = tmp_path / "run"
    folder.mkdir()
    np.save(folder / "detections_zurich_city_13_b.npy", dets)
    n = V.main(["--detections_folder", str(folder), "--dataset_directory", str(tmp_path / "unused"),
                "--vis_time_step_us", "1000", "--event_time_window_us", "5000", "--write_to_output"], source=src)
    t0, t1 = src.t_range()
    stamps = np.arange(t0, t1, 1000)
    files = sorted((folder / "visualization").glob("*.png"))
    assert n == len(stamps) == len(files) == 300 and files[-1].name == "000299.png"
    drawn = 0
    for s in range(0, len(stamps), 7):
        got = np.asarray(Image.open(folder / "visualization" / ("%06d.png" % s)).convert("RGB"))[..., ::-1]
        want, labels = _expected(src, s, stamps[s], dets)
        assert got.shape == want.shape
        assert np.array_equal(got[~labels], want[~labels]), s
        drawn += int(labels.any())
    assert drawn > 10


def test_script_frames_without_detections_are_events_and_images():
    import visualize_detections as V
    src = MemorySource()
    args = V.build_parser().parse_args(["--vis_time_step_us", "1000", "--event_time_window_us", "5000"])
    frames = {}
    n = V.visualize(args, src, lambda s, f: frames.__setitem__(s, f.copy()), detections=None)
    stamps = np.arange(*src.t_range(), 1000)
    assert n == len(stamps) == len(frames)
    for s in range(0, len(stamps), 3):
        assert np.array_equal(frames[s], _expected(src, s, stamps[s])[0]), s
