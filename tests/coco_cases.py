"""Deterministic evaluation cases for tests/test_coco_match_cpu.py and tests/test_coco_match_gpu.py (plain module, no test
in it).

Every generator returns ``(ground_truth, detections)``: one dict per image, ``boxes`` float32 [n, 4] (x1, y1, x2, y2),
``labels`` int64 [n], detections also ``scores`` float32 [n] -- CPU tensors, the input of ``evaluate_detection`` and of
``DetectionBuffer.update``.  Two classes everywhere.  The expected values are always the host evaluator's
(``coco_eval._evaluate_image`` / ``evaluate_detection``); nothing here looks at the device matcher.

The hand-made cases use small integer coordinates, so that every area, intersection and IoU named in their docstrings is
exact in float64 (and the float32 subtraction x2 - x1 is exact too)."""
import numpy as np
import torch

CLASSES = ("car", "pedestrian")
SWEEP_SEED = 3            # chosen on the CPU: tests/test_coco_match_cpu.py::test_the_sweep_is_not_vacuous holds for it


def _gt(boxes, labels):
    return {"boxes": torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), "labels": torch.tensor(labels, dtype=torch.int64)}


def _dt(boxes, labels, scores):
    return dict(_gt(boxes, labels), scores=torch.tensor(scores, dtype=torch.float32))


def empties():
    """Class 0: image 0 has detections and no ground truth, image 1 ground truth and no detection, image 2 neither (its
    boxes are class 1, which keeps the image in the evaluation); image 3 has no ground truth at all and is skipped."""
    gts = [_gt([[10, 10, 60, 60]], [1]), _gt([[20, 20, 80, 90]], [0]), _gt([[5, 5, 45, 45]], [1]), _gt([], [])]
    dts = [_dt([[12, 12, 50, 50], [100, 100, 150, 150], [10, 10, 60, 60]], [0, 0, 1], [0.9, 0.8, 0.7]),
           _dt([[0, 0, 40, 40]], [1], [0.5]), _dt([[5, 5, 45, 45]], [1], [0.6]), _dt([[1, 1, 9, 9]], [0], [0.4])]
    return gts, dts


def out_of_range():
    """One image, one 20 x 20 ground-truth box (area 400: small) and the same box as its detection: in the medium and
    large ranges the ground truth is ignored and the detection is matched to ignored ground truth."""
    return [_gt([[30, 30, 50, 50]], [0])], [_dt([[30, 30, 50, 50]], [0], [0.9])]


def ties():
    """Image 0: ground truth A = (5, 10, 25, 30) and B = (15, 10, 35, 30); detection 0 = (10, 10, 30, 30) has IoU 300 / 500
    with both, so the later index (B) is taken; detection 1 = A, with a lower score, then still finds A free (IoU 1).  Taking
    A first would leave detection 1 with B at IoU 200 / 600 and unmatched.
    Image 1: two detections with the same score 0.5, the first far from the ground truth, the second on it: the stable
    order keeps (unmatched, matched)."""
    gts = [_gt([[5, 10, 25, 30], [15, 10, 35, 30]], [0, 0]), _gt([[100, 100, 140, 160]], [1])]
    dts = [_dt([[10, 10, 30, 30], [5, 10, 25, 30]], [0, 0], [0.9, 0.8]),
           _dt([[10, 10, 50, 70], [100, 100, 140, 160], [0, 0, 8, 8]], [1, 1, 1], [0.5, 0.5, 0.25])]
    return gts, dts


def exact_thresholds():
    """Detections 20 x 10 around ground truth lying inside them: IoU = area ratio = 100 / 200 = 0.5 in image 0 and
    150 / 200 = 0.75 in image 1, exactly; `iou >= thr` decides at the thresholds 0.5 and 0.75."""
    gts = [_gt([[0, 0, 10, 10]], [0]), _gt([[40, 40, 55, 50]], [0])]
    dts = [_dt([[0, 0, 20, 10]], [0], [0.9]), _dt([[40, 40, 60, 50]], [0], [0.8])]
    return gts, dts


def break_rule():
    """Medium range: the detection (0, 0, 90, 100), area 9000, lies inside ground truth 1 = (0, 0, 100, 100) (area 10000:
    ignored there, IoU 0.9) and around ground truth 0 = (0, 0, 60, 100) (evaluated, IoU 2 / 3).  Up to threshold 0.65 the
    evaluated box is kept although the ignored one overlaps more; from 0.7 on only the ignored one is left."""
    return [_gt([[0, 0, 60, 100], [0, 0, 100, 100]], [0, 0])], [_dt([[0, 0, 90, 100]], [0], [0.9])]


def degenerate():
    """Empty boxes on both sides (0 / 0 = NaN IoU: the host loop then takes every later open candidate) next to ordinary
    ones."""
    gts = [_gt([[10, 10, 10, 10], [10, 10, 30, 30], [50, 50, 50, 50]], [0, 0, 0])]
    dts = [_dt([[10, 10, 10, 10], [10, 10, 30, 30], [50, 50, 50, 50]], [0, 0, 0], [0.9, 0.8, 0.7])]
    return gts, dts


def crowded(n_gt, n_dt=130):
    """One image, one class: ``n_gt`` ground-truth boxes of 12 x 12 on a 16-pixel grid (32 per row), ``n_dt`` > MAX_DETS
    detections -- box k shifted by (k mod 5, k mod 3) pixels, scores descending in steps of 1 / 256 but laid out in a
    shuffled order, every seventh one doubled with the same score."""
    k = np.arange(n_gt)
    x, y = 16.0 * (k % 32), 16.0 * (k // 32)
    gt = np.stack([x, y, x + 12, y + 12], 1)
    j = np.arange(n_dt) % n_gt
    dt = gt[j] + np.stack([j % 5, j % 3, j % 5, j % 3], 1)
    scores = 1.0 - (np.arange(n_dt) - (np.arange(n_dt) % 7 == 6)) / 256.0
    perm = np.random.default_rng(n_gt).permutation(n_dt)
    return ([_gt(gt.tolist(), [0] * n_gt)],
            [_dt(dt[perm].tolist(), [0] * n_dt, scores[perm].tolist())])


def random_sweep(seed=SWEEP_SEED, n_images=64, width=320, height=240):
    """64 images, 2 classes, 0 - 12 ground-truth boxes and 0 - 40 detections each on a 320 x 240 canvas.  Box sides run
    from 6 to 150 pixels (small, medium and large areas).  Three detections in four are a ground-truth box of their image
    with its corners moved by up to a share a of its size, a drawn per detection between 0 and a fifth -- IoUs from about
    0.45 to 1, so every threshold sees matches and misses -- and with its class (one in ten flipped); the others are
    random boxes.  Scores are multiples of 1 / 64: ties happen."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for _ in range(n_images):
        n_g, n_d = int(rng.integers(0, 13)), int(rng.integers(0, 41))

        def boxes(n):
            side = np.exp(rng.uniform(np.log(6.0), np.log(150.0), (n, 2)))
            x1 = rng.uniform(0, width - side[:, 0].clip(max=width - 1))
            y1 = rng.uniform(0, height - side[:, 1].clip(max=height - 1))
            return np.stack([x1, y1, np.minimum(x1 + side[:, 0], width), np.minimum(y1 + side[:, 1], height)], 1)
        g_box, g_lab = boxes(n_g), rng.integers(0, 2, n_g)
        d_box, d_lab = boxes(n_d), rng.integers(0, 2, n_d)
        if n_g:
            src = rng.integers(0, n_g, n_d)
            near = rng.uniform(size=n_d) < 0.75
            size = np.tile(g_box[src, 2:] - g_box[src, :2], 2)
            jittered = g_box[src] + rng.uniform(-1.0, 1.0, (n_d, 4)) * rng.uniform(0.0, 0.2, (n_d, 1)) * size
            d_box[near] = jittered[near]
            flip = rng.uniform(size=n_d) < 0.1
            d_lab[near] = np.where(flip, 1 - g_lab[src], g_lab[src])[near]
        scores = rng.integers(1, 65, n_d) / 64.0
        gts.append(_gt(g_box.tolist(), g_lab.tolist()))
        dts.append(_dt(d_box.tolist(), d_lab.tolist(), scores.tolist()))
    return gts, dts


def small_cases():
    """name -> (ground truth, detections) of the hand-made cases."""
    return {"empties": empties(), "out_of_range": out_of_range(), "ties": ties(), "exact_thresholds": exact_thresholds(),
            "break_rule": break_rule(), "degenerate": degenerate()}


def forward_detections_form(dts, device, pad=3):
    """The detections of a batch as ``forward_detections`` hands them out: ``det[B, A, 6]`` (x1, y1, x2, y2, score, label;
    rows past an image's count hold garbage) and ``n_keep[B]`` int32, on ``device``."""
    A = max(len(d["boxes"]) for d in dts) + pad
    det = torch.full((len(dts), A, 6), -7.0)
    for b, d in enumerate(dts):
        n = len(d["boxes"])
        det[b, :n, :4], det[b, :n, 4], det[b, :n, 5] = d["boxes"], d["scores"], d["labels"].float()
    return det.to(device), torch.tensor([len(d["boxes"]) for d in dts], dtype=torch.int32).to(device)
