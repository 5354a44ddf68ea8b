"""Scenes for the event stream's mAP log and plan (dagr_stream_map_log / dagr_stream_map_plan), in numpy only: the CPU suite
runs MapDefinition on them, the GPU suite the kernels against MapDefinition.  A scene is ``dict(name, B, A, G, map,
n_classes, steps)``; a step is ``dict(det fp32 [B, A, 6], n_keep int32 [B], gt_box fp32 [B, G, 4], gt_label int32 [B, G],
n_gt int32 [B], t_ref int64 [B])``.  Rows behind the counts carry the sentinel -7, so that a kernel that reads past a count
shows."""
import numpy as np

from dagr_amd.streaming import MapDefinition
from dagr_amd.utils import coco_eval as CE

SENTINEL = -7.0
T0 = (1 << 33) + 12345


def _boxes(rng, n, lo=4.0, hi=120.0):
    xy = rng.uniform(0, 200, (n, 2))
    wh = rng.uniform(lo, hi, (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def _step(rng, B, A, G, k, n_keep, n_gt, n_classes=2, det_labels=None, gt_labels=None, scores=None):
    det = np.full((B, A, 6), SENTINEL, np.float32)
    gt_box = np.full((B, G, 4), SENTINEL, np.float32)
    gt_label = np.full((B, G), int(SENTINEL), np.int32)
    for b in range(B):
        nk, ng = max(int(n_keep[b]), 0), max(int(n_gt[b]), 0)
        det[b, :nk, :4] = _boxes(rng, nk)
        det[b, :nk, 4] = rng.choice(np.arange(1, 9) / 8.0, nk) if scores is None else scores[b][:nk]
        det[b, :nk, 5] = rng.integers(0, n_classes, nk) if det_labels is None else det_labels[b][:nk]
        gt_box[b, :ng] = _boxes(rng, ng)
        gt_label[b, :ng] = rng.integers(0, n_classes, ng) if gt_labels is None else gt_labels[b][:ng]
    return dict(det=det, n_keep=np.asarray(n_keep, np.int32), gt_box=gt_box, gt_label=gt_label,
                n_gt=np.asarray(n_gt, np.int32), t_ref=np.full(B, T0 + 1000 * k, np.int64) + np.arange(B) * 7)


def _overflow(B):
    """G = 4, A = 8 with max_dets = 5 (the cut), max_images = 5 overflowed by two steps in every lane; a lane with n_gt = -1,
    one with n_gt = 0 and one with n_keep = 0 (with B = 1: one step each)."""
    rng, steps = np.random.default_rng(40 + B), []
    for k in range(9 if B == 1 else 8):
        n_keep, n_gt = rng.integers(1, 9, B), rng.integers(1, 5, B)
        if B == 1:
            if k == 1:
                n_gt[0] = -1
            if k == 2:
                n_gt[0] = 0
            if k == 3:
                n_keep[0] = 0
        elif k == 2:
            n_gt[0], n_gt[1], n_keep[2] = -1, 0, 0
        n_keep[0] = 8 if k == 0 else n_keep[0]                     # the cut is met at least once
        steps.append(_step(rng, B, 8, 4, k, n_keep, n_gt))
    return dict(name=f"overflow-B{B}", B=B, A=8, G=4, map=dict(max_images=5, max_dets=5), n_classes=2, steps=steps)


def _wide():
    """A = 130 rows in a lane, more than two waves' worth, nothing cut; 120 of them in class 0: the MAX_DETS column cut."""
    rng, steps = np.random.default_rng(7), []
    for k, nk in enumerate((130, 129)):
        labels = [np.where(np.arange(130) % 13 == 0, 1.0, 0.0)]
        steps.append(_step(rng, 1, 130, 4, k, [nk], [3], det_labels=labels, scores=[rng.permutation(130) / 130.0]))
    return dict(name="wide-A130", B=1, A=130, G=4, map=dict(max_images=3, max_dets=None), n_classes=2, steps=steps)


def _classes(n_classes):
    """Two lanes, G = 4, A = 8, written out: an (image, class) with detections only and one with ground truth only; with
    three classes also a class nobody has (2) and labels outside [0, n_classes): 7 and -1 in the ground truth, 5, -1, 0.5 and
    NaN in the detections."""
    rng, steps = np.random.default_rng(11 + n_classes), []
    odd = n_classes == 3
    # lane 0: class 0 has ground truth only, class 1 detections only; lane 1: both classes have both
    steps.append(_step(rng, 2, 8, 4, 0, [3, 5], [2, 4], det_labels=[[1, 1, 1], [0, 1, 0, 1, 1]], gt_labels=[[0, 0], [1, 0, 1, 0]]))
    steps.append(_step(rng, 2, 8, 4, 1, [6, 2], [3, 1],
                       det_labels=[[0, 5 if odd else 1, -1 if odd else 0, 0.5 if odd else 1, np.nan if odd else 0, 1], [1, 1]],
                       gt_labels=[[1, 7 if odd else 0, -1 if odd else 1], [0]]))
    steps.append(_step(rng, 2, 8, 4, 2, [0, 4], [2, -1], det_labels=[[], [0, 0, 0, 0]], gt_labels=[[1, 1], []]))
    steps.append(_step(rng, 2, 8, 4, 3, [8, 8], [4, 4], n_classes=2))
    return dict(name=f"classes-{n_classes}", B=2, A=8, G=4, map=dict(max_images=6, max_dets=None), n_classes=n_classes, steps=steps)


def _empty():
    rng = np.random.default_rng(3)
    steps = [_step(rng, 2, 8, 4, 0, [3, 3], [-1, 0])]
    return dict(name="empty-log", B=2, A=8, G=4, map=dict(max_images=4, max_dets=None), n_classes=2, steps=steps)


def log_cases():
    return [_overflow(1), _overflow(3), _wide()]


def plan_cases():
    return [_classes(2), _classes(3), _wide(), _empty(), _overflow(3)]


def metrics_scene():
    """Three lanes, six instants, two classes, G = 8, A = 24.  Ground truth with sides around the 32^2 and 96^2 area bounds
    (31 x 33, 32 x 32, 33 x 32, 95 x 97, 96 x 96, 97 x 96 among them); detections that are the ground truth moved by a
    few pixels, with some missing, plus false positives; scores in eighths, the same few values in every lane and at every
    instant, so that the order of equal scores is the image order."""
    rng = np.random.default_rng(2024)
    sides = [(12, 14), (31, 33), (32, 32), (33, 32), (60, 50), (95, 97), (96, 96), (97, 96), (130, 110), (20, 45)]
    B, A, G, steps = 3, 24, 8, []
    for k in range(6):
        det = np.full((B, A, 6), SENTINEL, np.float32)
        gt_box, gt_label = np.full((B, G, 4), SENTINEL, np.float32), np.full((B, G), int(SENTINEL), np.int32)
        n_keep, n_gt = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for b in range(B):
            ng = int(rng.integers(3, G + 1))
            wh = np.array([sides[i] for i in rng.integers(0, len(sides), ng)], np.float64)
            xy = rng.uniform(0, 150, (ng, 2))
            gt_box[b, :ng] = np.concatenate([xy, xy + wh], 1)
            gt_label[b, :ng] = rng.integers(0, 2, ng)
            rows = []
            for g in range(ng):
                if rng.random() < 0.8:                            # a detection of this box, more or less well placed
                    shift = rng.normal(0, 0.06, 4) * np.concatenate([wh[g], wh[g]])
                    label = gt_label[b, g] if rng.random() < 0.9 else 1 - gt_label[b, g]
                    rows.append(list(gt_box[b, g] + shift) + [rng.integers(3, 9) / 8.0, label])
            for _ in range(int(rng.integers(1, 5))):              # false positives
                rows.append(list(_boxes(rng, 1, 10, 110)[0]) + [rng.integers(1, 7) / 8.0, rng.integers(0, 2)])
            rows.sort(key=lambda r: -r[4])
            det[b, :len(rows)] = np.asarray(rows, np.float32)
            n_keep[b], n_gt[b] = len(rows), ng
        if k == 4:
            n_gt[1] = -1                                          # a lane without labels at this instant
        steps.append(dict(det=det, n_keep=n_keep, gt_box=gt_box, gt_label=gt_label, n_gt=n_gt,
                          t_ref=np.full(B, T0 + 1000 * k, np.int64)))
    return dict(name="metrics", B=B, A=A, G=G, map=dict(max_images=8, max_dets=None), n_classes=2, steps=steps)


def run_definition(scene, each=None):
    """MapDefinition through the scene's steps; ``each(k, step, definition)`` after every step."""
    d = MapDefinition(scene["B"], scene["map"])
    for k, s in enumerate(scene["steps"]):
        d.step(s["det"], s["n_keep"], s["gt_box"], s["gt_label"], s["n_gt"], s["t_ref"])
        if each is not None:
            each(k, s, d)
    return d


def expected_plan(d, n_classes):
    """What dagr_stream_map_plan has to produce for the definition's images: ``build_jobs`` / ``column_layout`` /
    ``accumulate_groups`` on them, in the plan's arrays."""
    gt, dt = d.images()
    jobs = CE.build_jobs(CE.evaluated_images(gt, dt), n_classes)
    kept, o_off, n_out, gi_off, n_gign = CE.column_layout(jobs)
    group, group_ptr = CE.accumulate_groups(jobs, n_classes)
    J = len(jobs)
    totals = [J, len(jobs.gt), len(jobs.dt), n_out, n_gign, int(jobs.table[:, 1].max()) if J else 0,
              int(jobs.table[:, 3].max()) if J else 0, sum(len(v["boxes"]) for v in dt)]
    return dict(gt=jobs.gt, dt=jobs.dt, scores=jobs.scores,
                jobs=np.concatenate([jobs.table, o_off[:, None], gi_off[:, None]], 1).astype(np.int64), rng=jobs.rng,
                info=np.stack([group, kept, o_off, gi_off], 1).astype(np.int64).reshape(-1, 4),
                col_group=np.repeat(group, kept).astype(np.int64), entry_group=np.repeat(group, jobs.table[:, 1]).astype(np.int64),
                group_ptr=group_ptr, totals=np.asarray(totals, np.int64))
