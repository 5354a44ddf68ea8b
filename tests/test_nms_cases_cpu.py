"""The detection-tail fixtures of tests/nms_cases.py, checked with the oracle alone: when a GPU test of
tests/test_postprocess_paths_gpu.py fails, the fixture and its expected value have already been vouched for here, so the
failure points at the kernel."""
import pytest
import torch

from oracle.postprocess import nms, postprocess_network_output
from tests import nms_cases as nc


def _rows(pred, C, anchors):
    boxes, score, label, _ = nc.rows_of(pred, C)
    return boxes[anchors], score[anchors], label[anchors]


@pytest.mark.parametrize("A", [1, 2, 3, 64, 65, 129, 256, 257, 1024])
def test_staircase_closed_form_is_the_oracles_answer(A):
    pred = nc.staircase(A)
    boxes, score, _, _ = nc.rows_of(pred, 1)
    assert torch.equal(nms(boxes, score, 0.5), nc.staircase_survivors(A))
    assert torch.equal(nc.expected_anchors(pred, 1), nc.staircase_survivors(A))
    shuffled, perm = nc.staircase(A, 3, cls=2, perm_seed=A)
    assert torch.equal(nc.expected_anchors(shuffled, 3), nc.staircase_survivors(A, perm))
    assert nc.pred_margin(pred, 1) > 0.03                  # 7/13 and 4/16 are far from 0.5


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_exact_threshold_pair_is_kept_under_every_class_offset(cls):
    pred = nc.exact_threshold(3, cls)
    boxes, _, label, _ = nc.rows_of(pred, 3)
    b = nc.offset_boxes(boxes, label)
    assert torch.equal(b[0], torch.tensor([0.0, 0.0, 4.0, 4.0]) + 641.0 * cls)
    w = (torch.min(b[0, 2:], b[1, 2:]) - torch.max(b[0, :2], b[1, :2])).clamp(min=0)
    inter = w[0] * w[1]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert float(inter / (area[0] + area[1] - inter)) == 0.5           # exactly, in fp32
    assert nc.expected_anchors(pred, 3).tolist() == [0, 1]
    det, = postprocess_network_output(pred[None], 3, nc.CONF, nc.IOU, height=nc.HEIGHT, width=nc.WIDTH)
    assert det["labels"].tolist() == [cls, cls] and len(det["boxes"]) == 2
    # ... and just below the threshold the second one goes
    assert nc.expected_anchors(pred, 3, iou=0.4999).tolist() == [0]


def test_degenerate_boxes_suppress_nothing_and_classes_are_separated():
    pred = nc.degenerate()
    assert nc.expected_anchors(pred, 2).tolist() == [0, 1, 2, 3, 4, 5, 6, 8, 9]


def test_fixed_cases_have_the_survivors_their_names_promise():
    for A in (64, 257, 1024):
        assert nc.counts(nc.all_survive(A, 3, 6), 3) == (A, A)
        pred = nc.one_survives(A, 3, 8)
        assert nc.counts(pred, 3) == (A, 1)
        assert nc.expected_anchors(pred, 3).tolist() == [int(torch.argmax(pred[:, 4]))]
        assert nc.counts(nc.none_pass(A, 3, 5), 3) == (0, 0)


@pytest.mark.parametrize("kind,A,C,seed", nc.random_cases(), ids=lambda v: str(v))
def test_random_cases_have_their_margin_and_are_not_vacuous(kind, A, C, seed):
    """No candidate pair within 2e-6 of the IoU threshold (nms_cases' docstring has the derivation), and -- a cap against
    vacuous cases, not a measurement -- at least A/4 suppressed and A/8 surviving candidates.  The cap starts at 63
    boxes: one box cannot be suppressed, so at A = 1 and 2 it cannot hold."""
    pred = nc.make(kind, A, C, seed)
    cand, surv = nc.counts(pred, C)
    margin = nc.pred_margin(pred, C)
    print(f"{kind} A={A} C={C} seed={seed}: {cand} candidates, {surv} survivors, min |IoU - thr| = {margin:.3g}")
    assert margin >= nc.MARGIN
    if A >= nc.VACUITY_FROM:
        assert 4 * (cand - surv) >= A and 8 * surv >= A
    # the helper that names the surviving anchors and the oracle's own entry point agree
    det, = postprocess_network_output(pred[None], C, nc.CONF, nc.IOU, height=nc.HEIGHT, width=nc.WIDTH)
    boxes, score, label = _rows(pred, C, nc.expected_anchors(pred, C))
    assert torch.equal(det["boxes"], boxes) and torch.equal(det["scores"], score) and torch.equal(det["labels"], label)


def test_ties_cases_have_few_distinct_scores():
    pred = nc.make("ties", 1024, 1, nc.ties_seed(1024))
    _, score, _ = _rows(pred, 1, nc.expected_anchors(pred, 1))
    assert len(torch.unique(score)) <= 64 < len(score)


def test_derived_cases_have_their_margin():
    """The dagr_nms_batched inputs (other candidates: a valid mask instead of the confidence mask), the scattered case
    (padding rows are no candidates) and the filter_boxes case (its own offset)."""
    for A in nc.SIZES:
        C = nc.classes_for(A)
        args = nc.nms_inputs(nc.make("crowded", A, C, nc.crowded_seed(A)), C, seed=A)
        assert nc.nms_margin(*args) >= nc.MARGIN, A
    pred, _ = nc.batch_of_eight(1024)                      # dagr_nms_batched takes all of an image's boxes
    for b in range(8):
        assert nc.nms_margin(*nc.nms_inputs(pred[b], nc.BATCH_CLASSES, seed=b, p_invalid=0.0, p_nan=0.0)) >= nc.MARGIN, b
    base = nc.make("crowded", nc.SCATTER_FROM, nc.SCATTER_CLASSES, nc.SCATTER_SEED)
    boxes, score, label, _ = nc.rows_of(base, nc.SCATTER_CLASSES)
    assert nc.nms_margin(boxes, score, label, torch.ones(len(score))) >= nc.MARGIN
    for A in nc.SCATTER_TO:
        padded, pos = nc.scatter(base, A, seed=A)
        assert torch.equal(nc.expected_anchors(padded, nc.SCATTER_CLASSES), pos[nc.expected_anchors(base, nc.SCATTER_CLASSES)])
    x, y, w, h, labels, scores, offset = nc.viz_case()
    boxes = torch.from_numpy(nc.np.stack([x, y, x + w, y + h], -1))
    assert nc.min_iou_margin(nc.offset_boxes(boxes, torch.from_numpy(labels), offset).numpy(), nc.VIZ_IOU) >= nc.MARGIN
    mask = nc.viz_expected()
    assert 4 * int(mask.sum()) >= 128 and 4 * int((~mask).sum()) >= 1024


def test_min_iou_margin_sees_a_pair_at_the_threshold():
    boxes = torch.tensor([[0.0, 0.0, 4.0, 4.0], [0.0, 0.0, 4.0, 2.0], [100.0, 100.0, 110.0, 110.0]])
    assert nc.min_iou_margin(boxes.numpy(), 0.5) == 0.0
    assert nc.min_iou_margin(boxes.numpy(), 0.25) == 0.25
