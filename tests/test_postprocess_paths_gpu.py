"""csrc/nms.hip on both of its paths -- rank sort + ballot masks + one-wave chain (A <= 256) and bitonic network +
one barrier per candidate (256 < A <= 1024) -- against oracle.postprocess, at every size around the 64-bit mask words and
the switch, on the cases of tests/nms_cases.py (tests/test_nms_cases_cpu.py vouches for the fixtures).

Bars: n_keep, labels and the anchor every output row came from are EQUAL to the oracle's; the score and the four box
coordinates of every surviving row are BIT-EQUAL to it (both sides do the same IEEE fp32 operations in the same order:
``cx - w/2``, ``w + x1``, ``obj * cls``; the library is built with -ffp-contract=off).  Rows at and beyond n_keep[b] are
unspecified by the ABI and not looked at."""
import numpy as np
import pytest
import torch

from dagr_amd import _lib
from tests import nms_cases as nc

pytestmark = pytest.mark.gpu


def _run(pred, C, conf=nc.CONF, iou=nc.IOU):
    """dagr_postprocess through the product's wrapper: (det[B, A, 6], n_keep[B]) on the CPU."""
    from dagr_amd.model.utils import postprocess_device
    det, n_keep = postprocess_device(pred.cuda(), C, conf, iou, height=nc.HEIGHT, width=nc.WIDTH)
    torch.cuda.synchronize()
    return det.cpu(), n_keep.cpu()


def _check(pred, C, what, **kw):
    det, n_keep = _run(pred, C, kw.get("conf", nc.CONF), kw.get("iou", nc.IOU))
    for b in range(pred.shape[0]):
        nc.check_rows(det[b], int(n_keep[b]), pred[b], C, f"{what}, image {b}", **kw)
    return det, n_keep


@pytest.mark.parametrize("A", nc.SIZES)
@pytest.mark.parametrize("kind", ["crowded", "ties"])
def test_random_cases_match_the_oracle_at_every_size(kind, A):
    C = nc.classes_for(A)
    seed = nc.crowded_seed(A) if kind == "crowded" else nc.ties_seed(A)
    _check(nc.make(kind, A, C, seed)[None], C, f"{kind} A={A} C={C} seed={seed}")


@pytest.mark.parametrize("A", [1, 2, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 512, 1023, 1024])
def test_staircase_keeps_exactly_the_even_boxes(A):
    """Closed form, not only the oracle: a suppressed box must not suppress (only box 0 would stay), and no bit may be
    lost at a mask-word boundary (an odd box would stay)."""
    pred = nc.staircase(A)
    det, n_keep = _check(pred[None], 1, f"staircase A={A}", anchors=nc.staircase_survivors(A))
    assert int(n_keep[0]) == (A + 1) // 2
    assert det[0, :int(n_keep[0]), 0].tolist() == [float(6 * k) for k in range((A + 1) // 2)]     # x1 = 3k, k even


@pytest.mark.parametrize("A", [65, 129, 256, 257, 1024])
def test_shuffled_staircase_keeps_exactly_the_even_boxes(A):
    pred, perm = nc.staircase(A, 3, cls=2, perm_seed=A)
    det, n_keep = _check(pred[None], 3, f"shuffled staircase A={A}", anchors=nc.staircase_survivors(A, perm))
    assert det[0, :int(n_keep[0]), 0].tolist() == [float(6 * k) for k in range((A + 1) // 2)]


@pytest.mark.parametrize("A", [1, 64, 255, 256, 257, 1000, 1024])
def test_all_one_and_none_survive(A):
    """n_keep = A (at 1024 every wave that owns sorted positions contributes to the front-compaction), 1 and 0."""
    for C in (1, 3):
        det, n_keep = _check(torch.stack([nc.all_survive(A, C, 6), nc.one_survives(A, C, 8), nc.none_pass(A, C, 5)]), C,
                             f"all / one / none A={A} C={C}")
        assert n_keep.tolist() == [A, 1, 0]


@pytest.mark.parametrize("A", nc.BATCH_SIZES)
def test_eight_different_images_in_one_launch(A):
    pred, names = nc.batch_of_eight(A)
    det, n_keep = _check(pred, nc.BATCH_CLASSES, f"batch of eight A={A} ({', '.join(names)})")
    assert int(n_keep[1]) == 0 and int(n_keep[3]) == A and int(n_keep[6]) == 1
    assert int(n_keep[4]) == (A + 1) // 2 and int(n_keep[5]) == (A + 1) // 2


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_iou_exactly_at_the_threshold_is_kept(cls):
    """``>``, not ``>=``: IoU((0,0,4,4), (0,0,4,2)) is exactly 0.5 in fp32, under every class offset."""
    pred = nc.exact_threshold(3, cls)
    _, n_keep = _check(pred[None], 3, f"exact threshold, class {cls}")
    assert int(n_keep[0]) == 2
    _, n_keep = _check(pred[None], 3, f"just below, class {cls}", iou=0.4999)
    assert int(n_keep[0]) == 1
    # the same pair among 300 boxes (the other implementation): the first two of a padded case
    padded = torch.cat([pred, nc.none_pass(298, 3, 5)])
    _, n_keep = _check(padded[None], 3, f"exact threshold among 300, class {cls}")
    assert int(n_keep[0]) == 2


@pytest.mark.parametrize("A", [11, 300])
def test_degenerate_boxes(A):
    pred = nc.degenerate()
    if A > len(pred):
        pred = torch.cat([pred, nc.none_pass(A - len(pred), 2, 5)])
    _, n_keep = _check(pred[None], 2, f"degenerate A={A}")
    assert int(n_keep[0]) == 9


@pytest.mark.parametrize("A", nc.SCATTER_TO)
def test_both_implementations_on_one_problem(A):
    """A 175-anchor crowded case (rank sort + masks) and the same anchors scattered among boxes below the confidence
    threshold up to A = 300 / 1024 (bitonic network + barrier loop): the same rows, bit for bit, and the oracle's."""
    C = nc.SCATTER_CLASSES
    base = nc.make("crowded", nc.SCATTER_FROM, C, nc.SCATTER_SEED)
    padded, pos = nc.scatter(base, A, seed=A)
    det_s, n_s = _check(base[None], C, "unpadded")
    det_l, n_l = _check(padded[None], C, f"scattered to A={A}", anchors=pos[nc.expected_anchors(base, C)])
    n = int(n_s[0])
    assert int(n_l[0]) == n and n >= nc.SCATTER_FROM // 8
    assert torch.equal(nc.bits(det_l[0, :n]), nc.bits(det_s[0, :n]))


# ---------------------------------------------------------------------------------------------------------------------
# dagr_nms_batched through ctypes

def _nms_batched(boxes, score, cls, valid, iou=nc.IOU, class_offset=nc.CLASS_OFFSET):
    """boxes[B, A, 4], score / cls / valid[B, A] (CPU) -> order_out, keep_out[B, A], n_keep[B] (CPU)."""
    B, A = score.shape
    dev = torch.device("cuda")
    d = [t.contiguous().to(dev) for t in (boxes.float(), score.float(), cls.to(torch.int32), valid.to(torch.uint8))]
    order = torch.full((B, A), -1, dtype=torch.int32, device=dev)
    keep = torch.full((B, A), -1, dtype=torch.int32, device=dev)
    n_keep = torch.full((B,), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().dagr_nms_batched(*(_lib.ptr(t) for t in d), B, A, float(iou), float(class_offset), _lib.ptr(order),
                                           _lib.ptr(keep), _lib.ptr(n_keep), _lib.cur_stream(dev)), "nms_batched")
    torch.cuda.synchronize()
    return order.cpu().long(), keep.cpu(), n_keep.cpu()


def _check_nms(boxes, score, cls, valid, what, **kw):
    order, keep, n_keep = _nms_batched(boxes[None], score[None], cls[None], valid[None], **kw)
    order, keep = order[0], keep[0]
    A = len(score)
    head, rest, kept = nc.nms_expected(boxes, score, cls, valid, **kw)
    assert sorted(order.tolist()) == list(range(A)), f"{what}: order_out is no permutation"
    assert order[:len(head)].tolist() == head.tolist(), f"{what}: ranked part of order_out"
    assert sorted(order[len(head):].tolist()) == rest.tolist(), f"{what}: invalid / NaN boxes are not last"
    assert set(keep.tolist()) <= {0, 1}
    got = order[keep != 0]
    assert got.tolist() == kept.tolist(), (f"{what}: kept {len(got)}, oracle {len(kept)}; missing "
                                           f"{sorted(set(kept.tolist()) - set(got.tolist()))[:16]}, spurious "
                                           f"{sorted(set(got.tolist()) - set(kept.tolist()))[:16]}")
    assert int(n_keep[0]) == len(kept), what
    return got


@pytest.mark.parametrize("A", nc.SIZES)
def test_nms_batched_order_and_keep(A):
    """The same geometry with a valid mask and NaN scores: order_out is the full permutation (valid boxes by descending
    score, ties by ascending index, then everything else), keep_out / n_keep are oracle.postprocess.nms's."""
    C = nc.classes_for(A)
    _check_nms(*nc.nms_inputs(nc.make("crowded", A, C, nc.crowded_seed(A)), C, seed=A), f"crowded A={A} C={C}")
    # ties (no margin needed beyond the crowded one's: the same boxes, scores rounded to multiples of 1/8)
    boxes, score, cls, valid = nc.nms_inputs(nc.make("crowded", A, C, nc.crowded_seed(A)), C, seed=A)
    _check_nms(boxes, torch.ceil(score * 8.0) / 8.0, cls, valid, f"ties A={A} C={C}")


@pytest.mark.parametrize("A", [64, 65, 129, 256, 257, 1024])
def test_nms_batched_staircase_and_extremes(A):
    pred, perm = nc.staircase(A, 1, perm_seed=A)
    boxes, score, label, _ = nc.rows_of(pred, 1)
    ones = torch.ones(A, dtype=torch.uint8)
    got = _check_nms(boxes, score, label.int(), ones, f"shuffled staircase A={A}")
    assert got.tolist() == nc.staircase_survivors(A, perm).tolist()
    # every second box invalid: the remaining ones (IoU 4/16) all stay
    valid = (perm % 2 == 0).to(torch.uint8)
    got = _check_nms(boxes, score, label.int(), valid, f"staircase with the odd boxes invalid A={A}")
    assert len(got) == (A + 1) // 2
    # nothing valid; everything NaN
    _check_nms(boxes, score, label.int(), torch.zeros(A, dtype=torch.uint8), f"nothing valid A={A}")
    _check_nms(boxes, torch.full((A,), float("nan")), label.int(), ones, f"all scores NaN A={A}")
    boxes, score, label, _ = nc.rows_of(nc.all_survive(A, 3, 6), 3)
    assert len(_check_nms(boxes, score, label.int(), ones, f"all survive A={A}")) == A


def test_nms_batched_eight_images_in_one_launch():
    A, C = 1024, nc.BATCH_CLASSES
    pred, names = nc.batch_of_eight(A)
    ins = [nc.nms_inputs(pred[b], C, seed=b, p_invalid=0.0, p_nan=0.0) for b in range(8)]
    order, keep, n_keep = _nms_batched(*(torch.stack([i[k] for i in ins]) for k in range(4)))
    for b in range(8):
        head, rest, kept = nc.nms_expected(*ins[b])
        assert order[b].tolist() == head.tolist(), names[b]
        assert order[b][keep[b] != 0].tolist() == kept.tolist(), names[b]
        assert int(n_keep[b]) == len(kept), names[b]


@pytest.mark.parametrize("A", nc.SCATTER_TO)
def test_nms_batched_both_implementations_on_one_problem(A):
    C = nc.SCATTER_CLASSES
    base = nc.make("crowded", nc.SCATTER_FROM, C, nc.SCATTER_SEED)
    boxes, score, label, _ = nc.rows_of(base, C)
    small = _check_nms(boxes, score, label.int(), torch.ones(len(score), dtype=torch.uint8), "unpadded")
    padded, pos = nc.scatter(base, A, seed=A, low=False)
    boxes, score, label, _ = nc.rows_of(padded, C)
    valid = torch.zeros(A, dtype=torch.uint8)
    valid[pos] = 1
    large = _check_nms(boxes, score, label.int(), valid, f"scattered to A={A}")
    assert large.tolist() == pos[small].tolist()


def test_filter_boxes_on_a_crowded_1024_box_case():
    """The product's other caller (dagr.visualization.bbox_viz): its mask is the oracle's."""
    from dagr_amd.visualization.bbox_viz import filter_boxes
    x, y, w, h, labels, scores, _ = nc.viz_case()
    got = filter_boxes(x, y, w, h, labels, scores, nc.VIZ_CONF, nc.VIZ_IOU)
    want = nc.viz_expected()
    assert got.dtype == np.bool_ and got.shape == want.shape
    assert np.array_equal(got, want), (f"{int(got.sum())} boxes, oracle {int(want.sum())}; differ at "
                                       f"{np.nonzero(got != want)[0][:16].tolist()}")
