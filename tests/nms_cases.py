"""Deterministic detection-tail cases for tests/test_nms_cases_cpu.py, tests/test_postprocess_paths_gpu.py and
tests/test_heads_finish_gpu.py (plain module, no test in it).

Every generator returns decoded head rows ``pred[A, 5 + C]`` = (cx, cy, w, h, obj, cls...) as a float32 CPU tensor, the
input of ``postprocess_network_output``; ``nms_inputs`` turns such rows into the boxes / scores / classes that
``dagr_nms_batched`` takes.  The expected values come from ``oracle.postprocess`` (the written-out torchvision greedy
NMS) and, for the staircase, from a closed form.

The random cases are conditioned on themselves, never on the kernel under test: ``min_iou_margin`` recomputes every
candidate pair's IoU in float64 from the float32 class-offset boxes, and a case is only used when no pair lies within
``MARGIN`` of the threshold.  The fp32 IoU expression ``inter / (area_i + area_j - inter)`` is about eight roundings of
2^-24 and the subtraction in the union amplifies them at most three times: <= 1e-6 absolute on a quantity <= 1, so with
2e-6 of room the fp32 decision is the real-number decision, whatever the evaluation order."""
import numpy as np
import torch

WIDTH, HEIGHT = 640, 480
CLASS_OFFSET = float(max(WIDTH, HEIGHT) + 1)        # 641: postprocess_network_output's idxs * (max_dim + 1)
CONF, IOU = 0.05, 0.5
MARGIN = 2e-6

SIZES = (1, 2, 63, 64, 65, 128, 129, 175, 192, 193, 255, 256, 257, 300, 511, 512, 513, 700, 1000, 1023, 1024)
_CLASSES = (1, 2, 3, 8)
# below this many boxes "a quarter suppressed, an eighth surviving" says nothing (one box cannot be suppressed)
VACUITY_FROM = 63


def classes_for(A):
    """The class count the crowded / ties case of size A uses: 1, 2, 3, 8 in turn over SIZES."""
    return _CLASSES[SIZES.index(A) % len(_CLASSES)]


def crowded(A, C, seed, ties=False):
    """Box centres around up to a dozen cluster centres on a 640 x 480 image (fewer clusters for few boxes, so that a
    cluster still holds several boxes of one class), sizes 30 - 90 px, random objectness and class scores.  ``ties``:
    objectness and class scores are multiples of 1/8, so that many candidates share a score and the tie rule (ascending
    anchor index) decides the order and, through it, who suppresses whom."""
    g = torch.Generator().manual_seed(seed)
    n_clusters = max(1, min(12, A // (16 * C)))
    centres = torch.rand((n_clusters, 2), generator=g) * torch.tensor([WIDTH - 160.0, HEIGHT - 160.0]) + 80.0
    which = torch.randint(0, n_clusters, (A,), generator=g)
    pred = torch.zeros((A, 5 + C), dtype=torch.float32)
    pred[:, :2] = centres[which] + torch.randn((A, 2), generator=g) * 12.0
    pred[:, 2:4] = torch.rand((A, 2), generator=g) * 60.0 + 30.0
    pred[:, 4] = torch.rand((A,), generator=g)
    pred[:, 5:] = torch.rand((A, C), generator=g)
    if ties:
        pred[:, 4:] = torch.ceil(pred[:, 4:] * 8.0) / 8.0
    return pred


def staircase(A, C=1, cls=0, perm_seed=None):
    """A boxes of 10 x 10 at x = 3k, all of class ``cls``, strictly descending scores 1 - k/2048 (exact in fp32).
    IoU(k, k+1) = 7/13 > 0.5 and IoU(k, k+2) = 4/16 < 0.5: exactly the even k survive.  An implementation that lets a
    suppressed box suppress keeps only box 0; one that loses a bit at a mask-word boundary keeps an odd box.
    ``perm_seed``: the same boxes under a random permutation of the anchor order (returns ``(pred, perm)`` with
    ``pred[i]`` = box ``perm[i]``), so that the sort does the work."""
    k = torch.arange(A, dtype=torch.float32)
    pred = torch.zeros((A, 5 + C), dtype=torch.float32)
    pred[:, 0] = 3.0 * k + 5.0
    pred[:, 1] = 5.0
    pred[:, 2:4] = 10.0
    pred[:, 4] = 1.0 - k / 2048.0
    pred[:, 5 + cls] = 1.0
    if perm_seed is None:
        return pred
    perm = torch.randperm(A, generator=torch.Generator().manual_seed(perm_seed))
    return pred[perm], perm


def staircase_survivors(A, perm=None):
    """Closed form: the anchors that survive, in the order of the output rows (descending score = ascending k)."""
    even = torch.arange(0, A, 2)
    if perm is None:
        return even
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(len(perm))
    return inv[even]


def all_survive(A, C, seed):
    """A pairwise disjoint boxes (10 x 8 in the 20 x 15 cells of a 32 x 32 grid), random scores and classes, every
    one above the confidence threshold: n_keep = A."""
    g = torch.Generator().manual_seed(seed)
    k = torch.arange(A)
    pred = torch.zeros((A, 5 + C), dtype=torch.float32)
    pred[:, 0] = (k % 32).float() * 20.0 + 10.0
    pred[:, 1] = (k // 32).float() * 15.0 + 7.5
    pred[:, 2] = 10.0
    pred[:, 3] = 8.0
    pred[:, 4] = torch.rand((A,), generator=g) * 0.5 + 0.5
    pred[:, 5:] = torch.rand((A, C), generator=g) * 0.5 + 0.5
    return pred


def one_survives(A, C, seed):
    """A identical boxes of class 0 with distinct scores (a permutation of (k + 1) / 1025): only the best one stays."""
    perm = torch.randperm(A, generator=torch.Generator().manual_seed(seed))
    pred = torch.zeros((A, 5 + C), dtype=torch.float32)
    pred[:, 0] = 100.0
    pred[:, 1] = 120.0
    pred[:, 2] = 50.0
    pred[:, 3] = 40.0
    pred[:, 4] = (perm.float() + 1.0) / 1025.0 * 0.5 + 0.5
    pred[:, 5] = 1.0
    return pred


def none_pass(A, C, seed):
    """A crowded case with every objectness scaled below the confidence threshold: n_keep = 0."""
    pred = crowded(A, C, seed)
    pred[:, 4] *= 0.04
    return pred


def exact_threshold(C, cls):
    """Boxes (0, 0, 4, 4) and (0, 0, 4, 2) of class ``cls``: IoU = 8 / 16 is exactly 0.5 in fp32, also after the class
    offset (641 * cls and the sums are exact floats), so at threshold 0.5 both are kept (``>``, not ``>=``)."""
    pred = torch.zeros((2, 5 + C), dtype=torch.float32)
    pred[0, :4] = torch.tensor([2.0, 2.0, 4.0, 4.0])
    pred[1, :4] = torch.tensor([2.0, 1.0, 4.0, 2.0])
    pred[:, 4] = torch.tensor([0.9, 0.8])
    pred[:, 5 + cls] = 1.0
    return pred


def degenerate(C=2):
    """Zero-area and negative-width boxes (IoU 0/0 = NaN compares false on both sides: nothing is suppressed by or
    through them), next to ordinary boxes that do suppress each other, and two boxes of different classes at the same
    place (the class offset must separate them)."""
    rows = [
        # cx, cy, w, h, obj, class
        (50.0, 50.0, 0.0, 20.0, 0.95, 0),     # zero width
        (50.0, 50.0, 0.0, 20.0, 0.90, 0),     # the same again: 0/0
        (50.0, 50.0, 0.0, 0.0, 0.85, 0),      # a point
        (50.0, 50.0, 0.0, 0.0, 0.84, 0),
        (50.0, 50.0, -8.0, 20.0, 0.80, 0),    # negative width: x2 < x1
        (50.0, 50.0, -8.0, 20.0, 0.79, 0),
        (50.0, 50.0, 30.0, 30.0, 0.75, 0),    # an ordinary box around them all
        (51.0, 50.0, 30.0, 30.0, 0.70, 0),    # suppressed by the previous one
        (200.0, 100.0, 40.0, 40.0, 0.65, 0),  # two classes at the same place: both stay
        (200.0, 100.0, 40.0, 40.0, 0.60, 1),
        (200.0, 100.0, 40.0, 40.0, 0.55, 1),  # ... and the third is suppressed by the second
    ]
    pred = torch.zeros((len(rows), 5 + C), dtype=torch.float32)
    for i, (cx, cy, w, h, obj, c) in enumerate(rows):
        pred[i, :5] = torch.tensor([cx, cy, w, h, obj])
        pred[i, 5 + c] = 1.0
    return pred


def scatter(pred, A, seed, low=True):
    """``pred``'s rows in their order at random positions among A rows; the other rows are boxes in the same place with
    an objectness below the confidence threshold (``low``) -- or, for dagr_nms_batched, rows to be marked invalid.
    Returns ``(padded, positions)``."""
    g = torch.Generator().manual_seed(seed)
    n = pred.shape[0]
    pos = torch.sort(torch.randperm(A, generator=g)[:n]).values
    out = crowded(A, pred.shape[1] - 5, seed + 1)
    out[:, 4] *= 0.04 if low else 1.0
    out[pos] = pred
    return out, pos


# --------------------------------------------------------------------------------------------------------------------
# the reference's arithmetic on such rows (fp32 torch CPU ops in model/utils.py's order) and what follows from it

def rows_of(pred, C):
    """Per anchor: xyxy box, score, label and the confidence mask, in postprocess_network_output's op order
    (``cx - w/2``, ``w + x1``, ``obj * cls``, ``score * cls >= conf``)."""
    p = pred.clone()
    p[:, :2] -= p[:, 2:4] / 2
    p[:, 2:4] += p[:, :2]
    cc, label = torch.max(p[:, 5:5 + C], 1)
    score = p[:, 4] * cc
    return p[:, :4].contiguous(), score, label, score * cc


def offset_boxes(boxes, labels, class_offset=CLASS_OFFSET):
    """float32 class-offset boxes: ``boxes + label * offset`` (batched_nms_coordinate_trick)."""
    return boxes + (labels.float() * float(class_offset))[:, None]


def expected_anchors(pred, C, conf=CONF, iou=IOU, class_offset=CLASS_OFFSET):
    """The anchors whose rows the post-processing returns, in output order (oracle.postprocess.nms on the candidates'
    class-offset boxes; ``argsort(stable)`` = ties by ascending anchor)."""
    from oracle.postprocess import nms
    boxes, score, label, masked = rows_of(pred, C)
    cand = torch.nonzero(masked >= conf).flatten()
    if len(cand) == 0:
        return cand
    keep = nms(offset_boxes(boxes[cand], label[cand], class_offset), score[cand], iou)
    return cand[keep]


def counts(pred, C, conf=CONF, iou=IOU):
    """(candidates, survivors) of a case."""
    _, _, _, masked = rows_of(pred, C)
    return int((masked >= conf).sum()), int(len(expected_anchors(pred, C, conf, iou)))


def min_iou_margin(boxes_offset, iou=IOU):
    """Smallest ``|IoU - iou|`` over all pairs of the given float32 (class-offset) boxes, IoU recomputed in float64.
    Pairs with a zero union (0/0) are skipped: they have no IoU to be near the threshold.  ``inf`` below two boxes."""
    b = np.asarray(boxes_offset, dtype=np.float32).astype(np.float64)
    n = len(b)
    if n < 2:
        return float("inf")
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    best = float("inf")
    for lo in range(0, n, 256):
        c = b[lo:lo + 256]
        w = np.clip(np.minimum(c[:, None, 2], b[None, :, 2]) - np.maximum(c[:, None, 0], b[None, :, 0]), 0, None)
        h = np.clip(np.minimum(c[:, None, 3], b[None, :, 3]) - np.maximum(c[:, None, 1], b[None, :, 1]), 0, None)
        inter = w * h
        union = area[lo:lo + 256, None] + area[None, :] - inter
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.abs(inter / union - iou)
        d[np.arange(len(c)), np.arange(lo, lo + len(c))] = np.inf       # a box with itself
        d[union == 0] = np.inf
        best = min(best, float(np.nanmin(d)))
    return best


def pred_margin(pred, C, conf=CONF, iou=IOU):
    """``min_iou_margin`` over the candidates of a ``pred`` case."""
    boxes, _, label, masked = rows_of(pred, C)
    cand = masked >= conf
    return min_iou_margin(offset_boxes(boxes[cand], label[cand]).numpy(), iou)


def nms_inputs(pred, C, seed, p_invalid=0.15, p_nan=0.05):
    """``dagr_nms_batched``'s inputs from a ``pred`` case: xyxy boxes, scores, classes (int32), and a valid mask with
    about ``p_invalid`` of the boxes switched off; about ``p_nan`` of the scores are NaN (never kept, sorted after
    every valid box)."""
    g = torch.Generator().manual_seed(seed)
    boxes, score, label, _ = rows_of(pred, C)
    A = pred.shape[0]
    valid = (torch.rand((A,), generator=g) >= p_invalid).to(torch.uint8)
    score = score.clone()
    score[torch.rand((A,), generator=g) < p_nan] = float("nan")
    return boxes, score, label.to(torch.int32), valid


def nms_expected(boxes, score, cls, valid, iou=IOU, class_offset=CLASS_OFFSET):
    """``(order_head, rest, kept)``: the ranked boxes (valid, score not NaN) by descending score with ties by ascending
    index -- the head of ``order_out`` --, the set of the others, and the anchors that oracle.postprocess.nms keeps."""
    from oracle.postprocess import nms
    ranked = torch.nonzero((valid != 0) & ~torch.isnan(score)).flatten()
    rest = torch.nonzero(~((valid != 0) & ~torch.isnan(score))).flatten()
    head = ranked[torch.argsort(score[ranked], descending=True, stable=True)]
    kept = ranked[nms(offset_boxes(boxes[ranked], cls[ranked], class_offset), score[ranked], iou)] if len(ranked) \
        else ranked
    return head, rest, kept


def nms_margin(boxes, score, cls, valid, iou=IOU, class_offset=CLASS_OFFSET):
    ranked = (valid != 0) & ~torch.isnan(score)
    return min_iou_margin(offset_boxes(boxes[ranked], cls[ranked], class_offset).numpy(), iou)


def bits(t):
    return t.contiguous().view(torch.int32)


def check_rows(det, n, pred, C, what, conf=CONF, iou=IOU, anchors=None, class_offset=CLASS_OFFSET):
    """One image's device rows ``det[:n]`` (CPU tensors) against the oracle on ``pred[A, 5 + C]``: n_keep, the anchor
    every row came from (recovered from the bit pattern of the row) and the labels are EQUAL, score and box are
    BIT-EQUAL.  ``anchors``: a closed form for the surviving anchors, where there is one."""
    from oracle.postprocess import postprocess_network_output
    want_anchors = expected_anchors(pred, C, conf, iou, class_offset) if anchors is None else anchors
    side = int(class_offset) - 1
    want, = postprocess_network_output(pred[None], C, conf, iou, height=side, width=side)
    assert len(want["boxes"]) == len(want_anchors), what
    boxes, score, label, _ = rows_of(pred, C)
    got = det[:n]
    table = {}
    for a in range(pred.shape[0]):
        key = tuple(bits(torch.cat([boxes[a], score[a:a + 1], label[a:a + 1].float()])).tolist())
        table.setdefault(key, []).append(a)
    found = [table.get(tuple(bits(r).tolist())) for r in got]
    flat = [f[0] if f is not None and len(f) == 1 else f for f in found]       # None: a row that is no anchor's
    seen = set(a for a in flat if isinstance(a, int))
    assert n == len(want_anchors), (f"{what}: n_keep {n}, oracle {len(want_anchors)}; missing anchors "
                                    f"{sorted(set(want_anchors.tolist()) - seen)[:16]}, spurious "
                                    f"{sorted(seen - set(want_anchors.tolist()))[:16]}")
    assert flat == want_anchors.tolist(), (f"{what}: rows come from anchors {flat[:24]}..., "
                                           f"oracle {want_anchors.tolist()[:24]}...")
    assert torch.equal(got[:, 5].long(), want["labels"]), what
    assert torch.equal(bits(got[:, 4]), bits(want["scores"])), f"{what}: scores differ in bits"
    assert torch.equal(bits(got[:, :4]), bits(want["boxes"])), f"{what}: boxes differ in bits"


# --------------------------------------------------------------------------------------------------------------------
# the random cases the GPU tests use: (kind, A, C, seed).  tests/test_nms_cases_cpu.py asserts the margin and the
# vacuity cap on every one of them.

# Seeds are base + A, moved up to the first seed whose case has its margin and clears the cap.  That search ran
# with the oracle alone (no kernel was involved).
_SEED_BUMP = {("crowded", 64): 1, ("crowded", 65): 2, ("crowded", 257): 1, ("ties", 1023): 1}


# The cases of random_cases() as the oracle sees them (conf 0.05, IoU 0.5; tests/test_nms_cases_cpu.py prints the same):
#   kind         A  C  seed  cand  surv  min |IoU - thr|
#   crowded      1  1   101     1     1  inf
#   ties         1  1  7001     1     1  inf
#   crowded      2  2   102     1     1  inf
#   ties         2  2  7002     2     2  5.00e-01
#   crowded     63  3   163    52    26  7.72e-04
#   ties        63  3  7063    61    24  1.00e-04
#   crowded     64  8   165    60    39  1.86e-03
#   ties        64  8  7064    64    40  1.61e-03
#   crowded     65  1   167    43    26  1.90e-03
#   ties        65  1  7065    44    27  1.75e-03
#   crowded    128  2   228    92    58  2.31e-04
#   ties       128  2  7128   110    52  8.72e-05
#   crowded    129  3   229   113    58  1.17e-03
#   ties       129  3  7129   124    61  1.02e-04
#   crowded    175  8   275   160    76  1.51e-04
#   ties       175  8  7175   175    78  1.67e-05
#   crowded    192  1   292   112    62  4.76e-04
#   ties       192  1  7192   136    70  1.71e-05
#   crowded    193  2   293   157    84  4.35e-04
#   ties       193  2  7193   164    86  1.08e-03
#   crowded    255  3   355   220   110  4.76e-05
#   ties       255  3  7255   241   113  1.20e-04
#   crowded    256  8   356   235   128  4.01e-04
#   ties       256  8  7256   256   115  2.02e-04
#   crowded    257  1   358   152    76  2.91e-04
#   ties       257  1  7257   184    88  9.23e-05
#   crowded    300  2   400   243   123  1.22e-04
#   ties       300  2  7300   273   126  1.39e-04
#   crowded    511  3   611   460   224  2.75e-04
#   ties       511  3  7511   488   225  8.50e-05
#   crowded    512  8   612   473   240  1.59e-05
#   ties       512  8  7512   510   251  1.82e-05
#   crowded    513  1   613   318   119  3.65e-05
#   ties       513  1  7513   379   129  1.87e-04
#   crowded    700  2   800   564   214  2.53e-05
#   ties       700  2  7700   633   271  9.47e-05
#   crowded   1000  3  1100   876   379  2.02e-05
#   ties      1000  3  8000   958   367  2.79e-06
#   crowded   1023  8  1123   954   456  1.32e-05
#   ties      1023  8  8024  1020   451  2.21e-05
#   crowded   1024  1  1124   630   168  3.49e-05
#   ties      1024  1  8024   720   191  2.55e-05
#   crowded    256  3   287   220   111  1.50e-04
#   ties       256  3   297   244   119  7.68e-05
#   crowded    256  3   307   220   117  1.18e-04
#   crowded   1024  3  1055   897   348  6.00e-06
#   ties      1024  3  1056   970   377  2.48e-05
#   crowded   1024  3  1075   912   389  5.07e-05
#   crowded    175  3   175   155    74  2.11e-04


def crowded_seed(A):
    return 100 + A + _SEED_BUMP.get(("crowded", A), 0)


def ties_seed(A):
    return 7000 + A + _SEED_BUMP.get(("ties", A), 0)


def random_cases():
    """Every (kind, A, C, seed) with random geometry that a GPU test compares with the oracle."""
    out = []
    for A in SIZES:
        out.append(("crowded", A, classes_for(A), crowded_seed(A)))
        out.append(("ties", A, classes_for(A), ties_seed(A)))
    for A in BATCH_SIZES:
        for kind, seed in zip(("crowded", "ties", "crowded"), BATCH_SEEDS[A]):
            out.append((kind, A, BATCH_CLASSES, seed))
    out.append(("crowded", SCATTER_FROM, SCATTER_CLASSES, SCATTER_SEED))
    return out


def make(kind, A, C, seed):
    return crowded(A, C, seed, ties=(kind == "ties"))


BATCH_SIZES = (256, 1024)
BATCH_SEEDS = {256: (287, 297, 307), 1024: (1055, 1056, 1075)}      # crowded, ties, crowded (chosen as _SEED_BUMP)
BATCH_CLASSES = 3
SCATTER_FROM, SCATTER_CLASSES, SCATTER_SEED = 175, 3, 175
SCATTER_TO = (300, 1024)
VIZ_SEED, VIZ_CONF, VIZ_IOU = 4243, 0.3, 0.45


def viz_case():
    """A crowded 1024-box, two-class case in ``bbox_viz.filter_boxes``' terms: ``(x, y, w, h, labels, scores, offset)``
    as numpy arrays, ``offset`` = its class offset (largest coordinate + 1 in float32, torchvision batched_nms)."""
    boxes, score, label, _ = rows_of(crowded(1024, 2, VIZ_SEED), 2)
    x, y = boxes[:, 0].numpy(), boxes[:, 1].numpy()
    w, h = (boxes[:, 2] - boxes[:, 0]).numpy(), (boxes[:, 3] - boxes[:, 1]).numpy()
    offset = float(np.float32(max((x + w).max(), (y + h).max(), x.max(), y.max())) + np.float32(1))
    return x, y, w, h, label.numpy(), score.numpy(), offset


def viz_expected():
    """``filter_boxes``' mask by the oracle: ``scores > conf`` and kept by the class-wise NMS over ALL the boxes."""
    from oracle.postprocess import nms
    x, y, w, h, labels, scores, offset = viz_case()
    boxes = torch.from_numpy(np.stack([x, y, x + w, y + h], -1))
    keep = nms(offset_boxes(boxes, torch.from_numpy(labels), offset), torch.from_numpy(scores), VIZ_IOU)
    mask = torch.zeros(len(x), dtype=torch.bool)
    mask[keep] = True
    return (mask & (torch.from_numpy(scores) > VIZ_CONF)).numpy()


def batch_of_eight(A):
    """B = 8 images of A anchors and BATCH_CLASSES classes, a different case each, among them an empty and a full one.
    Returns ``(pred[8, A, 5 + C], names)``."""
    C = BATCH_CLASSES
    sh, _ = staircase(A, C, cls=2, perm_seed=A + 1)
    s0, s1, s2 = BATCH_SEEDS[A]
    imgs = [("crowded", crowded(A, C, s0)), ("none", none_pass(A, C, 5)), ("ties", crowded(A, C, s1, ties=True)),
            ("all survive", all_survive(A, C, 6)), ("staircase", staircase(A, C, cls=1)), ("staircase shuffled", sh),
            ("one survives", one_survives(A, C, 8)), ("crowded", crowded(A, C, s2))]
    return torch.stack([p for _, p in imgs]), [n for n, _ in imgs]
