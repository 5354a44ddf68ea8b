"""Mirror of ``format_data`` (``src/dagr/utils/buffers.py:33-44``): the input contract of the hot path.
On device tensors the normalisation runs through ``dagr_format_events`` (libdagr_hip) when the batch
carries the dataset's raw dtypes (pos int16[N,2], t int32[N], x int8[N,1]); any other dtype takes the
same arithmetic through torch ops (true division in fp32)."""
import ctypes

import torch

from .. import _lib


def format_data(data, normalizer=None):
    geo = getattr(data, "_geometry", None)
    if geo is None:
        # one read-back for the three scalars (they sit on the device once the batch does); kept on the batch for the
        # layers that ask again (EV_TGN)
        w, h, tw = data.width, data.height, data.time_window
        if torch.is_tensor(w) and w.is_cuda:
            geo = tuple(int(v) for v in torch.stack((w.reshape(-1)[0], h.reshape(-1)[0], tw.reshape(-1)[0])).tolist())
        else:
            geo = (int(w[0]), int(h[0]), int(tw[0]))
        data._geometry = geo
    W, H, T = geo
    if hasattr(data, "image"):
        data.image = data.image.float() / 255.0
    pos, t, x = data.pos, data.t, data.x
    if (normalizer is None and pos.is_cuda and pos.dtype == torch.int16 and t.dtype == torch.int32
            and x.dtype == torch.int8 and pos.is_contiguous() and t.is_contiguous() and x.is_contiguous()):
        N = pos.shape[0]
        pos_out = torch.empty((N, 3), dtype=torch.float32, device=pos.device)
        feat = torch.empty((N, 1), dtype=torch.float32, device=pos.device)
        _lib.check(_lib.lib().dagr_format_events(_lib.ptr(pos), _lib.ptr(t), _lib.ptr(x), N, W, H, T,
                                                 _lib.ptr(pos_out), _lib.ptr(feat), _lib.cur_stream(pos.device)),
                   "format_events")
        data.pos, data.x = pos_out, feat
    else:
        if normalizer is None:
            normalizer = torch.tensor([W, H, T], device=pos.device)
        data.pos = torch.cat([pos, t.view((-1, 1))], dim=-1) / normalizer
        data.x = x.float()
    data.t = None
    return data


# ---------------------------------------------------------------------------------------------------------------
# Detection records and the evaluation buffer (src/dagr/utils/buffers.py:46-122).
DETECTION_DTYPE = [("t", "<u8"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("class_id", "u1"),
                   ("class_confidence", "<f4")]


def detections_to_records(det, t):
    """One image's detections ``{boxes[x1,y1,x2,y2], labels[, scores]}`` -> the structured array the reference writes
    (``bbox_t_to_ndarray`` buffers.py:46-66 / ``to_npy`` run_test_interframe.py:21-32).  Ground-truth dicts carry no
    scores: the confidence column is dropped for them, as the reference does."""
    import numpy as np
    boxes = np.asarray(det["boxes"].cpu() if torch.is_tensor(det["boxes"]) else det["boxes"], dtype=np.float32)
    labels = np.asarray(det["labels"].cpu() if torch.is_tensor(det["labels"]) else det["labels"])
    has_scores = "scores" in det
    rec = np.zeros((len(boxes),), dtype=DETECTION_DTYPE if has_scores else DETECTION_DTYPE[:-1])
    rec["t"] = t
    if len(boxes):
        rec["x"], rec["y"] = boxes[:, 0], boxes[:, 1]
        rec["w"], rec["h"] = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
        rec["class_id"] = labels
        if has_scores:
            rec["class_confidence"] = np.asarray(det["scores"].cpu() if torch.is_tensor(det["scores"]) else det["scores"])
    return rec


def bbox_t_to_ndarray(bbox, t):
    """The reference's name for ``detections_to_records`` (buffers.py:46-66)."""
    return detections_to_records(bbox, t)


def compile(detections, sequences, timestamps):        # noqa: A001  (the reference's module-level name, buffers.py:69-80)
    """Per-sequence concatenation of the per-image record arrays."""
    import numpy as np
    out = {}
    for det, seq, t in zip(detections, sequences, timestamps):
        out.setdefault(seq, []).append(detections_to_records(det, t))
    return {k: np.concatenate(v) for k, v in out.items() if len(v) > 0}


class DictBuffer:
    """Running mean of dictionaries with the same keys (buffers.py:124-146; the FLOP script's accumulator)."""

    def __init__(self):
        self.running_mean = None
        self.n = 0

    def update(self, dictionary):
        if self.running_mean is None:
            self.running_mean = {k: 0 for k in dictionary}
        self.running_mean = {k: self.n / (self.n + 1) * self.running_mean[k] + dictionary[k] / (self.n + 1)
                             for k in dictionary}
        self.n += 1

    def save(self, path):
        torch.save(self.running_mean, path)

    def compute(self):
        return self.running_mean


class _DeviceRows:
    """Rows of ``width`` float32 columns appended into one device array that doubles when it is full.  The number of rows
    of every append is known on the host (a tensor's shape), so an append is a device-to-device copy and nothing waits."""

    def __init__(self, width):
        self.width, self.n, self.buf = width, 0, None

    def append(self, rows):
        n = rows.shape[0]
        if self.buf is None or self.n + n > self.buf.shape[0]:
            grown = torch.empty((max(1024, 2 * (self.n + n)), self.width), dtype=torch.float32, device=rows.device)
            if self.n:
                grown[:self.n].copy_(self.buf[:self.n])
            self.buf = grown
        self.buf[self.n:self.n + n].copy_(rows)
        self.n += n
        return self.n - n

    def rows(self, device):
        return self.buf[:self.n] if self.buf is not None else torch.empty((0, self.width), dtype=torch.float32, device=device)


class DetectionBuffer:
    """Collects detections / ground truth of a test run on the host (buffers.py:100-122).  ``compute`` hands them to the
    COCO-protocol evaluation of ``utils/coco_eval.py`` (pycocotools / detectron2 in the reference; restated in numpy here).

    ``on_device=True``: the boxes stay on the GPU until ``compile`` / ``compute`` -- ``update`` and ``update_device``
    append into growing device arrays without a copy to the host and without a synchronisation, ONE copy brings
    everything back, and the greedy matcher of the evaluation runs as ``dagr_coco_match``.  The metrics are the floats the
    host path returns.  ``last_host_fallback_jobs``: after ``compute``, how many (image, class) pairs were beyond the
    kernel's per-job bounds and were matched on the host instead.

    ``accumulate_on_device`` (with ``on_device=True`` only): the accumulation of the evaluation runs on the GPU as well
    (``dagr_coco_accumulate``) and only the precision array comes back -- the same floats again.  None: the process default
    (``utils.testing.accumulate_on_device``, off unless set) when ``on_device``, else off."""

    def __init__(self, height, width, classes, on_device=False, accumulate_on_device=None):
        self.height, self.width, self.classes = height, width, classes
        self.on_device = bool(on_device)
        if accumulate_on_device is None:
            from . import testing
            accumulate_on_device = self.on_device and testing.accumulate_on_device_default()
        if accumulate_on_device and not self.on_device:
            raise ValueError("DetectionBuffer: accumulate_on_device=True needs on_device=True")
        self.accumulate_on_device = bool(accumulate_on_device)
        self.last_host_fallback_jobs = 0
        self._reset()

    def _reset(self):
        self.detections, self.ground_truth, self.image_ids = [], [], []
        # on_device: rows (x1, y1, x2, y2, score, label) / (x1, y1, x2, y2, label); one entry per image in _pending:
        # (first detection row, rows or None, index into _counts or None, has scores, first ground-truth row, rows)
        self._det, self._gt, self._counts, self._pending, self._device = _DeviceRows(6), _DeviceRows(5), [], [], None

    def update(self, detections, groundtruth, dataset=None, height=None, width=None, image_ids=None):
        """``image_ids``: the GLOBAL index of every image of the batch in the run (sharded runs: the images of a rank are
        a subset); default: a running count, i.e. the order of arrival."""
        n0 = len(self.image_ids)
        if image_ids is not None and len(image_ids) != len(detections):
            raise ValueError(f"DetectionBuffer.update: {len(image_ids)} image ids for {len(detections)} images")
        if self.on_device:
            if len(groundtruth) != len(detections):
                raise ValueError(f"DetectionBuffer.update: {len(groundtruth)} ground-truth entries for {len(detections)} images")
            for d, g in zip(detections, groundtruth):
                dev = self._use_device(d["boxes"])
                boxes = d["boxes"].to(dev, torch.float32).reshape(-1, 4)
                scores = d["scores"].to(dev, torch.float32).reshape(-1, 1) if "scores" in d else torch.ones_like(boxes[:, :1])
                rows = torch.cat((boxes, scores, d["labels"].to(dev, torch.float32).reshape(-1, 1)), 1)
                self._pending.append((self._det.append(rows), rows.shape[0], None, "scores" in d) + self._append_gt(g))
        else:
            self.detections.extend({k: v.cpu() for k, v in d.items()} for d in detections)
            self.ground_truth.extend({k: v.cpu() for k, v in d.items()} for d in groundtruth)
        self.image_ids.extend(image_ids if image_ids is not None else range(n0, n0 + len(detections)))

    def update_device(self, det, n_keep, groundtruth, image_ids=None):
        """``forward_detections``' arrays as they are: ``det[B, A, 6]`` rows (x1, y1, x2, y2, score, label) and
        ``n_keep[B]``, the number of leading rows of every image that are detections -- both on the device, and the counts
        stay there (``det`` and ``n_keep`` are copied at once: a captured window rewrites them).  ``groundtruth``: one
        ``{boxes, labels}`` per image.  All ``A`` rows of an image are kept until ``compile`` / ``compute``."""
        if not self.on_device:
            raise RuntimeError("DetectionBuffer.update_device needs on_device=True")
        B, A = (det.shape[0], det.shape[1]) if det.dim() == 3 else (-1, -1)
        if det.dim() != 3 or det.shape[2] != 6 or n_keep.shape != (B,) or len(groundtruth) != B:
            raise ValueError(f"DetectionBuffer.update_device: det {tuple(det.shape)}, n_keep {tuple(n_keep.shape)}, "
                             f"{len(groundtruth)} ground-truth entries")
        if image_ids is not None and len(image_ids) != B:
            raise ValueError(f"DetectionBuffer.update_device: {len(image_ids)} image ids for {B} images")
        n0 = len(self.image_ids)
        dev = self._use_device(det)
        first = self._det.append(det.to(torch.float32).reshape(B * A, 6))
        self._counts.append(n_keep.to(dev, torch.int32).clamp(0, A))
        at = sum(c.shape[0] for c in self._counts) - B
        for b in range(B):
            self._pending.append((first + b * A, None, at + b, True) + self._append_gt(groundtruth[b]))
        self.image_ids.extend(image_ids if image_ids is not None else range(n0, n0 + B))

    def _use_device(self, t):
        if self._device is None:
            self._device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return self._device

    def _append_gt(self, g):
        dev = self._device
        rows = torch.cat((g["boxes"].to(dev, torch.float32).reshape(-1, 4), g["labels"].to(dev, torch.float32).reshape(-1, 1)), 1)
        return self._gt.append(rows), rows.shape[0]

    def _to_host(self):
        """on_device: ONE copy of everything collected -> the per-image lists the host path keeps (idempotent)."""
        if not self._pending:
            return
        dev = self._device
        det, gt = self._det.rows(dev), self._gt.rows(dev)
        counts = torch.cat(self._counts) if self._counts else torch.empty((0,), dtype=torch.int32, device=dev)
        flat = torch.cat((det.reshape(-1), gt.reshape(-1), counts.view(torch.float32))).cpu()
        det, gt = flat[:det.numel()].view(-1, 6), flat[det.numel():det.numel() + gt.numel()].view(-1, 5)
        counts = flat[det.numel() + gt.numel():].view(torch.int32).tolist()
        for d0, d_n, at, has_scores, g0, g_n in self._pending:
            rows = det[d0:d0 + (d_n if at is None else counts[at])]
            d = {"boxes": rows[:, :4], "scores": rows[:, 4], "labels": rows[:, 5].long()}
            if not has_scores:
                del d["scores"]
            self.detections.append(d)
            self.ground_truth.append({"boxes": gt[g0:g0 + g_n, :4], "labels": gt[g0:g0 + g_n, 4].long()})
        self._det, self._gt, self._counts, self._pending = _DeviceRows(6), _DeviceRows(5), [], []

    def compile(self, sequences, timestamps):
        def by_sequence(items):
            import numpy as np
            out = {}
            for det, seq, t in zip(items, sequences, timestamps):
                out.setdefault(seq, []).append(detections_to_records(det, t))
            return {k: np.concatenate(v) for k, v in out.items()}
        if self.on_device:
            self._to_host()
        return by_sequence(self.detections), by_sequence(self.ground_truth)

    def compute(self, gather=True, group=None):
        """mAP & co over everything collected since the last call (buffers.py:113-122).  Under a process group (window
        batches sharded over the GPUs of a node) the ranks' images are gathered first -- detections AND ground truth, in
        global image order -- and every rank evaluates the whole run: ONE mAP, the number the reference's single process
        prints (run_test.py:61-65).  That makes this call a COLLECTIVE over ``group`` (default group when None): every
        rank has to make it, with image ids that are unique over the ranks (``update(image_ids=...)``).
        ``gather=False``: this rank's images only, no communication (a caller that scores on one rank).
        ``on_device``: the same contract -- the gather starts from this rank's one host copy, and the matcher runs on the
        GPU of the calling rank."""
        from .coco_eval import evaluate_detection
        from ..parallel import gather_evaluation
        if self.on_device:
            self._to_host()
        if gather:
            dets, gts, _ = gather_evaluation(self.detections, self.ground_truth, self.image_ids, group=group)
        else:
            order = sorted(range(len(self.image_ids)), key=lambda i: int(self.image_ids[i]))
            dets, gts = [self.detections[i] for i in order], [self.ground_truth[i] for i in order]
        if self.on_device:
            stats = {}
            out = evaluate_detection(gts, dets, height=self.height, width=self.width, classes=self.classes, on_device=True,
                                     device=self._device, stats=stats, accumulate_on_device=self.accumulate_on_device)
            self.last_host_fallback_jobs = stats.get("host_fallback_jobs", 0)
        else:
            out = evaluate_detection(gts, dets, height=self.height, width=self.width, classes=self.classes)
        self._reset()
        return {k.replace("AP", "mAP"): v for k, v in out.items()}
