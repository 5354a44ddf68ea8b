"""Detection metrics with the interface of ``src/dagr/utils/coco_eval.py`` (``evaluate_detection`` :64-94): AP, AP_50,
AP_75, AP_S, AP_M, AP_L of per-image detections against per-image ground truth.

The reference converts both lists to COCO dictionaries (:175-233) and hands them to ``pycocotools.COCO`` +
``detectron2``'s ``COCOeval_opt`` -- third-party, absent here, **parity unpinned**.  The evaluation protocol those
packages implement is public and is restated below in numpy (``_evaluate_image`` / ``_accumulate`` follow COCOeval's
``evaluateImg`` / ``accumulate`` / ``summarize``: greedy score-ordered matching per IoU threshold in {0.50 .. 0.95}, 100
detections per image, area ranges all / small < 32^2 / medium / large > 96^2 with out-of-range ground truth ignored,
101-point interpolated precision, mean over classes with at least one ground-truth box).

What is the reference's own and kept: images without ground truth are not evaluated (``_match_times`` walks the
ground-truth timestamps, :110-144 -- and ``_to_prophesee`` leaves every timestamp at 0, so one image = one window holding
all of its boxes and detections), class ids shift by one, boxes are (x1, y1, x2, y2) on input and (x, y, w, h) in the
evaluation, an evaluation without any detection returns zeros (:45-49)."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DETS = 100
OUT_KEYS = ("AP", "AP_50", "AP_75", "AP_S", "AP_M", "AP_L")


def _xywh(d):
    b = np.asarray(d["boxes"].cpu() if hasattr(d["boxes"], "cpu") else d["boxes"], dtype=np.float64).reshape(-1, 4)
    # through float32 like the reference's structured array (BBOX_DTYPE: '<f4')
    b = b.astype(np.float32)
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(np.float64)


def _arr(v, dtype):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v).astype(dtype).reshape(-1)


def _iou_xywh(d, g):
    """IoU matrix [len(d), len(g)] of (x, y, w, h) boxes (maskApi bbIou, iscrowd = 0)."""
    if len(d) == 0 or len(g) == 0:
        return np.zeros((len(d), len(g)))
    w = np.minimum(d[:, None, 0] + d[:, None, 2], g[None, :, 0] + g[None, :, 2]) - np.maximum(d[:, None, 0], g[None, :, 0])
    h = np.minimum(d[:, None, 1] + d[:, None, 3], g[None, :, 1] + g[None, :, 3]) - np.maximum(d[:, None, 1], g[None, :, 1])
    inter = np.where((w > 0) & (h > 0), w * h, 0.0)
    union = (d[:, 2] * d[:, 3])[:, None] + (g[:, 2] * g[:, 3])[None, :] - inter
    return inter / union


def _evaluate_image(gt, dt, scores, area_rng):
    """One (image, class, area range): matches of the score-sorted detections per IoU threshold.
    Returns (scores sorted, matched [T, D] bool, det ignored [T, D] bool, gt ignored [G] bool) or None when empty."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    g_area = gt[:, 2] * gt[:, 3]
    g_ign = (g_area < area_rng[0]) | (g_area > area_rng[1])
    g_order = np.argsort(g_ign, kind="mergesort")                    # evaluated ground truth first
    gt, g_ign = gt[g_order], g_ign[g_order]
    d_order = np.argsort(-scores, kind="mergesort")[:MAX_DETS]
    dt, scores = dt[d_order], scores[d_order]
    ious = _iou_xywh(dt, gt)
    T, D, G = len(IOU_THRS), len(dt), len(gt)
    gtm = -np.ones((T, G), dtype=np.int64)
    dtm = np.zeros((T, D), dtype=bool)
    dt_ign = np.zeros((T, D), dtype=bool)
    for ti, thr in enumerate(IOU_THRS):
        for di in range(D):
            best, m = min(thr, 1 - 1e-10), -1
            for gi in range(G):
                if gtm[ti, gi] >= 0:
                    continue
                if m > -1 and not g_ign[m] and g_ign[gi]:
                    break                                            # only ignored ground truth left: keep the match
                if ious[di, gi] < best:
                    continue
                best, m = ious[di, gi], gi
            if m == -1:
                continue
            dt_ign[ti, di] = g_ign[m]
            dtm[ti, di] = True
            gtm[ti, m] = di
    d_area = dt[:, 2] * dt[:, 3]
    out_of_range = (d_area < area_rng[0]) | (d_area > area_rng[1])
    dt_ign = dt_ign | (~dtm & out_of_range[None, :])
    return scores, dtm, dt_ign, g_ign


def _accumulate(per_image):
    """Precision at the 101 recall points per IoU threshold for one (class, area range); None without ground truth."""
    per_image = [e for e in per_image if e is not None]
    if not per_image:
        return None
    scores = np.concatenate([e[0] for e in per_image])
    order = np.argsort(-scores, kind="mergesort")
    dtm = np.concatenate([e[1] for e in per_image], axis=1)[:, order]
    dt_ign = np.concatenate([e[2] for e in per_image], axis=1)[:, order]
    n_gt = int(sum((~e[3]).sum() for e in per_image))
    if n_gt == 0:
        return None
    tps = np.cumsum(dtm & ~dt_ign, axis=1).astype(np.float64)
    fps = np.cumsum(~dtm & ~dt_ign, axis=1).astype(np.float64)
    precision = np.zeros((len(IOU_THRS), len(REC_THRS)))
    for ti in range(len(IOU_THRS)):
        tp, fp = tps[ti], fps[ti]
        rc = tp / n_gt
        pr = tp / (fp + tp + np.spacing(1))
        for i in range(len(pr) - 1, 0, -1):                          # precision envelope
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        idx = np.searchsorted(rc, REC_THRS, side="left")
        ok = idx < len(pr)
        precision[ti, ok] = pr[idx[ok]]
    return precision


def evaluated_images(gt_boxes_list, dt_boxes_list):
    """What the reference's ``_convert_to_coco_format`` (:15-60) hands to COCO: one entry per image WITH ground truth, in
    input order -- (gt boxes xywh, gt classes, detection boxes xywh, detection classes, scores)."""
    images = []
    for gt, dt in zip(gt_boxes_list, dt_boxes_list):
        g_box = _xywh(gt)
        if len(g_box) == 0:
            continue                                                 # KPIs only where there is at least one box (:29-30)
        d_box = _xywh(dt)
        d_score = _arr(dt["scores"], np.float32).astype(np.float64) if "scores" in dt else np.ones(len(d_box))
        images.append((g_box, _arr(gt["labels"], np.int64), d_box, _arr(dt["labels"], np.int64), d_score))
    return images


class JobList:
    """The matcher's work as one flat list.  A job is one (image, class, area range) with at least one ground-truth box
    or one detection of that class: the calls of ``_evaluate_image`` that do not return None.  The boxes of an
    (image, class) are stored once and shared by its four area ranges.

    ``gt`` [NG, 4], ``dt`` [ND, 4] (x, y, w, h), ``scores`` [ND] float64; ``table`` [J, 4] int64 = (first ground-truth
    row, G, first detection row, D); ``rng`` [J, 2] float64; ``key`` [J, 3] int64 = (class, area range, index of the image
    in ``evaluated_images``' list), ascending."""

    def __init__(self, gt, dt, scores, table, rng, key):
        self.gt, self.dt, self.scores, self.table, self.rng, self.key = gt, dt, scores, table, rng, key

    def __len__(self):
        return len(self.table)

    def arrays(self, j):
        """Job j as ``_evaluate_image``'s arguments."""
        g0, g, d0, d = (int(v) for v in self.table[j])
        return self.gt[g0:g0 + g], self.dt[d0:d0 + d], self.scores[d0:d0 + d], self.rng[j]


def build_jobs(images, n_classes):
    """``evaluated_images``' list -> ``JobList``."""
    gt, dt, sc, table, rng, key = [], [], [], [], [], []
    n_g = n_d = 0
    for c in range(n_classes):
        groups = []
        for i, (g, gl, d, dl, s) in enumerate(images):
            gm, dm = gl == c, dl == c
            g_c, d_c = g[gm], d[dm]
            if len(g_c) == 0 and len(d_c) == 0:
                continue
            gt.append(g_c), dt.append(d_c), sc.append(s[dm])
            groups.append((i, n_g, len(g_c), n_d, len(d_c)))
            n_g, n_d = n_g + len(g_c), n_d + len(d_c)
        for ai, r in enumerate(AREA_RNG):
            for i, g0, g_n, d0, d_n in groups:
                table.append((g0, g_n, d0, d_n)), rng.append(r), key.append((c, ai, i))

    def cat(parts, shape):
        return np.concatenate(parts, 0) if parts else np.zeros(shape)
    return JobList(cat(gt, (0, 4)), cat(dt, (0, 4)), cat(sc, (0,)), np.asarray(table, dtype=np.int64).reshape(-1, 4),
                   np.asarray(rng, dtype=np.float64).reshape(-1, 2), np.asarray(key, dtype=np.int64).reshape(-1, 3))


def match_jobs_host(jobs, which=None):
    """``_evaluate_image`` job by job: ``{job: (scores sorted, dtm, dt_ign, g_ign)}`` for the jobs ``which`` (all)."""
    return {int(j): _evaluate_image(*jobs.arrays(int(j))) for j in (range(len(jobs)) if which is None else which)}


def device_bounds():
    """(G, D) one job of ``dagr_coco_match`` takes (include/dagr_hip.h: DAGR_COCO_MAX_GT, DAGR_COCO_MAX_DT)."""
    import ctypes
    from .. import _lib
    g, d, m = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _lib.lib().dagr_coco_match_bounds(ctypes.byref(g), ctypes.byref(d), ctypes.byref(m))
    if m.value < MAX_DETS:
        raise RuntimeError(f"dagr_coco_match matches {m.value} detections per job, the protocol needs {MAX_DETS}")
    return g.value, d.value


class DeviceMatches:
    """What ``coco_match_device(to_host=False)`` leaves on the device: ``order`` int32 [n_out], ``dtm`` / ``dt_ign`` uint8
    [T, n_out], ``g_ign`` uint8 [n_gign] and ``status`` int32 [1] -- views of ONE buffer, in the columns ``o_off`` / entries
    ``gi_off`` of the jobs ``which`` -- plus ``scores`` float64 [ND] (``jobs.scores``) and ``table`` int64 [len(which), 6]
    (first ground-truth row, G, first detection row, D, first column, first ``g_ign`` entry)."""

    def __init__(self, which, o_off, kept, gi_off, order, dtm, dt_ign, g_ign, status, scores, table):
        self.which, self.o_off, self.kept, self.gi_off = which, o_off, kept, gi_off
        self.order, self.dtm, self.dt_ign, self.g_ign, self.status = order, dtm, dt_ign, g_ign, status
        self.scores, self.table = scores, table


def column_layout(jobs):
    """Where every job of the list keeps its results when ALL jobs share the output arrays: (kept [J] = min(D, MAX_DETS),
    first column [J], number of columns, first ``g_ign`` entry [J], number of entries)."""
    kept = np.minimum(jobs.table[:, 3], MAX_DETS)
    return kept, np.cumsum(kept) - kept, int(kept.sum()), np.cumsum(jobs.table[:, 1]) - jobs.table[:, 1], int(jobs.table[:, 1].sum())


def _match_layout(T, n_out, n_gign):
    """Where the matcher's outputs lie in their ONE buffer (one buffer = one copy back): status int32 | order int32[n_out] |
    dtm, dt_ign uint8[T, n_out] | g_ign uint8[n_gign] -- (at_order, at_dtm, at_ign, at_gign, bytes)."""
    at_order, at_dtm = 4, 4 + 4 * n_out
    at_ign, at_gign = at_dtm + T * n_out, at_dtm + 2 * T * n_out
    return at_order, at_dtm, at_ign, at_gign, at_gign + n_gign


def match_launch(gt, dt, scores, jobs6, rng, thrs, J, n_gt, n_dt, max_g, max_d, n_out, n_gign, device, zeroed=False):
    """``dagr_coco_match`` on device arrays (``c_void_p``, the header's layouts) with host sizes: one launch (none for
    ``J = 0``), no synchronisation.  Returns (the output buffer of ``_match_layout``, its views ``(order, dtm, dt_ign, g_ign,
    status)``); ``zeroed``: the buffer starts as zeros instead of uninitialised."""
    import torch
    from .. import _lib
    T = len(IOU_THRS)
    at_order, at_dtm, at_ign, at_gign, nbytes = _match_layout(T, n_out, n_gign)
    res = (torch.zeros if zeroed else torch.empty)((nbytes,), dtype=torch.uint8, device=device)
    base = res.data_ptr()
    if J:
        _lib.check(_lib.lib().dagr_coco_match(
            gt, dt, scores, jobs6, rng, thrs, T, MAX_DETS, J, n_gt, n_dt, max_g, max_d, n_out, n_gign,
            _lib.c_void_p(base + at_order), _lib.c_void_p(base + at_dtm), _lib.c_void_p(base + at_ign),
            _lib.c_void_p(base + at_gign), _lib.c_void_p(base), _lib.cur_stream(device)), "coco_match")
    elif not zeroed:
        res[:4].zero_()                                               # (the status word the launch would have cleared)
    return res, (res[at_order:at_dtm].view(torch.int32), res[at_dtm:at_ign].view(T, n_out),
                 res[at_ign:at_gign].view(T, n_out), res[at_gign:], res[:4].view(torch.int32))


def coco_match_device(jobs, which, device, to_host=True, all_columns=False):
    """``dagr_coco_match`` for the jobs ``which`` (all within the kernel's bounds): two copies to the device (one float64,
    one int64 array), ONE launch, ONE copy back.  ``{job: (order, dtm, dt_ign, g_ign)}`` with ``order`` the indices of the
    job's detections by descending score, cut to ``MAX_DETS``.

    ``to_host=False``: no copy back and no synchronisation -- a ``DeviceMatches``; its ``status`` is for the caller to
    read.  ``all_columns``: the output arrays have the columns of every job of the list (``column_layout``), those of the
    jobs outside ``which`` zeroed, instead of the columns of ``which`` alone."""
    import torch
    from .. import _lib
    which = np.asarray(which, dtype=np.int64)
    tab = jobs.table[which]
    T, J = len(IOU_THRS), len(which)
    if all_columns:
        kept, o_off, n_out, gi_off, n_gign = column_layout(jobs)
        kept, o_off, gi_off = kept[which], o_off[which], gi_off[which]
    else:
        kept = np.minimum(tab[:, 3], MAX_DETS)
        o_off, gi_off = np.cumsum(kept) - kept, np.cumsum(tab[:, 1]) - tab[:, 1]
        n_out, n_gign = int(kept.sum()), int(tab[:, 1].sum())
    n_gt, n_dt = len(jobs.gt), len(jobs.dt)
    f64 = np.concatenate([jobs.gt.reshape(-1), jobs.dt.reshape(-1), jobs.scores, jobs.rng[which].reshape(-1), IOU_THRS])
    i64 = np.concatenate([tab, o_off[:, None], gi_off[:, None]], 1)
    at_order, at_dtm, at_ign, at_gign, _ = _match_layout(T, n_out, n_gign)
    with torch.cuda.device(device):
        fd = torch.from_numpy(np.ascontiguousarray(f64, dtype=np.float64)).to(device)
        jd = torch.from_numpy(np.ascontiguousarray(i64, dtype=np.int64)).to(device)
        f0 = fd.data_ptr()

        def f64_at(n_doubles):
            return _lib.c_void_p(f0 + 8 * n_doubles)
        res, views = match_launch(f64_at(0), f64_at(4 * n_gt), f64_at(4 * n_gt + 4 * n_dt), _lib.ptr(jd),
                                  f64_at(4 * n_gt + 5 * n_dt), f64_at(4 * n_gt + 5 * n_dt + 2 * J), J, n_gt, n_dt,
                                  int(tab[:, 1].max()) if J else 0, int(tab[:, 3].max()) if J else 0, n_out, n_gign, device,
                                  zeroed=all_columns)
        if not to_host:
            return DeviceMatches(which, o_off, kept, gi_off, *views, fd[4 * n_gt + 4 * n_dt:4 * n_gt + 5 * n_dt], jd)
        host = res.cpu().numpy()
    if host[:4].view(np.int32)[0] != 0:
        raise RuntimeError("dagr_coco_match: a job did not fit its arrays (status 1)")
    order = host[at_order:at_dtm].view(np.int32)
    dtm = host[at_dtm:at_ign].view(np.bool_).reshape(T, n_out)
    dt_ign = host[at_ign:at_gign].view(np.bool_).reshape(T, n_out)
    g_ign = host[at_gign:].view(np.bool_)
    out = {}
    for n, j in enumerate(which):
        o, k, gi, g_n = int(o_off[n]), int(kept[n]), int(gi_off[n]), int(tab[n, 1])
        out[int(j)] = (order[o:o + k], dtm[:, o:o + k], dt_ign[:, o:o + k], g_ign[gi:gi + g_n])
    return out


def match_jobs_device(jobs, device=None, stats=None):
    """``match_jobs_host`` with the matcher on the GPU (``coco_match_device``).  A job beyond the kernel's per-job bounds
    is matched on the host; the four area ranges of an (image, class) share their boxes, so they go together, and
    ``stats["host_fallback_jobs"]`` counts such an (image, class) once."""
    import torch
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"match_jobs_device: the matcher runs on a GPU, not on {device}")
    max_g, max_d = device_bounds()
    fits = (jobs.table[:, 1] <= max_g) & (jobs.table[:, 3] <= max_d)
    on_dev, on_host = np.flatnonzero(fits), np.flatnonzero(~fits)
    out = match_jobs_host(jobs, on_host)
    if stats is not None:
        stats["host_fallback_jobs"] = len({(int(c), int(i)) for c, _, i in jobs.key[on_host]})
        stats["device_jobs"] = int(len(on_dev))
    if len(on_dev):
        for j, (order, dtm, dt_ign, g_ign) in coco_match_device(jobs, on_dev, device).items():
            out[j] = (jobs.scores[jobs.table[j, 2] + order], dtm, dt_ign, g_ign)
    return out


def accumulate_groups(jobs, n_classes):
    """The groups of ``_accumulate`` in ``column_layout``'s columns.  ``build_jobs`` orders the jobs by (class, area range,
    image), so the columns of a (class, area range) are ONE contiguous run, images ascending and the matcher's order inside
    an image: the order ``_accumulate`` concatenates in.  Returns (group = class * len(AREA_RNG) + area range of every
    job [J], group_ptr [n_groups + 1] over the columns)."""
    kept = column_layout(jobs)[0]
    n_groups = n_classes * len(AREA_RNG)
    group = jobs.key[:, 0] * len(AREA_RNG) + jobs.key[:, 1]
    if np.any(np.diff(group) < 0):
        raise RuntimeError("accumulate_groups: the job list is not ordered by (class, area range)")
    cols = np.zeros(n_groups, dtype=np.int64)
    np.add.at(cols, group, kept)
    return group.astype(np.int64), np.concatenate([[0], np.cumsum(cols)]).astype(np.int64)


def score_order(scores, col_group):
    """``perm`` of ``dagr_coco_accumulate`` (torch, on the tensors' device): the columns group after group and inside a
    group as ``np.argsort(-scores, kind="mergesort")`` leaves them -- descending score, equal scores in column order, NaN
    last.  Two stable sorts: by score over everything, then by group."""
    import torch
    by_score = torch.sort(0.0 - scores, stable=True).indices             # 0 - s: -0.0 and 0.0 are one key
    by_group = torch.sort(col_group[by_score], stable=True).indices
    return by_score[by_group].to(torch.int32)


def accumulate_tile():
    """Positions one workgroup of ``dagr_coco_accumulate`` takes at a time (DAGR_COCO_ACC_TILE)."""
    from .. import _lib
    return int(_lib.lib().dagr_coco_accumulate_tile())


def accumulate_workspace_bytes(n_thr, n_cols):
    """Bytes of workspace ``dagr_coco_accumulate`` needs (dagr_coco_accumulate_workspace_bytes)."""
    from .. import _lib
    need = int(_lib.lib().dagr_coco_accumulate_workspace_bytes(n_thr, n_cols))
    if need == 0:
        _lib.check(-1, "coco_accumulate_workspace_bytes")
    return need


def coco_accumulate_device(dtm, dt_ign, perm, group_ptr, group_ngt, precision=None, workspace_bytes=None):
    """``dagr_coco_accumulate`` on device tensors: ``dtm`` / ``dt_ign`` uint8 or bool [T, n_cols], ``perm`` int32 [n_cols],
    ``group_ptr`` int64 [n_groups + 1], ``group_ngt`` int64 [n_groups].  Returns (precision float64 [T, len(REC_THRS),
    n_groups], status int32 [1]), both on the device and not synchronised; status 1: a bad ``perm`` / ``group_ptr``,
    ``precision`` untouched.  ``precision`` / ``workspace_bytes``: a caller's output array / another workspace size."""
    import torch
    from .. import _lib
    device = dtm.device
    T, n_cols = dtm.shape
    n_groups = group_ngt.shape[0]
    if dt_ign.shape != dtm.shape or perm.shape != (n_cols,) or group_ptr.shape != (n_groups + 1,):
        raise ValueError(f"coco_accumulate_device: dtm {tuple(dtm.shape)}, dt_ign {tuple(dt_ign.shape)}, perm "
                         f"{tuple(perm.shape)}, group_ptr {tuple(group_ptr.shape)}, group_ngt {tuple(group_ngt.shape)}")

    def flags(x):
        return (x.view(torch.uint8) if x.dtype == torch.bool else x.to(torch.uint8)).contiguous()
    dtm, dt_ign = flags(dtm), flags(dt_ign)
    perm, group_ptr = perm.to(torch.int32).contiguous(), group_ptr.to(torch.int64).contiguous()
    group_ngt = group_ngt.to(torch.int64).contiguous()
    L = _lib.lib()
    with torch.cuda.device(device):
        ws_bytes = accumulate_workspace_bytes(T, n_cols) if workspace_bytes is None else int(workspace_bytes)
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=device)
        rec = torch.from_numpy(REC_THRS).to(device)
        if precision is None:
            precision = torch.empty((T, len(REC_THRS), n_groups), dtype=torch.float64, device=device)
        status = torch.zeros((1,), dtype=torch.int32, device=device)
        _lib.check(L.dagr_coco_accumulate(_lib.ptr(dtm), _lib.ptr(dt_ign), _lib.ptr(perm), _lib.ptr(group_ptr),
                                          _lib.ptr(group_ngt), _lib.ptr(rec), len(REC_THRS), float(np.spacing(1)), T, n_groups,
                                          n_cols, _lib.ptr(ws), ws_bytes, _lib.ptr(precision), _lib.ptr(status),
                                          _lib.cur_stream(device)), "coco_accumulate")
    return precision, status


def accumulate_device(scores, dtm, dt_ign, col_group, group_ptr, group_ngt):
    """``_accumulate`` of every group at once, on the device arrays of the matcher (``coco_match_device(to_host=False,
    all_columns=True)``): ``scores`` float64 [n_cols] and ``col_group`` int64 [n_cols] per column, ``dtm`` / ``dt_ign``
    [T, n_cols].  -> ``coco_accumulate_device``'s (precision, status)."""
    return coco_accumulate_device(dtm, dt_ign, score_order(scores, col_group), group_ptr, group_ngt)


def precision_on_device(jobs, n_classes, device=None, stats=None):
    """Job list -> ``dagr_coco_match`` -> ``dagr_coco_accumulate`` -> the precision array [T, R, classes, area ranges], the
    only thing copied back (with the two status words).  A job beyond the matcher's bounds is matched on the host, as in
    ``match_jobs_device``, and uploaded into its columns."""
    import torch
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"precision_on_device: the evaluation runs on a GPU, not on {device}")
    T, A = len(IOU_THRS), len(AREA_RNG)
    max_g, max_d = device_bounds()
    fits = (jobs.table[:, 1] <= max_g) & (jobs.table[:, 3] <= max_d)
    on_dev, on_host = np.flatnonzero(fits), np.flatnonzero(~fits)
    from_host = match_jobs_host(jobs, on_host)
    kept, o_off, n_cols, gi_off, n_gign = column_layout(jobs)
    group, group_ptr = accumulate_groups(jobs, n_classes)
    n_groups = n_classes * A
    if stats is not None:
        stats["host_fallback_jobs"] = len({(int(c), int(i)) for c, _, i in jobs.key[on_host]})
        stats["device_jobs"] = int(len(on_dev))
        stats["accumulate_device_groups"] = int(len(np.unique(group)))
    m = coco_match_device(jobs, on_dev, device, to_host=False, all_columns=True)
    with torch.cuda.device(device):
        per_job = np.stack([group, kept, jobs.table[:, 1], jobs.table[:, 2]], 1).reshape(-1)
        i64 = torch.from_numpy(np.concatenate([per_job, group_ptr]).astype(np.int64)).to(device)
        per_job, group_ptr_d = i64[:4 * len(jobs)].view(-1, 4), i64[4 * len(jobs):]
        col_group = torch.repeat_interleave(per_job[:, 0], per_job[:, 1], output_size=n_cols)
        col_first = torch.repeat_interleave(per_job[:, 3], per_job[:, 1], output_size=n_cols)
        entry_group = torch.repeat_interleave(per_job[:, 0], per_job[:, 2], output_size=n_gign)
        scores = m.scores[col_first + m.order.long()] if n_cols else m.scores[:0]
        if len(on_host):                                              # host-matched jobs: into their columns / entries
            cols = np.concatenate([o_off[j] + np.arange(kept[j]) for j in on_host])
            entries = np.concatenate([gi_off[j] + np.arange(jobs.table[j, 1]) for j in on_host])
            at = torch.from_numpy(np.concatenate([cols, entries]).astype(np.int64)).to(device)
            cols_d, entries_d = at[:len(cols)], at[len(cols):]
            scores[cols_d] = torch.from_numpy(np.concatenate([from_host[int(j)][0] for j in on_host])).to(device)
            flag = np.concatenate([np.concatenate([from_host[int(j)][k] for j in on_host], 1) for k in (1, 2)], 0)
            flag = torch.from_numpy(flag.astype(np.uint8)).to(device)
            m.dtm[:, cols_d], m.dt_ign[:, cols_d] = flag[:T], flag[T:]
            m.g_ign[entries_d] = torch.from_numpy(np.concatenate([from_host[int(j)][3] for j in on_host]).astype(np.uint8)).to(device)
        return precision_read_back(scores, m.dtm, m.dt_ign, m.g_ign, m.status, col_group, entry_group, group_ptr_d, n_classes)[0]


def precision_read_back(scores, dtm, dt_ign, g_ign, match_status, col_group, entry_group, group_ptr, n_classes, also=None):
    """From the matcher's device arrays to the precision array on the host: ``group_ngt`` from ``g_ign``, ``score_order``,
    ``dagr_coco_accumulate``, and ONE copy back of the precision array, the two status words and ``also`` (a contiguous
    device tensor, or None).  Returns (precision float64 [T, R, classes, area ranges], the bytes of ``also``); raises on
    either status."""
    import torch
    T, A = len(IOU_THRS), len(AREA_RNG)
    group_ngt = torch.zeros((n_classes * A,), dtype=torch.int64, device=dtm.device)
    group_ngt.index_add_(0, entry_group, (g_ign == 0).to(torch.int64))
    precision, status = accumulate_device(scores, dtm, dt_ign, col_group, group_ptr, group_ngt)
    parts = (precision.reshape(-1).view(torch.uint8), status.view(torch.uint8), match_status.view(torch.uint8))
    extra = also.reshape(-1).view(torch.uint8) if also is not None else None
    back = torch.cat(parts + ((extra,) if extra is not None else ())).cpu().numpy()
    n_prec = 8 * T * len(REC_THRS) * n_classes * A
    acc_status, match_status = back[n_prec:n_prec + 8].view(np.int32)
    if match_status != 0:
        raise RuntimeError("dagr_coco_match: a job did not fit its arrays (status 1)")
    if acc_status != 0:
        raise RuntimeError("dagr_coco_accumulate: perm or group_ptr outside the arrays (status 1)")
    return back[:n_prec].view(np.float64).reshape(T, len(REC_THRS), n_classes, A).copy(), back[n_prec + 8:].copy()


def summarize(prec):
    """The six numbers of the protocol from the precision array [T, R, classes, area ranges] (-1: nothing to average)."""
    def mean(sel):
        v = sel[sel > -1]
        return float(v.mean()) if v.size else -1.0
    return {"AP": mean(prec[:, :, :, 0]), "AP_50": mean(prec[0, :, :, 0]), "AP_75": mean(prec[5, :, :, 0]),
            "AP_S": mean(prec[:, :, :, 1]), "AP_M": mean(prec[:, :, :, 2]), "AP_L": mean(prec[:, :, :, 3])}


class StreamMapPlan:
    """``dagr_stream_map_plan``'s workspace and output arrays for a log of ``B`` lanes, ``max_images`` images a lane, ``G``
    ground-truth rows and ``max_dets`` detection rows an image: allocated once, sized from the capacities
    (include/dagr_hip.h has the formulas), on ``device``.  ``run(state)`` is the one call: no host synchronisation.
    Memory: 40 bytes for every detection row the log can hold (``B * max_images * max_dets``), 64 for every ground-truth
    row, and 32 for each of an image's first ``min(max_dets, 100 * classes)`` rows -- 1.6 GB at B = 8, 1200 images and 4096
    rows a lane, 70 MB with ``max_dets = 100``."""

    def __init__(self, B, max_images, G, max_dets, n_classes, device):
        import torch
        from .. import _lib
        self.sizes, self.n_classes, self.device = (int(B), int(max_images), int(G), int(max_dets)), int(n_classes), device
        N, A, C = int(B) * int(max_images), len(AREA_RNG), int(n_classes)
        pairs, cols = N * min(C, G + max_dets), N * min(max_dets, MAX_DETS * C)
        need = int(_lib.lib().dagr_stream_map_plan_workspace_bytes(B, max_images, C))
        if need == 0:
            raise ValueError(f"stream map plan: batch_size = {B}, max_images = {max_images} and {C} classes are out of range "
                             f"(1..{_lib.DEFINES['DAGR_MAP_MAX_CLASSES']} classes, batch_size * max_images * classes < 2**28)")

        def new(shape, dtype):
            return torch.zeros(shape, dtype=dtype, device=device)
        self.workspace = new((need,), torch.uint8)
        self.gt, self.dt, self.scores = new((N * G, 4), torch.float64), new((N * max_dets, 4), torch.float64), new((N * max_dets,), torch.float64)
        self.jobs, self.rng, self.info = new((A * pairs, 6), torch.int64), new((A * pairs, 2), torch.float64), new((A * pairs, 4), torch.int64)
        self.col_group, self.entry_group = new((A * cols,), torch.int64), new((A * N * G,), torch.int64)
        self.group_ptr, self.totals = new((C * A + 1,), torch.int64), new((8,), torch.int64)
        self.area_rngs = torch.from_numpy(np.asarray(AREA_RNG, dtype=np.float64)).to(device)
        self.iou_thrs = torch.from_numpy(IOU_THRS).to(device)

    def run(self, state):
        """The plan of the log in ``state`` (a uint8 device tensor of ``dagr_stream_map_bytes``)."""
        from .. import _lib
        P = _lib.ptr
        _lib.check(_lib.lib().dagr_stream_map_plan(
            P(state), state.numel(), *self.sizes, self.n_classes, P(self.area_rngs), len(AREA_RNG), MAX_DETS,
            P(self.workspace), self.workspace.numel(), P(self.gt), P(self.dt), P(self.scores), P(self.jobs), P(self.rng),
            P(self.info), P(self.col_group), P(self.entry_group), P(self.group_ptr), P(self.totals),
            _lib.cur_stream(self.device)), "stream_map_plan")

    def precision(self, also=None):
        """From the plan ``run`` left to the precision array: the totals block read back (one small copy: the C entries of
        match and accumulate take host sizes), ``dagr_coco_match``, then ``precision_read_back``.  Returns (the totals as a
        dict, precision [T, R, classes, area ranges] or None when the log holds no detection row, the bytes of ``also``)."""
        import torch
        from .. import _lib
        P = _lib.ptr
        names = ("n_jobs", "n_gt", "n_dt", "n_out", "n_gign", "max_gt", "max_dt", "logged_dets")
        tot = dict(zip(names, (int(v) for v in self.totals.cpu().numpy())))
        J, n_out, n_gign = tot["n_jobs"], tot["n_out"], tot["n_gign"]
        if tot["logged_dets"] == 0 or J == 0:                         # zeros, or -1 everywhere: nothing to launch
            extra = also.reshape(-1).view(torch.uint8).cpu().numpy().copy() if also is not None else None
            prec = None if tot["logged_dets"] == 0 else -np.ones((len(IOU_THRS), len(REC_THRS), self.n_classes, len(AREA_RNG)))
            return tot, prec, extra
        with torch.cuda.device(self.device):
            _, (order, dtm, dt_ign, g_ign, status) = match_launch(
                P(self.gt), P(self.dt), P(self.scores), P(self.jobs), P(self.rng), P(self.iou_thrs), J, tot["n_gt"],
                tot["n_dt"], tot["max_gt"], tot["max_dt"], n_out, n_gign, self.device)
            info = self.info[:J]
            col_first = torch.repeat_interleave(self.jobs[:J, 2], info[:, 1], output_size=n_out)
            scores = self.scores[col_first + order.long()] if n_out else self.scores[:0]
            prec, extra = precision_read_back(scores, dtm, dt_ign, g_ign, status, self.col_group[:n_out],
                                              self.entry_group[:n_gign], self.group_ptr, self.n_classes, also=also)
        return tot, prec, extra


def _precision_from_jobs(images, n_classes, matcher):
    """Job list -> matcher -> per (class, area range) the per-image tuples, in image order, -> ``_accumulate``."""
    jobs = build_jobs(images, n_classes)
    matched = matcher(jobs)
    per_image = {}
    for j, (c, ai, _) in enumerate(jobs.key):                        # ascending image index inside a (class, area range)
        per_image.setdefault((int(c), int(ai)), []).append(matched[j])
    prec = -np.ones((len(IOU_THRS), len(REC_THRS), n_classes, len(AREA_RNG)))
    for (c, ai), entries in per_image.items():
        p = _accumulate(entries)
        if p is not None:
            prec[:, :, c, ai] = p
    return prec


def evaluate_detection(gt_boxes_list, dt_boxes_list, classes=("car", "pedestrian"), height=240, width=304,
                       time_tol=50000, on_device=False, device=None, stats=None, accumulate_on_device=False):
    """gt / dt: one dict per image, ``boxes`` [n, 4] (x1, y1, x2, y2), ``labels`` [n], detections also ``scores`` [n].
    ``on_device``: the greedy matcher runs as ``dagr_coco_match`` on ``device`` (default: the current GPU) instead of
    ``_evaluate_image``; the same booleans reach the same ``_accumulate``, so the result is the same floats.
    ``stats`` (a dict) then receives ``host_fallback_jobs`` and ``device_jobs``.
    ``accumulate_on_device`` (needs ``on_device``): ``_accumulate`` runs on the device too, as ``dagr_coco_accumulate`` on
    the matcher's arrays where they are, and only the precision array [10, 101, classes, 4] comes back -- again the same
    floats.  ``stats`` also receives ``accumulate_device_groups``, the (class, area range) groups that had a job."""
    if accumulate_on_device and not on_device:
        raise ValueError("evaluate_detection: accumulate_on_device=True needs on_device=True")
    images = evaluated_images(gt_boxes_list, dt_boxes_list)
    if sum(len(im[2]) for im in images) == 0:
        return {k: 0 for k in OUT_KEYS}
    if accumulate_on_device:
        prec = precision_on_device(build_jobs(images, len(classes)), len(classes), device, stats)
    elif on_device:
        prec = _precision_from_jobs(images, len(classes), lambda jobs: match_jobs_device(jobs, device, stats))
    else:
        prec = -np.ones((len(IOU_THRS), len(REC_THRS), len(classes), len(AREA_RNG)))
        for c in range(len(classes)):
            for ai, rng in enumerate(AREA_RNG):
                per_image = [_evaluate_image(g[gl == c], d[dl == c], s[dl == c], rng) for g, gl, d, dl, s in images]
                p = _accumulate(per_image)
                if p is not None:
                    prec[:, :, c, ai] = p
    return summarize(prec)
