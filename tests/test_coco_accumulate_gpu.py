"""The COCO-protocol accumulation on the device (csrc/coco_accumulate.hip: dagr_coco_accumulate; utils/coco_eval.py:
accumulate_device / evaluate_detection(accumulate_on_device=True); DetectionBuffer(accumulate_on_device=True)) against the
host's ``_accumulate`` and ``evaluate_detection`` on the same inputs.  Everything is compared with ``np.array_equal`` /
``==`` on float64: the kernel makes the host's divisions on the host's integers, so there is nothing to tolerate."""
import functools

import numpy as np
import pytest
import torch

from tests import coco_cases as cc
from dagr_amd.utils import coco_eval as ce
from dagr_amd.utils.buffers import DetectionBuffer

pytestmark = pytest.mark.gpu
T, R = len(ce.IOU_THRS), len(ce.REC_THRS)
MAX_GT = 256                                   # DAGR_COCO_MAX_GT


def _device():
    return torch.device("cuda", 0)


def _group(seed, n, n_gt, density=0.5, ignored=0.2, values=8):
    """One group's matched arrays as ``_accumulate`` gets them from one image: (scores [n] from ``values`` distinct
    values -- so that the stable order decides --, dtm [T, n], dt_ign [T, n], g_ign [n_gt] all evaluated)."""
    rng = np.random.default_rng(seed)
    scores = rng.integers(1, values + 1, n) / float(values)
    return scores, rng.uniform(size=(T, n)) < density, rng.uniform(size=(T, n)) < ignored, np.zeros(n_gt, dtype=bool)


def _host(groups):
    """``_accumulate`` per group -> [T, R, G], -1 where it returns None."""
    want = -np.ones((T, R, len(groups)))
    for g, entries in enumerate(groups):
        p = ce._accumulate(entries)
        if p is not None:
            want[:, :, g] = p
    return want


def _device_arrays(groups):
    """The groups' entries laid out as the matcher's columns: group after group, entries in order."""
    flat = [(g, e) for g, entries in enumerate(groups) for e in entries if e is not None]
    n_cols = sum(len(e[0]) for _, e in flat)
    cat = (lambda k, axis: np.concatenate([e[k] for _, e in flat], axis)) if flat else None
    scores = cat(0, 0) if flat else np.zeros(0)
    dtm = cat(1, 1) if flat else np.zeros((T, 0), dtype=bool)
    dt_ign = cat(2, 1) if flat else np.zeros((T, 0), dtype=bool)
    col_group = np.concatenate([np.full(len(e[0]), g, dtype=np.int64) for g, e in flat]) if flat else np.zeros(0, np.int64)
    count = np.bincount(col_group, minlength=len(groups))
    group_ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    n_gt = np.array([sum(int((~e[3]).sum()) for e in entries if e is not None) for entries in groups], dtype=np.int64)
    assert group_ptr[-1] == n_cols
    dev = _device()
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scores, dtm, dt_ign, col_group, group_ptr, n_gt))


def _run(groups):
    precision, status = ce.accumulate_device(*_device_arrays(groups))
    assert status.item() == 0
    got = precision.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (T, R, len(groups))
    return got


def _check(groups):
    got, want = _run(groups), _host(groups)
    for g in range(len(groups)):
        assert np.array_equal(got[:, :, g], want[:, :, g]), (g, np.argwhere(got[:, :, g] != want[:, :, g])[:4])
    return got


def _lengths():
    tile = ce.accumulate_tile()
    return [0, 1, tile - 1, tile, tile + 1, 3 * tile + 1]


@pytest.mark.parametrize("which", range(6))
def test_segment_lengths_around_the_tile(which):
    n = _lengths()[which]
    got = _check([[_group(100 + which, n, n_gt=max(1, n // 3))]])
    assert (got == 0).all() if n == 0 else (got > 0).any()


def test_several_groups_in_one_call():
    tile = ce.accumulate_tile()
    a, b = _group(1, tile + 7, 300), _group(2, 50, 0)                 # b: detections, no ground truth -> -1
    no_dets = (np.zeros(0), np.zeros((T, 0), dtype=bool), np.zeros((T, 0), dtype=bool), np.zeros(3, dtype=bool))
    all_ignored_gt = _group(3, 40, 5)
    all_ignored_gt = all_ignored_gt[:3] + (np.ones(5, dtype=bool),)
    groups = [[a], [], [b], [no_dets], [_group(4, 3 * tile + 1, 900), None, _group(5, 9, 2)], [all_ignored_gt],
              [_group(6 + i, n, 7) for i, n in enumerate(_lengths())]]
    got = _check(groups)
    assert (got[:, :, 1] == -1).all() and (got[:, :, 2] == -1).all() and (got[:, :, 5] == -1).all()
    assert (got[:, :, 3] == 0).all()                                    # ground truth without a detection: zeros
    assert (got[:, :, 0] > 0).any() and (got[:, :, 4] > 0).any() and (got[:, :, 6] > 0).any()


def test_score_ties_within_and_across_images():
    """Eight score values over 2500 detections of 60 images: the result depends on the order of equal scores, which is
    image, then the order inside the image.  The reversed tie order gives another result on the host, so the case decides."""
    rng = np.random.default_rng(21)
    entries = [_group(300 + i, int(rng.integers(0, 90)), int(rng.integers(0, 6))) for i in range(60)]
    _check([entries, entries[::-1], entries[:30]])
    assert not np.array_equal(ce._accumulate(entries), ce._accumulate(entries[::-1]))


@pytest.mark.parametrize("n_gt", [1, 4, 10, 20, 25, 50, 100, 101])
def test_recall_hits_the_recall_points_exactly(n_gt):
    """Exactly ``n_gt`` counted matches at every threshold: tp / n_gt runs through k / n_gt, which equals recall points."""
    n = ce.accumulate_tile() + 1
    rng = np.random.default_rng(n_gt)
    scores, _, _, g_ign = _group(n_gt, n, n_gt)
    dtm, dt_ign = np.zeros((T, n), dtype=bool), rng.uniform(size=(T, n)) < 0.2
    for t in range(T):
        hit = rng.choice(n, n_gt, replace=False)
        dtm[t, hit], dt_ign[t, hit] = True, False
    entry = (scores, dtm, dt_ign, g_ign)
    tp = np.cumsum((dtm & ~dt_ign)[:, np.argsort(-scores, kind="mergesort")], 1)
    assert tp[:, -1].tolist() == [n_gt] * T
    hits = np.intersect1d(np.arange(1, n_gt + 1) / n_gt, ce.REC_THRS)
    assert len(hits) >= (1 if n_gt == 101 else min(n_gt, 4))           # bit-equal recall values and recall points exist
    got = _check([[entry]])
    assert (got[:, -1, 0] > 0).all()                                    # recall 1.0 is reached


def test_extreme_rows():
    n = 2 * ce.accumulate_tile() + 5
    scores, dtm, dt_ign, g_ign = _group(40, n, 64)
    dt_ign[0] = True                                                    # everything ignored
    dtm[1], dt_ign[1] = True, False                                     # everything matches
    dtm[2], dt_ign[2] = False, False                                    # nothing matches: recall stays 0
    got = _check([[(scores, dtm, dt_ign, g_ign)]])
    assert (got[0, :, 0] == 0).all()
    assert (got[1, :, 0] == 1.0).all()                                  # 2 / (2 + eps) = 1 lifts 1 / (1 + eps)
    assert (got[2, :, 0] == 0).all()


def test_precision_that_rises_late():
    """False positives first, the matches at the end of a segment of 3 tiles + 1: the envelope lifts every earlier entry,
    across the tile borders; and a saw-tooth whose envelope changes from tile to tile."""
    tile = ce.accumulate_tile()
    n = 3 * tile + 1
    scores = 1.0 - np.arange(n) / (2.0 * n)                            # already in order, no ties
    late = np.zeros((T, n), dtype=bool)
    for t in range(T):
        late[t, n - 1 - 50 * (t + 1):] = True                           # the last 50 (t + 1) + 1 entries match
        if t % 2:
            late[t, 5] = True                                            # ... and an early one: recall leaves 0 at once
    none = np.zeros((T, n), dtype=bool)
    saw = np.zeros((T, n), dtype=bool)
    for t in range(T):
        period = 97 + 31 * t
        saw[t] = (np.arange(n) % period) >= period - 3 - t              # short bursts of matches at the end of each period
    got = _check([[(scores, late, none, np.zeros(200, dtype=bool))], [(scores, saw, none, np.zeros(150, dtype=bool))]])
    pr = [np.cumsum(late[t]) / (np.arange(n) + 1.0 + np.spacing(1)) for t in (0, 1)]
    assert got[0, 0, 0] == got[0, 1, 0] == pr[0][-1] == pr[0].max()      # lifted from the last entry to the first
    assert got[1, 0, 0] == pr[1][5] > pr[1][-1] == got[1, 1, 0]          # the early match stands above the late rise


def test_bad_arguments_are_reported_and_nothing_is_written():
    tile = ce.accumulate_tile()
    scores, dtm, dt_ign, col_group, group_ptr, n_gt = _device_arrays([[_group(50, tile + 3, 9)], [_group(51, 30, 4)]])
    perm = ce.score_order(scores, col_group)
    n_cols = perm.shape[0]

    def run(perm=perm, group_ptr=group_ptr, **kw):
        out = torch.full((T, R, 2), 7.0, dtype=torch.float64, device=_device())
        _, status = ce.coco_accumulate_device(dtm, dt_ign, perm, group_ptr, n_gt, precision=out, **kw)
        return out.cpu().numpy(), status.item()
    good, status = run()
    assert status == 0 and (good != 7.0).all()
    for at, value in ((0, -1), (tile + 1, n_cols), (n_cols - 1, 2 ** 31 - 1)):
        bad = perm.clone()
        bad[at] = value
        out, status = run(perm=bad)
        assert status == 1 and (out == 7.0).all(), (at, value)
    for ptr in ([0, n_cols + 1, n_cols], [5, 3, n_cols], [-1, 4, n_cols], [0, 4, n_cols + 1]):
        out, status = run(group_ptr=torch.tensor(ptr, dtype=torch.int64, device=_device()))
        assert status == 1 and (out == 7.0).all(), ptr
    need = ce.accumulate_workspace_bytes(T, n_cols)
    out = torch.full((T, R, 2), 7.0, dtype=torch.float64, device=_device())
    with pytest.raises(RuntimeError, match="workspace"):
        ce.coco_accumulate_device(dtm, dt_ign, perm, group_ptr, n_gt, precision=out, workspace_bytes=need - 1)
    assert (out.cpu().numpy() == 7.0).all()
    again, status = run()                                               # and the next good call is not disturbed
    assert status == 0 and np.array_equal(again, good)


# ---- end to end ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """(ground truth, detections, host metrics) -- computed once per case, never changed."""
    if name == "run200":
        gts, dts = cc.random_sweep(seed=11, n_images=200)
    elif name == "sweep+over":                                          # the sweep and one (image, class) beyond the matcher
        gts, dts = cc.random_sweep()
        g, d = cc.crowded(MAX_GT + 1)
        gts, dts = gts[:40] + g + gts[40:], dts[:40] + d + dts[40:]
    elif name.startswith("crowded"):
        gts, dts = cc.crowded(int(name[len("crowded"):]))
    else:
        gts, dts = cc.random_sweep() if name == "sweep" else cc.small_cases()[name]
    with np.errstate(invalid="ignore"):
        return gts, dts, ce.evaluate_detection(gts, dts, classes=cc.CLASSES)


END_TO_END = sorted(cc.small_cases()) + [f"crowded{MAX_GT}", "sweep", "run200"]


@pytest.mark.parametrize("name", END_TO_END)
def test_metrics_with_the_accumulation_on_the_device_are_the_host_floats(name):
    gts, dts, want = case(name)
    stats = {}
    got = ce.evaluate_detection(gts, dts, classes=cc.CLASSES, on_device=True, accumulate_on_device=True, stats=stats)
    assert list(got) == list(want)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    jobs = ce.build_jobs(ce.evaluated_images(gts, dts), len(cc.CLASSES))
    assert stats["host_fallback_jobs"] == 0 and stats["device_jobs"] == len(jobs)
    assert stats["accumulate_device_groups"] == len({(int(c), int(a)) for c, a, _ in jobs.key})


def test_the_precision_array_is_the_host_array_and_the_run_is_not_vacuous():
    gts, dts, want = case("run200")
    assert all(0.0 < want[k] < 1.0 for k in ce.OUT_KEYS), want
    jobs = ce.build_jobs(ce.evaluated_images(gts, dts), len(cc.CLASSES))
    host = ce._precision_from_jobs(ce.evaluated_images(gts, dts), len(cc.CLASSES), ce.match_jobs_host)
    got = ce.precision_on_device(jobs, len(cc.CLASSES))
    assert got.shape == host.shape == (T, R, 2, 4) and np.array_equal(got, host)
    assert all((host[:, :, c, a] > 0).any() for c in range(2) for a in range(4))      # both classes, all four area ranges


@pytest.mark.parametrize("name", [f"crowded{MAX_GT + 1}", "sweep+over"])
def test_host_matched_jobs_are_uploaded_into_their_columns(name):
    gts, dts, want = case(name)
    stats = {}
    got = ce.evaluate_detection(gts, dts, classes=cc.CLASSES, on_device=True, accumulate_on_device=True, stats=stats)
    assert got == want and list(got) == list(want)
    jobs = ce.build_jobs(ce.evaluated_images(gts, dts), len(cc.CLASSES))
    assert stats["host_fallback_jobs"] == 1 and stats["device_jobs"] == len(jobs) - len(ce.AREA_RNG)
    assert want["AP"] > 0


@pytest.mark.parametrize("name", ["sweep", "empties", "sweep+over"])
def test_detection_buffer_accumulating_on_the_device_equals_the_default_buffer(name):
    gts, dts, want = case(name)
    dev = _device()
    host = DetectionBuffer(240, 320, cc.CLASSES)
    buf = DetectionBuffer(240, 320, cc.CLASSES, on_device=True, accumulate_on_device=True)
    for b0 in range(0, len(gts), 8):
        g, d = gts[b0:b0 + 8], dts[b0:b0 + 8]
        host.update(d, g)
        buf.update([{k: v.to(dev) for k, v in x.items()} for x in d], [{k: v.to(dev) for k, v in x.items()} for x in g])
    want_map = host.compute(gather=False)
    assert want_map == {k.replace("AP", "mAP"): v for k, v in want.items()}
    assert buf.compute(gather=False) == want_map
    assert buf.last_host_fallback_jobs == (1 if name == "sweep+over" else 0)
    assert buf.compute(gather=False) == {k.replace("AP", "mAP"): 0 for k in ce.OUT_KEYS}
