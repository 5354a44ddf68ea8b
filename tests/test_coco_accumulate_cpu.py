"""CPU suite of the device accumulation (utils/coco_eval.py: column_layout / accumulate_groups / score_order /
evaluate_detection(accumulate_on_device=...); DetectionBuffer(accumulate_on_device=...)): the column layout and ``perm``
reproduce ``_accumulate``'s order, the new keyword is checked and off by default, and ``dagr_coco_accumulate`` rejects bad
arguments before any device work."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import coco_cases as cc
from dagr_amd import _lib
from dagr_amd.utils import coco_eval as ce
from dagr_amd.utils import testing
from dagr_amd.utils.buffers import DetectionBuffer


def _tie_heavy(seed=5, n_images=40):
    """``random_sweep`` with every score drawn from 8 values: equal scores inside an image and across images."""
    gts, dts = cc.random_sweep(seed=seed, n_images=n_images)
    rng = np.random.default_rng(seed)
    for d in dts:
        d["scores"] = torch.from_numpy(rng.integers(1, 9, len(d["scores"])) / 8.0).float()
    return gts, dts


@pytest.mark.parametrize("name", ["sweep", "tie_heavy", "ties", "empties"])
def test_layout_and_perm_give_the_order_of_accumulate(name):
    gts, dts = {"sweep": cc.random_sweep, "tie_heavy": _tie_heavy, "ties": cc.ties, "empties": cc.empties}[name]()
    jobs = ce.build_jobs(ce.evaluated_images(gts, dts), len(cc.CLASSES))
    matched = ce.match_jobs_host(jobs)
    kept, o_off, n_cols, gi_off, n_gign = ce.column_layout(jobs)
    group, group_ptr = ce.accumulate_groups(jobs, len(cc.CLASSES))
    assert n_cols == sum(len(matched[j][0]) for j in range(len(jobs))) and group_ptr[-1] == n_cols
    assert n_gign == sum(len(matched[j][3]) for j in range(len(jobs)))
    scores = np.zeros(n_cols)
    for j in range(len(jobs)):
        assert kept[j] == len(matched[j][0])
        scores[o_off[j]:o_off[j] + kept[j]] = matched[j][0]
    perm = ce.score_order(torch.from_numpy(scores), torch.from_numpy(np.repeat(group, kept))).numpy()
    assert perm.dtype == np.int32 and sorted(perm.tolist()) == list(range(n_cols))
    seen = 0
    for g in range(len(cc.CLASSES) * len(ce.AREA_RNG)):
        mine = [j for j in range(len(jobs)) if group[j] == g]             # ascending image index: the host's per_image list
        assert [jobs.key[j, 2] for j in mine] == sorted(jobs.key[j, 2] for j in mine)
        cols = np.concatenate([o_off[j] + np.arange(kept[j]) for j in mine]) if mine else np.zeros(0, np.int64)
        cat = np.concatenate([matched[j][0] for j in mine]) if mine else np.zeros(0)
        want = cols[np.argsort(-cat, kind="mergesort")]                   # _accumulate's `order`, in columns
        assert np.array_equal(perm[group_ptr[g]:group_ptr[g + 1]], want), g
        seen += len(want)
        if name == "tie_heavy" and len(cat) > 16:
            assert len(np.unique(cat)) <= 8 < len(cat)                   # the stable order decided
    assert seen == n_cols


def test_score_order_zeros_and_nan_sort_as_numpy_does():
    s = np.array([0.5, -0.0, np.nan, 0.0, 0.5, -0.0, 1.0, np.nan, 0.0])
    for group in (np.zeros(9, np.int64), np.array([1, 1, 1, 1, 0, 0, 0, 0, 0])):
        perm = ce.score_order(torch.from_numpy(s), torch.from_numpy(group)).numpy()
        want = np.concatenate([np.flatnonzero(group == g)[np.argsort(-s[group == g], kind="mergesort")] for g in (0, 1)])
        assert np.array_equal(perm, want)


def test_accumulate_on_device_needs_on_device():
    gts, dts = cc.ties()
    with pytest.raises(ValueError, match="on_device"):
        ce.evaluate_detection(gts, dts, classes=cc.CLASSES, accumulate_on_device=True)
    with pytest.raises(ValueError, match="on_device"):
        DetectionBuffer(240, 320, cc.CLASSES, accumulate_on_device=True)
    with pytest.raises(ValueError, match="on_device"):
        DetectionBuffer(240, 320, cc.CLASSES, on_device=False, accumulate_on_device=True)


def test_defaults_keep_the_call_path(monkeypatch):
    """Without the keyword nothing of the new path runs: the host path and ``on_device=True`` still end in ``_accumulate``."""
    gts, dts = cc.random_sweep(n_images=16)
    calls = {"accumulate": 0, "match": 0}
    accumulate = ce._accumulate

    def counted(per_image):
        calls["accumulate"] += 1
        return accumulate(per_image)

    def match(jobs, device=None, stats=None):
        calls["match"] += 1
        return ce.match_jobs_host(jobs)

    def never(*a, **k):
        raise AssertionError("the device accumulation ran without accumulate_on_device=True")
    monkeypatch.setattr(ce, "_accumulate", counted)
    monkeypatch.setattr(ce, "match_jobs_device", match)
    for name in ("precision_on_device", "accumulate_device", "coco_accumulate_device"):
        monkeypatch.setattr(ce, name, never)
    want = ce.evaluate_detection(gts, dts, classes=cc.CLASSES)
    assert calls == {"accumulate": 8, "match": 0}
    assert ce.evaluate_detection(gts, dts, classes=cc.CLASSES, accumulate_on_device=False) == want
    assert ce.evaluate_detection(gts, dts, classes=cc.CLASSES, on_device=True) == want
    assert calls["match"] == 1 and calls["accumulate"] > 16
    assert ce.evaluate_detection(gts, dts, classes=cc.CLASSES, on_device=True, accumulate_on_device=False) == want
    assert calls["match"] == 2


def test_the_process_default_reaches_the_buffer_only_with_on_device():
    assert DetectionBuffer(240, 320, cc.CLASSES, on_device=True).accumulate_on_device is False
    testing.accumulate_on_device(True)
    try:
        assert DetectionBuffer(240, 320, cc.CLASSES, on_device=True).accumulate_on_device is True
        assert DetectionBuffer(240, 320, cc.CLASSES, on_device=True, accumulate_on_device=False).accumulate_on_device is False
        assert DetectionBuffer(240, 320, cc.CLASSES).accumulate_on_device is False
    finally:
        testing.accumulate_on_device(False)
    assert DetectionBuffer(240, 320, cc.CLASSES, on_device=True, accumulate_on_device=True).accumulate_on_device is True


def test_argument_checks_of_the_entry_point():
    """Rejected on the host before any device work, so this runs without a GPU."""
    L = _lib.lib()
    tile = ce.accumulate_tile()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dagr_hip.h")).read()
    assert f"#define DAGR_COCO_ACC_TILE {tile}\n" in header and tile % 64 == 0
    need = L.dagr_coco_accumulate_workspace_bytes(10, 5000)
    assert need >= 10 * 5000
    assert L.dagr_coco_accumulate_workspace_bytes(10, -1) == 0 and b"bad size" in L.dagr_last_error()
    assert L.dagr_coco_accumulate_workspace_bytes(17, 8) == 0
    one = ctypes.c_void_p(16)     # non-NULL, aligned, never dereferenced
    eps = float(np.spacing(1))

    def call(n_rec=101, n_thr=10, n_groups=8, n_cols=5000, ws=need, status=one, perm=one, eps=eps):
        return L.dagr_coco_accumulate(one, one, perm, one, one, one, n_rec, eps, n_thr, n_groups, n_cols, one, ws, one, status,
                                      None)
    assert call(ws=need - 1) == -1 and b"workspace" in L.dagr_last_error()
    assert call(n_rec=129) != 0 and b"recall points" in L.dagr_last_error()
    assert call(n_rec=0) != 0
    assert call(n_thr=17) != 0 and b"thresholds" in L.dagr_last_error()
    assert call(n_cols=-1) != 0 and b"bad sizes" in L.dagr_last_error()
    assert call(n_cols=1 << 31) != 0 and b"bad sizes" in L.dagr_last_error()
    assert call(status=None) != 0 and b"NULL" in L.dagr_last_error()
    assert call(perm=None) != 0 and b"NULL" in L.dagr_last_error()
    assert call(perm=ctypes.c_void_p(18)) != 0 and b"aligned" in L.dagr_last_error()
    assert call(eps=0.0) != 0 and b"eps" in L.dagr_last_error()
