"""CPU suite of the device evaluation path (utils/coco_eval.py: build_jobs / match_jobs_* / evaluate_detection(on_device=True)):
the job list and the reassembly around the matcher, with the matcher stubbed by the host's ``_evaluate_image``; the
cases of tests/coco_cases.py say what their docstrings say; the bounds of ``dagr_coco_match``."""
import ctypes
import os

import numpy as np
import pytest

from tests import coco_cases as cc
from dagr_amd import _lib
from dagr_amd.utils import coco_eval as ce

ALL = dict(cc.small_cases(), crowded=cc.crowded(40), sweep=cc.random_sweep())


@pytest.fixture
def host_matcher(monkeypatch):
    """``evaluate_detection(on_device=True)`` with ``_evaluate_image`` in the place of the kernel; counts the calls of
    ``_accumulate``, which has to stay the function the host path uses."""
    calls = {"match": 0, "accumulate": 0}
    accumulate = ce._accumulate

    def match(jobs, device=None, stats=None):
        calls["match"] += 1
        return ce.match_jobs_host(jobs)

    def counted(per_image):
        calls["accumulate"] += 1
        return accumulate(per_image)
    monkeypatch.setattr(ce, "match_jobs_device", match)
    monkeypatch.setattr(ce, "_accumulate", counted)
    return calls


@pytest.mark.parametrize("name", sorted(ALL))
def test_job_list_and_reassembly_give_the_host_result(name, host_matcher):
    gts, dts = ALL[name]
    with np.errstate(invalid="ignore"):
        want = ce.evaluate_detection(gts, dts, classes=cc.CLASSES)
        n_host = host_matcher["accumulate"]
        got = ce.evaluate_detection(gts, dts, classes=cc.CLASSES, on_device=True)
    assert got == want and list(got) == list(want)
    assert host_matcher["match"] == 1
    # the host path accumulates every (class, area range); the job path those that have a job: the same function
    assert n_host == len(cc.CLASSES) * len(ce.AREA_RNG) and 0 < host_matcher["accumulate"] - n_host <= n_host


def test_job_list_is_the_non_empty_calls_of_the_matcher():
    gts, dts = cc.empties()
    images = ce.evaluated_images(gts, dts)
    assert len(images) == 3                                            # the image without ground truth is not evaluated
    jobs = ce.build_jobs(images, len(cc.CLASSES))
    want = [(c, ai, i) for c in range(2) for ai in range(len(ce.AREA_RNG)) for i, (g, gl, d, dl, s) in enumerate(images)
            if (gl == c).sum() + (dl == c).sum() > 0]
    assert [tuple(k) for k in jobs.key.tolist()] == want
    assert (0, 0, 2) not in want and (0, 0, 0) in want and (0, 0, 1) in want      # class 0: image 2 has neither
    for j, (c, ai, i) in enumerate(want):
        g, gl, d, dl, s = images[i]
        gj, dj, sj, rng = jobs.arrays(j)
        assert np.array_equal(gj, g[gl == c]) and np.array_equal(dj, d[dl == c]) and np.array_equal(sj, s[dl == c])
        assert list(rng) == list(ce.AREA_RNG[ai])
    # the four area ranges of an (image, class) share one copy of its boxes
    assert len(jobs.gt) == sum(len(im[0]) for im in images) and len(jobs.dt) == sum(len(im[2]) for im in images)


def test_no_detection_at_all_is_zeros_on_both_paths(host_matcher):
    gts, dts = cc.empties()
    none = [{"boxes": d["boxes"][:0], "labels": d["labels"][:0], "scores": d["scores"][:0]} for d in dts]
    assert ce.evaluate_detection(gts, none, classes=cc.CLASSES, on_device=True) == {k: 0 for k in ce.OUT_KEYS}
    assert host_matcher["match"] == 0


def test_the_cases_are_what_they_say():
    def jobs_of(case):
        jobs = ce.build_jobs(ce.evaluated_images(*case), 2)
        with np.errstate(invalid="ignore"):
            return jobs, ce.match_jobs_host(jobs)
    thr = ce.IOU_THRS
    # ties: detection 0 takes the LATER of two equal candidates, so detection 1 still finds A; equal scores keep their order
    jobs, res = jobs_of(cc.ties())
    j = [tuple(k) for k in jobs.key.tolist()].index((0, 0, 0))
    g, d, s, _ = jobs.arrays(j)
    iou = ce._iou_xywh(d, g)
    assert iou[0, 0] == iou[0, 1] == 0.6 and iou[1, 0] == 1.0 and iou[1, 1] == 200 / 600
    assert res[j][1][0].tolist() == [True, True] and res[j][1][3].tolist() == [False, True]      # thr 0.5 / 0.65
    j = [tuple(k) for k in jobs.key.tolist()].index((1, 0, 1))
    assert res[j][0].tolist() == [0.5, 0.5, 0.25] and res[j][1][0].tolist() == [False, True, False]
    # exact thresholds: 0.5 and 0.75 are hit exactly, and `>=` matches there and not one threshold later
    jobs, res = jobs_of(cc.exact_thresholds())
    keys = [tuple(k) for k in jobs.key.tolist()]
    for image, value in ((0, 0.5), (1, 0.75)):
        g, d, s, _ = jobs.arrays(keys.index((0, 0, image)))
        assert ce._iou_xywh(d, g)[0, 0] == value
        assert res[keys.index((0, 0, image))][1][:, 0].tolist() == [bool(min(t, 1 - 1e-10) <= value) for t in thr]
    assert res[keys.index((0, 0, 0))][1][:, 0].sum() == 1
    # break rule (medium range): matched at every threshold up to 0.9 -- to the evaluated box while it reaches the threshold,
    # then to the ignored one
    jobs, res = jobs_of(cc.break_rule())
    _, dtm, dt_ign, g_ign = res[[tuple(k) for k in jobs.key.tolist()].index((0, 2, 0))]
    assert g_ign.tolist() == [False, True]
    assert dtm[:, 0].tolist() == [t <= 0.9 for t in thr] and dt_ign[:, 0].tolist() == [2 / 3 < t <= 0.9 for t in thr]
    # out of range: in the medium range the only ground truth is ignored and the detection is matched to it
    jobs, res = jobs_of(cc.out_of_range())
    _, dtm, dt_ign, g_ign = res[[tuple(k) for k in jobs.key.tolist()].index((0, 2, 0))]
    assert g_ign.tolist() == [True] and dtm.all() and dt_ign.all()
    # degenerate: a NaN IoU is really there
    jobs, _ = jobs_of(cc.degenerate())
    g, d, s, _ = jobs.arrays(0)
    with np.errstate(invalid="ignore"):
        assert np.isnan(ce._iou_xywh(d, g)).any()


def test_the_sweep_is_not_vacuous():
    gts, dts = cc.random_sweep()
    assert len(gts) == 64 and max(len(g["boxes"]) for g in gts) <= 12 and max(len(d["boxes"]) for d in dts) <= 40
    out = ce.evaluate_detection(gts, dts, classes=cc.CLASSES)
    for k in ce.OUT_KEYS:
        assert 0.0 < out[k] < 1.0, (k, out[k])
    jobs = ce.build_jobs(ce.evaluated_images(gts, dts), 2)
    res = ce.match_jobs_host(jobs)
    for ai in range(len(ce.AREA_RNG)):
        mine = [res[j] for j in range(len(jobs)) if jobs.key[j, 1] == ai]
        # per area range: evaluated ground truth, and detections both matched and unmatched, at the first and last threshold
        assert sum((~e[3]).sum() for e in mine) > 0
        for t in (0, len(ce.IOU_THRS) - 1):
            counted = [(e[1][t] & ~e[2][t]).sum() for e in mine], [(~e[1][t] & ~e[2][t]).sum() for e in mine]
            assert sum(counted[0]) > 0 and sum(counted[1]) > 0, (ai, t)


def test_bounds_and_argument_checks_of_the_entry_point():
    """Rejected on the host before any device work, so this runs without a GPU."""
    L = _lib.lib()
    max_g, max_d = ce.device_bounds()
    assert (max_g, max_d) == (256, 4096)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dagr_hip.h")).read()
    assert f"#define DAGR_COCO_MAX_GT {max_g}\n" in header and f"#define DAGR_COCO_MAX_DT {max_d}\n" in header
    one = ctypes.c_void_p(16)     # non-NULL, aligned, never dereferenced

    def call(n_thr=10, max_dets=100, n_jobs=1, g=1, d=1, status=one, jobs=one):
        return L.dagr_coco_match(one, one, one, jobs, one, one, n_thr, max_dets, n_jobs, 8, 8, g, d, 8, 8, one, one, one, one,
                                 status, None)
    assert call(g=max_g + 1) != 0 and b"ground truth does not fit" in L.dagr_last_error()
    assert call(d=max_d + 1) != 0 and b"DAGR_COCO_MAX_DT" in L.dagr_last_error()
    assert call(n_thr=17) != 0 and b"thresholds" in L.dagr_last_error()
    assert call(n_thr=0) != 0
    assert call(max_dets=101) != 0 and b"max_dets" in L.dagr_last_error()
    assert call(n_jobs=-1) != 0 and b"bad sizes" in L.dagr_last_error()
    assert call(status=None) != 0 and b"NULL" in L.dagr_last_error()
