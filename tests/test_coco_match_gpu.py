"""The COCO-protocol matcher on the device (csrc/coco_match.hip: dagr_coco_match; utils/coco_eval.py; DetectionBuffer(on_device=True))
against the host evaluator on the cases of tests/coco_cases.py.  Everything is compared exactly: both paths feed the same
booleans to the same numpy accumulation, so the metrics are the same floats, not close ones."""
import functools

import numpy as np
import pytest
import torch

from tests import coco_cases as cc
from dagr_amd.utils import coco_eval as ce
from dagr_amd.utils.buffers import DetectionBuffer

pytestmark = pytest.mark.gpu
MAX_GT = 256                                   # DAGR_COCO_MAX_GT (tests/test_coco_match_cpu.py holds it to the header)


@functools.lru_cache(maxsize=None)
def case(name):
    """(ground truth, detections, job list, host matches per job, host metrics) -- computed once per case, never changed."""
    if name.startswith("crowded"):
        gts, dts = cc.crowded(int(name[len("crowded"):]))
    else:
        gts, dts = cc.random_sweep() if name == "sweep" else cc.small_cases()[name]
    jobs = ce.build_jobs(ce.evaluated_images(gts, dts), len(cc.CLASSES))
    with np.errstate(invalid="ignore"):
        return gts, dts, jobs, ce.match_jobs_host(jobs), ce.evaluate_detection(gts, dts, classes=cc.CLASSES)


IN_BOUNDS = sorted(cc.small_cases()) + [f"crowded{MAX_GT}", "sweep"]


@pytest.mark.parametrize("name", IN_BOUNDS)
def test_every_job_equals_the_host_matcher(name):
    gts, dts, jobs, want, _ = case(name)
    assert ce.device_bounds()[0] == MAX_GT
    got = ce.coco_match_device(jobs, np.arange(len(jobs)), torch.device("cuda", 0))
    assert sorted(got) == sorted(want) == list(range(len(jobs))) and len(jobs) > 0
    for j in range(len(jobs)):
        order, dtm, dt_ign, g_ign = got[j]
        scores, w_dtm, w_dt_ign, w_g_ign = want[j]
        _, _, s, _ = jobs.arrays(j)
        assert np.array_equal(order, np.argsort(-s, kind="mergesort")[:ce.MAX_DETS]), (name, j)
        assert np.array_equal(s[order], scores)
        assert dtm.dtype == np.bool_ and dtm.shape == w_dtm.shape and np.array_equal(dtm, w_dtm), (name, j)
        assert dt_ign.shape == w_dt_ign.shape and np.array_equal(dt_ign, w_dt_ign), (name, j)
        assert g_ign.shape == w_g_ign.shape and np.array_equal(g_ign, w_g_ign), (name, j)


@pytest.mark.parametrize("name", IN_BOUNDS + [f"crowded{MAX_GT + 1}"])
def test_metrics_on_device_are_the_host_floats(name):
    gts, dts, jobs, _, want = case(name)
    stats = {}
    got = ce.evaluate_detection(gts, dts, classes=cc.CLASSES, on_device=True, stats=stats)
    assert got == want and list(got) == list(want)
    over = name == f"crowded{MAX_GT + 1}"
    assert stats["host_fallback_jobs"] == (1 if over else 0)
    assert stats["device_jobs"] == (0 if over else len(jobs))


def test_the_sweep_and_the_cut_are_not_vacuous():
    _, _, jobs, matched, out = case("sweep")
    assert all(0.0 < out[k] < 1.0 for k in ce.OUT_KEYS), out
    for ai in range(len(ce.AREA_RNG)):
        assert any(jobs.table[j, 1] > 0 and jobs.table[j, 3] > 0 for j in range(len(jobs)) if jobs.key[j, 1] == ai)
    _, dts, jobs, matched, _ = case(f"crowded{MAX_GT}")
    assert jobs.table[0, 1] == MAX_GT and jobs.table[0, 3] > ce.MAX_DETS and matched[0][1].shape[1] == ce.MAX_DETS


def test_a_job_beyond_the_bound_is_an_argument_error():
    _, _, jobs, _, _ = case(f"crowded{MAX_GT + 1}")
    with pytest.raises(RuntimeError, match="does not fit"):
        ce.coco_match_device(jobs, np.arange(len(jobs)), torch.device("cuda", 0))


# ---- DetectionBuffer(on_device=True) ---------------------------------------------------------------------------------
def _on(device, dicts):
    return [{k: v.to(device) for k, v in d.items()} for d in dicts]


def _feed(buffer, gts, dts, device, how, batch=8):
    """The images in batches of eight, inputs on the device beforehand; no call of ``update*`` may synchronise."""
    batches = []
    for b0 in range(0, len(gts), batch):
        g, d = _on(device, gts[b0:b0 + batch]), dts[b0:b0 + batch]
        batches.append((g, cc.forward_detections_form(d, device) if how == "update_device" else _on(device, d),
                        list(range(b0, b0 + len(g)))))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for g, d, ids in batches:
            if how == "update_device":
                buffer.update_device(d[0], d[1], g, image_ids=ids)
            else:
                buffer.update(d, g, image_ids=ids)
    finally:
        torch.cuda.set_sync_debug_mode(mode)


@pytest.mark.parametrize("name", ["sweep", "empties", f"crowded{MAX_GT + 1}"])
def test_detection_buffer_on_device_equals_the_host_buffer(name):
    gts, dts, _, _, want = case(name)
    device = torch.device("cuda", 0)
    host = DetectionBuffer(240, 320, cc.CLASSES)
    host.update(dts, gts)
    sequences, stamps = [f"seq{i % 3}" for i in range(len(gts))], [1000 * i for i in range(len(gts))]
    w_det, w_gt = host.compile(sequences, stamps)
    want_map = host.compute(gather=False)
    assert want_map == {k.replace("AP", "mAP"): v for k, v in want.items()}
    for how in ("update", "update_device"):
        buf = DetectionBuffer(240, 320, cc.CLASSES, on_device=True)
        _feed(buf, gts, dts, device, how)
        g_det, g_gt = buf.compile(sequences, stamps)
        assert sorted(g_det) == sorted(w_det) and sorted(g_gt) == sorted(w_gt)
        for k in w_det:
            assert g_det[k].dtype == w_det[k].dtype and np.array_equal(g_det[k], w_det[k]), (how, k)
            assert g_gt[k].dtype == w_gt[k].dtype and np.array_equal(g_gt[k], w_gt[k]), (how, k)
        assert buf.compute(gather=False) == want_map, how
        assert buf.last_host_fallback_jobs == (1 if name == f"crowded{MAX_GT + 1}" else 0)
        assert buf.image_ids == [] and buf.compute(gather=False) == {k.replace("AP", "mAP"): 0 for k in ce.OUT_KEYS}


def test_update_device_needs_the_device_buffer():
    gts, dts, _, _, _ = case("ties")
    det, n_keep = cc.forward_detections_form(dts, torch.device("cuda", 0))
    with pytest.raises(RuntimeError, match="on_device"):
        DetectionBuffer(240, 320, cc.CLASSES).update_device(det, n_keep, gts)
