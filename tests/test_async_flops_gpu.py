"""FLOP accounting on the device (dagr_async_flops): evaluate_flops(dense=True) on the HIP path reproduces the counts of
the reference's own evaluate_flops (tests/golden/ref_py_flops.json) as integers, key by key; accounting leaves the
outputs alone; scripts/count_flops.py writes flops_per_layer.pth."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "ref_py_flops.json")) as f:
    GOLDEN = json.load(f)


class _Batch:
    pass


def _setup(c):
    from oracle import model as om
    from dagr_amd.model.networks.dagr import DAGR
    from dagr_amd.utils import synthetic as syn
    from dagr_amd.utils.testing_weights import randomize_
    W, H, B = c["W"], c["H"], c["B"]
    args = om.default_args(batch_size=B, **c["overrides"])
    torch.manual_seed(c["seed"])
    model = randomize_(DAGR(args, height=H, width=W), seed=c["seed"]).eval().cuda()
    model.cache_luts(width=W, height=H, radius=args.radius)
    ev = {k: np.asarray(v) for k, v in c["events"].items()}
    d = _Batch()
    d.pos = torch.from_numpy(syn.format_data_np(ev["x"], ev["y"], ev["t"], W, H)).cuda()
    d.x = torch.from_numpy(ev["p"].astype(np.float32)).view(-1, 1).cuda()
    d.batch = torch.from_numpy(ev["b"].astype(np.int64)).cuda()
    d.width, d.height, d.time_window = torch.tensor([W] * B), torch.tensor([H] * B), torch.tensor([1000000] * B)
    d.num_graphs = B
    if getattr(args, "use_image", False):
        d.image = (torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(c["seed"])).float()
                   / 255).cuda()
    return model, d


@pytest.mark.parametrize("case", sorted(GOLDEN["cases"]))
def test_dense_flops_equal_the_reference(case):
    from dagr.asynchronous.evaluate_flops import evaluate_flops
    c = GOLDEN["cases"][case]
    model, d = _setup(c)
    res = evaluate_flops(model, d, dense=True, return_all_samples=True)
    want = c["dense"]
    assert len(res["flops_per_layer_batch"]) == len(want["flops_per_layer_batch"])
    for got, ref in zip(res["flops_per_layer_batch"], want["flops_per_layer_batch"]):
        assert list(got) == list(ref) or sorted(got) == sorted(ref)
        for k in ref:
            assert isinstance(got[k], int) and got[k] == ref[k], (case, k, got[k], ref[k])
    assert dict(res["flops_per_layer"]) == want["flops_per_layer"]
    assert res["total_flops"] == want["total_flops"]


def _split_last(d):
    """evaluate_flops' split of a one-sample batch: every event but the last, then the last."""
    parts = []
    for sl in (slice(None, -1), slice(-1, None)):
        p = _Batch()
        p.pos, p.x, p.batch = d.pos[sl], d.x[sl], d.batch[sl]
        p.width, p.height, p.time_window, p.num_graphs = d.width, d.height, d.time_window, 1
        parts.append(p)
    return parts


def _same(dets_a, dets_b):
    assert len(dets_a) == len(dets_b)
    for a, b in zip(dets_a, dets_b):                     # one detections dict per image
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_accounting_leaves_window_and_update_outputs_unchanged():
    """An accounted window, then an incremental update of it: window and update outputs are bit-identical to the same
    two calls without accounting."""
    from dagr.asynchronous import make_model_asynchronous, make_model_synchronous
    c = GOLDEN["cases"]["s_oldvoxel_b1"]
    model, d = _setup(c)
    initial, new = _split_last(d)
    with torch.no_grad():
        make_model_asynchronous(model)
        win_plain = model.forward(initial, reset=True, return_targets=False)[0]
        upd_plain = model.forward(new, reset=False, return_targets=False)[0]
        make_model_asynchronous(model, log_flops=True)
        win_acc = model.forward(initial, reset=True, return_targets=False)[0]
        assert len(model.backbone.pool1.asy_flops_log) == 1
        make_model_synchronous(model)
        make_model_asynchronous(model)
        upd_acc = model.forward(new, reset=False, return_targets=False)[0]
    _same(win_plain, win_acc)
    _same(upd_plain, upd_acc)


def test_count_flops_script(tmp_path):
    from oracle import model as om
    from dagr_amd.model.networks.dagr import DAGR
    from dagr_amd.utils.testing_weights import randomize_
    model = randomize_(DAGR(om.default_args(batch_size=2), height=480, width=640), seed=5)
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema": model.state_dict()}, ckpt)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "count_flops.py"), "--config", "config/dagr-s-dsec.yaml",
           "--checkpoint", str(ckpt), "--batch_size", "2", "--output_directory", str(out), "--dense",
           "--windows", "2", "--events_per_window", "3000"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = torch.load(out / "flops_per_layer.pth")
    assert len(res) > 0 and sum(res.values()) > 0
