"""Training at the event-level widths 8 and 32 (``--base_width`` 0.25 / 1.0): loss and gradients of the HIP layers against
the oracle, on the smallest case and with the bars of
tests/test_training_gpu.py::test_training_loss_and_gradients_match_the_oracle (losses 5e-4, gradients 2e-3 of their scale)."""
import pytest
import torch

from dagr_amd.utils.buffers import format_data
from tests.test_training_gpu import _rel, _training_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bw", [0.25, 1.0])
def test_training_loss_and_gradients_match_the_oracle_at_other_event_widths(bw):
    from oracle import train as otr
    W, H, B = 240, 180, 2
    args, model, sd, batch, ev, b = _training_case(W, H, B, 2500, 1, base_width=bw)
    assert model.backbone.conv_block1.conv_block1.conv.weight.shape[2] == int(bw * 32)
    ref = otr.training_losses(sd, args, H, W, ev[0], ev[1], ev[2], ev[3], b, B, batch.bbox, batch.bbox_batch)
    ref[0].backward()
    out = model(format_data(batch.cuda()))
    assert out["num_fg"] == ref[5], "SimOTA matched a different number of anchors"
    for k, r in zip(("total_loss", "iou_loss", "conf_loss", "cls_loss"), (ref[0], ref[1], ref[2], ref[3])):
        print(k, float(out[k]), float(r))
        assert abs(float(out[k]) - float(r)) <= 5e-4 * max(1.0, abs(float(r))), (k, float(out[k]), float(r))
    out["total_loss"].backward()
    params = dict(model.named_parameters())
    checked, errs = 0, []
    for k, v in sd.items():
        if not v.requires_grad or v.grad is None:
            assert k not in params or params[k].grad is None or float(params[k].grad.abs().max()) == 0.0, k
            continue
        gh = params[k].grad
        assert gh is not None, f"no gradient reached {k}"
        errs.append((_rel(gh, v.grad), k))
        checked += 1
    assert checked >= 60
    errs.sort()
    print("largest gradient errors:", errs[-3:])
    assert errs[-1][0] < 2e-3, errs[-5:]
