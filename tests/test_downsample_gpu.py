"""Device event downsampler (dagr.data.downsample.downsample_events, csrc/downsample.hip) against the restated reference
loop (oracle/downsample.py <- scripts/downsample_events.py:91-124): same surviving events, same integrator state, over
two consecutive chunks that share the change map (the way the reference streams a recording); at cell areas that are no
power of two, against the reference script's own recorded outputs (tests/golden/ref_py_downsample_factors.npz); and the
refusal of an event outside the cell grid."""
import numpy as np
import pytest
import torch

from oracle import downsample as od
from dagr_amd.utils import synthetic as syn
from tests import downsample_factor_cases as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("factor,stream", [(2, "edges"), (2, "uniform"), (4, "edges")])
def test_downsample_matches_reference_loop(factor, stream):
    from dagr_amd.data.downsample import downsample_events
    W, H = 640, 480
    Wo, Ho = W // factor, H // factor
    gen = syn.edges_window if stream == "edges" else syn.uniform_window
    cm_o = cm_d = None
    for chunk in range(2):
        x, y, t, p = gen(60000, W, H, seed=90 + chunk)
        ev = dict(x=x.astype(np.int64), y=y.astype(np.int64), t=t.astype(np.int64), p=p.astype(np.int8))
        want, cm_o = od.downsample_events({k: v.copy() for k, v in ev.items()}, H, W, Ho, Wo, change_map=cm_o)
        dev = {k: torch.from_numpy(v).cuda() for k, v in ev.items()}
        got, cm_d = downsample_events(dev, H, W, Ho, Wo, change_map=cm_d)
        assert len(want["t"]) > 5
        for k in ("x", "y", "t", "p"):
            assert np.array_equal(got[k].cpu().numpy().astype(np.int64), want[k].astype(np.int64)), (chunk, k)
        assert np.array_equal(cm_d.cpu().numpy(), cm_o)


@pytest.mark.parametrize("fx,fy", fc.CASES, ids=fc.IDS)
def test_downsample_equals_the_reference_script_at_areas_that_are_no_power_of_two(fx, fy):
    """k_downsample_cells against what the reference's own scripts/downsample_events.py kept and left in its change map
    (tests/golden/ref_py_downsample_factors.npz), bit for bit, over two chunks on the carried device map: at areas 3, 6, 9,
    12, 15 and 25 the reference's float64 quotient ``p * 1.0 / (fx * fy)`` and an increment rounded to fp32 first part ways
    (tests/test_downsample_factors_cpu.py); 2x2 is the control."""
    from dagr_amd.data.downsample import downsample_events
    fc.check_inputs(fx, fy)
    cm = None
    for c, (ev, (mask, sv, want_map)) in enumerate(zip(fc.chunks(fx, fy), fc.expected(fx, fy))):
        dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in ev.items()}
        dev["i"] = torch.arange(len(ev["t"]), device="cuda")
        got, cm = downsample_events(dev, fc.CH * fy, fc.CW * fx, fc.CH, fc.CW, change_map=cm)
        got_mask = np.zeros(len(mask), bool)
        got_mask[got["i"].cpu().numpy()] = True
        print(f"{fx}x{fy} chunk {c}: kept flags that differ {int((got_mask != mask).sum())}, "
              f"cells that differ {int((cm.cpu().numpy() != want_map).sum())}")
        assert np.array_equal(got_mask, mask), c
        for k in ("x", "y", "t", "p"):
            assert np.array_equal(got[k].cpu().numpy().astype(np.int64), sv[k].astype(np.int64)), (c, k)
        assert cm.dtype == torch.float32 and np.array_equal(cm.cpu().numpy(), want_map), c


def test_an_event_outside_the_cell_grid_is_refused_by_name_and_nothing_runs():
    """640 -> 213 at fx = 3: x = 639 lies in the strip right of the last whole cell (x // 3 = 213), where the reference's loop
    raises IndexError; unchecked, the event would alias into the next row's first cell, and below the last row write past the
    end of the map.  The route refuses before its launch and names the first such event; the map is as it was."""
    from dagr_amd.data.downsample import downsample_events
    x = np.array([5, 638, 17, 639, 639, 2], np.int64)
    y = np.array([7, 8, 479, 100, 479, 3], np.int64)
    ev = dict(x=x, y=y, t=np.arange(6, dtype=np.int64) * 10, p=np.array([1, -1, 1, 1, -1, 1], np.int8))
    with pytest.raises(IndexError):
        od.downsample_events({k: v.copy() for k, v in ev.items()}, 480, 640, 160, 213)
    dev = {k: torch.from_numpy(v).cuda() for k, v in ev.items()}
    cm = torch.rand((160, 213), device="cuda")
    before = cm.clone()
    with pytest.raises(ValueError, match=r"event 3 \(x = 639, y = 100\).*cell \(213, 33\).*213 x 160"):
        downsample_events(dev, 480, 640, 160, 213, change_map=cm)
    assert torch.equal(cm, before)
    dev["y"][3:5] = torch.tensor([100, 100], device="cuda")
    dev["x"][3:5] = torch.tensor([0, 0], device="cuda")
    dev["y"][2] = 481                                           # below the last row of a 160-row map: cell row 160
    with pytest.raises(ValueError, match=r"event 2 \(x = 17, y = 481\)"):
        downsample_events(dev, 483, 640, 160, 213, change_map=cm)
    dev["x"][0] = -1                                            # and left of the first cell
    with pytest.raises(ValueError, match=r"event 0 \(x = -1, y = 7\)"):
        downsample_events(dev, 483, 640, 160, 213, change_map=cm)
    assert torch.equal(cm, before)


def test_downsample_script_on_the_device_matches_the_reference_main_loop(tmp_path):
    """scripts/downsample_events.py end to end with the device kernel: 230 123 events in three chunks (the last one partial,
    with the reference's {0, 1} polarities), the change map resident on the GPU in between -> the digests of the reference
    script's own main loop (tests/golden/ref_py_data.npz)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    import downsample_events as D
    from tests.test_data_refpy import G, _check_stream_output, _stream_case
    dst = tmp_path / "events_2x.npz"
    counts = D.main(["--input_path", str(_stream_case(tmp_path)), "--output_path", str(dst), "--input_height", "48",
                     "--input_width", "64", "--output_height", "24", "--output_width", "32"])
    assert counts["t"] == int(G["stream_count"])
    _check_stream_output(dst)
