"""The image branch with the layers that the selection rule (engine._split_min_rows) hands to the split-bf16 MFMA kernel
(csrc/gemm_split_bf16.hip): the engine says which path every folded convolution took, the maps stay within the image
branch's bar of the plain eval-mode modules, and a captured window replays to the eager launches' bits."""
import pytest
import torch

from dagr_amd.utils import synthetic as syn
from tests.test_engine_gpu import _dev_window, _setup

pytestmark = pytest.mark.gpu

W, H, B = 320, 215, 2


@pytest.fixture(scope="module")
def rig():
    args, model, sd = _setup(W, H, B, seed=8, use_image=True, img_net="resnet50")
    return model, model.engine()


def test_selected_layers_run_the_split_kernel_and_the_maps_match_the_modules(rig):
    model, eng = rig
    image = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(5)).cuda()
    assert eng.image_branch_paths() == {}, "no layer has run yet"
    with torch.no_grad():
        feats, cnn_out = eng._image_branch(image)
        feats_ref, outs_ref = model.backbone.net(image)
        outs_ref = outs_ref[-eng.num_scales:]
        resized = [torch.nn.functional.interpolate(f, o) for f, o in zip(outs_ref, eng.out_sizes)]
        cnn_ref = model.head.cnn_head(resized)
    paths = eng.image_branch_paths()
    split = sorted(n for n, p in paths.items() if p == "split")
    print(f"split-bf16 layers at {W}x{H}, B = {B}: {split}")
    assert set(paths.values()) <= {"split", "library"}
    one_by_one = [n for n in split if not n.endswith("conv2")]
    assert one_by_one, f"no 1x1 convolution ran on the split kernel: {paths}"
    # (no 3x3 runs on it at this size: the rule takes layer2's only from 32 768 output pixels up -- the test below)
    assert not [n for n in split if n.endswith("conv2")]
    assert "library" in paths.values(), "layer1 and the narrow dconvs stay with the library"
    worst = 0.0
    pairs = list(zip(feats, feats_ref)) + [(a, b) for k in cnn_ref for a, b in zip(cnn_out[k], cnn_ref[k])]
    assert len(pairs) > len(feats)
    for a, b in pairs:
        scale = max(1.0, float(b.abs().max()))
        worst = max(worst, float((a - b).abs().max()) / scale)
        assert float((a - b).abs().max()) <= 2e-4 * scale
    print(f"largest |engine - modules| / max(1, max |modules|) = {worst:.2e}")


def test_a_captured_window_with_the_image_branch_replays_to_the_eager_bits():
    """The window with the image branch inside, captured and replayed, against the launch-by-launch path of the same engine:
    the same bits.  The split kernel has no atomics and nothing that depends on how it is launched, but the stride-2 3x3
    convolutions beside it stay with the library, whose default kernels split K with atomic adds: two EAGER image branches of
    one engine already differ from `layer2.0.conv2` (a library layer) on, with the split layers in or out, and so do two
    replays (measured: max |difference| 1.7e2 - 3.2e2 on outputs up to 3.4e7, i.e. 1e-5 relative).  The comparison therefore
    asks the library for its deterministic kernels (torch.backends.cudnn.deterministic) on a model and an engine of its own;
    what is left to differ is the split kernel and the capture."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        args, model, sd = _setup(W, H, B, seed=8, use_image=True, img_net="resnet50")
        eng = model.engine().set_low_latency(True)
        win = _dev_window(syn.uniform_window, 3000, B, W, H, 51)
        img = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(7)).cuda()
        with torch.no_grad():
            eager = eng.forward_raw(*win, image=img, trace={}).clone()
            for _ in range(5):                      # two warm-up windows, the capture, then replays
                replay = eng.forward_raw(*win, image=img).clone()
        assert eng._wg is not None, "the window was not captured"
        eng.check_status()
        n_split = sum(p == "split" for p in eng.image_branch_paths().values())
        print(f"captured window with {n_split} split-bf16 layers: max |replay - eager| = {float((replay - eager).abs().max()):.3e}")
        assert n_split >= 1
        assert torch.equal(replay, eager), f"max |replay - eager| = {float((replay - eager).abs().max()):.3e}"
    finally:
        torch.backends.cudnn.deterministic = before


def test_a_3x3_convolution_runs_the_split_kernel_where_the_rule_selects_it():
    """layer2's stride-1 3x3 convolutions (C = 128) are selected from 32 768 output pixels: B = 7 at 640 x 480 is 33 600.
    Trunk only (the stages' maps against the plain modules), one forward each."""
    from dagr_amd import engine as E
    Wf, Hf, Bf = 640, 480, 7
    args, model, sd = _setup(Wf, Hf, Bf, seed=9, use_image=True, img_net="resnet50")
    eng = model.engine()
    image = torch.rand((Bf, 3, Hf, Wf), generator=torch.Generator().manual_seed(6)).cuda()
    with torch.no_grad():
        feats, _ = eng._image_branch(image)
        feats_ref, _ = model.backbone.net(image)
    paths = eng.image_branch_paths()
    three = sorted(n for n, p in paths.items() if p == "split" and n.endswith("conv2"))
    print(f"split-bf16 3x3 layers at {Wf}x{Hf}, B = {Bf}: {three}")
    assert three and all(n.startswith("module.layer2.") for n in three), paths
    assert E._split_min_rows(128, 128, 9) <= Bf * 60 * 80
    for a, b in zip(feats, feats_ref):
        assert float((a - b).abs().max()) <= 2e-4 * max(1.0, float(b.abs().max()))
