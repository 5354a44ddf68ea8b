"""The image branch's trunk at the size the benchmark's step runs it (640 x 480, B = 8): every folded convolution whose
(M, K, N, taps) the selection rule (engine._split_min_rows) admits reports the split-bf16 kernel, and every feature map stays
within the image branch's bar of the plain eval-mode modules."""
import pytest
import torch

from tests.test_engine_gpu import _setup

pytestmark = pytest.mark.gpu

W, H, B = 640, 480, 8


def test_every_layer_the_rule_selects_runs_the_split_kernel_at_the_benchmark_size():
    from dagr_amd import engine as E
    args, model, sd = _setup(W, H, B, seed=10, use_image=True, img_net="resnet50")
    eng = model.engine()
    image = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        feats, _ = eng._image_branch(image)
        feats_ref, _ = model.backbone.net(image)
    paths = eng.image_branch_paths()
    mods = dict(eng._net_f.named_modules())
    expected = {}
    for name in paths:
        parts = name.split(".")                     # module.layerL.block.conv
        if len(parts) < 4 or not parts[1].startswith("layer"):
            continue
        level, block, m = int(parts[1][5:]), int(parts[2]), mods[name]
        down = 2 ** (level + 1)                     # the layer's output is the image / 4, 8, 16, 32
        if block == 0 and level > 1 and parts[3] == "conv1":
            down //= 2                              # the first block's conv1 still runs at the layer's input size
        rows = B * (H // down) * (W // down)
        if isinstance(m, E._Conv1x1Gemm):
            K, N = m.wt.shape
            least = E._split_min_rows(K, N, 1)
        elif isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (1, 1):
            least = E._split_min_rows(m.in_channels, m.out_channels, 9)
        else:
            continue
        if least is not None and rows >= least:
            expected[name] = rows
    print(f"the rule selects {len(expected)} of {len(paths)} layers at {W}x{H}, B = {B}: {sorted(expected)}")
    assert expected, "the rule selects nothing at the benchmark's size"
    wrong = sorted(n for n in expected if paths[n] != "split")
    assert not wrong, f"selected by the rule, run by the library: {wrong}"
    worst = 0.0
    for a, b in zip(feats, feats_ref):
        scale = max(1.0, float(b.abs().max()))
        worst = max(worst, float((a - b).abs().max()) / scale)
        assert float((a - b).abs().max()) <= 2e-4 * scale
    print(f"largest |engine - modules| / max(1, max |modules|) = {worst:.2e}")
