"""Level-0 widths 8 / 16 / 32 without a GPU: the engine's weight packing for the tiled level-0 conv against a direct
einsum of the module's weights, and the width-aware entry points in header, library and bindings."""
import os
import re

import pytest
import torch

from oracle import model as om
from dagr_amd.utils.testing_weights import randomize_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dagr_spline_conv_l0_tiles_w", "dagr_spline_conv_l0_tiles_rows_w", "dagr_async_update_w")


def _bn(norm):
    m = norm.module
    scale = m.weight / torch.sqrt(m.running_var + m.eps)
    return scale, m.bias - m.running_mean * scale


@pytest.mark.parametrize("use_image", [False, True])
@pytest.mark.parametrize("bw", [0.25, 0.5, 1.0])
def test_pack_l0_rows_are_the_modules_weights_with_bn_folded(bw, use_image):
    from dagr_amd.engine import _l0_block, _pack_l0
    from dagr_amd.model.networks.dagr import DAGR
    c = int(bw * 32)
    args = om.default_args(base_width=bw, use_image=use_image, img_net="resnet18")
    model = randomize_(DAGR(args, height=215, width=320), seed=3).eval().double()
    l0 = model.backbone.conv_block1
    nf = c if use_image else 0
    cols = list(range(1, 1 + nf)) + [0, 1 + nf, 2 + nf]        # the engine's row: [image feats | polarity | pos_xy]
    assert _l0_block(len(cols)) == (nf, 3) and _l0_block(c) == (c, 0)
    win = (1, 3, 0, 5)
    taps = [(1 + a) + 5 * b for b in range(5) for a in range(3)]
    g = torch.Generator().manual_seed(c)
    with torch.no_grad():
        # first conv: tap sums A[tap, channel] and the node's own row, in the reference's channel order
        conv, norm = l0.conv_block1.conv, l0.conv_block1.norm
        cin = conv.weight.shape[1]
        A, xr = torch.randn((15, cin), generator=g).double(), torch.randn((cin,), generator=g).double()
        scale, shift = _bn(norm)
        want = (torch.einsum("tc,tco->o", A, conv.weight[taps]) + conv.lin.weight @ xr) * scale + shift
        k, cskip, w, s = _pack_l0(conv, norm, win, device="cpu", cols_in=cols)
        assert (k, cskip) == (cin, 0) and tuple(w.shape) == (16 * cin, c) and tuple(s.shape) == (c,)
        got = torch.cat([A[:, cols].reshape(-1), xr[cols]]) @ w.double() + s.double()
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)
        # second conv + skip Linear on the (permuted) input row
        blk = l0.conv_block2
        A, xr = torch.randn((15, c), generator=g).double(), torch.randn((c,), generator=g).double()
        xs = torch.randn((cin,), generator=g).double()
        scale, shift = _bn(blk.norm)
        s_scale, s_shift = _bn(blk.norm_skip)
        want = (torch.einsum("tc,tco->o", A, blk.conv.weight[taps]) + blk.conv.lin.weight @ xr) * scale + shift \
            + (blk.lin.mlp.weight @ xs) * s_scale + s_shift
        k, cskip, w, s = _pack_l0(blk.conv, blk.norm, win, skip=(blk.lin, blk.norm_skip), device="cpu", cols_skip=cols)
        assert (k, cskip) == (c, cin) and tuple(w.shape) == (16 * c + cin, c)
        got = torch.cat([A.reshape(-1), xr, xs[cols]]) @ w.double() + s.double()
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)


def test_pack_l0_refuses_other_widths_and_names_the_supported_ones():
    from dagr_amd.engine import _pack_l0
    from dagr_amd.model.networks.dagr import DAGR
    model = DAGR(om.default_args(base_width=0.75), height=215, width=320)
    l0 = model.backbone.conv_block1
    with pytest.raises(NotImplementedError, match="8, 16, 32"):
        _pack_l0(l0.conv_block1.conv, l0.conv_block1.norm, (1, 3, 0, 5), device="cpu")


def test_width_entry_points_declared_exported_and_bound():
    from dagr_amd import _lib
    header = open(os.path.join(ROOT, "include", "dagr_hip.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert "{8, 16, 32}" in header
    # argument lists: the 16-column entry points' with the width in front (behind the argument block for the update)
    for old in ("dagr_spline_conv_l0_tiles", "dagr_spline_conv_l0_tiles_rows"):
        assert _lib.SIGNATURES[old + "_w"][1][1:] == _lib.SIGNATURES[old][1]
    assert len(_lib.SIGNATURES["dagr_async_update_w"][1]) == len(_lib.SIGNATURES["dagr_async_update"][1]) + 1
