"""SplineConv backward (training path, first slice): gradients of ``MySplineConv.forward`` w.r.t. x, weight[25, cin, cout],
the root weight and the bias -- tap aggregation + its transpose in HIP, the two weight-side contractions as library
GEMMs -- against autograd through a float64 evaluation of the op built on the oracle's torch_spline_conv basis.

The float64 reference aggregates taps first (``A[n, 25, cin]`` by ``index_add``, then one product with the weights): the
per-edge ``cin x cout`` weight gather of the op's textbook form does not fit at the dagr-l widths or at a million edges."""
import functools

import numpy as np
import pytest
import torch

from oracle import graph as og
from oracle import model as om
from oracle import ops as oo
from dagr_amd.data import Data

pytestmark = pytest.mark.gpu


def _scale(t):
    return max(1.0, float(t.abs().max())) if t.numel() else 1.0


def _err(got, want):
    return float((got.cpu().double() - want).abs().max()) if want.numel() else 0.0


def _float64_reference(conv, x, src, dst, attr, g):
    """out = sum_k A[:, k] . W[k] + x . root^T + bias with A[n, k] = sum over n's in-edges of basis_k(attr) x[src], and the
    gradients of <out, g> w.r.t. x, weight, root and bias by float64 autograd on the CPU."""
    xd = x.detach().double().cpu().requires_grad_(True)
    Wd = conv.weight.detach().double().cpu().requires_grad_(True)
    Rd = conv.lin.weight.detach().double().cpu().requires_grad_(True)
    bd = conv.bias.detach().double().cpu().requires_grad_(True)
    n, cin = xd.shape
    cout = Wd.shape[2]
    src, dst = torch.as_tensor(src, dtype=torch.int64), torch.as_tensor(dst, dtype=torch.int64)
    basis, index = oo.spline_basis(torch.as_tensor(attr).double())
    xs = xd[src]
    A = torch.zeros((n * 25, cin), dtype=torch.float64)
    for s in range(4):
        A.index_add_(0, dst * 25 + index[:, s], basis[:, s:s + 1] * xs)
    ref = A.view(n, 25 * cin) @ Wd.reshape(25 * cin, cout) + xd @ Rd.t() + bd
    ref.backward(g.double().cpu())
    return ref.detach(), dict(x=xd.grad, weight=Wd.grad, root=Rd.grad, bias=bd.grad)


def _check(conv, x, out, ref, grads, bar=1e-4):
    assert _err(out.detach(), ref) <= bar * _scale(ref)
    for name, got in (("x", x.grad), ("weight", conv.weight.grad), ("root", conv.lin.weight.grad), ("bias", conv.bias.grad)):
        assert got is not None, name
        want = grads[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err = _err(got, want) / _scale(want)
        assert err <= bar, (name, err)


@pytest.mark.parametrize("mode", ["train_exact_offsets", "eval_lut_domain"])
@pytest.mark.parametrize("n,cin,cout,max_deg", [
    (300, 8, 6, 9), (1000, 66, 64, 12), (40, 3, 16, 30),
    (66000, 16, 16, 4),        # event-level shape: skinny-GEMM forward, gA rebuilt in the scatter
    # dagr-l (net_stem_width 1): layer3.conv_block1, layer4/5.conv_block1 (three channel passes per lane), head.cls_pred1
    # (100 classes), head.obj_pred1 -- every one on k_tap_scatter_grad<64>
    (3000, 66, 128, 12), (3000, 130, 128, 12), (2000, 128, 100, 10), (2000, 128, 1, 10),
    (3000, 16, 64, 12),        # cin <= 16 with cout > 16: k_tap_scatter_grad<16>
    (3000, 17, 16, 12),        # the first cin on the <64> side
    (65536, 3, 8, 4),          # the library's own GEMM in the forward at cout 8, n exactly at its threshold
    (0, 66, 128, 12),          # no nodes: empty input gradient, zero weight gradients
])
def test_spline_conv_gradients_match_float64_autograd(n, cin, cout, max_deg, mode):
    from dagr_amd.model.layers.spline_conv import MySplineConv
    rng = np.random.default_rng(n + cin)
    args = om.default_args()
    W_, H_ = 320, 215
    torch.manual_seed(n)
    conv = MySplineConv(cin, cout, args=args, bias=True)
    with torch.no_grad():
        conv.bias.uniform_(-0.5, 0.5)
    conv = conv.cuda()
    rx, ry, M = 12, 11, 0.0625
    conv.init_lut(height=H_, width=W_, Mx=M, rx=rx, ry=ry)
    # a graph whose Cartesian attributes sit on the integer offset grid the table covers
    deg = rng.integers(0, max_deg + 1, size=n)
    dst = np.repeat(np.arange(n), deg)
    src = rng.integers(0, max(n, 1), size=len(dst))
    dx, dy = rng.integers(-rx, rx + 1, len(dst)), rng.integers(-ry, ry + 1, len(dst))
    attr = np.stack([dx / (2 * M * W_) + 0.5, dy / (2 * M * H_) + 0.5], 1).astype(np.float32).reshape(-1, 2)
    x = torch.from_numpy(rng.standard_normal((n, cin)).astype(np.float32)).cuda().requires_grad_(True)
    data = Data(x=x, edge_index=torch.from_numpy(np.stack([src, dst]).reshape(2, -1)).cuda(),
                edge_attr=torch.from_numpy(attr).cuda())
    if mode == "eval_lut_domain":
        conv.eval()                  # codes = message_lut's table coordinates (spline_conv.py:41-42)
    else:
        data.edge_attr_max = M       # training mode: exact offsets recovered from the attributes (Cartesian sets this)
    out = conv(data).x
    assert out.shape == (n, cout)
    g = torch.from_numpy(rng.standard_normal((n, cout)).astype(np.float32)).cuda()
    out.backward(g)
    ref, grads = _float64_reference(conv, x, src, dst, attr, g)
    _check(conv, x, out, ref, grads)
    if n == 0:
        assert x.grad.shape == (0, cin)
        for p in (conv.weight, conv.lin.weight, conv.bias):
            assert p.grad.shape == p.shape and not bool(p.grad.any())


@functools.lru_cache(maxsize=1)
def _hub_graph():
    """A hot spot: 60 000 events on 2 x 2 pixels and 3 000 on a 10 x 10 halo, all in the window's last 15 ms (96 x 64
    sensor, radius 4, dt 10 ms, K 16, Q 128).  Lone halo pixels next to the burst become sources of >10 000 edges."""
    rng = np.random.default_rng(29)
    W, H, cx, cy, n_core, n_halo = 96, 64, 40, 30, 60000, 3000
    x = np.concatenate([rng.integers(cx, cx + 2, n_core), rng.integers(cx - 4, cx + 6, n_halo)]).astype(np.int32)
    y = np.concatenate([rng.integers(cy, cy + 2, n_core), rng.integers(cy - 4, cy + 6, n_halo)]).astype(np.int32)
    t = np.sort(rng.integers(985000, 1000001, n_core + n_halo)).astype(np.int32)
    perm = rng.permutation(n_core + n_halo)
    x, y = x[perm], y[perm]
    ei = og.build_window_graph(x, y, t, np.zeros(len(x), np.int32), W, H, 1, 4, 10000, K=16, Q=128)
    return x, y, ei, W, H


@pytest.mark.parametrize("signs", ["same_sign", "random_sign"])
@pytest.mark.parametrize("cin,cout", [(16, 16), (16, 32), (18, 64)],
                         ids=["fused_w_16_16", "scatter16_16_32", "scatter64_18_64"])
def test_spline_conv_backward_at_a_high_out_degree_hub(cin, cout, signs):
    """The input gradient of a node sums one term per out-edge.  The scatter adds them as 64-bit fixed-point integers; with
    every term at full magnitude and of one sign (all weights and the root one power of two, g = 1) the hub's sum is
    (out-degree + 1) x max|gA| exactly, and must not wrap."""
    from dagr_amd.model.layers.spline_conv import MySplineConv
    xs_, ys_, ei, W_, H_ = _hub_graph()
    n = len(xs_)
    src, dst = ei[0], ei[1]
    outdeg = np.bincount(src, minlength=n)
    assert outdeg.max() > 8192, outdeg.max()         # more one-sign full-magnitude terms than a 2^50 / max|gA| scale holds
    M = 0.0625
    dx, dy = xs_[src] - xs_[dst], ys_[src] - ys_[dst]
    attr = np.stack([dx / (2 * M * W_) + 0.5, dy / (2 * M * H_) + 0.5], 1).astype(np.float32)
    rng = np.random.default_rng(cin * 100 + cout)
    torch.manual_seed(cin + cout)
    conv = MySplineConv(cin, cout, args=om.default_args(), bias=True)
    with torch.no_grad():
        if signs == "same_sign":
            conv.weight.fill_(1 / 16)
            conv.lin.weight.fill_(1 / 16)
            conv.bias.zero_()
        else:
            conv.bias.uniform_(-0.5, 0.5)
    conv = conv.cuda()
    conv.init_lut(height=H_, width=W_, Mx=M, rx=6, ry=4)
    x = torch.from_numpy(rng.standard_normal((n, cin)).astype(np.float32)).cuda().requires_grad_(True)
    data = Data(x=x, edge_index=torch.from_numpy(ei).cuda(), edge_attr=torch.from_numpy(attr).cuda())
    data.edge_attr_max = M
    out = conv(data).x
    g = (torch.ones((n, cout)) if signs == "same_sign" else torch.from_numpy(rng.standard_normal((n, cout)).astype(np.float32)))
    out.backward(g.cuda())
    ref, grads = _float64_reference(conv, x, src, dst, attr, g)
    _check(conv, x, out, ref, grads)
    if signs == "same_sign":
        hub = int(outdeg.argmax())
        want = grads["x"][hub]
        exact = (outdeg[hub] + 1) * cout / 16               # every basis sums to one
        assert float((want - exact).abs().max()) <= 1e-9 * exact
        err = float((x.grad[hub].cpu().double() - want).abs().max() / want.abs().max())
        assert err <= 1e-6, (hub, outdeg[hub], x.grad[hub, :4].tolist(), want[:4].tolist())
