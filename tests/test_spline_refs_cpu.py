"""tests/spline_refs.py against the textbook form of SplineConv on the CPU: per edge, What = sum_s basis_s * W[tap_s] with
(basis, tap) from oracle.ops.spline_basis in float64, then x_src @ What, summed per destination.  The references
re-associate that sum per destination and tap (as the kernels do), so agreement to 1e-12 pins both the basis and the
bookkeeping (codes, windows, row layout of the weight matrix)."""
import numpy as np
import pytest
import torch

from oracle import ops as oo
from tests import spline_refs as sr


def _pseudo(idx, r, den):
    """fp32 division, float64 from there on: the one rounding spline_refs shares with the kernels."""
    q = torch.from_numpy((np.asarray(idx, np.int64) - r).astype(np.float32)) / np.float32(den)
    return q.double() + 0.5


def _textbook(T, dst, src, ix, iy, x, W, rx, ry, den):
    """out[T, cout]: sum over edges of x[src] @ (sum_s basis_s W[index_s])."""
    out = np.zeros((T, W.shape[2]))
    if len(dst) == 0:
        return out
    basis, index = oo.spline_basis(torch.stack([_pseudo(ix, rx, den[0]), _pseudo(iy, ry, den[1])], 1))
    assert basis.dtype == torch.float64
    basis, index = basis.numpy(), index.numpy()
    W = W.astype(np.float64)
    for e in range(len(dst)):
        What = sum(basis[e, s] * W[index[e, s]] for s in range(4))
        out[dst[e]] += x[src[e]].astype(np.float64) @ What
    return out


@pytest.mark.parametrize("rx,ry,den_x,den_y", sr.L0_DOMAINS)
def test_axis_and_tap_window_match_spline_basis(rx, ry, den_x, den_y):
    for r, den in ((rx, den_x), (ry, den_y)):
        idx = np.arange(2 * r + 1)
        basis, index = oo.spline_basis(_pseudo(idx, r, den).view(-1, 1))       # D = 1: S = 2
        k0, k1, b0, b1 = sr.axis(idx, r, den)
        assert np.array_equal(k0, index[:, 0].numpy()) and np.array_equal(k1, index[:, 1].numpy())
        assert np.abs(b0 - basis[:, 0].numpy()).max() <= 1e-12 and np.abs(b1 - basis[:, 1].numpy()).max() <= 1e-12
        used = np.concatenate([index[:, s][basis[:, s] != 0].numpy() for s in range(2)])
        assert sr.tap_window(r, den) == (used.min(), used.max() - used.min() + 1)
        assert ((b0 >= 0) & (b0 <= 1) & (b1 >= 0) & (b1 <= 1)).all()          # the offsets stay inside the spline's domain


def test_tap_windows_cover_the_four_forms():
    forms = {(sr.tap_window(rx, dx)[1], sr.tap_window(ry, dy)[1]) for rx, ry, dx, dy in sr.L0_DOMAINS}
    assert forms == {(3, 3), (3, 5), (5, 3), (5, 5)}


@pytest.mark.parametrize("rx,ry,den_x,den_y", sr.L0_DOMAINS)
def test_l0_table_is_the_outer_product_of_the_axes(rx, ry, den_x, den_y):
    (fx, cx), (fy, cy) = sr.tap_window(rx, den_x), sr.tap_window(ry, den_y)
    tab = sr.l0_table(rx, ry, den_x, den_y, (fx, cx, fy, cy))
    sy = 2 * ry + 1
    assert tab.shape == ((2 * rx + 1) * sy, (cx * cy + 3) // 4 * 4)
    code = np.arange(tab.shape[0])
    basis, index = oo.spline_basis(torch.stack([_pseudo(code // sy, rx, den_x), _pseudo(code % sy, ry, den_y)], 1))
    want = np.zeros_like(tab)
    for s in range(4):
        kx, ky = index[:, s].numpy() % 5, index[:, s].numpy() // 5
        ok = basis[:, s].numpy() != 0
        np.add.at(want, (code[ok], (kx[ok] - fx) + cx * (ky[ok] - fy)), basis[:, s].numpy()[ok])
    assert np.abs(tab - want).max() <= 1e-12
    assert (tab[:, cx * cy:] == 0).all()
    assert np.abs(tab.sum(1) - 1).max() <= 1e-12


@pytest.mark.parametrize("N,K,cin,cskip,dom,relu", [(50, 24, 3, 0, 0, True), (23, 8, 19, 0, 2, False),
                                                    (31, 17, 16, 19, 4, True), (1, 4, 16, 3, 5, False)])
def test_conv_l0_matches_the_per_edge_form(N, K, cin, cskip, dom, relu):
    rx, ry, den_x, den_y = sr.L0_DOMAINS[dom]
    rng = np.random.default_rng(N + cin)
    deg = rng.integers(0, K + 1, size=N)
    deg[0] = K
    src = rng.integers(0, N, size=(N, K)).astype(np.int32)
    code = rng.integers(0, (2 * rx + 1) * (2 * ry + 1), size=(N, K)).astype(np.int16)
    x = rng.standard_normal((N, cin)).astype(np.float32)
    xs = rng.standard_normal((N, cskip)).astype(np.float32) if cskip else None
    W = rng.standard_normal((25, cin, 16)).astype(np.float32)
    root = rng.standard_normal((cin, 16)).astype(np.float32)
    wskip = rng.standard_normal((cskip, 16)).astype(np.float32) if cskip else None
    shift = rng.standard_normal(16).astype(np.float32)
    got = sr.conv_l0(src, code, deg, x, xs, W, root, wskip, shift, relu, rx, ry, (den_x, den_y))
    dst = np.repeat(np.arange(N), deg)
    slot = np.concatenate([np.arange(d) for d in deg])
    c = code[dst, slot].astype(np.int64)
    want = _textbook(N, dst, src[dst, slot], c // (2 * ry + 1), c % (2 * ry + 1), x, W, rx, ry, (den_x, den_y))
    want += x.astype(np.float64) @ root
    if cskip:
        want += xs.astype(np.float64) @ wskip
    want += shift
    if relu:
        want = np.maximum(want, 0)
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("T,cin,cskip,N,max_deg,relu,r,den", [
    (50, 6, 0, 7, 9, True, 7, (14.0, 17.5)),
    (33, 18, 5, 21, 12, False, (7, 5), (14.0, 17.5)),
    (16, 3, 5, 7, 0, True, 7, (14.0, 17.5)),              # no edges
    (40, 4, 0, 3, 30, False, (2, 6), (6.0, 12.0)),
])
def test_conv_csr_matches_the_per_edge_form(T, cin, cskip, N, max_deg, relu, r, den):
    rx, ry = (r, r) if np.isscalar(r) else r
    rng = np.random.default_rng(T * 3 + cin)
    deg = rng.integers(0, max_deg + 1, size=T)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    E = int(rowptr[-1])
    col = rng.integers(0, T, size=E).astype(np.int32)
    ix, iy = rng.integers(0, 2 * rx + 1, size=E), rng.integers(0, 2 * ry + 1, size=E)
    code = (ix | (iy << 16)).astype(np.int32)
    x = rng.standard_normal((T, cin)).astype(np.float32)
    xs = rng.standard_normal((T, cskip)).astype(np.float32) if cskip else None
    Wm = rng.standard_normal((26 * cin + cskip, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    got = sr.conv_csr(rowptr, col, code, x, xs, Wm, bias, relu, r, den)
    dst = np.repeat(np.arange(T), deg)
    want = _textbook(T, dst, col, ix, iy, x, Wm[:25 * cin].reshape(25, cin, N), rx, ry, den)
    want += x.astype(np.float64) @ Wm[25 * cin:26 * cin]
    if cskip:
        want += xs.astype(np.float64) @ Wm[26 * cin:]
    want += bias
    if relu:
        want = np.maximum(want, 0)
    assert np.abs(got - want).max() <= 1e-12
