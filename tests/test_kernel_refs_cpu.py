"""tests/kernel_refs.py against independent implementations on the CPU: torch's float64 relu / silu / max_pool2d / addmm,
oracle.model.sample_features (itself pinned to the reference's goldens by tests/test_oracle_refpy.py) and np.cumsum.
The GPU tests of the image-branch kernels, the sampler and the scan lean on these references."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model as om
from tests import kernel_refs as kr


def _rng(seed):
    return np.random.default_rng(seed)


def test_add_relu_and_bias_relu():
    r = _rng(0)
    y, z = r.standard_normal((5, 7, 8)), r.standard_normal((5, 7, 8))
    b = r.standard_normal(8)
    assert np.array_equal(kr.add_relu(y, z), torch.relu(torch.from_numpy(y) + torch.from_numpy(z)).numpy())
    assert np.array_equal(kr.bias_relu(y, b), torch.relu(torch.from_numpy(y) + torch.from_numpy(b)).numpy())
    y32, z32 = y.astype(np.float32), z.astype(np.float32)
    got = kr.add_relu(y32, z32, np.float32)
    assert got.dtype == np.float32
    assert np.array_equal(got, torch.relu(torch.from_numpy(y32) + torch.from_numpy(z32)).numpy())
    # NaN and the infinities as torch.relu(y + z) has them
    y32 = np.array([np.nan, 1, np.inf, np.inf, -np.inf, -np.inf, 2, -0.0], np.float32)
    z32 = np.array([1, np.nan, -np.inf, np.inf, -np.inf, 5, np.inf, 0.0], np.float32)
    got = kr.add_relu(y32, z32, np.float32)
    want = torch.relu(torch.from_numpy(y32) + torch.from_numpy(z32)).numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    assert kr.relu_equal(want, got) and not kr.relu_equal(np.where(np.isnan(want), 0, want), got)


def test_relu_equal_is_bitwise_off_zero_and_sign_blind_at_zero():
    ref = np.array([0.0, 1.0, 0.0, 3.5], np.float32)
    assert kr.relu_equal(np.array([-0.0, 1.0, 0.0, 3.5], np.float32), ref)
    assert not kr.relu_equal(np.array([0.0, np.nextafter(np.float32(1), np.float32(2)), 0.0, 3.5], np.float32), ref)
    assert not kr.relu_equal(np.array([1e-30, 1.0, 0.0, 3.5], np.float32), ref)


def test_silu():
    v = np.concatenate([_rng(1).uniform(-100, 100, 4096), [0.0, -0.0, -88.0, -89.0, -100.0, 100.0]])
    want = F.silu(torch.from_numpy(v)).numpy()
    got = kr.silu(v)
    assert np.all(np.abs(got - want) <= 4 * np.finfo(np.float64).eps * np.abs(want))
    b = _rng(2).uniform(-1, 1, 8)
    y = _rng(3).uniform(-50, 50, (9, 8))
    assert np.allclose(kr.bias_silu(y, b), F.silu(torch.from_numpy(y) + torch.from_numpy(b)).numpy(), rtol=1e-14, atol=0)
    y32, b32 = y.astype(np.float32), b.astype(np.float32)
    assert np.array_equal(kr.bias_silu(y32, b32, np.float32), kr.silu((y32 + b32).astype(np.float64)))


def test_ulp_error():
    one = np.float32(1)
    up = np.nextafter(one, np.float32(2))
    assert kr.ulp_error(np.array([one, up, -one, 0.0, -0.0], np.float32), np.array([1.0, 1.0, -1.0, -0.0, 0.0])).tolist() \
        == [0, 1, 0, 0, 0]
    tiny = np.float32(1e-45)     # the smallest subnormal: one step either side of zero
    assert kr.ulp_error(np.array([tiny, -tiny], np.float32), np.array([0.0, float(tiny)])).tolist() == [1, 2]


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (1, 2, 3, 4), (3, 5, 4, 8), (2, 7, 8, 64), (1, 12, 11, 4)])
def test_bn_relu_maxpool(shape):
    r = _rng(sum(shape))
    x = r.standard_normal(shape)
    sc, sh = r.standard_normal(shape[3]), r.standard_normal(shape[3])
    got, mag = kr.bn_relu_maxpool(x, sc, sh)
    t = torch.from_numpy(x * sc + sh).permute(0, 3, 1, 2)
    want = F.max_pool2d(F.relu(t), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    assert got.shape == want.shape == (shape[0], kr.pooled_size(shape[1]), kr.pooled_size(shape[2]), shape[3])
    assert np.array_equal(got, want)
    wmag = F.max_pool2d(torch.from_numpy(np.abs(x * sc) + np.abs(sh)).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert np.array_equal(mag, wmag.numpy())
    # every affine value negative: all zeros, none of them from the padding
    got, _ = kr.bn_relu_maxpool(np.abs(x) + 0.1, -np.abs(sc) - 0.1, -np.abs(sh))
    assert np.array_equal(got, np.zeros_like(want))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("act", [0, 1])
def test_gemm_epilogue(bias, res, act):
    r = _rng(4)
    M, K, N = 13, 37, 9
    A, W = r.standard_normal((M, K)), r.standard_normal((K, N))
    b = r.standard_normal(N) if bias else None
    R = r.standard_normal((M, N)) if res else None
    got, mag = kr.gemm_epilogue(A, W, b, R, act)
    base = torch.zeros((M, N), dtype=torch.float64)
    if bias:
        base = base + torch.from_numpy(b)
    if res:
        base = base + torch.from_numpy(R)
    want = torch.addmm(base, torch.from_numpy(A), torch.from_numpy(W))
    want = torch.relu(want) if act else want
    assert np.allclose(got, want.numpy(), rtol=0, atol=1e-13)
    wmag = torch.addmm(base.abs() if not (bias and res) else torch.from_numpy(np.abs(b) + np.abs(R)),
                       torch.from_numpy(np.abs(A)), torch.from_numpy(np.abs(W)))
    assert np.allclose(mag, wmag.numpy(), rtol=0, atol=1e-13)
    assert np.all(np.abs(got) <= mag + 1e-13)


@pytest.mark.parametrize("B", [1, 2, 3, 4, 7, 8])
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (9, 13)])
def test_sample_features(B, hw):
    h, w = hw
    W, H, C, N = 320, 215, 5, 200
    r = _rng(10 * B + h)
    pos = r.uniform(0, 1, (N, 3)).astype(np.float32)
    pos[:6, 0] = [0.0, (W - 1) / W, 1.0, -1e-3, 0.5, 0.25]           # sensor edges, one past, slightly negative
    pos[:6, 1] = [0.0, (H - 1) / H, 1.0, 0.5, -1e-3, (H - 1) / H]
    batch = r.integers(0, B, N)
    batch[:2 * B] = np.repeat(np.arange(B), 2)
    feat = r.standard_normal((B, h, w, C)).astype(np.float32)
    want = om.sample_features(torch.from_numpy(pos), torch.from_numpy(batch), torch.from_numpy(feat).permute(0, 3, 1, 2),
                              W, H).numpy()
    bar = 1e-5 * max(1.0, float(np.abs(feat).max()))
    for T in (np.float64, np.float32):
        got, mag = kr.sample_features(pos, batch, feat, W, H, coord_dtype=T)
        assert got.shape == want.shape == (N, C)
        assert float(np.abs(got - want).max()) <= bar
        assert np.all(np.abs(got) <= mag)
    # the corner weights sum to one inside the volume: a constant map samples to the constant ...
    inside = (pos[:, 0] >= 0) & (pos[:, 0] <= (W - 1) / W) & (pos[:, 1] >= 0) & (pos[:, 1] <= (H - 1) / H)
    got, _ = kr.sample_features(pos, batch, np.ones((B, h, w, 1)), W, H)
    assert np.allclose(got[inside], 1.0, atol=1e-12)
    # ... and past the map's edge the missing corners count as zero
    assert np.all(got[~inside] <= 1.0 + 1e-12)
    if (h, w) != (1, 1):
        assert got[2, 0] < 1.0 - 1e-4 and got[3, 0] < 1.0 - 1e-4


def test_exclusive_scan():
    r = _rng(5)
    for n in (1, 2, 100, 4097):
        v = r.integers(0, 16, n).astype(np.int32)
        want = np.concatenate([[0], np.cumsum(v.astype(np.int64))[:-1]])
        got = kr.exclusive_scan(v)
        assert got.dtype == np.int64 and np.array_equal(got, want)
    v = np.array([2 ** 30, 2 ** 30, 5, 2 ** 30], np.int32)       # no int32 wrap inside the reference
    assert kr.exclusive_scan(v).tolist() == [0, 2 ** 30, 2 ** 31, 2 ** 31 + 5]
