"""Plain numpy restatements, in float64 / int64, of the operations behind the image-branch kernels (csrc/dense.hip,
csrc/gemm_lt.hip), the feature sampler (csrc/sample.hip) and the scan (csrc/scan.hip).  The GPU tests of those kernels
compare against these; tests/test_kernel_refs_cpu.py pins every one of them to an independent implementation (torch on
the CPU, oracle.model, np.cumsum), so a wrong reference fails without a GPU.

Each function that backs a derived error bound also returns the magnitude the bound is stated in."""
import numpy as np


def add_relu(y, z, dtype=np.float64):
    """relu(y + z) computed in ``dtype``; NaN stays NaN (np.maximum propagates it, as torch.relu)."""
    with np.errstate(invalid="ignore"):
        return np.maximum(np.asarray(y, dtype) + np.asarray(z, dtype), dtype(0))


def bias_relu(y, bias, dtype=np.float64):
    """relu(y[..., c] + bias[c]) computed in ``dtype`` (channels last)."""
    return np.maximum(np.asarray(y, dtype) + np.asarray(bias, dtype), dtype(0))


def silu(v):
    """v / (1 + exp(-v)) in float64."""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(-v))


def bias_silu(y, bias, sum_dtype=np.float64):
    """silu(y[..., c] + bias[c]) in float64; ``sum_dtype`` = np.float32 rounds the sum as an fp32 add does first."""
    return silu(np.asarray(y, sum_dtype) + np.asarray(bias, sum_dtype))


def pooled_size(n):
    """Output length of a 3 / stride 2 / pad 1 window over n inputs."""
    return (n - 1) // 2 + 1


def bn_relu_maxpool(x, scale, shift):
    """maxpool 3x3 / s2 / p1 of relu(x * scale[c] + shift[c]) over x[B, H, W, C] (padding never wins: -inf).
    Returns (y[B, OH, OW, C], mag) with mag = max over the window of |x * scale| + |shift|."""
    x = np.asarray(x, np.float64)
    scale, shift = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    B, H, W, C = x.shape
    OH, OW = pooled_size(H), pooled_size(W)
    v = np.full((B, H + 2, W + 2, C), -np.inf)
    m = np.full((B, H + 2, W + 2, C), -np.inf)
    v[:, 1:H + 1, 1:W + 1] = np.maximum(x * scale + shift, 0.0)
    m[:, 1:H + 1, 1:W + 1] = np.abs(x * scale) + np.abs(shift)
    y = np.full((B, OH, OW, C), -np.inf)
    mag = np.full((B, OH, OW, C), -np.inf)
    for dy in range(3):
        for dx in range(3):
            y = np.maximum(y, v[:, dy:dy + 2 * OH:2, dx:dx + 2 * OW:2])
            mag = np.maximum(mag, m[:, dy:dy + 2 * OH:2, dx:dx + 2 * OW:2])
    return y, mag


def gemm_epilogue(A, Wt, bias=None, R=None, act=0):
    """act(A[M, K] @ Wt[K, N] + bias[N] + R[M, N]) in float64, act 0 none / 1 ReLU.
    Returns (D, mag) with mag = |A| @ |Wt| + |bias| + |R|."""
    A, Wt = np.asarray(A, np.float64), np.asarray(Wt, np.float64)
    d = A @ Wt
    mag = np.abs(A) @ np.abs(Wt)
    if bias is not None:
        d = d + np.asarray(bias, np.float64)
        mag = mag + np.abs(np.asarray(bias, np.float64))
    if R is not None:
        d = d + np.asarray(R, np.float64)
        mag = mag + np.abs(np.asarray(R, np.float64))
    if act:
        d = np.maximum(d, 0.0)
    return d, mag


def sample_features(pos, batch, feat, width, height, coord_dtype=np.float64):
    """``sample_features`` / ``_sample_features`` (net.py:193-221) + grid_sample(bilinear, align_corners=True, zero
    padding) over the volume [C, D = B, h, w], on a channels-last ``feat[B, h, w, C]``; pos[N, >= 2] normalised, batch[N].

    The coordinates and the eight corner weights are computed in ``coord_dtype``, one rounded operation per step in the
    order csrc/sample.hip documents (no step is a multiply feeding an add):
        g = (2 * (pos * size)) / (size - 1) - 1;  i = ((g + 1) / 2) * (n - 1);  w0 = (floor(i) + 1) - i,  w1 = i - floor(i)
        weight = (wx * wy) * wz
    sum(w_i * f_i) over the corners inside the volume is accumulated in float64.  Returns (out[N, C], mag[N, C]) with
    mag = sum |w_i * f_i|."""
    T = coord_dtype
    feat = np.asarray(feat, np.float64)
    B, h, w, C = feat.shape
    pos = np.asarray(pos)
    N = pos.shape[0]
    Bn = B if B > 1 else 2

    def index(g, size, n):
        g = (T(2) * g) / T(size - 1) - T(1)
        return ((g + T(1)) / T(2)) * T(n - 1)

    ix = index(pos[:, 0].astype(T) * T(width), width, w)
    iy = index(pos[:, 1].astype(T) * T(height), height, h)
    iz = index(np.asarray(batch).astype(T), Bn, B)
    out = np.zeros((N, C))
    mag = np.zeros((N, C))
    fx, fy, fz = np.floor(ix), np.floor(iy), np.floor(iz)
    wx = ((fx + T(1)) - ix, ix - fx)
    wy = ((fy + T(1)) - iy, iy - fy)
    wz = ((fz + T(1)) - iz, iz - fz)
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                wgt = (wx[dx] * wy[dy]) * wz[dz]
                assert wgt.dtype == T
                x, y, z = fx.astype(np.int64) + dx, fy.astype(np.int64) + dy, fz.astype(np.int64) + dz
                ok = (x >= 0) & (x < w) & (y >= 0) & (y < h) & (z >= 0) & (z < B)
                f = feat[np.clip(z, 0, B - 1), np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]      # [N, C]
                term = np.where(ok[:, None], wgt.astype(np.float64)[:, None] * f, 0.0)
                out += term
                mag += np.abs(term)
    return out, mag


def exclusive_scan(v):
    """out[i] = v[0] + ... + v[i-1] in int64."""
    v = np.asarray(v, np.int64)
    return np.cumsum(v, dtype=np.int64) - v


def ordered_f32(x):
    """float32 -> int64 that orders like the floats and steps by one per ulp (-0 and +0 both map to 0)."""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def ulp_error(got, ref64):
    """|got - round_to_float32(ref64)| in float32 ulps, elementwise."""
    return np.abs(ordered_f32(got) - ordered_f32(np.asarray(ref64, np.float64).astype(np.float32)))


def relu_equal(got, ref):
    """The bar of the ReLU kernels: bit-equal wherever the reference is non-zero (NaN included: NaN where and only
    where the reference has one), numerically equal -- either zero -- where it is zero."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False
    nz = (ref != 0) & ~nan
    return bool(np.array_equal(got.view(np.int32)[nz], ref.view(np.int32)[nz]) and np.all(got[~nz & ~nan] == 0))
