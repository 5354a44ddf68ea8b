"""dagr_gemm_split_bf16 / dagr_conv3x3_split_bf16 (csrc/gemm_split_bf16.hip: fp32 GEMMs rebuilt from three bf16 pieces per
operand and six bf16 MFMA products) called directly.

Two bars, both against float64 (tests/kernel_refs.py):
 (i)  elementwise, the bound of tests/test_gemm_epilogue_gpu.py: |got - ref| <= (K + 3) * 2^-24 * (|A| @ |W| + |b| + |R|)
      (K = 9 C for the 3x3);
 (ii) max |err| / max |ref| at most TWICE the same figure of the fp32 library path on the same operands, measured here
      (dagr_gemm_epilogue; torch's fp32 conv2d for the 3x3).  The six-product form sits below the fp32 GEMM's error, a form
      with any of the six products missing at 5-12x it (2^-16 relative terms dropped): 2 passes the first, fails the rest.
"""
import numpy as np
import pytest
import torch

from dagr_amd import _lib
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
INVALID, UNSUPPORTED = -1, -4      # DAGR_ERR_INVALID_ARG, DAGR_ERR_UNSUPPORTED
K_MIN = 32                         # the kernel's K-tile: the smallest K (and C of a 3x3) it takes


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return _lib.cur_stream(torch.device("cuda:0"))


def _last_error():
    return _lib.lib().dagr_last_error().decode("utf-8", "replace")


def _padded(a, ld, fill=SENTINEL):
    out = np.full(a.shape[:-1] + (ld,), fill, np.float32)
    out[..., :a.shape[-1]] = a
    return out


def _pack(W):
    """Wt[K, N] -> (rc, packed planes on the device)."""
    L = _lib.lib()
    K, N = W.shape
    n = int(L.dagr_gemm_split_bf16_packed_bytes(K, N))
    out = torch.empty(max(n, 16), dtype=torch.uint8, device="cuda")
    dW = _dev(W)
    rc = L.dagr_gemm_split_bf16_pack(_lib.ptr(dW), K, N, _lib.ptr(out), n, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(dW.cpu().numpy(), W), "the pack wrote its input"
    return rc, out


def _operands(M, K, N, bias, res, seed):
    """ReLU-shaped activations, He-scaled weights (what the image branch feeds its convolutions)."""
    r = np.random.default_rng(seed)
    A = np.maximum(r.standard_normal((M, K), dtype=np.float32), 0) + (r.random((M, K), dtype=np.float32) < 0.05) * np.float32(-0.5)
    W = (r.standard_normal((K, N), dtype=np.float32) * np.float32(np.sqrt(2.0 / K))).astype(np.float32)
    b = r.standard_normal(N, dtype=np.float32) * np.float32(0.1) if bias else None
    R = r.standard_normal((M, N), dtype=np.float32) if res else None
    return A.astype(np.float32), W, b, R


def _split(A, W, b, R, act, lda=None, ldr=None, ldd=None, tile=0, geom=None):
    """Runs dagr_gemm_split_bf16 on device copies and checks that it wrote none of its inputs.  ``geom`` = (B, H, W, stride)
    for a strided 1x1 (A is then the [B*H*W, K] pixel matrix); returns (rc, D[M, ldd]) with D pre-filled with the sentinel."""
    K, N = W.shape
    lda, ldr, ldd = lda or K, ldr or N, ldd or N
    Bi, H, Wd, s = geom or (0, 0, 0, 1)
    M = A.shape[0] if geom is None else Bi * ((H - 1) // s + 1) * ((Wd - 1) // s + 1)
    rc, wp = _pack(W)
    assert rc == 0, _last_error()
    hA = _padded(A, lda)
    hR = None if R is None else _padded(R, ldr)
    dA, db, dR = _dev(hA), _dev(b), _dev(hR)
    packed_before = wp.clone()
    dD = torch.full((M, ldd), SENTINEL, dtype=torch.float32, device="cuda")
    rc = _lib.lib().dagr_gemm_split_bf16(_lib.ptr(dA), M, K, lda, _lib.ptr(wp), N, _lib.ptr(db), _lib.ptr(dR), ldr, act,
                                         _lib.ptr(dD), ldd, Bi, H, Wd, s, tile, _stream())
    torch.cuda.synchronize()
    for d, h in ((dA, hA), (db, b), (dR, hR)):
        if d is not None:
            assert np.array_equal(d.cpu().numpy(), h), "an input was written"
    assert torch.equal(wp, packed_before), "the packed weights were written"
    return rc, dD.cpu().numpy()


_WS = {}


def _library(A, W, b, R, act):
    """The fp32 library path on the same operands (dagr_gemm_epilogue)."""
    if "t" not in _WS:
        _WS["t"] = torch.empty(int(_lib.lib().dagr_gemm_epilogue_workspace_bytes()), dtype=torch.uint8, device="cuda")
    ws = _WS["t"]
    M, K = A.shape
    N = W.shape[1]
    dA, dW, db, dR = _dev(A), _dev(W), _dev(b), _dev(R)
    dD = torch.empty((M, N), dtype=torch.float32, device="cuda")
    rc = _lib.lib().dagr_gemm_epilogue(_lib.ptr(dA), M, K, K, _lib.ptr(dW), N, _lib.ptr(db), _lib.ptr(dR), N, act, _lib.ptr(dD), N,
                                       _lib.ptr(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, _last_error()
    return dD.cpu().numpy()


def _assert_both_bars(got, lib, ref, mag, K, what):
    err = np.abs(got - ref)
    bound = (K + 3) * 2.0 ** -24 * mag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    scale = max(float(np.abs(ref).max()), 1e-300)
    mine, theirs = float(err.max()) / scale, float(np.abs(lib - ref).max()) / scale
    print(f"split_bf16 {what}: max |err| / bound = {worst:.3f}; max|err|/max|ref| split {mine:.2e}, library {theirs:.2e}")
    assert np.all(err <= bound), f"{what}: max |err| / bound = {worst}"
    assert mine <= 2.0 * theirs, f"{what}: split {mine:.3e} > 2 x library {theirs:.3e}"


def _check_gemm(A, W, b, R, act, what, **kw):
    rc, D = _split(A, W, b, R, act, **kw)
    assert rc == 0, _last_error()
    ref, mag = kr.gemm_epilogue(A, W, b, R, act)
    _assert_both_bars(D[:, :W.shape[1]], _library(A, W, b, R, act), ref, mag, A.shape[1], what)
    return D


@pytest.mark.parametrize("N", [16, 64, 144, 256])
@pytest.mark.parametrize("K", [K_MIN, 64, 576])
@pytest.mark.parametrize("M", [1, 7, 129, 300])
def test_shapes_that_are_no_multiple_of_a_tile(M, K, N):
    A, W, b, R = _operands(M, K, N, True, False, seed=M + K + N)
    _check_gemm(A, W, b, R, 1, f"({M}, {K}, {N})")


@pytest.mark.parametrize("tile", [1, 2])
def test_each_tile_configuration_with_several_tiles_each_way(tile):
    """300 x 256: 5 x 2 tiles of 64 x 128, 10 x 2 of 32 x 128; both configurations sum in the same order."""
    A, W, b, R = _operands(300, 64, 256, True, True, seed=5)
    D = _check_gemm(A, W, b, R, 1, f"tile {tile}", tile=tile)
    rc, other = _split(A, W, b, R, 1, tile=3 - tile)
    assert rc == 0, _last_error()
    assert np.array_equal(D.view(np.int32), other.view(np.int32)), "the two tile configurations give different bits"


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("act", [0, 1])
def test_all_eight_epilogues(bias, res, act):
    A, W, b, R = _operands(129, 64, 64, bias, res, seed=17)
    D = _check_gemm(A, W, b, R, act, f"bias={bias} R={res} act={act}")
    if act:
        assert (D == 0).any() and (D > 0).any()
    else:
        assert (D < 0).any()


def test_padded_leading_dimensions_untouched_padding_and_same_bits_twice():
    M, K, N = 129, 64, 144
    A, W, b, R = _operands(M, K, N, True, True, seed=23)
    D = _check_gemm(A, W, b, R, 1, "padded lda / ldr / ldd", lda=K + 4, ldr=N + 4, ldd=N + 8)
    assert D.shape == (M, N + 8) and np.all(D[:, N:] == SENTINEL), "the padding columns of D were written"
    rc, again = _split(A, W, b, R, 1, lda=K + 4, ldr=N + 4, ldd=N + 8)
    assert rc == 0, _last_error()
    assert np.array_equal(D.view(np.int32), again.view(np.int32)), "same operands, different bits"


def _stress(shape, seed):
    """Random values with rows (last axis runs along K for A; transpose for W) that stress the three-piece split."""
    r = np.random.default_rng(seed)
    n, K = shape
    X = r.standard_normal((n, K), dtype=np.float32)
    sign = np.where(r.random(K) < 0.5, -1.0, 1.0).astype(np.float32)
    X[0] = (10.0 ** r.uniform(-3, 3, K)).astype(np.float32) * sign                 # magnitudes 1e-3 ... 1e3 in one row
    X[1] = (2.0 ** r.integers(-12, 12, K)).astype(np.float32) * sign               # exact powers of two
    X[2] = (X[2].view(np.int32) | 0xFFFF).view(np.float32)                         # low 16 mantissa bits all ones: the first
    #                                                                                piece rounds up, the second is negative
    X[3] = -np.abs(X[3])                                                           # negative
    X[4] = 0.0                                                                     # zeros
    tiny = (r.uniform(0.4e-38, 3e-38, K)).astype(np.float32) * sign                # around FLT_MIN (1.18e-38), both sides
    X[5] = np.where(np.arange(K) % 2 == 0, tiny, X[5])                             # near 1e-38 among ordinary values
    X[6, ::3] = 0.0
    return X


@pytest.mark.parametrize("K", [64, 576])
def test_operands_that_stress_the_split(K):
    M, N = 129, 64
    A = _stress((M, K), seed=K)
    W = np.ascontiguousarray(_stress((N, K), seed=K + 1).T) * np.float32(np.sqrt(2.0 / K))
    r = np.random.default_rng(3)
    b = r.standard_normal(N, dtype=np.float32) * np.float32(0.1)
    _check_gemm(A, W.astype(np.float32), b, None, 0, f"stress K={K}")


def test_unsupported_shapes_are_refused_with_a_message():
    L = _lib.lib()
    assert L.dagr_gemm_split_bf16_packed_bytes(48, 64) == 0 and L.dagr_gemm_split_bf16_packed_bytes(64, 24) == 0
    assert L.dagr_gemm_split_bf16_packed_bytes(64, 64) > 0
    for K, N in ((48, 64), (64, 24)):
        W = np.ones((K, N), np.float32)
        rc, _ = _pack(W)
        assert rc == UNSUPPORTED and "multiple" in _last_error()
    rc, wp = _pack(np.ones((64, 64), np.float32))
    assert rc == 0
    A = torch.ones((8, 128), device="cuda")
    D = torch.full((8, 64), SENTINEL, device="cuda")
    for K, N, lda, want in ((48, 64, 48, UNSUPPORTED), (64, 24, 64, UNSUPPORTED), (64, 64, 66, INVALID), (64, 64, 32, INVALID)):
        rc = L.dagr_gemm_split_bf16(_lib.ptr(A), 8, K, lda, _lib.ptr(wp), N, None, None, N, 0, _lib.ptr(D), 64, 0, 0, 0, 1, 0,
                                    _stream())
        assert rc == want and "dagr_gemm_split_bf16" in _last_error(), (K, N, lda, rc, _last_error())
    rc = L.dagr_conv3x3_split_bf16(_lib.ptr(A), 1, 2, 4, 16, 16, _lib.ptr(wp), 64, None, None, 64, 0, _lib.ptr(D), 64, 0, _stream())
    assert rc == UNSUPPORTED and "dagr_conv3x3_split_bf16" in _last_error()
    torch.cuda.synchronize()
    assert bool((D == SENTINEL).all()), "a refused call wrote D"


@pytest.mark.parametrize("hw", [(5, 7), (6, 8)])
def test_a_strided_1x1_reads_every_second_pixel_in_place(hw):
    H, Wd = hw
    Bi, K, N, s = 2, 64, 64, 2
    r = np.random.default_rng(H * Wd)
    x = r.standard_normal((Bi, H, Wd, K), dtype=np.float32)
    W = (r.standard_normal((K, N), dtype=np.float32) * np.float32(np.sqrt(2.0 / K))).astype(np.float32)
    b = r.standard_normal(N, dtype=np.float32) * np.float32(0.1)
    sliced = np.ascontiguousarray(x[:, ::s, ::s, :]).reshape(-1, K)          # slice, then GEMM
    rc, D = _split(x.reshape(-1, K), W, b, None, 1, geom=(Bi, H, Wd, s))
    assert rc == 0, _last_error()
    assert D.shape[0] == sliced.shape[0]
    ref, mag = kr.gemm_epilogue(sliced, W, b, None, 1)
    _assert_both_bars(D, _library(sliced, W, b, None, 1), ref, mag, K, f"stride 2 of {H}x{Wd}")
    # a wrong M for the geometry is refused
    wp = _pack(W)[1]
    dA, dD = _dev(x), torch.empty((sliced.shape[0] + 1, N), device="cuda")
    rc = _lib.lib().dagr_gemm_split_bf16(_lib.ptr(dA), sliced.shape[0] + 1, K, K, _lib.ptr(wp), N, None, None, N, 0,
                                         _lib.ptr(dD), N, Bi, H, Wd, s, 0, _stream())
    assert rc == INVALID


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 7), (9, 6)])
def test_conv3x3_against_float64_conv2d(hw, epilogue):
    """Distinct values per image and pixel: a read across the seam between the two images, or past a border, shows."""
    H, Wd = hw
    Bi = 2
    F = torch.nn.functional
    for C in (K_MIN, 64):
        for N in (16, 64):
            g = torch.Generator().manual_seed(H * 100 + Wd * 10 + C + N)
            x = torch.randn((Bi, C, H, Wd), generator=g) + torch.arange(1, Bi * H * Wd + 1, dtype=torch.float32).view(Bi, 1, H, Wd) * 0.25
            w = torch.randn((N, C, 3, 3), generator=g) * (2.0 / (9 * C)) ** 0.5
            b = torch.randn((N,), generator=g) * 0.1 if epilogue else None
            ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), 1, 1)
            mag = F.conv2d(x.double().abs(), w.double().abs(), None if b is None else b.double().abs(), 1, 1)
            lib = F.conv2d(x.cuda(), w.cuda(), None if b is None else b.cuda(), 1, 1)
            if epilogue:
                ref, lib = ref.clamp_min(0), lib.clamp_min(0)
            rc, wp = _pack(w.permute(2, 3, 1, 0).reshape(9 * C, N).contiguous().numpy())
            assert rc == 0, _last_error()
            hx = x.permute(0, 2, 3, 1).contiguous()
            dx, db = hx.cuda(), None if b is None else b.cuda()
            dD = torch.full((Bi * H * Wd, N), SENTINEL, device="cuda")
            rc = _lib.lib().dagr_conv3x3_split_bf16(_lib.ptr(dx), Bi, H, Wd, C, C, _lib.ptr(wp), N, _lib.ptr(db), None, N,
                                                    1 if epilogue else 0, _lib.ptr(dD), N, 0, _stream())
            torch.cuda.synchronize()
            assert rc == 0, _last_error()
            assert torch.equal(dx.cpu(), hx), "the input map was written"

            def nhwc(t):
                return t.permute(0, 2, 3, 1).reshape(-1, N).cpu().numpy()
            _assert_both_bars(dD.cpu().numpy(), nhwc(lib), nhwc(ref), nhwc(mag), 9 * C,
                              f"3x3 {H}x{Wd} C={C} N={N} epilogue={epilogue}")
