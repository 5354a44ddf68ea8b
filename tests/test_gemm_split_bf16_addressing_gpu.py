"""The split-bf16 kernel's A-row addressing (csrc/gemm_split_bf16.hip): the rows come through one buffer descriptor with
per-row offsets computed in front of the K loop, and a masked row (beyond M, a 3x3 tap outside the image or across the
seam between two images) is an offset past the descriptor's extent, which reads as zero.  Every test runs on every variant
of the `_variant` entry points.

 1. The bits of the kernel as it was before this addressing (tests/golden/split_bf16_parent_bits.npz: operand pools and the
    D that build gave; every case takes the leading elements of the pools).  Equality, no tolerance.
 2. The A view inside a NaN-filled allocation: finite, the bits of the same operands in a clean buffer, and inside both
    float64 bars of tests/test_gemm_split_bf16_gpu.py.
 3. M = 1, tile rows - 1, tile rows + 1 for the 32- and the 64-row tiles, against float64.
 4. 3x3 with H = 1 / W = 1 (every side tap masked) and a zero image in front of one with large values: against float64
    conv2d, and the zero image's output is exactly bias / ReLU(bias).
 5. A view of 2^31 bytes or more is refused (DAGR_ERR_UNSUPPORTED, a message, nothing launched, D untouched).
"""
import os

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from tests import kernel_refs as kr
from tests.test_gemm_split_bf16_gpu import (SENTINEL, UNSUPPORTED, _assert_both_bars, _dev, _last_error, _library, _operands,
                                            _pack, _stream)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_bf16_parent_bits.npz")
VARIANTS = tuple(range(1, _lib.DEFINES["DAGR_SPLIT_VARIANT_LAST"] + 1))

ROWS = [(1, 32, 16), (33, 64, 80), (65, 96, 64), (130, 160, 144)]                              # (M, K, N), lda = K + 4
STRIDED = [(1, 4, 4, 32, 16, 2), (2, 5, 7, 64, 64, 2), (2, 3, 3, 96, 80, 3)]                   # (B, H, W, K, N, s)
CONVS = [(1, 1, 1, 32, 16), (2, 2, 3, 32, 64), (2, 5, 7, 64, 80), (1, 9, 8, 96, 144)]          # (B, H, W, C, N)
CASES = [("rows", c) for c in ROWS] + [("strided", c) for c in STRIDED] + [("conv", c) for c in CONVS]


def _out_dim(n, s):
    return (n - 1) // s + 1


def case_key(kind, case, epilogue):
    return f"{kind}_{'_'.join(str(v) for v in case)}_{'full' if epilogue else 'none'}"


def case_operands(kind, case, pools):
    """(A[rows, K] as the kernel's A view without its pitch, W[Kw, N], bias[N], R[M, N]) from the leading pool elements."""
    if kind == "rows":
        M, K, N = case
        rows, Kw = M, K
    elif kind == "strided":
        B, H, W, K, N, s = case
        rows, Kw, M = B * H * W, K, B * _out_dim(H, s) * _out_dim(W, s)
    else:
        B, H, W, K, N = case
        rows = M = B * H * W
        Kw = 9 * K
    A = np.ascontiguousarray(pools["apool"][:rows * K].reshape(rows, K))
    Wt = np.ascontiguousarray(pools["wpool"][:Kw * N].reshape(Kw, N))
    return A, Wt, np.ascontiguousarray(pools["bpool"][:N]), np.ascontiguousarray(pools["rpool"][:M * N].reshape(M, N))


def run(kind, case, variant, dA, lda, wp, db, dR, act):
    """One launch of the `_variant` entry point of the case's kind.  dA: device tensor whose first element is the view's
    first; lda its pitch in floats.  Returns (rc, D[M, N]) with D pre-filled with the sentinel."""
    L = _lib.lib()
    if kind == "conv":
        B, H, W, C, N = case
        M = B * H * W
    elif kind == "strided":
        B, H, W, K, N, s = case
        M = B * _out_dim(H, s) * _out_dim(W, s)
    else:
        M, K, N = case
    dD = torch.full((M, N), SENTINEL, dtype=torch.float32, device="cuda")
    if kind == "conv":
        rc = L.dagr_conv3x3_split_bf16_variant(_lib.ptr(dA), B, H, W, C, lda, _lib.ptr(wp), N, _lib.ptr(db), _lib.ptr(dR), N, act,
                                               _lib.ptr(dD), N, variant, _stream())
    else:
        geom = (B, H, W, s) if kind == "strided" else (0, 0, 0, 1)
        rc = L.dagr_gemm_split_bf16_variant(_lib.ptr(dA), M, K, lda, _lib.ptr(wp), N, _lib.ptr(db), _lib.ptr(dR), N, act,
                                            _lib.ptr(dD), N, *geom, variant, _stream())
    torch.cuda.synchronize()
    return rc, dD


def pitched(A, lda, fill):
    out = np.full((A.shape[0], lda), fill, np.float32)
    out[:, :A.shape[1]] = A
    return out


def case_pitch(kind, case):
    return case[1] + 4 if kind == "rows" else case[3]


def run_case(kind, case, epilogue, pools, variants=VARIANTS):
    """{variant: D on the host} of one golden case."""
    A, Wt, b, R = case_operands(kind, case, pools)
    lda = case_pitch(kind, case)
    rc, wp = _pack(Wt)
    assert rc == 0, _last_error()
    dA = _dev(pitched(A, lda, SENTINEL))
    db, dR = (_dev(b), _dev(R)) if epilogue else (None, None)
    out = {}
    for v in variants:
        rc, D = run(kind, case, v, dA, lda, wp, db, dR, 1 if epilogue else 0)
        assert rc == 0, _last_error()
        out[v] = D.cpu()
    return out


def _same_bits(a, b):
    return torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. the parent's bits
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("epilogue", [False, True], ids=["none", "bias+R+relu"])
@pytest.mark.parametrize("kind,case", CASES, ids=[f"{k}{c}" for k, c in CASES])
def test_the_bits_of_the_kernel_before_the_buffer_addressing(kind, case, epilogue, golden):
    want = torch.from_numpy(golden[case_key(kind, case, epilogue)])
    for v, D in run_case(kind, case, epilogue, golden).items():
        assert not bool((D == SENTINEL).any()), f"variant {v} left part of D unwritten"
        assert _same_bits(D, want), f"{kind} {case}: variant {v} gives other bits than the recorded ones"


# ---- 2. poisoned surroundings
def _poisoned(A, lda, front, back):
    """The view A[rows, K] with pitch lda inside a NaN allocation: 4 floats, `front` floats, the view (its pitch padding NaN,
    the last row without padding), `back` floats.  Returns (allocation, view) -- the view is a slice of the allocation."""
    rows, K = A.shape
    extent = (rows - 1) * lda + K
    host = np.full(4 + front + extent + back, np.nan, np.float32)
    body = host[4 + front:4 + front + extent]
    for r in range(rows):
        body[r * lda:r * lda + K] = A[r]
    big = torch.from_numpy(host).cuda()
    return big, big[4 + front:]


def _float64_conv(x, Wt, b, R, act, B, H, W, C, N):
    """(ref, mag, fp32 library result) of the 3x3 as [B H W, N]; x is [B H W, C], Wt is [9 C, N] in (tap, channel) order."""
    F = torch.nn.functional
    xt = torch.from_numpy(x).view(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    wt = torch.from_numpy(Wt).view(3, 3, C, N).permute(3, 2, 0, 1).contiguous()
    bt = None if b is None else torch.from_numpy(b)

    def nhwc(t):
        return t.permute(0, 2, 3, 1).reshape(-1, N)
    ref = nhwc(F.conv2d(xt.double(), wt.double(), None if bt is None else bt.double(), 1, 1))
    mag = nhwc(F.conv2d(xt.double().abs(), wt.double().abs(), None if bt is None else bt.double().abs(), 1, 1))
    lib = nhwc(F.conv2d(xt.cuda(), wt.cuda(), None if bt is None else bt.cuda(), 1, 1)).cpu()
    if R is not None:
        ref, mag, lib = ref + torch.from_numpy(R).double(), mag + torch.from_numpy(R).double().abs(), lib + torch.from_numpy(R)
    if act:
        ref, lib = ref.clamp_min(0), lib.clamp_min(0)
    return ref.numpy(), mag.numpy(), lib.numpy()


def _reference(kind, case, A, Wt, b, R, act):
    """(ref, mag, library, K of the bound)"""
    if kind == "conv":
        B, H, W, C, N = case
        return _float64_conv(A, Wt, b, R, act, B, H, W, C, N) + (9 * C,)
    if kind == "strided":
        B, H, W, K, N, s = case
        A = np.ascontiguousarray(A.reshape(B, H, W, K)[:, ::s, ::s, :]).reshape(-1, K)
    ref, mag = kr.gemm_epilogue(A, Wt, b, R, act)
    return ref, mag, _library(A, Wt, b, R, act), A.shape[1]


POISON = [("rows", (1, 32, 16)), ("rows", (65, 96, 80)), ("rows", (130, 160, 144)), ("strided", (2, 5, 7, 64, 64, 2)),
          ("strided", (2, 3, 3, 96, 80, 3)), ("conv", (1, 1, 1, 32, 16)), ("conv", (2, 2, 3, 32, 64)), ("conv", (2, 5, 7, 64, 80))]


@pytest.mark.parametrize("epilogue", [False, True], ids=["none", "bias+R+relu"])
@pytest.mark.parametrize("kind,case", POISON, ids=[f"{k}{c}" for k, c in POISON])
def test_a_view_in_a_nan_allocation_reads_nothing_outside_itself(kind, case, epilogue):
    r = np.random.default_rng(sum(case))
    K, N = (case[1], case[2]) if kind == "rows" else (case[3], case[4])
    rows = case[0] if kind == "rows" else case[0] * case[1] * case[2]
    M = rows if kind != "strided" else case[0] * _out_dim(case[1], case[5]) * _out_dim(case[2], case[5])
    A = _operands(rows, K, N, False, False, seed=sum(case))[0]
    Wt = (r.standard_normal(((9 if kind == "conv" else 1) * K, N), dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    b = r.standard_normal(N, dtype=np.float32) * np.float32(0.1) if epilogue else None
    R = r.standard_normal((M, N), dtype=np.float32) if epilogue else None
    act = 1 if epilogue else 0
    lda = K + 4
    # rows before and behind: two pitches; a 3x3 gets a whole NaN image (and two more rows) on either side
    around = 2 * lda + (case[1] * case[2] * lda if kind == "conv" else 0)
    big, view = _poisoned(A, lda, around, around)
    clean = _dev(A)
    rc, wp = _pack(Wt)
    assert rc == 0, _last_error()
    db, dR = _dev(b), _dev(R)
    ref, mag, lib, Kb = _reference(kind, case, A, Wt, b, R, act)
    before = big.clone()
    for v in VARIANTS:
        rc, D = run(kind, case, v, view, lda, wp, db, dR, act)
        assert rc == 0, _last_error()
        assert bool(torch.isfinite(D).all()), f"{kind} {case} variant {v}: read the poison"
        rc, D0 = run(kind, case, v, clean, K, wp, db, dR, act)
        assert rc == 0, _last_error()
        assert _same_bits(D.cpu(), D0.cpu()), f"{kind} {case} variant {v}: other bits than in a clean buffer"
        _assert_both_bars(D.cpu().numpy(), lib, ref, mag, Kb, f"poisoned {kind} {case} variant {v}")
    assert torch.equal(big.view(torch.int32), before.view(torch.int32)), "the allocation was written"


# ---- 3. masked rows at every tile edge
@pytest.mark.parametrize("M", [1, 31, 33, 63, 65])
def test_masked_rows_at_the_edges_of_both_row_tiles(M):
    K, N = 64, 80
    A, Wt, b, R = _operands(M, K, N, True, True, seed=900 + M)
    ref, mag = kr.gemm_epilogue(A, Wt, b, R, 1)
    lib = _library(A, Wt, b, R, 1)
    rc, wp = _pack(Wt)
    assert rc == 0, _last_error()
    dA, db, dR = _dev(A), _dev(b), _dev(R)
    for v in VARIANTS:
        rc, D = run("rows", (M, K, N), v, dA, K, wp, db, dR, 1)
        assert rc == 0, _last_error()
        _assert_both_bars(D.cpu().numpy(), lib, ref, mag, K, f"rows M={M} variant {v}")


@pytest.mark.parametrize("hw", [(1, 1), (31, 1), (3, 11), (7, 9), (5, 13)])          # 1, 31, 33, 63, 65 pixels
def test_masked_pixels_at_the_edges_of_both_row_tiles_3x3(hw):
    H, W = hw
    C, N = 32, 48
    case = (1, H, W, C, N)
    r = np.random.default_rng(H * 100 + W)
    x = r.standard_normal((H * W, C), dtype=np.float32)
    Wt = (r.standard_normal((9 * C, N), dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    b = r.standard_normal(N, dtype=np.float32) * np.float32(0.1)
    ref, mag, lib, Kb = _reference("conv", case, x, Wt, b, None, 1)
    rc, wp = _pack(Wt)
    assert rc == 0, _last_error()
    dx, db = _dev(x), _dev(b)
    for v in VARIANTS:
        rc, D = run("conv", case, v, dx, C, wp, db, None, 1)
        assert rc == 0, _last_error()
        _assert_both_bars(D.cpu().numpy(), lib, ref, mag, Kb, f"3x3 {H}x{W} variant {v}")


# ---- 4. 3x3 borders and seam
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("hw", [(1, 6), (6, 1), (1, 1), (5, 7)])
def test_conv3x3_borders_and_the_seam_behind_a_zero_image(hw, act):
    H, W = hw
    B, N = 2, 80
    for C in (32, 96):
        case = (B, H, W, C, N)
        r = np.random.default_rng(H * 10 + W + C)
        x = np.zeros((B, H * W, C), np.float32)
        x[1] = r.standard_normal((H * W, C), dtype=np.float32) * np.float32(1e3) + np.float32(1e3)
        x = x.reshape(B * H * W, C)
        Wt = (r.standard_normal((9 * C, N), dtype=np.float32) * np.float32(0.1)).astype(np.float32)
        b = r.standard_normal(N, dtype=np.float32) * np.float32(0.1)
        ref, mag, lib, Kb = _reference("conv", case, x, Wt, b, None, act)
        rc, wp = _pack(Wt)
        assert rc == 0, _last_error()
        dx, db = _dev(x), _dev(b)
        first = np.broadcast_to(np.maximum(b, 0) if act else b, (H * W, N))
        for v in VARIANTS:
            rc, D = run("conv", case, v, dx, C, wp, db, None, act)
            assert rc == 0, _last_error()
            D = D.cpu().numpy()
            _assert_both_bars(D, lib, ref, mag, Kb, f"3x3 {H}x{W} C={C} act={act} variant {v}")
            assert np.array_equal(D[:H * W], first), f"3x3 {H}x{W} C={C} variant {v}: image 1 leaks into image 0"


# ---- 5. refusal
REFUSED = [("rows", (2, 32, 16), 1 << 29),                   # (lda + 32) * 4 > 2^31
           ("rows", (2, 32, 16), (1 << 29) - 32),            # exactly 2^31 bytes
           ("strided", (1, 3, 1, 32, 16, 2), 1 << 28),       # the last pixel of the map is 2 pitches in
           ("conv", (1, 1, 2, 32, 16), 1 << 29),
           ("conv", (1, 1, 2, 32, 16), 1 << 27)]             # 2^29 + 128 bytes alone, 2^31 with the base (W + 1) pixels back


@pytest.mark.parametrize("kind,case,lda", REFUSED)
def test_a_view_of_2_to_the_31_bytes_is_refused_before_any_launch(kind, case, lda):
    K, N = (case[1], case[2]) if kind == "rows" else (case[3], case[4])
    rc, wp = _pack(np.ones(((9 if kind == "conv" else 1) * K, N), np.float32))
    assert rc == 0, _last_error()
    dA = torch.ones(64, device="cuda")
    fn = "dagr_conv3x3_split_bf16_variant" if kind == "conv" else "dagr_gemm_split_bf16_variant"
    for v in VARIANTS:
        rc, D = run(kind, case, v, dA, lda, wp, None, None, 0)
        assert rc == UNSUPPORTED, (rc, _last_error())
        assert fn in _last_error() and "2^31" in _last_error(), _last_error()
        assert bool((D == SENTINEL).all()), "a refused call wrote D"
