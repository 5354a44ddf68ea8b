"""Every form of the split-bf16 kernel (csrc/gemm_split_bf16.hip) behind dagr_gemm_split_bf16_variant /
dagr_conv3x3_split_bf16_variant: the four four-wave tiles and the 64 x 128 tile on eight waves (every code of the header, 1 to
DAGR_SPLIT_VARIANT_LAST).  Every variant must give the bits of the first entry points' tile 3 (64 x 64), which
tests/test_gemm_split_bf16_gpu.py holds to the float64 reference: no tolerance here, equality.

Slice counts 1 to 5 leave the K loop in its prologue alone, run it with an odd and an even number of slices and (for a loop
with a three-stage ring) through every position and the wrap; the N values end in a partial column tile at both tile widths;
M = 1 and 65 leave most rows of a tile masked."""
import numpy as np
import pytest
import torch

from dagr_amd import _lib
from tests.test_gemm_split_bf16_gpu import SENTINEL, _dev, _last_error, _operands, _pack, _stream

pytestmark = pytest.mark.gpu

LAST = _lib.DEFINES["DAGR_SPLIT_VARIANT_LAST"]
VARIANTS = tuple(range(1, LAST + 1))
BASE_TILE = 3                       # 64 x 64, by the first entry points


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _gemm(entry, code, dA, M, K, lda, wp, N, db, dR, ldr, act, ldd, geom=(0, 0, 0, 1)):
    """One call of dagr_gemm_split_bf16 (entry "tile") or dagr_gemm_split_bf16_variant; D pre-filled with the sentinel."""
    L = _lib.lib()
    fn = L.dagr_gemm_split_bf16 if entry == "tile" else L.dagr_gemm_split_bf16_variant
    dD = torch.full((M, ldd), SENTINEL, dtype=torch.float32, device="cuda")
    rc = fn(_lib.ptr(dA), M, K, lda, _lib.ptr(wp), N, _lib.ptr(db), _lib.ptr(dR), ldr, act, _lib.ptr(dD), ldd, *geom, code,
            _stream())
    torch.cuda.synchronize()
    return rc, dD


def _conv(entry, code, dx, B, H, W, C, wp, N, db, act):
    L = _lib.lib()
    fn = L.dagr_conv3x3_split_bf16 if entry == "tile" else L.dagr_conv3x3_split_bf16_variant
    dD = torch.full((B * H * W, N), SENTINEL, dtype=torch.float32, device="cuda")
    rc = fn(_lib.ptr(dx), B, H, W, C, C, _lib.ptr(wp), N, _lib.ptr(db), None, N, act, _lib.ptr(dD), N, code, _stream())
    torch.cuda.synchronize()
    return rc, dD


def _all_variants_equal_the_base(A, W, b, R, act, what, ldd=None, geom=None):
    """Runs tile 3 and every variant on the same device operands; returns tile 3's D."""
    K, N = W.shape
    ldd = ldd or N
    rc, wp = _pack(W)
    assert rc == 0, _last_error()
    dA, db, dR = _dev(A), _dev(b), _dev(R)
    if geom is None:
        M, g = A.shape[0], (0, 0, 0, 1)
    else:
        Bi, H, Wd, s = geom
        M, g = Bi * ((H - 1) // s + 1) * ((Wd - 1) // s + 1), geom
    rc, base = _gemm("tile", BASE_TILE, dA, M, K, K, wp, N, db, dR, N, act, ldd, g)
    assert rc == 0, _last_error()
    assert not bool((base[:, :N] == SENTINEL).any()), f"{what}: tile 3 left part of D unwritten"
    for v in VARIANTS:
        rc, D = _gemm("variant", v, dA, M, K, K, wp, N, db, dR, N, act, ldd, g)
        assert rc == 0, _last_error()
        assert np.array_equal(_bits(base), _bits(D)), f"{what}: variant {v} gives other bits than tile 3"
    assert torch.equal(dA.cpu(), torch.from_numpy(A)), "an input was written"
    return base


@pytest.mark.parametrize("K", [32, 64, 96, 128, 160])          # 1 to 5 slices
@pytest.mark.parametrize("M", [1, 65, 130, 300])
def test_every_variant_gives_the_bits_of_tile_3(M, K):
    for N in (16, 64, 80, 144, 272):
        A, W, b, R = _operands(M, K, N, True, True, seed=7000 + 1000 * M + 10 * K + N)
        _all_variants_equal_the_base(A, W, b, R, 1, f"({M}, {K}, {N})")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("act", [0, 1])
def test_all_eight_epilogues_on_every_variant(bias, res, act):
    A, W, b, R = _operands(130, 96, 144, bias, res, seed=31)
    _all_variants_equal_the_base(A, W, b, R, act, f"bias={bias} R={res} act={act}")


def test_padded_ldd_is_left_alone_and_a_second_call_repeats_the_bits():
    M, K, N = 130, 160, 144
    A, W, b, R = _operands(M, K, N, True, True, seed=37)
    first = _all_variants_equal_the_base(A, W, b, R, 1, "ldd = N + 8", ldd=N + 8)
    assert first.shape == (M, N + 8) and bool((first[:, N:] == SENTINEL).all()), "the padding columns of D were written"
    again = _all_variants_equal_the_base(A, W, b, R, 1, "ldd = N + 8, again", ldd=N + 8)      # compares all of D, padding too
    assert np.array_equal(_bits(first), _bits(again)), "same operands, different bits"


@pytest.mark.parametrize("hw", [(5, 7), (6, 8)])
def test_a_strided_1x1_on_every_variant(hw):
    H, Wd = hw
    Bi, K, N, s = 2, 96, 80, 2
    r = np.random.default_rng(H * Wd + 1)
    x = r.standard_normal((Bi * H * Wd, K), dtype=np.float32)
    W = (r.standard_normal((K, N), dtype=np.float32) * np.float32(np.sqrt(2.0 / K))).astype(np.float32)
    b = r.standard_normal(N, dtype=np.float32) * np.float32(0.1)
    _all_variants_equal_the_base(x, W, b, None, 1, f"stride 2 of {H}x{Wd}", geom=(Bi, H, Wd, s))


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 7), (9, 6)])
def test_conv3x3_on_every_variant(hw, epilogue):
    H, Wd = hw
    Bi = 2
    for C in (32, 64):
        for N in (16, 80):
            g = torch.Generator().manual_seed(H * 100 + Wd * 10 + C + N + 5)
            x = torch.randn((Bi, H, Wd, C), generator=g) + torch.arange(1, Bi * H * Wd + 1, dtype=torch.float32).view(Bi, H, Wd, 1) * 0.25
            w = (torch.randn((9 * C, N), generator=g) * (2.0 / (9 * C)) ** 0.5).numpy()
            b = torch.randn((N,), generator=g) * 0.1 if epilogue else None
            rc, wp = _pack(w)
            assert rc == 0, _last_error()
            dx, db = x.cuda(), None if b is None else b.cuda()
            act = 1 if epilogue else 0
            rc, base = _conv("tile", BASE_TILE, dx, Bi, H, Wd, C, wp, N, db, act)
            assert rc == 0, _last_error()
            assert not bool((base == SENTINEL).any())
            for v in VARIANTS:
                rc, D = _conv("variant", v, dx, Bi, H, Wd, C, wp, N, db, act)
                assert rc == 0, _last_error()
                assert np.array_equal(_bits(base), _bits(D)), f"3x3 {H}x{Wd} C={C} N={N}: variant {v} gives other bits than tile 3"
            assert torch.equal(dx.cpu(), x), "the input map was written"


def test_a_variant_past_the_last_is_refused_and_writes_nothing():
    A, W, b, R = _operands(8, 32, 16, False, False, seed=1)
    rc, wp = _pack(W)
    assert rc == 0, _last_error()
    rc, D = _gemm("variant", LAST + 1, _dev(A), 8, 32, 32, wp, 16, None, None, 16, 0, 16)
    assert rc == -1 and "dagr_gemm_split_bf16_variant" in _last_error()
    assert bool((D == SENTINEL).all()), "a refused call wrote D"
    x = torch.ones((1, 2, 4, 32), device="cuda")
    rc, wp = _pack(np.ones((9 * 32, 16), np.float32))
    assert rc == 0, _last_error()
    rc, D = _conv("variant", LAST + 1, x, 1, 2, 4, 32, wp, 16, None, 0)
    assert rc == -1 and "dagr_conv3x3_split_bf16_variant" in _last_error()
    assert bool((D == SENTINEL).all()), "a refused call wrote D"
