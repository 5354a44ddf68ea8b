"""The two-stage K loop of the split-bf16 kernel (csrc/gemm_split_bf16.hip) and its 64-column tiles, called directly: slice
counts that leave the loop with no steady state, with both stages in use and with an odd and an even number of slices; the
four tiles the entry points take; the same bits from every tile and from every call.  Both bars of
tests/test_gemm_split_bf16_gpu.py hold for every result."""
import numpy as np
import pytest

from tests.test_gemm_split_bf16_gpu import SENTINEL, _check_gemm, _last_error, _operands, _split

pytestmark = pytest.mark.gpu

TILES = (1, 2, 3, 4)               # 64 x 128, 32 x 128, 64 x 64, 32 x 64


def _bits(D):
    return np.ascontiguousarray(D).view(np.int32)


@pytest.mark.parametrize("K", [32, 64, 96, 160])           # 1, 2, 3 and 5 slices
@pytest.mark.parametrize("M", [1, 65, 130])
def test_every_slice_count_on_every_tile_gives_the_same_bits(M, K):
    for N in (16, 64, 80, 144):
        A, W, b, R = _operands(M, K, N, True, True, seed=1000 * M + 10 * K + N)
        D = _check_gemm(A, W, b, R, 1, f"({M}, {K}, {N}) tile 0")
        for tile in TILES + (0,):
            rc, other = _split(A, W, b, R, 1, tile=tile)
            assert rc == 0, _last_error()
            assert np.array_equal(_bits(D), _bits(other)), f"({M}, {K}, {N}): tile {tile} gives other bits than tile 0"


@pytest.mark.parametrize("N", [64, 192])
def test_the_64_column_tiles_leave_the_padding_of_d_alone(N):
    M, K = 130, 96
    A, W, b, R = _operands(M, K, N, True, True, seed=N)
    first = None
    for tile in (3, 4, 0):
        D = _check_gemm(A, W, b, R, 1, f"N = {N} tile {tile}", ldd=N + 8, tile=tile)
        assert D.shape == (M, N + 8) and np.all(D[:, N:] == SENTINEL), "the padding columns of D were written"
        first = D if first is None else first
        assert np.array_equal(_bits(D), _bits(first)), f"tile {tile} gives other bits"


def test_a_tile_number_past_the_last_is_refused():
    A, W, b, R = _operands(8, 32, 16, False, False, seed=1)
    rc, D = _split(A, W, b, R, 0, tile=5)
    assert rc == -1 and "dagr_gemm_split_bf16" in _last_error()
    assert np.all(D == SENTINEL), "a refused call wrote D"
