"""The pooled-level SplineConv entry points on the operands the engine actually passes: padded input rows (ldx > cin,
ldskip > cskip), outputs that are column slices of wider rows (ldc > N, a base that is not 16-byte aligned), a
device-side row count below the bound, rx != ry -- and the paired launch dagr_spline_conv_fused_pair, which every head
scale of every window goes through (two column halves of one row in, two adjacent column slices of one predictor row out).
tests/test_spline_fused_gpu.py runs the same kernels with ldx == cin, ldskip == cskip, ldc == N on fresh allocations, where
an off-by-stride error or an epilogue that rounds the written width up to a tile cannot show.

Three kinds of assertion:
  * against float64 (tests/spline_refs.py:conv_csr, tests/kernel_refs.py:gemm_epilogue) at the bar of
    tests/test_spline_fused_gpu.py: max abs error <= 1e-4 of max(1, max|want|);
  * bit equality with the same kernel on other addresses (contiguous copies; the single launches of a paired or multi
    launch): the split and the summation order depend on (n_nodes_max, cin, cskip, N) alone;
  * every output cell outside the written slice -- columns beside it, rows past the device-side count, padding columns of
    the A matrix -- keeps the sentinel it was preset to, bit for bit.

Shapes stay at T <= 1300, far below the 48 x CUs rows at which dagr_spline_conv_fused switches to k_conv_fused_narrow."""
import ctypes

import numpy as np
import pytest
import torch

from tests import kernel_refs as kr
from tests.spline_refs import conv_csr
from tests.test_spline_fused_gpu import _pack_wq

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
CUT = 19            # rows between the device-side count and the static bound


def _graph(rng, T, max_deg, rx, ry):
    deg = rng.integers(0, max_deg + 1, size=T)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    E = int(rowptr[-1])
    col = rng.integers(0, T, size=E).astype(np.int32)
    code = (rng.integers(0, 2 * rx + 1, size=E) | (rng.integers(0, 2 * ry + 1, size=E) << 16)).astype(np.int32)
    return rowptr, col, code


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _keeps_sentinel(t):
    return bool((t == SENTINEL).all())


def _addr(t, elem_offset=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * elem_offset)


# --------------------------------------------------------------------------------------------- paired launch
PAIRS = [  # T, cin, N_a, N_b
    (280, 64, 5, 2),        # cls_pred | reg_pred of a head scale
    (1300, 64, 5, 100),
    (150, 128, 5, 1),       # the pass form (obj_pred)
    (700, 16, 5, 8),
]


@pytest.mark.parametrize("T,cin,N_a,N_b", PAIRS)
def test_pair_on_column_halves_and_adjacent_slices(T, cin, N_a, N_b):
    from dagr_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(T * 31 + cin + N_b)
    r, den = 7, (14.0, 17.5)
    rowptr, col, code = _graph(rng, T, 8, r, r)
    live = T - CUT
    x = rng.standard_normal((T, 2 * cin)).astype(np.float32)          # x_a | x_b: halves of one row
    K = 26 * cin
    Wm = [(rng.standard_normal((K, n)) / np.sqrt(K)).astype(np.float32) for n in (N_a, N_b)]
    bias = [rng.standard_normal(n).astype(np.float32) for n in (N_a, N_b)]
    want = [conv_csr(rowptr, col, code, x[:, h * cin:(h + 1) * cin], None, Wm[h], bias[h], False, r, den) for h in (0, 1)]
    ldc = N_a + N_b + 3
    d_rowptr, d_col, d_code, d_x = _dev(rowptr, dev), _dev(col, dev), _dev(code, dev), _dev(x, dev)
    Wq = [_pack_wq(_dev(w, dev)) for w in Wm]
    d_bias = [_dev(b, dev) for b in bias]
    n_ptr = torch.tensor([live], dtype=torch.int32, device=dev)
    S = _lib.cur_stream(dev)
    out = torch.full((T, ldc), SENTINEL, dtype=torch.float32, device=dev)
    assert (out.data_ptr() + 4 * N_a) % 16 != 0                       # the second base: 20 bytes past an aligned address
    _lib.check(L.dagr_spline_conv_fused_pair(P(n_ptr), T, P(d_rowptr), P(d_col), P(d_code), 2 * cin, cin, r, r, den[0],
                                             den[1], ldc, 0, _addr(d_x), P(Wq[0]), P(d_bias[0]), _addr(out), N_a,
                                             _addr(d_x, cin), P(Wq[1]), P(d_bias[1]), _addr(out, N_a), N_b, S), "pair")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for h, (c0, n) in enumerate(((0, N_a), (N_a, N_b))):
        scale = max(1.0, float(np.abs(want[h]).max()))
        err = np.abs(got[:live, c0:c0 + n] - want[h][:live]).max() / scale
        print(f"pair {(T, cin, N_a, N_b)} job {h}: max abs error / scale = {err:.3e}")
        assert err <= 1e-4, (h, err)
    assert _keeps_sentinel(out[:, N_a + N_b:]) and _keeps_sentinel(out[live:])

    # the same two convs as single launches on the same pointers and strides: bit-equal (launch_conv_jobs: a job's split
    # does not depend on which other jobs share the launch)
    single = torch.full((T, ldc), SENTINEL, dtype=torch.float32, device=dev)
    for h, (c0, n) in enumerate(((0, N_a), (N_a, N_b))):
        _lib.check(L.dagr_spline_conv_fused(P(n_ptr), T, P(d_rowptr), P(d_col), P(d_code), _addr(d_x, h * cin), 2 * cin, cin,
                                            None, 0, 0, r, r, den[0], den[1], P(Wq[h]), P(d_bias[h]), _addr(single, c0), ldc,
                                            n, 0, S), "single")
    torch.cuda.synchronize()
    assert _same_bits(out, single)


def test_pair_rejects_a_bad_second_weight_pointer():
    from dagr_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    out = torch.full((4, 16), SENTINEL, dtype=torch.float32, device=dev)
    S = _lib.cur_stream(dev)
    assert f.data_ptr() % 16 == 0
    for wq_b in (None, _addr(f, 1)):
        rc = L.dagr_spline_conv_fused_pair(None, 4, P(z), P(z), P(z), 32, 16, 7, 7, 14.0, 14.0, 16, 0, P(f), P(f), None,
                                           _addr(out), 5, _addr(f, 16), wq_b, None, _addr(out, 5), 2, S)
        assert rc != 0 and b"bad second conv" in L.dagr_last_error()
    torch.cuda.synchronize()
    assert _keeps_sentinel(out)


# --------------------------------------------------------------------------------------------- strided single / multi
STRIDED = [  # T, cin, cskip, N, max_deg, relu, (rx, ry), den
    (700, 32, 0, 64, 9, True, (7, 7), (14.0, 17.5)),          # one column block
    (200, 64, 0, 200, 6, False, (7, 7), (14.0, 17.5)),        # four column blocks
    (300, 128, 0, 256, 9, True, (7, 7), (14.0, 17.5)),        # the pass form
    (1000, 64, 32, 64, 12, True, (7, 7), (14.0, 17.5)),       # cskip > 0
    (300, 16, 0, 21, 5, True, (7, 7), (14.0, 17.5)),          # ragged N
    (500, 48, 16, 40, 8, True, (7, 5), (14.0, 12.5)),         # rx != ry
]
XPAD, SPAD, CPAD, C0 = 6, 2, 5, 3       # ldx = cin + 6, ldskip = cskip + 2, ldc = N + 5, output base at column 3


class _Job:
    """One random conv on strided device operands, its float64 result, and its contiguous copies."""

    def __init__(self, spec, dev):
        T, cin, cskip, N, max_deg, relu, (rx, ry), den = spec
        rng = np.random.default_rng(T * 131 + cin + N)
        self.spec, self.T, self.live, self.N, self.K = spec, T, T - CUT, N, 26 * cin + cskip
        rowptr, col, code = _graph(rng, T, max_deg, rx, ry)
        x = rng.standard_normal((T, cin + XPAD)).astype(np.float32)              # random padding: a read of it shows
        xs = rng.standard_normal((T, cskip + SPAD)).astype(np.float32) if cskip else None
        self.Wm = (rng.standard_normal((self.K, N)) / np.sqrt(self.K)).astype(np.float32)
        bias = rng.standard_normal(N).astype(np.float32)
        self.want = conv_csr(rowptr, col, code, x[:, :cin], xs[:, :cskip] if cskip else None, self.Wm, bias, relu, (rx, ry),
                             den)
        self.scale = max(1.0, float(np.abs(self.want).max()))
        self.rowptr, self.col, self.code = _dev(rowptr, dev), _dev(col, dev), _dev(code, dev)
        self.x, self.xs, self.bias = _dev(x, dev), (_dev(xs, dev) if cskip else None), _dev(bias, dev)
        self.xc = self.x[:, :cin].contiguous()
        self.xsc = self.xs[:, :cskip].contiguous() if cskip else None
        self.Wq = _pack_wq(_dev(self.Wm, dev))
        self.n_ptr = torch.tensor([self.live], dtype=torch.int32, device=dev)
        self.out = torch.full((T, N + CPAD), SENTINEL, dtype=torch.float32, device=dev)

    def fused_args(self, strided=True, out=None):
        """Argument tuple of dagr_spline_conv_fused (without the stream)."""
        from dagr_amd import _lib
        P = _lib.ptr
        T, cin, cskip, N, _, relu, (rx, ry), den = self.spec
        x, xs = (self.x, self.xs) if strided else (self.xc, self.xsc)
        ldx, ldskip = (cin + XPAD, cskip + SPAD if cskip else 0) if strided else (cin, cskip)
        C, ldc = (_addr(self.out if out is None else out, C0), N + CPAD) if strided else (P(out), N)
        return (P(self.n_ptr), T, P(self.rowptr), P(self.col), P(self.code), P(x), ldx, cin, P(xs), ldskip, cskip, rx, ry,
                den[0], den[1], P(self.Wq), P(self.bias), C, ldc, N, int(relu))

    def check_strided(self, buf, what):
        got = buf.cpu().numpy()
        err = np.abs(got[:self.live, C0:C0 + self.N] - self.want[:self.live]).max() / self.scale
        print(f"{what} {self.spec}: max abs error / scale = {err:.3e}")
        assert err <= 1e-4, (what, err)
        assert _keeps_sentinel(buf[:, :C0]) and _keeps_sentinel(buf[:, C0 + self.N:]) and _keeps_sentinel(buf[self.live:])


@pytest.mark.parametrize("spec", STRIDED)
def test_fused_on_strided_operands(spec):
    from dagr_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    S = _lib.cur_stream(dev)
    j = _Job(spec, dev)
    _lib.check(L.dagr_spline_conv_fused(*j.fused_args(), S), "fused, strided")
    outc = torch.full((j.T, j.N), SENTINEL, dtype=torch.float32, device=dev)
    _lib.check(L.dagr_spline_conv_fused(*j.fused_args(strided=False, out=outc), S), "fused, contiguous")
    torch.cuda.synchronize()
    j.check_strided(j.out, "fused")
    # the same kernel and summation order on other addresses
    assert _same_bits(j.out[:, C0:C0 + j.N], outc)


def test_multi_of_strided_jobs_equals_single_launches():
    from dagr_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    S = _lib.cur_stream(dev)
    jobs = [_Job(STRIDED[0], dev), _Job(STRIDED[4], dev)]
    names = ("n_nodes_ptr", "n_nodes_max", "rowptr", "col", "code", "x", "ldx", "cin", "xskip", "ldskip", "cskip", "rx", "ry",
             "den_x", "den_y", "Wq", "bias", "C", "ldc", "N", "relu")
    val = lambda a: a.value if isinstance(a, ctypes.c_void_p) else a
    arr = (_lib.ConvJob * 2)(*[_lib.ConvJob(**{k: val(a) for k, a in zip(names, j.fused_args())}) for j in jobs])
    _lib.check(L.dagr_spline_conv_fused_multi(arr, 2, S), "multi")
    singles = [torch.full_like(j.out, SENTINEL) for j in jobs]
    for j, o in zip(jobs, singles):
        _lib.check(L.dagr_spline_conv_fused(*j.fused_args(out=o), S), "single")
    torch.cuda.synchronize()
    for j, o in zip(jobs, singles):
        j.check_strided(j.out, "multi")
        assert _same_bits(j.out, o)


@pytest.mark.parametrize("spec", STRIDED)
def test_tap_aggregate_and_gemm_on_strided_operands(spec):
    """dagr_spline_tap_aggregate + dagr_gemm_bias_act on the same operands; the A matrix has lda > K and keeps its
    padding.  With ldw % 8 == 0 and 16-byte aligned A / Wm this is the MFMA GEMM (csrc/gemm.hip)."""
    from dagr_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    S = _lib.cur_stream(dev)
    j = _Job(spec, dev)
    T, cin, cskip, N, _, relu, (rx, ry), den = spec
    K = j.K
    lda = (K + 3) // 4 * 4 + 8
    ldw = (N + 7) // 8 * 8
    A = torch.full((T, lda), SENTINEL, dtype=torch.float32, device=dev)
    Wpad = torch.zeros((K, ldw), dtype=torch.float32, device=dev)
    Wpad[:, :N] = _dev(j.Wm, dev)
    _lib.check(L.dagr_spline_tap_aggregate(P(j.n_ptr), T, P(j.rowptr), P(j.col), P(j.code), P(j.x), cin + XPAD, cin, P(j.xs),
                                           cskip + SPAD if cskip else 0, cskip, rx, ry, den[0], den[1], P(A), lda, S),
               "tap_aggregate")
    _lib.check(L.dagr_gemm_bias_act(P(j.n_ptr), T, P(A), lda, P(Wpad), ldw, P(j.bias), _addr(j.out, C0), N + CPAD, K, N,
                                    int(relu), S), "gemm")
    torch.cuda.synchronize()
    assert _keeps_sentinel(A[:, K:]) and _keeps_sentinel(A[j.live:])
    assert _same_bits(A[:j.live, 25 * cin:26 * cin], j.x[:j.live, :cin])                     # the root copy
    if cskip:
        assert _same_bits(A[:j.live, 26 * cin:K], j.xs[:j.live, :cskip])
    j.check_strided(j.out, "tap_aggregate + gemm")


# --------------------------------------------------------------------------------------------- scalar-tile GEMM
GEMMS = [(1, 1, 1), (37, 83, 6), (300, 2132, 100), (130, 67, 7)]     # m_max, K, N; ldw = N, N % 8 != 0


@pytest.mark.parametrize("M,K,N", GEMMS)
def test_scalar_tile_gemm(M, K, N):
    """k_gemm_bias_act (csrc/spline_conv.hip), the 64x64x16 scalar-tile kernel dagr_gemm_bias_act picks when ldw % 8 != 0 or
    an operand is unaligned.  The MFMA kernel the aligned call picks sums K in another order (four K slices, reduced through
    LDS), so the two are NOT compared bit for bit: each is held to float64 on its own.

    ldc = N rounded up to the 64-column tile, plus 3: an epilogue that wrote its whole tile would land in the sentinel
    columns of the same row."""
    from dagr_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    S = _lib.cur_stream(dev)
    rng = np.random.default_rng(M * 7 + K + N)
    assert N % 8 != 0
    lda, ldw, ldc = K + 3, N, (N + 63) // 64 * 64 + 3
    A = rng.standard_normal((M, lda)).astype(np.float32)
    Wm = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    bias = np.zeros(ldc, np.float32)
    bias[:N] = rng.standard_normal(N)
    bias[N:] = 99.0                                                    # never read
    d_A, d_W, d_bias = _dev(A, dev), _dev(Wm, dev), _dev(bias, dev)
    for live in (None, M - min(M, CUT)):                               # m_ptr NULL, and a device-side count below m_max
        m_ptr = None if live is None else torch.tensor([live], dtype=torch.int32, device=dev)
        rows = M if live is None else live
        for with_bias in (False, True):
            for relu in (0, 1):
                want, _ = kr.gemm_epilogue(A[:, :K], Wm, bias[:N] if with_bias else None, act=relu)
                C = torch.full((M, ldc), SENTINEL, dtype=torch.float32, device=dev)
                _lib.check(L.dagr_gemm_bias_act(P(m_ptr), M, P(d_A), lda, P(d_W), ldw, P(d_bias) if with_bias else None,
                                                P(C), ldc, K, N, relu, S), "gemm")
                torch.cuda.synchronize()
                got = C.cpu().numpy()
                label = (M, K, N, live, with_bias, relu)
                if rows:
                    err = np.abs(got[:rows, :N] - want[:rows]).max() / max(1.0, float(np.abs(want).max()))
                    assert err <= 1e-4, (label, err)
                assert _keeps_sentinel(C[:, N:]) and _keeps_sentinel(C[rows:]), label
