"""The pooling merge fused into a SplineConv epilogue (csrc/gemm.hip: k_conv_fused with PoolFuse, pool_common.hpp:
pool_merge_node): dagr_spline_conv_fused_pool followed by dagr_pool_csr(n_max = 0) against the unfused pair,
dagr_spline_conv_fused followed by dagr_pool_csr(n_max = T), on the same random conv job.  The conv is the same kernel and
every pooling reduction is order-free, so the conv output and every pooling output are bit-identical; separately the
pooled result meets the bars of tests/test_pool_csr_direct_gpu.py against tests/pool_cases.py:pool_reference applied to
the conv's own output.  Three jobs go through one pair of workspaces: two nodes of each lie outside the grid (bit 0, sticky)
and the device-side node count is below the static bound; the second job's conv output is scaled down to about 2^-18 (inputs
times 2^-18, no bias), where the mean's rounding of every term to 2^-32 is far above an fp32 ulp."""
import ctypes

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from tests import pool_cases as pc
from tests.test_pool_csr_direct_gpu import (DEV, bits, c_desc, check_against_reference, new_workspace, output_buffers,
                                            snapshot)
from tests.test_spline_fused_gpu import _random_job

pytestmark = pytest.mark.gpu


def _pool_csr_dev(d, ws, n_ptr, n_max, x, ldx, pos, batch, rowptr, col, e_cap):
    L, P = _lib.lib(), _lib.ptr
    ob = output_buffers(d, e_cap)
    scratch = torch.zeros((max(n_max, 1),), dtype=torch.int32, device=DEV)
    cd = c_desc(d)
    _lib.check(L.dagr_pool_csr(ctypes.byref(cd), P(ws), P(n_ptr), n_max, P(x), ldx, P(pos), P(batch), P(rowptr), P(col),
                               P(scratch), P(ob.x), ob.ldo, 0, P(ob.pos), P(ob.batch), P(ob.counts), P(ob.rowptr), P(ob.col),
                               P(ob.code), ctypes.c_void_p(ob.counts.data_ptr() + 4), e_cap, _lib.cur_stream(DEV)),
               "pool_csr")
    return snapshot(ob, d, ws)


JOBS = [(1000, 900), (333, 333), (1210, 1100)]          # (T, live): no T is a multiple of 16


@pytest.mark.parametrize("N", [16, 24, 64])
@pytest.mark.parametrize("keep_order", [0, 1])
@pytest.mark.parametrize("aggr", [0, 1])
def test_fused_merge_equals_the_unfused_pair(aggr, keep_order, N):
    L, P = _lib.lib(), _lib.ptr
    S = _lib.cur_stream(DEV)
    cin = 32
    assert L.dagr_spline_conv_fused_passes(cin, 0) == 1            # only the single-pass form is fused
    d = pc.make_desc(15, 11, 2, N, 60, 44, aggr=aggr, keep_order=keep_order, append_pos=1)
    cd = c_desc(d)
    rng = np.random.default_rng(7000 + 100 * aggr + 10 * keep_order + N)
    ws_f, ws_u = new_workspace(d), new_workspace(d)
    sticky = 0
    for T, live in JOBS:
        assert T % 16 != 0
        job, out, keep = _random_job(rng, DEV, T, cin, 0, N, 6, True, live=live)
        n_ptr, d_rowptr, d_col = keep[0], keep[1], keep[2]
        d_col.remainder_(live)                                     # sources are live nodes
        if T == 333:                                               # outputs around 2^-18: the 2^-32 grid of the mean shows
            keep[4].mul_(2.0 ** -18)
            keep[7].zero_()
        pos, batch, _, _ = pc.random_level(d, T, rng, k=0)
        pos[5, 0], batch[17] = 1.25, d.B                           # two nodes outside the grid
        d_pos = torch.from_numpy(pos).to(DEV)
        d_batch = torch.from_numpy(batch.astype(np.int32)).to(DEV)
        rowptr, col = d_rowptr.cpu().numpy(), d_col.cpu().numpy()
        e_cap = int(rowptr[live]) + 5
        j = job
        # unfused: the conv, then accumulation + scan + emit
        _lib.check(L.dagr_spline_conv_fused(j.n_nodes_ptr, j.n_nodes_max, j.rowptr, j.col, j.code, j.x, j.ldx, j.cin, j.xskip,
                                            j.ldskip, j.cskip, j.rx, j.ry, j.den_x, j.den_y, j.Wq, j.bias, j.C, j.ldc, j.N,
                                            j.relu, S), "conv_fused")
        conv_u = out.clone()
        got_u = _pool_csr_dev(d, ws_u, n_ptr, T, conv_u, N, d_pos, d_batch, d_rowptr, d_col, e_cap)
        # fused: the conv with the accumulation in its epilogue, then scan + emit only
        out.fill_(7.0)
        scratch = torch.zeros((T,), dtype=torch.int32, device=DEV)
        _lib.check(L.dagr_spline_conv_fused_pool(j.n_nodes_ptr, j.n_nodes_max, j.rowptr, j.col, j.code, j.x, j.ldx, j.cin,
                                                 j.xskip, j.ldskip, j.cskip, j.rx, j.ry, j.den_x, j.den_y, j.Wq, j.bias,
                                                 j.C, j.ldc, j.N, j.relu, ctypes.byref(cd), P(ws_f), P(d_pos), P(d_batch),
                                                 P(scratch), S), "conv_fused_pool")
        got_f = _pool_csr_dev(d, ws_f, n_ptr, 0, out, N, d_pos, d_batch, d_rowptr, d_col, e_cap)
        assert torch.equal(out, conv_u)
        assert bool((out[live:] == 7.0).all()) and not bool((out[:live] == 7.0).all())
        assert (got_f.n_out, got_f.e_out, got_f.flags) == (got_u.n_out, got_u.e_out, got_u.flags)
        for key in ("x", "pos", "batch", "rowptr", "col", "code"):
            assert (bits(getattr(got_f, key)) == bits(getattr(got_u, key))).all(), key
        # ... and both are right
        ref = pc.pool_reference(d, conv_u.cpu().numpy()[:, :N], pos, batch, rowptr, col, e_cap, n=live)
        assert ref.flags == 1 and not ref.overflow_rows and ref.n_out > 100 and ref.e_out > 300
        sticky |= ref.flags
        check_against_reference(got_f, ref, d, expect_flags=sticky)
