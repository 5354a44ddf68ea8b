"""tests/pool_cases.py:pool_reference (the reference of the direct pooling tests) held to the oracle on the CPU:
oracle.ops.pooling(..., exact_mean=True) for nodes, features, positions and edges, oracle.ops.cartesian +
SplineConvParams.lut_index for the LUT codes, on random levels with voxel-boundary positions, shared t_max values and the
t == 1.0 leak (QUIRK-1), for both aggregations, with and without keep_temporal_ordering.  What the oracle has no word on
(nodes outside the grid, the 64-source bound, the edge capacity, the table range) is checked on constructed cases."""
import numpy as np
import pytest
import torch

from oracle import ops as oo
from tests import pool_cases as pc


def _pooling_params(d):
    pp = oo.PoolingParams(torch.tensor([d.vx, d.vy, 1.0]), d.W, d.H, d.B, torch.tensor(d.two_max) / 2,
                          "max" if d.aggr == 0 else "mean")
    assert float(pp.wh_inv[0, 0]) == d.inv_w and float(pp.wh_inv[0, 1]) == d.inv_h
    return pp


def _edge_index(rowptr, col):
    dst = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return torch.from_numpy(np.stack([col.astype(np.int64), dst]))


GRIDS = [  # gx, gy, B, W, H, n, domain
    (56, 40, 2, 320, 215, 1500, "net"),        # pool1 of the DSEC geometry
    (15, 11, 3, 60, 44, 900, "wide"),          # 4-pixel cells: a quarter of the nodes sit exactly on a voxel boundary
    (7, 5, 1, 320, 215, 400, "net"),           # pool4-like: a few crowded clusters
]


@pytest.mark.parametrize("keep_order", [0, 1])
@pytest.mark.parametrize("aggr", [0, 1])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}b{g[2]}")
def test_reference_equals_the_oracle_pooling(grid, aggr, keep_order):
    gx, gy, B, W, H, n, domain = grid
    C = 5
    d = pc.make_desc(gx, gy, B, C, W, H, aggr=aggr, keep_order=keep_order, domain=domain)
    rng = np.random.default_rng(gx * 100 + aggr * 10 + keep_order)
    pos, batch, rowptr, col = pc.random_level(d, n, rng)
    assert (pos[:, 2] == 1.0).sum() > 5                                # QUIRK-1 present
    grp = pc.raw_ids(d, pos, batch)
    x = pc.max_values(rng, grp, C) if aggr == 0 else pc.mean_values(rng, grp, C)
    ref = pc.pool_reference(d, x, pos, batch, rowptr, col, e_cap=1 << 30)
    pp = _pooling_params(d)
    tx = torch.from_numpy(x)
    want = oo.pooling(pp, tx.double() if aggr == 1 else tx, torch.from_numpy(pos), torch.from_numpy(batch).long(),
                      _edge_index(rowptr, col), exact_mean=True, keep_temporal_ordering=bool(keep_order))
    wx, wpos, wbatch, wei, wattr = want
    assert ref.n_out == wx.shape[0] and ref.flags & 7 == 0
    assert (ref.batch_out == wbatch.numpy()).all()
    assert (ref.pos_out[:, :2] == wpos[:, :2].numpy()).all()
    assert np.abs(ref.pos_out[:, 2] - wpos[:, 2].numpy()).max() <= 2.0 ** -24
    if aggr == 0:
        assert (ref.x_out == wx.numpy()).all()                          # -0.0 == +0.0 here; signs: the test below
    else:
        # the oracle's mean summed in float64: within one fp32 rounding of the exact one, plus what the float64 sum of
        # cancelling +-512 terms can lose
        w = wx.float().numpy()
        assert (np.abs(ref.x_out - w) <= 2.0 ** -23 * np.abs(w) + 2.0 ** -40).all()
        assert (np.abs(ref.x_exact - wx.numpy()) <= 2.0 ** -52 * np.abs(ref.x_exact) + 2.0 ** -40).all()
    # edges: the oracle's unique(dim=-1) columns are (source, destination) sorted by source; the reference is CSR
    dst = np.repeat(np.arange(ref.n_out), np.diff(ref.rowptr_out[:ref.n_out + 1]))
    got = np.stack([ref.col, dst])
    got = got[:, np.lexsort((got[1], got[0]))]
    assert got.shape == tuple(wei.shape) and (got == wei.numpy()).all()
    assert ref.e_out == wei.shape[1] > 50
    assert (np.diff(ref.rowptr_out[:-1]) >= 0).all() and (ref.rowptr_out[ref.n_out:-1] == ref.e_out).all()
    assert ref.rowptr_out[-1] == pc.UNWRITTEN and len(ref.rowptr_out) == pc.table_slots(d) + 2
    if keep_order:
        off = pc.pool_reference(pc.make_desc(gx, gy, B, C, W, H, aggr=aggr, domain=domain), x, pos, batch, rowptr, col,
                                e_cap=1 << 30)
        assert ref.e_out < off.e_out
        t_max = oo.scatter_max(torch.from_numpy(pos[:, 2:]), torch.from_numpy(ref.cluster), ref.n_out)[:, 0].numpy()
        dst_off = np.repeat(np.arange(off.n_out), np.diff(off.rowptr_out[:off.n_out + 1]))
        assert (t_max[off.col] == t_max[dst_off]).sum() > 0             # ties exist and are dropped both ways
    # LUT codes: T.Cartesian on the pooled positions, then message_lut's index with this domain's remapping matrix
    sc = oo.SplineConvParams(None, None, None)
    sc.remap = torch.Tensor([[d.r00, 0, d.r02], [0, d.r11, d.r12]])
    attr = oo.cartesian(torch.from_numpy(ref.pos_out), torch.from_numpy(np.stack([ref.col, dst])), pp.cart_max)
    ix, iy = sc.lut_index(attr)
    assert (ref.code == (ix | (iy << 16)).int().numpy()).all()
    inside = ((ix >= 0) & (ix <= 2 * d.rx) & (iy >= 0) & (iy <= 2 * d.ry)).numpy()
    assert bool(ref.flags & 8) == (not inside.all())
    # the oracle's own edge attributes are the same numbers
    order = np.lexsort((dst, ref.col))
    assert torch.equal(attr[torch.from_numpy(order)][:, :2], wattr[:, :2])


def test_reference_max_of_signed_zeros_and_specials():
    d = pc.make_desc(4, 4, 1, 6, 16, 16)
    pos = np.tile(np.array([[0.1, 0.1, 0.5]], np.float32), (3, 1))
    pos = np.concatenate([pos, np.array([[0.6, 0.6, 0.5]], np.float32)])
    x = np.array([[-0.0, -0.0, -np.inf, -1e-40, 1e-40, -np.inf],
                  [0.0, -0.0, -2.0, -2e-40, -3.0, -np.inf],
                  [-1.0, -3.0, -5.0, -1.0, -1e-40, -np.inf],
                  [-7.0, 0.0, np.inf, -0.0, 1.0, 2.0]], np.float32)
    ref = pc.pool_reference(d, x, pos, np.zeros(4, np.int32), np.zeros(5, np.int32), np.zeros(0, np.int32), 16)
    want = np.array([[0.0, -0.0, -2.0, -1e-40, 1e-40, -np.inf], [-7.0, 0.0, np.inf, -0.0, 1.0, 2.0]], np.float32)
    assert ref.n_out == 2 and (ref.x_out.view(np.int32) == want.view(np.int32)).all()


def test_reference_mean_is_exact_and_rounded_once():
    d = pc.make_desc(4, 4, 1, 3, 16, 16, aggr=1)
    # 1 + 2^-24 + 2^-60: the float64 quotient is exactly half way between two fp32 values, the true one lies above
    x = np.array([[3.0, 2.0 ** -20, 512.0], [2.0 ** -23, 2.0 ** 10, -512.0], [2.0 ** -59, -2.0 ** 10, 2.0 ** -30]], np.float32)
    x[:, 0] = [1.0, 1.0 + 2.0 ** -23, 1.0]
    pos = np.tile(np.array([[0.1, 0.1, 0.5]], np.float32), (3, 1))
    ref = pc.pool_reference(d, x, pos, np.zeros(3, np.int32), np.zeros(4, np.int32), np.zeros(0, np.int32), 16)
    assert ref.x_out[0, 1] == np.float32(2.0 ** -20 / 3) and ref.x_out[0, 2] == np.float32(2.0 ** -30 / 3)
    assert ref.x_exact[0, 0] == (3 + 2.0 ** -23) / 3
    f, dbl = pc._round_once((1 << 149) + (1 << 125) + 1, 1)       # 1 + 2^-24 + 2^-149
    assert dbl == 1 + 2.0 ** -24 and f == np.float32(1 + 2.0 ** -23)
    f, _ = pc._round_once((1 << 149) + (1 << 125), 1)             # the tie itself goes to even
    assert f == np.float32(1.0)


def test_reference_outside_nodes_and_flags():
    d = pc.make_desc(4, 4, 2, 1, 16, 16)
    cx, cy = pc.cell_centre(d, np.array([0, 1, 2, 3, 1]), np.array([0, 0, 0, 0, 1]))
    pos = np.stack([cx, cy, np.full(5, 0.5)], 1).astype(np.float32)
    batch = np.array([0, 0, 0, 0, 0], np.int32)
    bad = np.array([[1.0, 0.1, 0.5], [0.1, 0.1, 2.0], [0.1, 0.1, 0.5], [0.1, 0.1, 0.5]], np.float32)   # x >= gx vx, t = 2
    pos = np.concatenate([pos, bad])
    batch = np.concatenate([batch, [0, 0, 2, -1]]).astype(np.int32)              # batch = B, batch = -1
    rows = [[5, 6, 1], [0, 7, 8], [1], [2, 2, 3], [0], [0], [1], [2], [3]]
    rowptr, col = pc.csr_from_lists(rows)
    x = np.arange(9, dtype=np.float32).reshape(9, 1) + 100 * (np.arange(9) >= 5).reshape(9, 1)
    ref = pc.pool_reference(d, x, pos, batch, rowptr, col, e_cap=100)
    assert ref.flags == 1 and ref.n_out == 5 and (ref.cluster[5:] == -1).all()
    assert ref.x_out.max() == 4.0                                                 # the outside nodes' 100s took no part
    assert ref.col.tolist() == [1, 0, 1, 2, 0] and ref.rowptr_out[:6].tolist() == [0, 1, 2, 3, 4, 5]
    # the edge capacity: true counts and rows, bit 2
    capped = pc.pool_reference(d, x, pos, batch, rowptr, col, e_cap=2)
    assert capped.flags == 5 and capped.e_out == 5 and (capped.rowptr_out == ref.rowptr_out).all()
    # a narrow table: bit 3, codes still the wrapped formula
    far = pc.make_desc(4, 4, 2, 1, 16, 16, two_max=0.05)
    out = pc.pool_reference(far, x, pos, batch, rowptr, col, e_cap=100)
    assert out.flags == 9 and (out.col == ref.col).all() and not (out.code == ref.code).all()
    # only the first n nodes count
    rowptr, col = pc.csr_from_lists([[1], [0, 0], [1], [2, 2, 3], [0], [0], [1], [2], [3]])
    live = pc.pool_reference(d, x, pos, batch, rowptr, col, e_cap=100, n=5)
    assert live.flags == 0 and live.n_out == 5 and live.e_out == 5


def test_reference_row_bound_of_64_sources():
    d = pc.make_desc(16, 12, 1, 1, 64, 48)
    rng = np.random.default_rng(1)
    for n_src, flag in ((64, 0), (70, 2)):
        pos, batch, rowptr, col, dst_cell, src_cells = pc.fan_in_case(d, n_src, rng)
        x = np.zeros((len(pos), 1), np.float32)
        ref = pc.pool_reference(d, x, pos, batch, rowptr, col, e_cap=1000)
        row = int(ref.cluster[n_src])
        assert ref.flags == flag and ref.n_out == n_src + 1
        assert ref.rowptr_out[row + 1] - ref.rowptr_out[row] == 64
        assert (row in ref.overflow_rows) == (n_src > 64)
        if n_src > 64:
            assert len(ref.overflow_rows[row]) == 70
    # keep_order with ties: sources at the destination's t_max or above leave
    t_src = np.where(np.arange(64) % 3 == 0, 0.5, np.where(np.arange(64) % 3 == 1, 0.25, 0.75))
    pos, batch, rowptr, col, _, _ = pc.fan_in_case(d, 64, rng, t_src=t_src)
    dk = pc.make_desc(16, 12, 1, 1, 64, 48, keep_order=1)
    ref = pc.pool_reference(dk, np.zeros((len(pos), 1), np.float32), pos, batch, rowptr, col, e_cap=1000)
    row = int(ref.cluster[64])
    assert ref.flags == 0 and ref.rowptr_out[row + 1] - ref.rowptr_out[row] == 21


def test_recode_reference_is_the_pooling_code_in_another_domain():
    d = pc.make_desc(15, 11, 2, 1, 60, 44)
    rng = np.random.default_rng(3)
    pos, batch, rowptr, col = pc.random_level(d, 300, rng)
    ref = pc.pool_reference(d, np.zeros((300, 1), np.float32), pos, batch, rowptr, col, e_cap=1 << 30)
    rp = ref.rowptr_out[:ref.n_out + 1]
    code, written, flag = pc.recode_reference(ref.pos_out, rp, ref.col, ref.n_out, d, e_cap=1 << 30)
    assert flag == 0 and written.all() and (code == ref.code).all()
    code2, written2, _ = pc.recode_reference(ref.pos_out, rp, ref.col, ref.n_out - 10, d, e_cap=ref.e_out // 2)
    lim = min(int(rp[ref.n_out - 10]), ref.e_out // 2)
    assert written2.sum() == lim and (code2[:lim] == ref.code[:lim]).all()
