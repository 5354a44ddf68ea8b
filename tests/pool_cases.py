"""Reference and case builders for the direct tests of the voxel pooling (csrc/pooling.hip, pool_common.hpp, the fused
merge of gemm.hip).

``pool_reference`` restates everything ``dagr_pool_csr`` writes, in plain numpy / torch-CPU:
  * every decision the kernels take in fp32 is taken in fp32 here, one operation at a time (numpy does not fuse):
    the cluster id trunc(p / v), round_to_pixel (oracle.ops.round_to_pixel: torch.div(..., rounding_mode="floor")), the
    Cartesian attribute (oracle.ops.cartesian) and the LUT coordinate trunc((attr * r00 + r02) + 1e-3);
  * means are exact (Python integers: every fp32 is an integer multiple of 2^-149) and rounded once;
  * max is taken in float64, a tie between -0.0 and +0.0 gives +0.0 (the kernels' ordered-int mapping puts -0.0 below);
  * a node outside the grid (cx / cy out of range, ct not in {0, 1}, batch not in [0, B)) takes no part in anything, an
    edge whose source is such a node is dropped, bit 0 is expected;
  * batch_out = batch of the member with the largest node index;
  * edges = distinct (source cluster -> destination cluster) pairs without self pairs, rows ascending by source; with
    keep_order only those with t_max[dst] > t_max[src] (strict);
  * flags: bit 1 = a row with more than 64 distinct sources (before the keep_order filter: the set is filled first),
    bit 2 = e_out > e_cap, bit 3 = a LUT coordinate outside [0, 2 rx] x [0, 2 ry] among the edges that are written.
tests/test_pool_cases_cpu.py pins it to oracle.ops.pooling(..., exact_mean=True) and the codes to oracle.ops.cartesian +
SplineConvParams.lut_index, so that a wrong reference fails without a GPU.

``rowptr_out`` has T + 2 entries (include/dagr_hip.h); the kernels write entries 0 .. T (rows past the last cluster
repeat e_out) and never the spare last one, which the reference marks UNWRITTEN.
"""
import types

import numpy as np
import torch

from oracle import ops as oo

UNWRITTEN = -(1 << 31)          # marker of rowptr_out[T + 1]: no kernel writes it
ROW_SLOTS = 64                  # pool_common.hpp kRowSlots
SCAN_TILE = 2048                # pool_common.hpp kPoolScanTile
_SHIFT = 149                    # every finite fp32 is an integer multiple of 2^-149
f32 = np.float32


# --------------------------------------------------------------------------------------------------- descriptors
def make_desc(gx, gy, B, C, W, H, aggr=0, append_pos=0, keep_order=0, domain="wide", two_max=None):
    """Descriptor fields of dagr_pool_desc (B = batch_size, C = channels) as a namespace of python numbers.
    vx = fp32(1 / gx): the grid grid_cluster derives from it, trunc(0.9999999 / vx) + 1, is gx again (asserted).
    domain "wide": Cartesian max 1.0 and a LUT of (2 W + 1) x (2 H + 1) entries -- every edge of the unit square is in
    range; "net": what Net.__init__ / DAGR.cache_luts give a pooling of this voxel size (max = 2 max(vx, vy), rx =
    ceil(2 vx W)): sources up to two cells away are in range."""
    vx, vy = f32(1.0 / gx), f32(1.0 / gy)
    assert int(f32(0.9999999) / vx) + 1 == gx and int(f32(0.9999999) / vy) + 1 == gy
    if domain == "wide":
        M, rx, ry = 1.0, W, H
    else:
        M = 2.0 * float(max(vx, vy))
        rx, ry = int(np.ceil(2 * float(vx) * W)), int(np.ceil(2 * float(vy) * H))
    remap = torch.Tensor([[2 * M * W, 0, -M * W + rx], [0, 2 * M * H, -M * H + ry]])      # spline_conv.py:23-24
    return types.SimpleNamespace(
        gx=gx, gy=gy, B=B, C=C, vx=float(vx), vy=float(vy), inv_w=float(1 / torch.Tensor([W])[0]),
        inv_h=float(1 / torch.Tensor([H])[0]), two_max=float(f32(2 * M)) if two_max is None else float(f32(two_max)),
        r00=float(remap[0, 0]), r02=float(remap[0, 2]), r11=float(remap[1, 1]), r12=float(remap[1, 2]), rx=rx, ry=ry,
        aggr=aggr, append_pos=append_pos, keep_order=keep_order, W=W, H=H, cart_max=M)


def table_slots(d):
    return d.gx * d.gy * (d.B + 1)


# --------------------------------------------------------------------------------------------------- exact means
def _exact_sums(v, index, n_out):
    """Per-group sums of the fp32 array v[m, k] as Python integers in units of 2^-149 (object array [n_out, k])."""
    scaled = v.astype(np.float64) * 2.0 ** _SHIFT          # a power of two: exact, and below 2^1024
    ints = np.array([int(s) for s in scaled.ravel()], dtype=object).reshape(v.shape)
    order = np.argsort(index, kind="stable")
    starts = np.searchsorted(index[order], np.arange(n_out))
    return np.add.reduceat(ints[order], starts, axis=0)


def _round_once(total, count):
    """total * 2^-149 / count -> (the nearest fp32, the nearest float64).  int / int is correctly rounded in Python;
    going to fp32 through it rounds twice only when the double lands exactly between two fp32 values, which is settled
    with integers."""
    den = count << _SHIFT
    dbl = total / den
    flt = f32(dbl)
    if float(flt) != dbl and np.isfinite(flt):
        other = np.nextafter(flt, f32(np.inf) if dbl > float(flt) else f32(-np.inf))
        mid = (float(flt) + float(other)) / 2
        if dbl == mid:
            num_m, den_m = mid.as_integer_ratio()
            lhs, rhs = total * den_m, num_m * den
            if lhs != rhs:
                lo, hi = (flt, other) if flt < other else (other, flt)
                flt = hi if lhs > rhs else lo
    return flt, dbl


def _means(v, index, counts):
    n_out = len(counts)
    sums = _exact_sums(v, index, n_out)
    out32 = np.zeros((n_out, v.shape[1]), np.float32)
    out64 = np.zeros((n_out, v.shape[1]), np.float64)
    for c in range(n_out):
        for k in range(v.shape[1]):
            out32[c, k], out64[c, k] = _round_once(sums[c, k], int(counts[c]))
    return out32, out64


def lut_codes(d, pos_nodes, src, dst):
    """code = (ix & 0xffff) | (iy << 16) of the edges src -> dst between nodes at pos_nodes (fp32), int32 with C's
    wrap-around, and whether each edge's coordinates are inside the table."""
    if len(src) == 0:
        return np.zeros(0, np.int32), np.zeros(0, bool)
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    attr = oo.cartesian(torch.from_numpy(np.ascontiguousarray(pos_nodes, dtype=np.float32)), ei,
                        torch.tensor(d.two_max, dtype=torch.float32) / 2).numpy()
    assert attr.dtype == np.float32
    ix = np.trunc((attr[:, 0] * f32(d.r00) + f32(d.r02)) + f32(1e-3)).astype(np.int64)
    iy = np.trunc((attr[:, 1] * f32(d.r11) + f32(d.r12)) + f32(1e-3)).astype(np.int64)
    inside = (ix >= 0) & (ix <= 2 * d.rx) & (iy >= 0) & (iy <= 2 * d.ry)
    code = (((ix & 0xffff) | (iy << 16)) & 0xffffffff).astype(np.uint32).view(np.int32)
    return code, inside


# --------------------------------------------------------------------------------------------------- the reference
def pool_reference(d, x, pos, batch, rowptr, col, e_cap, n=None):
    """Everything dagr_pool_csr writes for the first n nodes (default: all) of the level (x[n, C], pos[n, 3], batch[n],
    CSR in-edges rowptr / col).  Returns a namespace: n_out, e_out, x_out[n_out, C] (fp32; mean: the exact mean rounded
    once), x_exact (float64, mean only), pos_out[n_out, 3], t_exact, batch_out, rowptr_out[T + 2], col[e_out],
    code[e_out], flags, cluster[n] (new id or -1) and overflow_rows {row: its full sorted source set}: such a row keeps
    64 of them (which 64 is not fixed; col / code hold the lowest 64 as a placeholder)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    batch = np.asarray(batch).astype(np.int64)
    rowptr = np.asarray(rowptr).astype(np.int64)
    col = np.asarray(col).astype(np.int64)
    n = len(pos) if n is None else min(int(n), len(pos))
    C, T = d.C, table_slots(d)
    assert x.shape[1] == C
    x, pos, batch = x[:n], pos[:n], batch[:n]
    # grid_cluster (torch_cluster): trunc(pos / size) per dimension in fp32; time voxel 1, batch voxel 1
    cx = np.trunc(pos[:, 0] / f32(d.vx)).astype(np.int64)
    cy = np.trunc(pos[:, 1] / f32(d.vy)).astype(np.int64)
    ct = np.trunc(pos[:, 2] / f32(1.0)).astype(np.int64)
    valid = (cx >= 0) & (cx < d.gx) & (cy >= 0) & (cy < d.gy) & (ct >= 0) & (ct <= 1) & (batch >= 0) & (batch < d.B)
    raw = cx + d.gx * (cy + d.gy * (ct + batch))
    ids = np.flatnonzero(valid)
    out = types.SimpleNamespace(T=T, overflow_rows={}, x_exact=None)
    out.cluster = np.full(n, -1, np.int64)
    flags = 1 if (~valid).any() else 0
    if len(ids) == 0:
        out.n_out = out.e_out = 0
        out.x_out, out.pos_out = np.zeros((0, C), np.float32), np.zeros((0, 3), np.float32)
        out.t_exact, out.batch_out = np.zeros(0), np.zeros(0, np.int64)
        out.rowptr_out = np.concatenate([np.zeros(T + 1, np.int64), [UNWRITTEN]])
        out.col, out.code, out.flags = np.zeros(0, np.int64), np.zeros(0, np.int32), flags
        return out
    unique, inv, perm, counts = oo.consecutive_cluster(torch.from_numpy(raw[ids]))
    inv, counts = inv.numpy(), counts.numpy()
    n_out = int(unique.numel())
    out.cluster[ids] = inv
    largest = np.full(n_out, -1, np.int64)
    np.maximum.at(largest, inv, ids)
    assert (ids[perm.numpy()] == largest).all()          # consecutive_cluster's perm: the last (= largest) member
    # features
    xv = x[ids]
    if d.aggr == 0:
        x64 = xv.astype(np.float64)
        mx = np.full((n_out, C), -np.inf)
        np.maximum.at(mx, inv, x64)
        pos_zero = np.zeros((n_out, C), bool)
        np.logical_or.at(pos_zero, inv, (x64 == 0) & ~np.signbit(x64))
        x_out = mx.astype(np.float32)
        zero = mx == 0
        x_out[zero] = np.where(pos_zero[zero], f32(0.0), f32(-0.0))
    else:
        x_out, out.x_exact = _means(xv, inv, counts)
    # positions: exact mean rounded once, then round_to_pixel on x, y
    p32, p64 = _means(pos[ids], inv, counts)
    wh_inv = torch.tensor([[d.inv_w, d.inv_h]], dtype=torch.float32)
    p32[:, :2] = oo.round_to_pixel(torch.from_numpy(p32[:, :2].copy()), wh_inv).numpy()
    # coarse edges
    deg = np.diff(rowptr[:n + 1])
    dst_node = np.repeat(np.arange(n), deg)
    src_node = col[rowptr[0]:rowptr[n]]
    assert len(src_node) == 0 or (src_node.min() >= 0 and src_node.max() < n), "sources must be live nodes"
    ok = valid[dst_node] & valid[src_node]
    cs, cd = out.cluster[src_node[ok]], out.cluster[dst_node[ok]]
    keep = cs != cd
    key = np.unique(cd[keep] * n_out + cs[keep])                # rows ascending, sources ascending within a row
    cd, cs = key // n_out, key % n_out
    in_deg = np.bincount(cd, minlength=n_out)
    over = np.flatnonzero(in_deg > ROW_SLOTS)
    if len(over):
        flags |= 2
    live = np.ones(len(cd), bool)
    if d.keep_order:
        t_max = np.full(n_out, -np.inf, np.float32)
        np.maximum.at(t_max, inv, pos[ids, 2])
        live = t_max[cd] > t_max[cs]
    for r in over:
        sel = np.flatnonzero(cd == r)
        out.overflow_rows[int(r)] = cs[sel].copy()
        passing = live[sel]
        if passing.all():
            live[sel[ROW_SLOTS:]] = False
        elif not passing.any():
            pass
        else:
            raise ValueError("a row beyond 64 sources whose sources the keep_order filter splits: size not determined")
    cd, cs = cd[live], cs[live]
    e_out = len(cd)
    row_n = np.bincount(cd, minlength=n_out)
    rp = np.concatenate([[0], np.cumsum(row_n)])
    out.rowptr_out = np.concatenate([rp, np.full(T - n_out, e_out, np.int64), [UNWRITTEN]])
    assert len(out.rowptr_out) == T + 2
    code, inside = lut_codes(d, p32, cs, cd)
    if (~inside[:min(e_out, e_cap)]).any():
        flags |= 8
    if e_out > e_cap:
        flags |= 4
    out.n_out, out.e_out, out.x_out, out.pos_out, out.t_exact = n_out, e_out, x_out, p32, p64[:, 2]
    out.batch_out, out.col, out.code, out.flags = batch[largest], cs, code, flags
    return out


def recode_reference(pos, rowptr, col, n, d, e_cap):
    """dagr_pool_recode: codes of the rows below n for the domain of d, entries below e_cap only.  Returns (code[E] with
    written[E] telling which entries the call writes, bit-3 flag)."""
    rowptr = np.asarray(rowptr).astype(np.int64)
    col = np.asarray(col).astype(np.int64)
    E = len(col)
    e_lim = min(int(rowptr[n]), e_cap, E)
    dst = np.repeat(np.arange(n), np.diff(rowptr[:n + 1]))[:e_lim]
    code, inside = lut_codes(d, pos, col[:e_lim], dst)
    full = np.zeros(E, np.int32)
    full[:e_lim] = code
    written = np.arange(E) < e_lim
    return full, written, (8 if (~inside).any() else 0)


# --------------------------------------------------------------------------------------------------- case builders
def csr_from_lists(src_lists):
    deg = np.array([len(s) for s in src_lists], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = np.array([s for row in src_lists for s in row], dtype=np.int32)
    return rowptr, col


def cell_centre(d, cx, cy):
    """A position inside voxel (cx, cy) whose fp32 division lands there whatever the rounding: the middle pixel-ish."""
    return (np.asarray(cx) + 0.5) * d.vx, (np.asarray(cy) + 0.5) * d.vy


def nodes_at_slots(d, slots, rng, jitter=0.3):
    """One node per entry of `slots` (table slots, repeats = more members): pos / batch that fall into exactly that slot.
    A slot of the last plane can only be reached by a t == 1.0 node of the last sample (QUIRK-1); the others are reached
    from their own sample, or -- one in four where possible -- by a t == 1.0 node of the sample below."""
    slots = np.asarray(slots, np.int64)
    cells = d.gx * d.gy
    plane, cell = slots // cells, slots % cells
    cx, cy = cell % d.gx, cell // d.gx
    leak = (plane == d.B) | ((plane > 0) & (rng.integers(0, 4, len(slots)) == 0))
    batch = np.where(leak, plane - 1, plane)
    px = (cx + 0.5 + rng.uniform(-jitter, jitter, len(slots))) * d.vx
    py = (cy + 0.5 + rng.uniform(-jitter, jitter, len(slots))) * d.vy
    t = np.where(leak, 1.0, np.floor(rng.uniform(0, 1, len(slots)) * 64) / 64)
    return np.stack([px, py, t], 1).astype(np.float32), batch.astype(np.int32)


def random_level(d, n, rng, k=5, leak_every=37, t_steps=8, reach=1):
    """A level of n nodes on the pixel grid of a W x H sensor (pos = pixel / extent in fp32, many of them exactly on a
    voxel boundary), t quantised to t_steps values (clusters share their t_max), every leak_every-th node at t == 1.0
    (QUIRK-1), and up to k in-edges per node from nodes of its sample at most `reach` voxels away (duplicates and
    self-loops included: the pooling has to drop them)."""
    W, H = d.W, d.H
    xp, yp = rng.integers(0, W, n), rng.integers(0, H, n)
    b = np.sort(rng.integers(0, d.B, n))
    pos = np.stack([xp.astype(np.float32) / f32(W), yp.astype(np.float32) / f32(H),
                    (np.floor(rng.uniform(0, 1, n) * t_steps) / t_steps).astype(np.float32)], 1).astype(np.float32)
    if leak_every:
        pos[leak_every - 1::leak_every, 2] = 1.0
    cx = np.trunc(pos[:, 0] / f32(d.vx)).astype(np.int64)
    cy = np.trunc(pos[:, 1] / f32(d.vy)).astype(np.int64)
    near = (np.abs(cx[:, None] - cx[None, :]) <= reach) & (np.abs(cy[:, None] - cy[None, :]) <= reach) & \
           (b[:, None] == b[None, :])
    rows = []
    for i in range(n):
        cand = np.flatnonzero(near[i])
        m = int(rng.integers(0, k + 1))
        rows.append(rng.choice(cand, size=m).tolist() if m else [])
    rowptr, col = csr_from_lists(rows)
    return pos, b.astype(np.int32), rowptr, col


def raw_ids(d, pos, batch):
    """Table slot of every node (valid nodes only make sense), for the value builders below."""
    cx = np.trunc(pos[:, 0] / f32(d.vx)).astype(np.int64)
    cy = np.trunc(pos[:, 1] / f32(d.vy)).astype(np.int64)
    ct = np.trunc(pos[:, 2]).astype(np.int64)
    return cx + d.gx * (cy + d.gy * (ct + np.asarray(batch, np.int64)))


def max_values(rng, group, C):
    """Features for max: per (cluster, channel) one of six kinds -- mixed signs, all negative, denormals of both signs,
    +-inf among finite values, -0.0 with +0.0 under negative values, and -0.0 with negative denormals only (the maximum
    is -0.0).  No NaN: the ordered-int mapping has no place for it and the reference pooling never sees one."""
    n = len(group)
    kind = (np.asarray(group)[:, None] + np.arange(C)[None, :]) % 6
    u = rng.standard_normal((n, C)).astype(np.float32)
    tiny = (rng.integers(1, 1000, (n, C)).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    sign = np.where(rng.integers(0, 2, (n, C)) == 0, f32(-1), f32(1))
    x = u * f32(3)
    x = np.where(kind == 1, -np.abs(u) - f32(0.5), x)
    x = np.where(kind == 2, sign * tiny, x)
    x = np.where(kind == 3, rng.choice(np.array([-np.inf, -np.inf, -3.5, 2.0, np.inf], np.float32), (n, C)), x)
    x = np.where(kind == 4, rng.choice(np.array([-0.0, 0.0, -1.0, -0.0], np.float32), (n, C)), x)
    x = np.where(kind == 5, np.where(rng.integers(0, 2, (n, C)) == 0, f32(-0.0), -tiny), x)
    return x.astype(np.float32)


def mean_values(rng, group, C):
    """Features for mean: magnitudes 2^-20 .. 2^10 with mixed signs; on every third (cluster, channel) the members
    alternate +-2^9 plus a small term, so that they cancel to a small mean.  |v| < 2^11: with up to 2048 members
    |v| n < 2^31, the range of the 2^-32 fixed-point accumulator."""
    n = len(group)
    group = np.asarray(group)
    e = rng.integers(-20, 11, (n, C)).astype(np.float64)
    x = (rng.uniform(1, 2, (n, C)) * 2.0 ** e * np.where(rng.integers(0, 2, (n, C)) == 0, -1.0, 1.0)).astype(np.float32)
    order = np.argsort(group, kind="stable")
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    first = np.searchsorted(group[order], group)
    alt = np.where((rank - first) % 2 == 0, 512.0, -512.0)[:, None]
    small = rng.uniform(-1, 1, (n, C)) * 2.0 ** -12
    cancel = ((group[:, None] + np.arange(C)[None, :]) % 3) == 1
    return np.where(cancel, (alt + small).astype(np.float32), x).astype(np.float32)


def fan_in_case(d, n_src, rng, dup=3, dst_members=4, dst_cell=None, t_dst=0.5, t_src=None):
    """One destination cluster whose members receive edges from n_src distinct source clusters (cells of sample 0 other
    than the destination's), each source inserted by `dup` edges spread over the destination's members, plus a few edges
    between the sources.  t_src: per-source t (default: all 0.25) -- with keep_order the sources at or above t_dst drop.
    Returns pos, batch, rowptr, col, the destination's table slot and the sources' slots."""
    cells = d.gx * d.gy
    dst_cell = cells // 2 if dst_cell is None else dst_cell
    others = np.array([c for c in range(cells) if c != dst_cell])
    src_cells = np.sort(rng.choice(others, size=n_src, replace=False))
    t_src = np.full(n_src, 0.25) if t_src is None else np.asarray(t_src, np.float64)
    px, py, t = [], [], []
    for c, ts in zip(src_cells, t_src):
        x_, y_ = cell_centre(d, c % d.gx, c // d.gx)
        px.append(x_); py.append(y_); t.append(ts)
    first_dst = n_src
    for m in range(dst_members):
        x_, y_ = cell_centre(d, dst_cell % d.gx, dst_cell // d.gx)
        px.append(x_ + (m - 1) * d.vx * 0.1); py.append(y_); t.append(t_dst if m == 0 else t_dst / 2)
    n = n_src + dst_members
    rows = [[] for _ in range(n)]
    for s in range(n_src):
        for r in range(dup):
            rows[first_dst + (s + r) % dst_members].append(s)
    for s in range(1, n_src, 7):                    # a few rows besides the big one
        rows[s].append(s - 1)
        rows[s].append(first_dst)
    for row in rows:
        rng.shuffle(row)
    rowptr, col = csr_from_lists(rows)
    pos = np.stack([px, py, t], 1).astype(np.float32)
    return pos, np.zeros(n, np.int32), rowptr, col, dst_cell, src_cells
