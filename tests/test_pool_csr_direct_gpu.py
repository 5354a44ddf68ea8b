"""dagr_pool_csr and dagr_pool_recode (csrc/pooling.hip: k_pool_accumulate, k_pool_order_rows, k_pool_scan_chained,
k_pool_emit, k_recode) on constructed inputs against tests/pool_cases.py:pool_reference.

Bars (every case unless it says otherwise): n_out, e_out, batch_out, rowptr_out, col, code, pos_out[:, :2] and the flag
word exact; max features bit for bit; mean features |got - ref| <= 2^-33 + 2^-23 |ref| with ref the exact mean (every
term is rounded to the nearest 2^-32: the average of n such errors is at most 2^-33; the division in double and the final
rounding to fp32 add less than one fp32 ulp); pos_out[:, 2] within 1e-6 of the exact mean; every buffer element the
contract does not cover -- rows at or beyond n_out, columns outside [xoff, xoff + C + 2 append_pos), col / code at or beyond
min(e_out, e_cap), rowptr_out[T + 1] -- still holds the sentinel it was filled with.

NaN features are left out: the ordered-int max has no place for them and the reference pooling never produces one.
Feature magnitudes stay below 2^20 and |v| * members below 2^31, the documented range of the mean's accumulator."""
import ctypes
import types

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from tests import pool_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SF = np.float32(-123456.0)              # sentinel of the float outputs
SI = np.int32(-1515870811)              # ... of the integer outputs (0xa5a5a5a5)
PAD = 64                                # sentinel entries behind col / code [e_cap]


def c_desc(d):
    return _lib.PoolDesc(batch_size=d.B, channels=d.C, gx=d.gx, gy=d.gy, vx=d.vx, vy=d.vy, inv_w=d.inv_w, inv_h=d.inv_h,
                         two_max=d.two_max, r00=d.r00, r02=d.r02, r11=d.r11, r12=d.r12, rx=d.rx, ry=d.ry, aggr=d.aggr,
                         append_pos=d.append_pos, keep_order=d.keep_order)


def new_workspace(d):
    L = _lib.lib()
    cd = c_desc(d)
    nbytes = L.dagr_pool_workspace_bytes(ctypes.byref(cd))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(L.dagr_pool_workspace_init(ctypes.byref(cd), _lib.ptr(ws), nbytes, _lib.cur_stream(DEV)), "ws_init")
    return ws


def device_level(d, x, pos, batch, rowptr, col, ldx=None):
    """The level's inputs on the device; x rows are ldx wide, the columns past C hold 1e30."""
    n_rows = len(pos)
    ldx = d.C if ldx is None else ldx
    xd = np.full((max(n_rows, 1), ldx), 1e30, np.float32)
    xd[:n_rows, :d.C] = x
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    col = np.asarray(col, np.int32)
    return types.SimpleNamespace(
        x=t(xd, np.float32), ldx=ldx, pos=t(pos if n_rows else np.zeros((1, 3)), np.float32),
        batch=t(batch if n_rows else np.zeros(1), np.int32), rowptr=t(rowptr, np.int32),
        col=t(col if len(col) else np.zeros(1), np.int32), n_rows=n_rows)


def output_buffers(d, e_cap, xoff=0, ldo=None):
    T = pc.table_slots(d)
    ldo = xoff + d.C + 2 * d.append_pos if ldo is None else ldo
    f = lambda shape: torch.full(shape, float(SF), dtype=torch.float32, device=DEV)
    i = lambda shape: torch.full(shape, int(SI), dtype=torch.int32, device=DEV)
    return types.SimpleNamespace(x=f((T, ldo)), pos=f((T, 3)), batch=i((T,)), counts=i((2,)), rowptr=i((T + 2,)),
                                 col=i((e_cap + PAD,)), code=i((e_cap + PAD,)), xoff=xoff, ldo=ldo, e_cap=e_cap)


def pool_status(d, ws):
    f = (ctypes.c_int32 * 1)()
    cd = c_desc(d)
    _lib.check(_lib.lib().dagr_pool_status(ctypes.byref(cd), _lib.ptr(ws), f, _lib.cur_stream(DEV)), "pool_status")
    return int(f[0])


def snapshot(ob, d, ws):
    flags = pool_status(d, ws)                      # synchronises the stream
    n_out, e_out = [int(v) for v in ob.counts.tolist()]
    return types.SimpleNamespace(n_out=n_out, e_out=e_out, x=ob.x.cpu().numpy(), pos=ob.pos.cpu().numpy(),
                                 batch=ob.batch.cpu().numpy(), rowptr=ob.rowptr.cpu().numpy(), col=ob.col.cpu().numpy(),
                                 code=ob.code.cpu().numpy(), flags=flags, xoff=ob.xoff, ldo=ob.ldo, e_cap=ob.e_cap)


def run_pool_csr(d, x, pos, batch, rowptr, col, e_cap, n_live=None, n_max=None, ws=None, ldx=None, xoff=0, ldo=None):
    """One dagr_pool_csr call: on `ws` or on a fresh workspace, every output pre-filled with a sentinel.  Returns the full
    buffers, the counts, the flag word (not asserted) and the workspace."""
    L = _lib.lib()
    P = _lib.ptr
    ws = new_workspace(d) if ws is None else ws
    lv = device_level(d, x, pos, batch, rowptr, col, ldx)
    n_max = lv.n_rows if n_max is None else n_max
    n_ptr = torch.tensor([lv.n_rows if n_live is None else n_live], dtype=torch.int32, device=DEV)
    ob = output_buffers(d, e_cap, xoff, ldo)
    scratch = torch.zeros((max(n_max, 1),), dtype=torch.int32, device=DEV)
    cd = c_desc(d)
    _lib.check(L.dagr_pool_csr(ctypes.byref(cd), P(ws), P(n_ptr), n_max, P(lv.x), lv.ldx, P(lv.pos), P(lv.batch),
                               P(lv.rowptr), P(lv.col), P(scratch), P(ob.x), ob.ldo, xoff, P(ob.pos), P(ob.batch),
                               P(ob.counts), P(ob.rowptr), P(ob.col), P(ob.code),
                               ctypes.c_void_p(ob.counts.data_ptr() + 4), e_cap, _lib.cur_stream(DEV)), "pool_csr")
    got = snapshot(ob, d, ws)
    got.ws = ws
    return got


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_against_reference(got, ref, d, expect_flags=None):
    """The bars of the module docstring.  Rows beyond 64 sources (ref.overflow_rows): 64 distinct, ascending members of the
    true set with their own codes; everything around them exact."""
    T, C = pc.table_slots(d), d.C
    n, xoff, e_cap = ref.n_out, got.xoff, got.e_cap
    assert (got.n_out, got.e_out) == (ref.n_out, ref.e_out)
    assert got.flags == (ref.flags if expect_flags is None else expect_flags)
    want_b = np.full(T, SI, np.int32)
    want_b[:n] = ref.batch_out
    assert (got.batch == want_b).all()
    want_r = ref.rowptr_out.copy()
    want_r[want_r == pc.UNWRITTEN] = SI
    assert (got.rowptr == want_r).all()
    m = min(ref.e_out, e_cap)
    want_col, want_code = np.full(e_cap + PAD, SI, np.int32), np.full(e_cap + PAD, SI, np.int32)
    want_col[:m], want_code[:m] = ref.col[:m], ref.code[:m]
    exact = np.ones(e_cap + PAD, bool)
    for row, members in ref.overflow_rows.items():
        lo, hi = int(ref.rowptr_out[row]), int(ref.rowptr_out[row + 1])
        assert hi <= e_cap
        exact[lo:hi] = False
        kept = got.col[lo:hi]
        assert hi - lo in (0, pc.ROW_SLOTS) and (np.diff(kept) > 0).all() and np.isin(kept, members).all()
        code, _ = pc.lut_codes(d, ref.pos_out, kept, np.full(hi - lo, row))
        assert (got.code[lo:hi] == code).all()
    assert (got.col[exact] == want_col[exact]).all() and (got.code[exact] == want_code[exact]).all()
    # positions
    want_p = np.full((T, 3), SF, np.float32)
    want_p[:n] = ref.pos_out
    assert (bits(got.pos[:, :2]) == bits(want_p[:, :2])).all()
    assert (bits(got.pos[n:, 2]) == bits(want_p[n:, 2])).all()
    if n:
        assert np.abs(got.pos[:n, 2].astype(np.float64) - ref.t_exact).max() <= 1e-6
    # features
    want_x = np.full((T, got.ldo), SF, np.float32)
    want_x[:n, xoff:xoff + C] = ref.x_out
    if d.append_pos:
        want_x[:n, xoff + C:xoff + C + 2] = ref.pos_out[:, :2]
    gx_ = got.x.copy()
    if d.aggr == 1 and n:
        g = gx_[:n, xoff:xoff + C].astype(np.float64)
        err = np.abs(g - ref.x_exact)
        bound = 2.0 ** -33 + 2.0 ** -23 * np.abs(ref.x_exact)
        assert (err <= bound).all(), f"mean features: {float((err - bound).max())} beyond the bound"
        gx_[:n, xoff:xoff + C] = ref.x_out
    assert (bits(gx_) == bits(want_x)).all()


def _features(d, rng, pos, batch):
    grp = pc.raw_ids(d, pos, batch)
    return pc.max_values(rng, grp, d.C) if d.aggr == 0 else pc.mean_values(rng, grp, d.C)


def _ref_and_run(d, x, pos, batch, rowptr, col, e_cap=None, n_live=None, **kw):
    full = pc.pool_reference(d, x, pos, batch, rowptr, col, e_cap=1 << 30, n=n_live)
    e_cap = full.e_out + 5 if e_cap is None else e_cap
    ref = pc.pool_reference(d, x, pos, batch, rowptr, col, e_cap=e_cap, n=n_live)
    got = run_pool_csr(d, x, pos, batch, rowptr, col, e_cap, n_live=n_live, **kw)
    return ref, got


# ------------------------------------------------------------------------------------------------ values and layouts
@pytest.mark.parametrize("append_pos", [0, 1])
@pytest.mark.parametrize("aggr", [0, 1])
@pytest.mark.parametrize("C", [1, 3, 64, 65, 130])
def test_values_widths_and_row_layouts(C, aggr, append_pos):
    """C below, at and above a wave's 64 lanes, input rows wider than C (ldx = C + 3), output rows that start at column 2
    and are 5 columns longer than what is written; max on negative / all-negative / denormal / infinite / signed-zero
    values, mean on magnitudes 2^-20 .. 2^10 and on members that cancel; voxel-boundary positions, t == 1.0 nodes."""
    d = pc.make_desc(15, 11, 2, C, 60, 44, aggr=aggr, append_pos=append_pos)
    rng = np.random.default_rng(1000 + 10 * C + 2 * aggr + append_pos)
    pos, batch, rowptr, col = pc.random_level(d, 1200, rng)
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col, ldx=C + 3, xoff=2, ldo=2 + C + 5)
    assert ref.flags == 0 and ref.n_out > 300 and ref.e_out > 1000
    assert (np.bincount(ref.cluster) == 1).any()                       # clusters of one among them
    check_against_reference(got, ref, d)


@pytest.mark.parametrize("aggr", [0, 1])
def test_keep_order_on_a_random_level(aggr):
    d = pc.make_desc(15, 11, 2, 3, 60, 44, aggr=aggr, keep_order=1, domain="net")
    rng = np.random.default_rng(77 + aggr)
    pos, batch, rowptr, col = pc.random_level(d, 1200, rng)
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    off = pc.pool_reference(pc.make_desc(15, 11, 2, 3, 60, 44, aggr=aggr, domain="net"), x, pos, batch, rowptr, col, 1 << 30)
    assert ref.flags == 0 and 0 < ref.e_out < off.e_out
    check_against_reference(got, ref, d)


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("how", ["n_max=0", "n_ptr=0"])
def test_empty_calls_write_counts_and_row_pointers_only(how):
    d = pc.make_desc(15, 11, 2, 3, 60, 44, aggr=1, append_pos=1)
    rng = np.random.default_rng(5)
    pos, batch, rowptr, col = pc.random_level(d, 50, rng)
    x = _features(d, rng, pos, batch)
    got = run_pool_csr(d, x, pos, batch, rowptr, col, 40, n_live=0, n_max=0 if how == "n_max=0" else 50)
    ref = pc.pool_reference(d, x, pos, batch, rowptr, col, 40, n=0)
    assert ref.n_out == ref.e_out == 0 and (ref.rowptr_out[:-1] == 0).all()
    check_against_reference(got, ref, d)


@pytest.mark.parametrize("aggr", [0, 1])
def test_one_node(aggr):
    d = pc.make_desc(15, 11, 2, 65, 60, 44, aggr=aggr, append_pos=1)
    rng = np.random.default_rng(6)
    pos = np.array([[0.5, 0.25, 1.0]], np.float32)               # a t == 1.0 node: its cluster is one plane up
    batch = np.array([1], np.int32)
    rowptr, col = pc.csr_from_lists([[0, 0]])                    # self loops only
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    assert ref.n_out == 1 and ref.e_out == 0 and ref.flags == 0
    check_against_reference(got, ref, d)


@pytest.mark.parametrize("aggr", [0, 1])
def test_device_side_count_below_the_static_bound(aggr):
    """*n_ptr < n_max: the rows at or beyond *n_ptr (positions outside the grid, huge features, a sample index out of
    range) change nothing and set no flag."""
    d = pc.make_desc(15, 11, 2, 3, 60, 44, aggr=aggr)
    rng = np.random.default_rng(8 + aggr)
    pos, batch, rowptr, col = pc.random_level(d, 700, rng)
    x = _features(d, rng, pos, batch)
    dead = 150
    pos = np.concatenate([pos, np.tile(np.array([[5.0, -3.0, 7.0]], np.float32), (dead, 1))])
    batch = np.concatenate([batch, np.full(dead, 99, np.int32)])
    x = np.concatenate([x, np.full((dead, 3), 3e38, np.float32)])
    rowptr = np.concatenate([rowptr, np.full(dead, rowptr[-1], np.int32)])
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col, n_live=700)
    assert ref.flags == 0 and ref.n_out > 250
    check_against_reference(got, ref, d)


@pytest.mark.parametrize("aggr", [0, 1])
def test_every_node_in_one_cluster(aggr):
    """2048 members of one voxel (every atomic of the launch hits the same accumulators) and one lone neighbour; mean:
    the largest member count the value range allows."""
    d = pc.make_desc(15, 11, 2, 3, 60, 44, aggr=aggr, append_pos=1)
    rng = np.random.default_rng(9 + aggr)
    n = 2048
    cx, cy = pc.cell_centre(d, 7, 5)
    pos = np.stack([cx + rng.uniform(-0.4, 0.4, n) * d.vx, cy + rng.uniform(-0.4, 0.4, n) * d.vy,
                    rng.uniform(0, 0.99, n)], 1).astype(np.float32)
    lone = np.array([[*pc.cell_centre(d, 8, 5), 0.5]], np.float32)
    pos = np.concatenate([pos, lone])
    batch = np.ones(n + 1, np.int32)
    rows = [[int(v) for v in rng.integers(0, n + 1, 3)] for _ in range(n)] + [[0, 5, 2047, n]]
    rowptr, col = pc.csr_from_lists(rows)
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    assert ref.n_out == 2 and ref.e_out == 2 and ref.flags == 0
    check_against_reference(got, ref, d)


def test_every_node_in_its_own_cluster():
    """One node per table slot, the last sample plane (t == 1.0 nodes only) included: n_out = T."""
    d = pc.make_desc(15, 11, 2, 3, 60, 44)
    rng = np.random.default_rng(10)
    T = pc.table_slots(d)
    pos, batch = pc.nodes_at_slots(d, rng.permutation(T), rng)
    rows = [[(i + 1) % T, (i * 7 + 3) % T, i] for i in range(T)]
    rowptr, col = pc.csr_from_lists(rows)
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    assert ref.n_out == T and ref.flags == 0 and ref.e_out > T
    check_against_reference(got, ref, d)


# ------------------------------------------------------------------------------------------------ scan tiles
def _tile_edge_case(d, rng, extra):
    T = pc.table_slots(d)
    tile = pc.SCAN_TILE
    slots = {0, T - 1}
    for k in range(tile, T + 1, tile):
        slots.update(s for s in (k - 1, k) if s < T)
    slots.update(int(s) for s in rng.integers(0, T, extra))
    slots = np.array(sorted(slots))
    slots = rng.permutation(np.concatenate([slots, slots[::3]]))          # every third slot has two members
    pos, batch = pc.nodes_at_slots(d, slots, rng)
    n = len(slots)
    rows = [[(i + 1) % n, (i * 7 + 3) % n, int(rng.integers(0, n))] for i in range(n)]     # edges across the tiles
    rowptr, col = pc.csr_from_lists(rows)
    return pos, batch, rowptr, col, slots


@pytest.mark.parametrize("gx,gy,B", [(89, 1, 22), (32, 32, 1), (64, 32, 1)], ids=["T+1=2048", "T+1=2049", "T+1=4097"])
def test_table_sizes_at_the_scan_tile_boundary(gx, gy, B):
    """T + 1 slots fill one tile exactly / spill one slot into a second / a third tile; slot 0, the last slot a node can
    reach (T - 1) and the slots on both sides of every tile boundary are occupied."""
    d = pc.make_desc(gx, gy, B, 2, 4 * gx, 4 * gy, aggr=1, append_pos=1)
    T = pc.table_slots(d)
    assert T + 1 == {89: 2048, 32: 2049, 64: 4097}[gx]
    rng = np.random.default_rng(gx)
    pos, batch, rowptr, col, slots = _tile_edge_case(d, rng, 60)
    assert (pc.raw_ids(d, pos, batch) == slots).all()
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    assert ref.flags == 0 and ref.n_out == len(np.unique(slots))
    check_against_reference(got, ref, d)


@pytest.mark.parametrize("keep_order", [0, 1])
def test_scan_beyond_one_look_back_window(keep_order):
    """gx = gy = 128, B = 8: T + 1 = 147457 slots, 73 scan tiles -- more than the 64 predecessors one look-back step
    reads.  Every tile that holds reachable slots (0 .. 71; tile 72 is the table's spare slot T alone) has a cluster,
    edges join clusters of different tiles: the new ids (through col), rowptr_out and the counts are exact."""
    d = pc.make_desc(128, 128, 8, 2, 512, 512, keep_order=keep_order)
    T = pc.table_slots(d)
    assert T == 147456 and (T + 1 + pc.SCAN_TILE - 1) // pc.SCAN_TILE == 73
    rng = np.random.default_rng(73 + keep_order)
    per_tile = np.arange(72) * pc.SCAN_TILE + rng.integers(0, pc.SCAN_TILE, 72)
    slots = rng.permutation(np.concatenate([per_tile, rng.integers(0, T, 3928)]))
    pos, batch = pc.nodes_at_slots(d, slots, rng)
    assert (pc.raw_ids(d, pos, batch) == slots).all()
    assert (np.unique(slots // pc.SCAN_TILE) == np.arange(72)).all()
    n = len(slots)
    rows = [[(i + 1) % n, (i * 7 + 3) % n, int(rng.integers(0, n))] for i in range(n)]
    rowptr, col = pc.csr_from_lists(rows)
    assert (slots[col] // pc.SCAN_TILE != np.repeat(slots, 3) // pc.SCAN_TILE).mean() > 0.9
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    assert ref.flags == 0 and ref.n_out > 3900
    check_against_reference(got, ref, d)


# ------------------------------------------------------------------------------------------------ set capacity
def _fan_desc(**kw):
    return pc.make_desc(16, 12, 1, 2, 64, 48, **kw)


def test_exactly_64_sources_fill_the_set():
    d = _fan_desc()
    rng = np.random.default_rng(64)
    pos, batch, rowptr, col, _, _ = pc.fan_in_case(d, 64, rng)
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    row = int(ref.cluster[64])
    assert ref.flags == 0 and not ref.overflow_rows and ref.rowptr_out[row + 1] - ref.rowptr_out[row] == 64
    check_against_reference(got, ref, d)
    kept = got.col[ref.rowptr_out[row]:ref.rowptr_out[row + 1]]
    assert (np.diff(kept) > 0).all() and len(kept) == 64


def test_70_sources_flag_and_keep_64_of_them():
    d = _fan_desc()
    rng = np.random.default_rng(70)
    pos, batch, rowptr, col, _, _ = pc.fan_in_case(d, 70, rng)
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    assert ref.flags == 2 and len(ref.overflow_rows) == 1 and ref.e_out > 64
    check_against_reference(got, ref, d)


def test_exactly_64_sources_with_keep_order_and_ties():
    """The recount of k_pool_order_rows on a full set: a third of the sources share the destination's t_max, a third are
    newer (both leave), a third are older (stay)."""
    d = _fan_desc(keep_order=1)
    rng = np.random.default_rng(65)
    t_src = np.where(np.arange(64) % 3 == 0, 0.5, np.where(np.arange(64) % 3 == 1, 0.25, 0.75))
    pos, batch, rowptr, col, _, _ = pc.fan_in_case(d, 64, rng, t_src=t_src)
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    row = int(ref.cluster[64])
    assert ref.flags == 0 and ref.rowptr_out[row + 1] - ref.rowptr_out[row] == 21
    check_against_reference(got, ref, d)


# ------------------------------------------------------------------------------------------------ edge capacity, recode
def run_recode(d, n_live, n_max, rowptr, col, pos, code_buf, e_cap):
    """dagr_pool_recode for the domain of d into code_buf (device int32); returns (codes, status word)."""
    L, P = _lib.lib(), _lib.ptr
    n_ptr = torch.tensor([n_live], dtype=torch.int32, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.check(L.dagr_pool_recode(P(n_ptr), n_max, P(rowptr), P(col), P(pos), d.two_max, d.r00, d.r02, d.r11, d.r12, d.rx,
                                  d.ry, P(code_buf), e_cap, P(status), _lib.cur_stream(DEV)), "pool_recode")
    torch.cuda.synchronize()
    return code_buf.cpu().numpy(), int(status[0])


def _dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


@pytest.mark.parametrize("keep_order", [0, 1])
def test_edge_capacity_half_the_edges(keep_order):
    """e_cap about half of e_out: bit 2, the true n_out / e_out / rowptr_out, the reference's col / code below e_cap,
    sentinels from e_cap on; dagr_pool_recode with the same e_cap rewrites exactly the entries below it."""
    d = pc.make_desc(15, 11, 2, 3, 60, 44, keep_order=keep_order)
    rng = np.random.default_rng(20 + keep_order)
    pos, batch, rowptr, col = pc.random_level(d, 1200, rng)
    x = _features(d, rng, pos, batch)
    full = pc.pool_reference(d, x, pos, batch, rowptr, col, 1 << 30)
    e_cap = full.e_out // 2 + 3
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col, e_cap=e_cap)
    assert ref.flags == 4 and ref.e_out == full.e_out and (ref.rowptr_out == full.rowptr_out).all()
    check_against_reference(got, ref, d)
    assert (got.col[e_cap:] == SI).all() and (got.code[e_cap:] == SI).all()
    buf = torch.full((e_cap + PAD,), int(SI), dtype=torch.int32, device=DEV)
    code, status = run_recode(d, ref.n_out, pc.table_slots(d), _dev_i32(got.rowptr), _dev_i32(got.col),
                              torch.from_numpy(got.pos).to(DEV), buf, e_cap)
    assert status == 0 and (code[:e_cap] == ref.code[:e_cap]).all() and (code[e_cap:] == SI).all()


# ------------------------------------------------------------------------------------------------ outside nodes
@pytest.mark.parametrize("aggr", [0, 1])
def test_nodes_outside_the_grid_take_no_part(aggr):
    """x >= gx vx, x < -vx, batch = B, batch = -1 and t = 2.0 among valid nodes, as destinations and as sources of edges
    into valid nodes, with features that would show in any result: bit 0, everything else as if they were not there."""
    d = pc.make_desc(15, 11, 2, 3, 60, 44, aggr=aggr, append_pos=1)
    rng = np.random.default_rng(30 + aggr)
    pos, batch, rowptr, col = pc.random_level(d, 600, rng)
    bad_pos = np.array([[1.07, 0.5, 0.5], [-0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 2.0], [0.5, 1.07, 0.5]],
                       np.float32)
    bad_batch = np.array([0, 1, 2, -1, 0, 1], np.int32)
    n0 = 600
    rows = [col[rowptr[i]:rowptr[i + 1]].tolist() for i in range(n0)]
    for k in range(6):
        for dst in rng.integers(0, n0, 4):
            rows[int(dst)].append(n0 + k)                       # an outside node as a source
    rows += [[int(v) for v in rng.integers(0, n0, 3)] for _ in range(6)]      # ... and as a destination
    rowptr, col = pc.csr_from_lists(rows)
    x = np.concatenate([_features(d, rng, pos, batch), np.full((6, 3), 1000.0, np.float32)])
    pos, batch = np.concatenate([pos, bad_pos]), np.concatenate([batch, bad_batch])
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    clean = pc.pool_reference(d, x[:n0], pos[:n0], batch[:n0], *pc.csr_from_lists([[s for s in r if s < n0] for r in rows[:n0]]),
                              e_cap=1 << 30)
    assert ref.flags == 1 and ref.n_out == clean.n_out and ref.e_out == clean.e_out
    check_against_reference(got, ref, d)


# ------------------------------------------------------------------------------------------------ LUT range
def test_lut_coordinates_out_of_range():
    """A Cartesian range far smaller than the edges: bit 3, codes still (ix & 0xffff) | (iy << 16) of the fp32 formula
    (negative and beyond-16-bit coordinates included), col exact -- from dagr_pool_csr and from dagr_pool_recode."""
    d = pc.make_desc(15, 11, 2, 3, 60, 44, two_max=0.1)
    rng = np.random.default_rng(40)
    pos, batch, rowptr, col = pc.random_level(d, 900, rng, reach=3)
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    ix = ref.code.astype(np.int64) & 0xffff
    assert ref.flags == 8 and (ix > 0x8000).any() and (ref.code < 0).any()
    check_against_reference(got, ref, d)
    buf = torch.full((ref.e_out + PAD,), int(SI), dtype=torch.int32, device=DEV)
    code, status = run_recode(d, ref.n_out, pc.table_slots(d), _dev_i32(got.rowptr), _dev_i32(got.col),
                              torch.from_numpy(got.pos).to(DEV), buf, ref.e_out)
    assert status == 8 and (code[:ref.e_out] == ref.code).all() and (code[ref.e_out:] == SI).all()


def test_recode_for_another_domain_with_a_device_side_count():
    """dagr_pool_recode on a pooled level for a second domain (the network's own two-cell table instead of the wide one),
    *n_ptr below n_max: exact codes for the rows below *n_ptr, the entries of the rows beyond it untouched."""
    d = pc.make_desc(15, 11, 2, 3, 60, 44, aggr=1)
    rng = np.random.default_rng(50)
    pos, batch, rowptr, col = pc.random_level(d, 900, rng)
    x = _features(d, rng, pos, batch)
    ref, got = _ref_and_run(d, x, pos, batch, rowptr, col)
    check_against_reference(got, ref, d)
    d2 = pc.make_desc(15, 11, 2, 3, 60, 44, domain="net")
    assert (d2.two_max, d2.r00, d2.rx) != (d.two_max, d.r00, d.rx)
    live = ref.n_out - 40
    rp = ref.rowptr_out[:ref.n_out + 1]
    want, written, flag = pc.recode_reference(ref.pos_out, rp, ref.col, live, d2, e_cap=ref.e_out)
    assert 0 < written.sum() < ref.e_out and flag == 0
    buf = torch.full((ref.e_out + PAD,), int(SI), dtype=torch.int32, device=DEV)
    code, status = run_recode(d2, live, ref.n_out, _dev_i32(got.rowptr), _dev_i32(got.col), torch.from_numpy(got.pos).to(DEV),
                              buf, ref.e_out)
    assert status == flag and (code[:ref.e_out][written] == want[written]).all()
    assert (code[:ref.e_out][~written] == SI).all() and (code[ref.e_out:] == SI).all()
    assert (want[written] != ref.code[written]).any()


# ------------------------------------------------------------------------------------------------ re-arm
def _same_outputs(a, b, ref):
    """Bit for bit, apart from WHICH 64 sources a row beyond the bound keeps (not fixed: first come, first served)."""
    assert (a.n_out, a.e_out) == (b.n_out, b.e_out)
    for key in ("x", "pos", "batch", "rowptr"):
        assert (bits(getattr(a, key)) == bits(getattr(b, key))).all(), key
    exact = np.ones(len(a.col), bool)
    for row in ref.overflow_rows:
        exact[int(ref.rowptr_out[row]):int(ref.rowptr_out[row + 1])] = False
    assert (a.col[exact] == b.col[exact]).all() and (a.code[exact] == b.code[exact]).all()


@pytest.mark.parametrize("keep_order", [0, 1])
@pytest.mark.parametrize("aggr", [0, 1])
def test_one_workspace_through_six_calls(aggr, keep_order):
    """Six calls on one workspace -- a level, an empty call, one that overflows a source set (bit 1), one that overflows
    the edge capacity (bit 2), one with nodes outside the grid (bit 0), a last level -- each equal, bit for bit, to the
    same call on a fresh workspace and right against the reference: whatever a flagged call leaves behind (accumulators of
    both epochs, source sets, row counters, t_max, the scan's ticket and tag) is re-armed.  The flag word is sticky."""
    d = pc.make_desc(16, 12, 2, 3, 64, 48, aggr=aggr, keep_order=keep_order, append_pos=1)
    rng = np.random.default_rng(600 + 2 * aggr + keep_order)
    calls = []
    lv = pc.random_level(d, 900, rng)
    calls.append((lv, None, None))
    calls.append((pc.random_level(d, 40, rng), None, 0))                                   # empty: *n_ptr = 0
    calls.append((pc.fan_in_case(d, 70, rng)[:4], None, None))                             # bit 1
    lv = pc.random_level(d, 800, rng)
    calls.append((lv, "half", None))                                                       # bit 2
    pos, batch, rowptr, col = pc.random_level(d, 500, rng)
    pos[::50, 0] = 1.25; batch[25::50] = 2; pos[10::50, 2] = 2.0                            # bit 0
    calls.append(((pos, batch, rowptr, col), None, None))
    calls.append((pc.random_level(d, 1000, rng), None, None))
    ws = new_workspace(d)
    sticky, seen = 0, []
    for (pos, batch, rowptr, col), cap, n_live in calls:
        valid = pc.pool_reference(d, np.zeros((len(pos), 3), np.float32), pos, batch, rowptr, col, 1 << 30).cluster >= 0
        grp = np.where(valid, pc.raw_ids(d, pos, np.clip(batch, 0, d.B - 1)), 0)
        x = pc.max_values(rng, grp, 3) if aggr == 0 else pc.mean_values(rng, grp, 3)
        full = pc.pool_reference(d, x, pos, batch, rowptr, col, 1 << 30, n=n_live)
        e_cap = full.e_out // 2 if cap == "half" else full.e_out + 5
        ref = pc.pool_reference(d, x, pos, batch, rowptr, col, e_cap, n=n_live)
        fresh = run_pool_csr(d, x, pos, batch, rowptr, col, e_cap, n_live=n_live)
        shared = run_pool_csr(d, x, pos, batch, rowptr, col, e_cap, n_live=n_live, ws=ws)
        check_against_reference(fresh, ref, d)
        _same_outputs(shared, fresh, ref)
        sticky |= fresh.flags
        assert shared.flags == sticky
        seen.append(fresh.flags)
    assert seen == [0, 0, 2, 4, 1, 0]
