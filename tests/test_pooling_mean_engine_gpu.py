"""``--pooling_aggr mean`` through the window engine (every other engine test runs ``max``; only pool4 is ``mean``
there): the AGGR = 1 forms of the level-0 streaming kernel (k_pool_l0_slots / k_pool_l0_slots_ord: 64-bit LDS atomics, the
window merge, the global path of t == 1.0 nodes), k_pool_finalize's mean branch (generic level-0 path),
k_pool_l0_add_rows' (asynchronous updates) and the fused conv + pool epilogue's at pool2 / pool3 -- against the oracle with
the bars of tests/test_engine_gpu.py:_compare, unchanged.

The level-0 kernel has a 16-byte form (VEC = 4: C % 4 == 0, ldx % 4 == 0, aligned rows) and a scalar one (VEC = 1).  Every
level-0 width the engine supports (8, 16, 32 channels, + 64 image channels with --use_image) takes the 16-byte form --
asserted below from C, ldx and the pointer -- so the scalar form is reached by calling dagr_pool_l0 on the engine's own
window with a 6-channel descriptor, and held to tests/pool_cases.py:pool_reference with the bars of
tests/test_pool_csr_direct_gpu.py (which the 16-channel form meets as well)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from oracle import model as om
from dagr_amd import _lib
from dagr_amd.utils import synthetic as syn
from tests import pool_cases as pc
from tests.test_async_update_gpu import _dev, _level1, _model
from tests.test_engine_gpu import (TOL, _compare, _edges_from_csr, _err, _events, _path_counters, _setup,
                                   _sorted_cols)
from tests.test_pool_csr_direct_gpu import c_desc, check_against_reference, new_workspace, output_buffers, snapshot

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
W, H, B = 320, 215, 2


def _takes_the_16_byte_form(eng):
    """launch_pool_l0_slots' choice, from what the engine hands it."""
    C, ldx = eng.pool_desc[0].channels, eng.hp0.shape[1]
    return C % 4 == 0 and ldx % 4 == 0 and eng.hp0.data_ptr() % 16 == 0


def _mean_engine(eng, keep_order=0):
    assert [d.aggr for d in eng.pool_desc] == [1, 1, 1, 1] and all(d.keep_order == keep_order for d in eng.pool_desc)


# ------------------------------------------------------------------------------------------------ whole engine
@pytest.mark.parametrize("stream", ["edges", "uniform"])
def test_engine_mean_matches_the_oracle(stream):
    gen = syn.edges_window if stream == "edges" else syn.uniform_window
    args, model, sd = _setup(W, H, B, seed=31, calibrate=gen, pooling_aggr="mean")
    eng = model.engine()
    _mean_engine(eng)
    _compare(args, model, sd, W, H, B, *_events(gen, 6000, B, W, H, seed=33), plain=True)
    assert _takes_the_16_byte_form(eng) and eng.pool_desc[0].channels == 16
    # the mean epilogue of dagr_spline_conv_fused_pool ran (pool2 and / or pool3 accumulate inside the conv)
    assert eng._pool_accumulated[0] or eng._pool_accumulated[1]


def test_mean_bitmap_and_generic_level0_paths_agree_and_match_the_oracle():
    """The three QUIRK-1 variants of test_coarse_edge_bitmap_and_generic_paths_agree with mean: no t == 1.0 event, the last
    event of every sample, every event.  Both level-0 paths (k_pool_emit after the bitmaps / k_pool_finalize + per-edge
    insertion) give the same pool1 level bit for bit, and both match the oracle."""
    args, model, sd = _setup(W, H, B, seed=34, pooling_aggr="mean")
    eng = model.engine()
    _mean_engine(eng)
    x, y, t, p, b, _ = _events(syn.edges_window, 6000, B, W, H, seed=11)
    last = np.flatnonzero(np.diff(np.concatenate([b, [B]])) != 0)
    for with_leak in (0, 1, 2):
        tt = np.minimum(t, 999999)
        if with_leak == 1:
            tt[last] = 1000000
        elif with_leak == 2:
            tt[:] = 1000000
        pp = syn.format_data_np(x, y, tt, W, H)
        assert (pp[:, 2].max() >= 1.0) == (with_leak > 0)
        dev_win = (torch.from_numpy(pp).to(DEV), torch.from_numpy(p.astype(np.float32)).view(-1, 1).to(DEV),
                   torch.from_numpy(b).to(DEV))
        snaps = []
        for fast in (True, False):
            eng.fast_coarse_edges = fast
            before = _path_counters(eng)["pool1_global_path"]
            tr = {}
            eng.forward_raw(*dev_win, trace=tr)
            eng.check_status()
            if with_leak:
                assert _path_counters(eng)["pool1_global_path"] > before
            snaps.append(tr["pool1"])
        eng.fast_coarse_edges = True
        for key in ("x", "pos", "batch", "rowptr", "col", "code"):
            assert torch.equal(snaps[0][key], snaps[1][key]), f"pool1 {key} differs (leak={with_leak})"
        # ... and the oracle's pool1, with _compare's bars for a pooled level
        tro = {}
        om.forward_events(sd, args, H, W, x, y, tt, p, b, B, trace=tro, exact_pos_mean=True)
        ho, oo_ = snaps[0], tro["pool1"]
        c = oo_["x"].shape[1]
        assert ho["x"].shape[0] == oo_["x"].shape[0]
        assert (ho["batch"].cpu().long() == oo_["batch"]).all()
        assert (ho["pos"].cpu()[:, :2] == oo_["pos"][:, :2]).all()
        assert (ho["pos"].cpu()[:, 2] - oo_["pos"][:, 2]).abs().max().item() < 1e-6
        assert _err(ho["x"][:, :c], oo_["x"]) < TOL
        assert (ho["x"].cpu()[:, c:c + 2] == ho["pos"].cpu()[:, :2]).all()
        eh = _sorted_cols(_edges_from_csr(ho["rowptr"], ho["col"]))
        eo = _sorted_cols(oo_["edge_index"].numpy())
        assert eh.shape == eo.shape and (eh == eo).all(), f"pool1 edges differ from the oracle (leak={with_leak})"
        if with_leak < 2:
            assert snaps[0]["col"].numel() > 300


@pytest.mark.parametrize("base_width,use_image", [(0.25, False), (1.0, False), (0.5, True)])
def test_level0_widths_with_mean(base_width, use_image):
    """8 and 32 level-0 channels, and the --use_image layout (16 + 64 channels in rows of 80): all of them 16-byte rows."""
    over = dict(use_image=True, img_net="resnet18") if use_image else {}
    args, model, sd = _setup(W, H, B, seed=35, calibrate=syn.edges_window, pooling_aggr="mean", base_width=base_width, **over)
    eng = model.engine()
    _mean_engine(eng)
    image = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(1)).cuda() if use_image else None
    with torch.no_grad():
        _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 5000, B, W, H, seed=37), image=image, plain=True)
    C = int(base_width * 32) + (64 if use_image else 0)
    assert eng.pool_desc[0].channels == C == eng.hp0.shape[1] and _takes_the_16_byte_form(eng)


def test_keep_temporal_ordering_with_mean():
    """The _ord kernels (t_max in the LDS window) with mean, the pruning launches at every level."""
    args, model, sd = _setup(W, H, B, seed=36, calibrate=syn.edges_window, pooling_aggr="mean", keep_temporal_ordering=True)
    _mean_engine(model.engine(), keep_order=1)
    _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 6000, B, W, H, seed=39), plain=True)


def test_updates_with_mean_equal_a_window_on_all_events():
    """k_pool_l0_add_rows with mean: after forward_append, level 1 equals level 1 of a window built from all the events,
    bit for bit (fixed-point sums do not depend on the order of arrival); the t == 1.0 events arrive in the updates."""
    args, model = _model(W, H, B, seed=3, pooling_aggr="mean")
    eng = model.engine()
    _mean_engine(eng)
    raw = [syn.edges_window(6000, W, H, seed=90 + s) for s in range(B)]
    cuts = [0, 4000, 5200, 5990, 5999, 6000]

    def part(lo, hi):
        xs = [np.concatenate([r[k][lo:hi] for r in raw]) for k in range(4)]
        b = np.concatenate([np.full(hi - lo, s, np.int64) for s in range(B)])
        return _dev(xs[0], xs[1], xs[2], xs[3], b, W, H)

    with torch.no_grad():
        eng.set_low_latency(False)
        eng.forward_raw(*part(cuts[0], cuts[1]))
        assert eng.can_append()
        for lo, hi in zip(cuts[1:-1], cuts[2:]):
            out_async = eng.forward_append(*part(lo, hi)).clone()
        eng.check_status()
        lvl_async = _level1(eng)
        out_full = eng.forward_raw(*part(0, 6000)).clone()
        eng.check_status()
        lvl_full = _level1(eng)
    assert lvl_async["n"] == lvl_full["n"] > 1000 and lvl_async["e"] == lvl_full["e"] > 1000
    for k in ("x", "pos", "batch", "rowptr", "col", "code"):
        assert torch.equal(lvl_async[k], lvl_full[k]), k
    assert torch.equal(out_async, out_full)


# ------------------------------------------------------------------------------------------------ level 0, directly
@pytest.fixture(scope="module")
def window():
    """One resident window of the default engine and its level-0 graph in EVENT order (what the reference takes: the
    member with the largest event id gives a cluster its sample)."""
    args, model, sd = _setup(W, H, B, seed=38)
    eng = model.engine()
    x, y, t, p, b, _ = _events(syn.edges_window, 4000, B, W, H, seed=41)
    for s_ in range(B):                                  # the last 400 events of every sample sit at t == 1.0 (QUIRK-1):
        t[np.flatnonzero(b == s_)[-400:]] = 1000000      # whole clusters go through the kernel's global path
    eng.forward_raw(*_dev(x, y, t, p, b, W, H), trace={})
    eng.check_status()
    N = eng._N
    # the level-0 rows stay in the engine's buffer: column j scaled by 2^-3j (exact), so that the channels span
    # magnitudes down to and below the 2^-32 grid of the mean's fixed-point terms
    eng.hp0[:N].mul_(2.0 ** (-3.0 * torch.arange(16, device=DEV)))
    se = eng.graph.node_order(N)[0].cpu().numpy().astype(np.int64)          # event id of every node row
    nbr_src, _, deg = [a.cpu().numpy() for a in eng._nbr]
    rows = [[] for _ in range(N)]
    for slot in range(N):
        rows[se[slot]] = se[nbr_src[slot, :deg[slot]]].tolist()
    rowptr, col = pc.csr_from_lists(rows)
    pos = np.empty((N, 3), np.float32)
    pos[se] = eng.pos_n[:N].cpu().numpy()
    hp0 = np.empty((N, eng.hp0.shape[1]), np.float32)
    hp0[se] = eng.hp0[:N].cpu().numpy()
    assert (pos[:, 2] >= 1.0).sum() >= 400 * B and eng.hp0.shape[1] == 16
    return types.SimpleNamespace(eng=eng, N=N, pos=pos, batch=eng._batch.cpu().numpy(), rowptr=rowptr, col=col, hp0=hp0)


def _pool_l0(win, d, fast, e_cap):
    eng, L, P = win.eng, _lib.lib(), _lib.ptr
    ws = new_workspace(d)
    ob = output_buffers(d, e_cap)
    g = eng.graph
    nbr_src, nbr_code, deg = eng._nbr
    scratch = torch.zeros((win.N,), dtype=torch.int32, device=DEV)
    cd = c_desc(d)
    _lib.check(L.dagr_pool_l0(ctypes.byref(cd), P(ws), ctypes.byref(g.desc), P(g.workspace), P(eng.xlo), P(eng.ylo),
                              P(eng.hp0), eng.hp0.shape[1], P(eng.pos_n), P(eng.batch_n), P(eng._batch),
                              1 if eng._batch.dtype == torch.int64 else 0, win.N, P(nbr_src), P(nbr_code) if fast else None,
                              P(deg), P(scratch), P(ob.x), ob.ldo, 0, P(ob.pos), P(ob.batch), P(ob.counts), P(ob.rowptr),
                              P(ob.col), P(ob.code), ctypes.c_void_p(ob.counts.data_ptr() + 4), e_cap,
                              _lib.cur_stream(DEV)), "pool_l0")
    return snapshot(ob, d, ws)


@pytest.mark.parametrize("keep_order", [0, 1])
@pytest.mark.parametrize("aggr", [0, 1])
@pytest.mark.parametrize("C", [6, 16])
def test_level0_kernel_forms_against_the_reference(window, C, aggr, keep_order):
    """dagr_pool_l0 on the engine's window with the first C channels of its level-0 rows (ldx = 16): C = 6 runs the scalar
    form (VEC = 1), C = 16 the 16-byte one; bitmap and generic coarse-edge paths, both aggregations, with and without
    keep_order, against the exact reference."""
    pd = window.eng.pool_desc[0]
    d = types.SimpleNamespace(gx=pd.gx, gy=pd.gy, B=pd.batch_size, C=C, vx=pd.vx, vy=pd.vy, inv_w=pd.inv_w, inv_h=pd.inv_h,
                              two_max=pd.two_max, r00=pd.r00, r02=pd.r02, r11=pd.r11, r12=pd.r12, rx=pd.rx, ry=pd.ry,
                              aggr=aggr, append_pos=1, keep_order=keep_order)
    vec4 = C % 4 == 0 and window.eng.hp0.shape[1] % 4 == 0 and window.eng.hp0.data_ptr() % 16 == 0
    assert vec4 == (C == 16)
    x = np.ascontiguousarray(window.hp0[:, :C])
    full = pc.pool_reference(d, x, window.pos, window.batch, window.rowptr, window.col, 1 << 30)
    e_cap = full.e_out + 5
    ref = pc.pool_reference(d, x, window.pos, window.batch, window.rowptr, window.col, e_cap)
    assert ref.flags == 0 and ref.n_out > 1000 and ref.e_out > 1000
    for fast in (True, False):
        check_against_reference(_pool_l0(window, d, fast, e_cap), ref, d)
