"""``--keep_temporal_ordering`` (pooling.py:69-72) through the window engine: a coarse edge src -> dst survives only if
t_max[dst] > t_max[src] (t_max = newest member of the cluster's input nodes; strict).  dagr_pool_desc.keep_order = 1
runs the filter in the pooling kernels (csrc/pooling.hip: t_max accumulators + one pruning launch per step), on every
path of the engine: level-0 bitmap and generic paths, pooled levels (fused and unfused accumulation), captured windows,
the asynchronous update.  The module path (Pooling.forward, host-side filter) and the oracle are the other sides."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import model as om
from oracle import ops as oo
from dagr_amd import _lib
from dagr_amd.utils import synthetic as syn
from tests.test_async_update_gpu import _dev, _level1, _model
from tests.test_engine_gpu import (TOL, _compare, _compare_one_scale, _dev_window, _edges_from_csr, _err, _events, _setup,
                                   _sorted_cols)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _pools(model):
    b = model.backbone
    return (b.pool1, b.pool2, b.pool3, b.pool4)


def _set_flag(model, on):
    for p in _pools(model):
        p.keep_temporal_ordering = on
    model.args.keep_temporal_ordering = on


def _edge_counts(tr):
    return [int(tr[f"pool{k}"]["col"].numel()) for k in range(1, 5)]


# ------------------------------------------------------------------------------------------------ 1. dagr_pool_csr
def _pool_csr(desc, x, pos, batch, rowptr, col):
    """One dagr_pool_csr call on level data (fresh workspace); returns (x, pos, batch, rowptr, col, code)."""
    L = _lib.lib()
    stream = _lib.cur_stream(DEV)
    n = x.shape[0]
    C = desc.channels
    T = desc.gx * desc.gy * (desc.batch_size + 1)
    nbytes = L.dagr_pool_workspace_bytes(ctypes.byref(desc))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(L.dagr_pool_workspace_init(ctypes.byref(desc), _lib.ptr(ws), nbytes, stream), "ws_init")
    counts = torch.tensor([n, 0], dtype=torch.int32, device=DEV)
    e_cap = 64 * T
    x_out = torch.zeros((T, C + 2), dtype=torch.float32, device=DEV)
    pos_out = torch.zeros((T, 3), dtype=torch.float32, device=DEV)
    batch_out = torch.zeros((T,), dtype=torch.int32, device=DEV)
    out_counts = torch.zeros((2,), dtype=torch.int32, device=DEV)
    rowptr_out = torch.zeros((T + 2,), dtype=torch.int32, device=DEV)
    col_out = torch.zeros((e_cap,), dtype=torch.int32, device=DEV)
    code_out = torch.zeros((e_cap,), dtype=torch.int32, device=DEV)
    scratch = torch.zeros((max(n, 1),), dtype=torch.int32, device=DEV)
    P = _lib.ptr
    _lib.check(L.dagr_pool_csr(ctypes.byref(desc), P(ws), P(counts), n, P(x), x.shape[1], P(pos), P(batch), P(rowptr),
                               P(col), P(scratch), P(x_out), C + 2, 0, P(pos_out), P(batch_out), P(out_counts),
                               P(rowptr_out), P(col_out), P(code_out), ctypes.c_void_p(out_counts.data_ptr() + 4), e_cap,
                               stream), "pool_csr")
    f = (ctypes.c_int32 * 1)()
    _lib.check(L.dagr_pool_status(ctypes.byref(desc), P(ws), f, stream), "pool_status")
    assert f[0] == 0, f"pool status {f[0]}"
    nc, ne = [int(v) for v in out_counts.tolist()]
    return (x_out[:nc, :C].cpu(), pos_out[:nc].cpu(), batch_out[:nc].cpu(), rowptr_out[:nc + 1].cpu(),
            col_out[:ne].cpu(), code_out[:ne].cpu())


@pytest.mark.parametrize("aggr", [0, 1])
def test_pool_csr_keep_order_matches_the_oracle(aggr):
    """dagr_pool_csr with keep_order = 1 on level-1 data of a seeded window whose t is quantised to eighths (many clusters
    share their t_max: the strict > drops such edges both ways) against oracle.ops.pooling(keep_temporal_ordering=True);
    every surviving edge keeps the LUT code it has with keep_order = 0."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=3)
    eng = model.engine()
    pos, feat, batch = _dev_window(syn.edges_window, 6000, B, W, H, seed=23)
    tr = {}
    eng.forward_raw(pos, feat, batch, trace=tr)
    lvl = tr["pool1"]
    d0 = copy.copy(eng.pool_desc[1])
    d0.aggr = aggr
    C = d0.channels
    x = tr["layer2"]["x"][:, :C].contiguous()
    p = lvl["pos"].clone()
    p[:, 2] = torch.floor(p[:, 2] * 8) / 8
    b = lvl["batch"].contiguous()
    rowptr, col = lvl["rowptr"].contiguous(), lvl["col"].contiguous()
    d1 = copy.copy(d0)
    d1.keep_order = 1
    assert _lib.lib().dagr_pool_workspace_bytes(ctypes.byref(d1)) > _lib.lib().dagr_pool_workspace_bytes(ctypes.byref(d0))
    got = _pool_csr(d1, x, p, b, rowptr, col)
    off = _pool_csr(d0, x, p, b, rowptr, col)
    pp = om.NetConstants(args, H, W).pools[1]
    pp.aggr = "max" if aggr == 0 else "mean"
    ei = torch.from_numpy(_edges_from_csr(rowptr, col)).long()
    ref = oo.pooling(pp, x.cpu(), p.cpu(), b.cpu().long(), ei, exact_mean=True, keep_temporal_ordering=True)
    ref_off = oo.pooling(pp, x.cpu(), p.cpu(), b.cpu().long(), ei, exact_mean=True)
    assert got[0].shape[0] == ref[0].shape[0]
    assert _err(got[0], ref[0]) < TOL
    assert torch.equal(got[1][:, :2], ref[1][:, :2]) and (got[1][:, 2] - ref[1][:, 2]).abs().max() < 1e-6
    assert torch.equal(got[2].long(), ref[2].long())
    eg = _sorted_cols(_edges_from_csr(got[3], got[4]))
    eo = _sorted_cols(ref[3].numpy())
    assert eg.shape == eo.shape and (eg == eo).all()
    # the case is not vacuous, and equal t_max occurs among the dropped edges
    e_off = ref_off[3]
    assert eo.shape[1] < e_off.shape[1]
    t_max = oo.scatter_max(p.cpu()[:, -1:], _cluster(pp, p.cpu(), b.cpu()), ref[0].shape[0])[:, 0]
    assert int((t_max[e_off[0]] == t_max[e_off[1]]).sum()) > 0
    # surviving edges carry their keep_order = 0 codes
    code_off = {(int(s), int(t_)): int(c) for s, t_, c in zip(off[4], np.repeat(np.arange(len(off[3]) - 1),
                                                                               np.diff(off[3].numpy())), off[5])}
    dst = np.repeat(np.arange(len(got[3]) - 1), np.diff(got[3].numpy()))
    for s, t_, c in zip(got[4].tolist(), dst.tolist(), got[5].tolist()):
        assert code_off[(s, t_)] == c


def _cluster(pp, pos, batch):
    pos4 = torch.cat([pos, batch.float().view(-1, 1)], dim=-1)
    cluster = oo.grid_cluster(pos4, pp.voxel_size, pp.start, pp.end)
    return oo.consecutive_cluster(cluster)[1]


# ------------------------------------------------------------------------------------------------ 2. level-0 paths
def test_level0_bitmap_and_generic_paths_agree_with_the_filter():
    """keep_order = 1 analogue of test_coarse_edge_bitmap_and_generic_paths_agree: both level-0 paths give the same
    rowptr / col / code, and the oracle's filtered pool1 edges, for the three QUIRK-1 variants."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=4, keep_temporal_ordering=True)
    eng = model.engine()
    assert all(d.keep_order == 1 for d in eng.pool_desc)
    x, y, t, p, b, _ = _events(syn.edges_window, 9000, B, W, H, seed=11)
    last = np.flatnonzero(np.diff(np.concatenate([b, [B]])) != 0)
    for with_leak in (0, 1, 2):
        tt = np.minimum(t, 999999)
        if with_leak == 1:
            tt[last] = 1000000
        elif with_leak == 2:
            tt[:] = 1000000
        pp = syn.format_data_np(x, y, tt, W, H)
        snaps = []
        for fast in (True, False):
            eng.fast_coarse_edges = fast
            tr = {}
            eng.forward_raw(torch.from_numpy(pp).to(DEV), torch.from_numpy(p.astype(np.float32)).view(-1, 1).to(DEV),
                            torch.from_numpy(b).to(DEV), trace=tr)
            eng.check_status()
            snaps.append(tr["pool1"])
        eng.fast_coarse_edges = True
        for key in ("rowptr", "col", "code"):
            assert torch.equal(snaps[0][key], snaps[1][key]), f"pool1 {key} differs (leak={with_leak})"
        tro = {}
        om.forward_events(sd, args, H, W, x, y, tt, p, b, B, trace=tro, exact_pos_mean=True)
        eh = _sorted_cols(_edges_from_csr(snaps[0]["rowptr"], snaps[0]["col"]))
        eo = _sorted_cols(tro["pool1"]["edge_index"].numpy())
        assert eh.shape == eo.shape and (eh == eo).all(), f"pool1 edges differ from the oracle (leak={with_leak})"
        if with_leak < 2:
            assert snaps[0]["col"].numel() > 300


# ------------------------------------------------------------------------------------------------ 3. whole engine
def _compare_flagged(args, model, sd, W, H, B, ev, **kw):
    """_compare on the flagged model; then the same window unflagged (the stamp rebuilds the engine): fewer edges."""
    dev_ev = (torch.from_numpy(ev[5]).to(DEV), torch.from_numpy(ev[3].astype(np.float32)).view(-1, 1).to(DEV),
              torch.from_numpy(ev[4]).to(DEV))
    _compare(args, model, sd, W, H, B, *ev, **kw)
    eng = model.engine()
    assert all(d.keep_order == 1 for d in eng.pool_desc)
    tr_on = {}
    eng.forward_raw(*dev_ev, image=kw.get("image"), trace=tr_on)
    _set_flag(model, False)
    try:
        eng_off = model.engine()
        assert eng_off is not eng and all(d.keep_order == 0 for d in eng_off.pool_desc)
        tr_off = {}
        eng_off.forward_raw(*dev_ev, image=kw.get("image"), trace=tr_off)
    finally:
        _set_flag(model, True)
    on, off = _edge_counts(tr_on), _edge_counts(tr_off)
    assert all(a <= b_ for a, b_ in zip(on, off)) and any(a < b_ for a, b_ in zip(on, off)), (on, off)
    return eng


@pytest.mark.parametrize("stream", ["uniform", "edges"])
def test_engine_small_b2_matches_the_oracle(stream):
    W, H, B = 320, 215, 2
    gen = syn.uniform_window if stream == "uniform" else syn.edges_window
    args, model, sd = _setup(W, H, B, seed=5, calibrate=gen, keep_temporal_ordering=True)
    eng = _compare_flagged(args, model, sd, W, H, B, _events(gen, 6000, B, W, H, seed=5), plain=True)
    assert any(eng._pool_accumulated[:3]), "the fused accumulation (dagr_spline_conv_fused_pool) did not run"


def test_engine_dagr_l_widths_matches_the_oracle():
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=6, calibrate=syn.edges_window, net_stem_width=1.0, yolo_stem_width=1.0,
                             keep_temporal_ordering=True)
    _compare_flagged(args, model, sd, W, H, B, _events(syn.edges_window, 5000, B, W, H, seed=17), plain=True)


def test_engine_one_scale_ncaltech_matches_the_oracle():
    """num_scales = 1: dagr_pool_recode runs on the filtered pool4 CSR."""
    W, H, B = 240, 180, 1
    args, model, sd = _setup(W, H, B, seed=7, net_stem_width=1.0, yolo_stem_width=1.0, num_scales=1,
                             dataset="ncaltech101", keep_temporal_ordering=True)
    _compare_one_scale(args, model, sd, W, H, B, *_events(syn.uniform_window, 6000, B, W, H, seed=19))


def test_engine_use_image_resnet18_matches_the_oracle():
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=4, calibrate=syn.edges_window, use_image=True, img_net="resnet18",
                             keep_temporal_ordering=True)
    image = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        _compare_flagged(args, model, sd, W, H, B, _events(syn.edges_window, 5000, B, W, H, seed=13), image=image,
                         plain=True)


def test_engine_vga_edges_b8_100k_matches_the_oracle():
    W, H, B = 640, 480, 8
    args, model, sd = _setup(W, H, B, seed=0, calibrate=syn.edges_window, keep_temporal_ordering=True)
    _compare_flagged(args, model, sd, W, H, B, _events(syn.edges_window, 100000, B, W, H, seed=1234), plain=True)


# ------------------------------------------------------------------------------------------------ 4. captured replay
def test_window_graph_replay_with_the_filter():
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=12, keep_temporal_ordering=True)
    eng = model.engine().set_low_latency(True)
    wins = [_dev_window(syn.edges_window, n, B, W, H, seed) for n, seed in ((4000, 41), (2500, 43), (6000, 45), (1, 47))]
    wins.append((torch.zeros((0, 3), device=DEV), torch.zeros((0, 1), device=DEV),
                 torch.zeros((0,), dtype=torch.int64, device=DEV)))
    eager = [eng.forward_raw(*w, trace={}).clone() for w in wins]
    got = []
    for rep in range(3):
        for k, w in enumerate(wins):
            got.append((k, eng.forward_raw(*w)))
    assert eng._wg is not None, "the window was not captured"
    eng.check_status()
    for k, o in got:
        assert torch.equal(o, eager[k]), k
    cap0 = eng.max_events
    big = _dev_window(syn.uniform_window, cap0 // B + 500, B, W, H, seed=49)
    want = eng.forward_raw(*big, trace={}).clone()
    for rep in range(3):
        assert torch.equal(eng.forward_raw(*big), want)
    assert eng.max_events > cap0 and eng._wg is not None
    assert torch.equal(eng.forward_raw(*wins[0]), eager[0])


# ------------------------------------------------------------------------------------------------ 5. incremental update
@pytest.mark.parametrize("B,stream", [(1, "uniform"), (2, "edges")])
def test_updates_with_the_filter_equal_a_window_on_all_events(B, stream):
    W, H = 320, 215
    args, model = _model(W, H, B, seed=3, keep_temporal_ordering=True)
    eng = model.engine()
    assert all(d.keep_order == 1 for d in eng.pool_desc)
    gen = syn.uniform_window if stream == "uniform" else syn.edges_window
    raw = [gen(6000, W, H, seed=90 + s) for s in range(B)]
    cuts = [0, 4000, 5200, 5990, 5999, 6000]        # the t == 1.0 events arrive in the updates

    def part(lo, hi):
        xs = [np.concatenate([r[k][lo:hi] for r in raw]) for k in range(4)]
        b = np.concatenate([np.full(hi - lo, s, np.int64) for s in range(B)])
        return _dev(xs[0], xs[1], xs[2], xs[3], b, W, H)

    with torch.no_grad():
        for tail_graph in (False, True):
            eng.set_low_latency(tail_graph)
            eng.forward_raw(*part(cuts[0], cuts[1]))
            assert eng.can_append()
            for lo, hi in zip(cuts[1:-1], cuts[2:]):
                out_async = eng.forward_append(*part(lo, hi)).clone()
            eng.check_status()
            lvl_async = _level1(eng)
            out_full = eng.forward_raw(*part(0, 6000), trace={}).clone()
            eng.check_status()
            lvl_full = _level1(eng)
            assert lvl_async["n"] == lvl_full["n"] and lvl_async["e"] == lvl_full["e"]
            for k in ("x", "pos", "batch", "rowptr", "col", "code"):
                assert torch.equal(lvl_async[k], lvl_full[k]), (tail_graph, k)
            assert torch.equal(out_async, out_full), tail_graph


def test_dagr_forward_through_the_engine_with_the_filter():
    """module_path_only = False: reset=False (incremental) == make_model_synchronous == one reset=True call, bit for
    bit; the engine's reset=True outputs agree with the module path's (Pooling modules filtering on the host)."""
    from dagr_amd.asynchronous import make_model_asynchronous, make_model_synchronous
    from dagr_amd.data import Batch, Data
    from dagr_amd.utils.buffers import format_data
    W, H, B = 320, 215, 2
    args, model = _model(W, H, B, seed=5, keep_temporal_ordering=True)
    assert model.module_path_only
    with pytest.raises(NotImplementedError, match="log_flops"):
        make_model_asynchronous(model, log_flops=True)
    raw = [syn.edges_window(5000, W, H, seed=40 + s) for s in range(B)]

    def batch_of(lo, hi):
        samples = []
        for s in range(B):
            x, y, t, p = (a[lo:hi] for a in raw[s])
            samples.append(Data(x=torch.from_numpy(p.reshape(-1, 1)), pos=torch.from_numpy(np.stack([x, y], -1)),
                                t=torch.from_numpy(t), width=W, height=H, time_window=1000000))
        return format_data(Batch.from_data_list(samples).cuda())

    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="module_path_only"):
            model(batch_of(0, 3000), reset=False, return_targets=False)
        out_mod = model.forward_modules(batch_of(0, 5000), reset=True)
        model.module_path_only = False
        out_eng = model.engine().forward_data(batch_of(0, 5000)).clone()
        cuts = [0, 3000, 4000, 4900, 4990, 4999, 5000]
        outs = {}
        for mode, convert in (("asynchronous", make_model_asynchronous), ("synchronous", make_model_synchronous)):
            convert(model)
            for k in range(len(cuts) - 1):
                det, = model(batch_of(cuts[k], cuts[k + 1]), reset=(k == 0), return_targets=False)
            outs[mode] = [{k: v.clone() for k, v in d.items()} for d in det]
        make_model_asynchronous(model)
        full, = model(batch_of(0, 5000), reset=True, return_targets=False)
    for a, s_, f in zip(outs["asynchronous"], outs["synchronous"], full):
        for key in ("boxes", "scores", "labels"):
            assert torch.equal(a[key], s_[key]), key
            assert torch.equal(a[key], f[key]), key
    assert sum(len(d["boxes"]) for d in full) > 0
    eng = model.engine()
    grid, stride = eng.grid_cache, eng.stride_cache
    un = lambda o: torch.cat([o[..., :2] / stride - grid, torch.log(o[..., 2:4] / stride), o[..., 4:]], -1)
    assert _err(un(out_mod), un(out_eng)) < TOL


# ------------------------------------------------------------------------------------------------ 6. off is off
def test_keep_order_zero_is_the_unflagged_engine():
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=9)
    w = _dev_window(syn.edges_window, 6000, B, W, H, seed=51)
    tr_a = {}
    out_a = model.engine().forward_raw(*w, trace=tr_a).clone()
    _set_flag(model, True)
    eng = model.engine()
    assert all(d.keep_order == 1 for d in eng.pool_desc)
    for d in eng.pool_desc:
        d.keep_order = 0
    tr_b = {}
    out_b = eng.forward_raw(*w, trace=tr_b).clone()
    eng.check_status()
    assert torch.equal(out_a, out_b)
    for k in range(1, 5):
        for key in ("x", "pos", "batch", "rowptr", "col", "code"):
            assert torch.equal(tr_a[f"pool{k}"][key], tr_b[f"pool{k}"][key]), (k, key)
