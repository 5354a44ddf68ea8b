"""GPU parity of the whole events-only hot path (graph -> SplineConv stack -> pooling -> head maps)
against the CPU oracle, stage by stage.  Tolerance for fp32 features / head outputs: 1e-4
(BASELINE.json north_star); graph indices, cluster assignments, pooled positions: exact."""
import numpy as np
import pytest
import torch

from oracle import model as om
from dagr_amd.utils import synthetic as syn
from dagr_amd.utils.testing_weights import randomize_

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _err(a, b):
    """1e-4 "abs/rel"  in the tensor's own unit: |a - b| <= 1e-4 * (unit + |b|) with unit = max(1, rms(b)).
    With random weights and image features the full-size windows reach |x| ~ 1e3 (one fp32 ulp there is 1.2e-4) and an
    output element is a sum of K ~ 3000 such terms that may cancel: an absolute 1e-4 on it would ask for more than
    fp32 holds, for the oracle as much as for the engine."""
    a, b = a.float().cpu(), b.float().cpu()
    if not a.numel():
        return 0.0
    unit = max(1.0, float(b.pow(2).mean().sqrt()))
    return ((a - b).abs() / (unit + b.abs())).max().item()


def _err_plain(a, b):
    """north_star's bar as written: |a - b| <= 1e-4 (1 + |b|), elementwise."""
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs() / (1 + b.abs())).max().item() if a.numel() else 0.0


def _calibrate(args, model, sd, W, H, gen, seed):
    """One oracle forward over a small calibration window batch (same geometry, same stream) with
    ``oracle.ops.calibrate_running_statistics``: the BatchNorm running statistics of `sd` become those of the model's own
    activations, i.e. seeded random weights turn into a "trained-like" model whose features are O(1) at every level."""
    import copy
    from oracle import ops as oo
    Bc = 2
    a = copy.copy(args)
    a.batch_size = Bc
    x, y, t, p, b = syn.batch_windows(gen, 6000, Bc, W, H, seed=seed)
    image_feat = cnn_out = None
    with torch.no_grad():
        if getattr(args, "use_image", False):
            img = torch.rand((Bc, 3, H, W), generator=torch.Generator().manual_seed(seed))
            feats, outs = model.backbone.net(img)
            nc = om.NetConstants(a, H, W)
            resized = [torch.nn.functional.interpolate(f, o) for f, o in zip(outs[-a.num_scales:], nc.output_sizes)]
            cnn_out, image_feat = model.head.cnn_head(resized), feats
        with oo.calibrate_running_statistics():
            om.forward_events(sd, a, H, W, x, y, t, p, b, Bc, image_feat=image_feat, cnn_out=cnn_out)
    model.load_state_dict(sd)


def _setup(W, H, B, seed=0, calibrate=None, **over):
    from dagr_amd.model.networks.dagr import DAGR
    torch.manual_seed(seed)
    args = om.default_args(batch_size=B, **over)
    model = randomize_(DAGR(args, height=H, width=W), seed=seed).eval()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if calibrate is not None:
        _calibrate(args, model, sd, W, H, calibrate, seed=900 + seed)
    model = model.cuda()
    model.cache_luts(width=W, height=H, radius=args.radius)
    return args, model, sd


def _log(name, rec):
    """Per-stage maximum errors of a named case -> one JSON line (DAGR_PARITY_LOG, default gpurun_out/ on a GPU box)."""
    import json
    import os
    path = os.environ.get("DAGR_PARITY_LOG")
    if path is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        path = os.path.join(root, "gpurun_out", "parity_stage_errors.jsonl")
    with open(path, "a") as f:
        f.write(json.dumps(dict(case=name, **rec)) + "\n")


def _path_counters(eng):
    """Which paths the last window took (device-side counters): pixels handed to k_fix_pixels (a segment beyond 64 events or
    beyond Q) and those among them that hold more than Q events, destinations deferred by the row kernel to the
    position-centric walk (> 320 candidates), destinations the row kernel answered from the inner rings of their
    neighbourhood (> 200 candidates), unsorted-timestamp fallback, and -- cumulative -- level-0 nodes the pooling merged
    through its global path."""
    import ctypes
    from dagr_amd import _lib
    g = eng.graph
    gc = (ctypes.c_int32 * 8)()
    _lib.check(eng.L.dagr_graph_counters(ctypes.byref(g.desc), _lib.ptr(g.workspace), ctypes.cast(gc, ctypes.c_void_p),
                                         _lib.cur_stream(eng.device)), "graph_counters")
    pc = (ctypes.c_int32 * 8)()
    _lib.check(eng.L.dagr_pool_counters(ctypes.byref(eng.pool_desc[0]), _lib.ptr(eng.pool_ws[0]),
                                        ctypes.cast(pc, ctypes.c_void_p), _lib.cur_stream(eng.device)), "pool_counters")
    return dict(long_pixels=int(gc[0]), beyond_fifo=int(gc[4]), deferred=int(gc[5]), unsorted=int(gc[6]),
                ring_limited=int(gc[7]), pool1_global_path=int(pc[5]))


def _events(gen, n, B, W, H, seed):
    x, y, t, p, b = syn.batch_windows(gen, n, B, W, H, seed=seed)
    pos = syn.format_data_np(x, y, t, W, H)
    return x, y, t, p, b, pos


def _edges_from_csr(rowptr, col):
    rowptr, col = rowptr.cpu().numpy(), col.cpu().numpy()
    dst = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return np.stack([col, dst])


def _sorted_cols(e):
    e = np.asarray(e)
    order = np.lexsort((e[1], e[0]))
    return e[:, order]


def _compare(args, model, sd, W, H, B, x, y, t, p, b, pos, image=None, plain=False, log=None):
    """plain=True: hold north_star's bar as written, |a - b| <= 1e-4 (1 + |b|) (cases with calibrated BatchNorm
    statistics, whose features are O(1)); otherwise the bar scaled by the tensor's rms (`_err`).  Both are recorded."""
    err = _err_plain if plain else _err
    rec = {"bar": "1e-4*(1+|b|)" if plain else "1e-4*(max(1,rms(b))+|b|)", "events": int(len(x)), "stages": {}}

    def note(stage, a, b_):
        rec["stages"][stage] = dict(plain=float(f"{_err_plain(a, b_):.3e}"), scaled=float(f"{_err(a, b_):.3e}"),
                                    absmax_ref=float(f"{float(b_.float().abs().max()) if b_.numel() else 0.0:.3e}"))
        return err(a, b_)
    dev = torch.device("cuda:0")
    eng = model.engine()
    tr_h = {}
    out_h = eng.forward_raw(torch.from_numpy(pos).to(dev), torch.from_numpy(p.astype(np.float32)).view(-1, 1).to(dev),
                            torch.from_numpy(b).to(dev), image=image, trace=tr_h)
    eng.check_status()
    tr_o = {}
    image_feat = cnn_out = None
    if image is not None:
        # the image branch is PyTorch on both sides; the oracle consumes the very feature maps the
        # engine sampled, so this checks sample_features + fusion, not MIOpen-vs-CPU conv rounding
        image_feat = [f.detach().float().cpu().contiguous() for f in eng._img_feats]
        cnn_out = {k: [o.detach().float().cpu().contiguous() for o in v] for k, v in eng._cnn_out.items()}
    # exact_pos_mean: see oracle/ops.py:pooling -- the floor of a pooled position hangs on the last bits of a mean whose
    # summation order the reference leaves unspecified; the engine's contract is the exact mean
    out_o, raw_o = om.forward_events(sd, args, H, W, x, y, t, p, b, B, trace=tr_o, image_feat=image_feat,
                                     cnn_out=cnn_out, exact_pos_mean=True)
    # graph indices: bit-exact (north_star's first clause), at whatever size the case has
    ei_h, _ = eng.graph.edge_index(tr_h["nbr"][0], tr_h["nbr"][2])
    assert ei_h.shape == tr_o["edge_index"].shape and torch.equal(ei_h.cpu(), tr_o["edge_index"]), \
        "edge_index differs from the oracle"
    rec["edges"] = int(ei_h.shape[1])
    rec["paths"] = _path_counters(eng)
    if image is not None:
        c = tr_o["x0_image"].shape[1]
        d0 = (tr_h["x0"].cpu()[:, :c] - tr_o["x0_image"]).abs().max().item()
        assert d0 < 1e-5, f"sampled level-0 image features differ by {d0}"
    # level 0 features
    d = note("layer1", tr_h["layer1"], tr_o["layer1"]["x"])
    assert d < TOL, f"layer1 features differ by {d}"
    # pooled levels
    for k in range(1, 5):
        ho, oo = tr_h[f"pool{k}"], tr_o[f"pool{k}"]
        assert ho["x"].shape[0] == oo["x"].shape[0], f"pool{k}: cluster count {ho['x'].shape[0]} vs {oo['x'].shape[0]}"
        c = oo["x"].shape[1]
        assert (ho["batch"].cpu().long() == oo["batch"]).all(), f"pool{k}: batch"
        assert (ho["pos"].cpu()[:, :2] == oo["pos"][:, :2]).all(), f"pool{k}: rounded xy not identical"
        dp = (ho["pos"].cpu()[:, 2] - oo["pos"][:, 2]).abs().max().item() if oo["pos"].numel() else 0.0
        assert dp < 1e-6, f"pool{k}: mean t differs by {dp}"
        dx = note(f"pool{k}", ho["x"][:, :c], oo["x"])
        assert dx < TOL, f"pool{k}: x differs by {dx}"
        assert (ho["x"].cpu()[:, c:c + 2] == ho["pos"].cpu()[:, :2]).all()
        eh = _sorted_cols(_edges_from_csr(ho["rowptr"], ho["col"]))
        eo = _sorted_cols(oo["edge_index"].numpy())
        assert eh.shape == eo.shape and (eh == eo).all(), f"pool{k}: coarse edges differ"
        hl, ol = tr_h[f"layer{k + 1}"], tr_o[f"layer{k + 1}"]
        dl = note(f"layer{k + 1}", hl["x"], ol["x"])
        assert dl < TOL, f"layer{k + 1} features differ by {dl}"
    # dense head maps (raw logits) and decoded outputs
    dense_h = eng._fused_dense if image is not None else tr_h["head_dense"]
    for i, dm in enumerate(dense_h):
        cls_o, reg_o, obj_o = raw_o[i]
        ref = torch.cat([reg_o, obj_o, cls_o], 1)
        dd = note(f"head_dense{i + 1}", dm, ref)
        assert dd < TOL, f"head scale {i + 1} differs by {dd}"
    rel = _decoded_err(eng, out_h, out_o, err)  # logit-domain comparison of the decoded outputs, plus a loose direct bound
    rec["stages"]["decoded_logit_domain"] = dict(plain=float(f"{_decoded_err(eng, out_h, out_o, _err_plain):.3e}"),
                                                 scaled=float(f"{_decoded_err(eng, out_h, out_o, _err):.3e}"))
    if log:
        _log(log, rec)
    assert rel < TOL, f"decoded outputs differ by {rel}"
    # (the loose direct bound on the decoded boxes: wh = exp(logit) * stride overflows fp32 on some anchors of random-weight
    # models at the largest windows -- there both sides must overflow alike, the finite entries are compared)
    bh, bo = out_h.cpu()[..., :4], out_o[..., :4]
    fin = torch.isfinite(bo)
    assert torch.equal(torch.isfinite(bh), fin) and torch.equal(bh[~fin], bo[~fin])
    assert _err(torch.where(fin, bh, torch.zeros_like(bh)), torch.where(fin, bo, torch.zeros_like(bo))) < 100 * TOL
    return out_h


def test_small_uniform_b2():
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, calibrate=syn.uniform_window)
    _compare(args, model, sd, W, H, B, *_events(syn.uniform_window, 6000, B, W, H, seed=5), plain=True)


def test_small_edges_b3_repeatable():
    W, H, B = 320, 215, 3
    args, model, sd = _setup(W, H, B, seed=1, calibrate=syn.edges_window)
    ev = _events(syn.edges_window, 8000, B, W, H, seed=7)
    o1 = _compare(args, model, sd, W, H, B, *ev, plain=True).clone()
    o2 = _compare(args, model, sd, W, H, B, *ev, plain=True)      # same buffers, second window: bit-identical
    assert torch.equal(o1, o2)


def test_vga_uniform_b1():
    W, H, B = 640, 480, 1
    args, model, sd = _setup(W, H, B, seed=2, calibrate=syn.uniform_window)
    _compare(args, model, sd, W, H, B, *_events(syn.uniform_window, 25000, B, W, H, seed=9), plain=True)


def test_empty_and_tiny_windows():
    """(The one engine case on RAW random BatchNorm statistics and the rms-scaled bar: three events cannot calibrate
    anything; every other case runs on calibrated statistics against the plain 1e-4 (1 + |b|) bar.)"""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=3)
    dev = torch.device("cuda:0")
    eng = model.engine()
    out = eng.forward_raw(torch.zeros((0, 3), device=dev), torch.zeros((0, 1), device=dev),
                          torch.zeros((0,), dtype=torch.int64, device=dev))
    eng.check_status()
    assert out.shape == (B, 175, 7)
    # all-zero dense maps -> decode of zeros: sigmoid(0)=0.5
    assert torch.allclose(out[..., 4:], torch.full_like(out[..., 4:], 0.5))
    x = np.array([10, 11, 300], np.int64); y = np.array([20, 20, 200], np.int64)
    t = np.array([999000, 1000000, 1000000], np.int64); p = np.array([1, -1, 1], np.int8); b = np.array([0, 0, 1], np.int64)
    _compare(args, model, sd, W, H, B, x, y, t, p, b, syn.format_data_np(x, y, t, W, H))


def test_use_image_resnet18_b2():
    """--use_image: sample_features at every level, 19/82/130-channel convs, CNN-head logit fusion."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=4, calibrate=syn.edges_window, use_image=True, img_net="resnet18")
    image = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 5000, B, W, H, seed=13), image=image, plain=True)


def test_dagr_l_widths_events_only():
    """dagr-l (net_stem_width = yolo_stem_width = 1: 128-channel levels, N = 256 fused head GEMM)."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=6, calibrate=syn.edges_window, net_stem_width=1.0, yolo_stem_width=1.0)
    _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 5000, B, W, H, seed=17), plain=True)


def test_max_neighbors_8_takes_the_generic_level0_kernel():
    """A checkpoint trained with max_neighbors != 16 (config key `max_neighbors`, dagr-s-dsec.yaml:10) runs on the generic
    level-0 kernel (k_conv_l0: any list length, 3x3 / 3x5 / 5x5 tap windows) instead of the 16-node tiles."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=21, calibrate=syn.edges_window, max_neighbors=8)
    assert not model.engine().l0_tiles
    _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 6000, B, W, H, seed=31), plain=True)


@pytest.mark.parametrize("name,width", [("dagr-m", 0.75), ("dagr-n", 0.25)])
def test_dagr_m_and_n_widths(name, width):
    """config/dagr-m-dsec.yaml / dagr-n-dsec.yaml (:23-24: net_stem_width = yolo_stem_width = 0.75 / 0.25): 96- and
    32-channel levels.  dagr-m's K = 26 * 98 + 98 sits past the fused pooled-level kernel's LDS tile: its convs take the
    aggregate + GEMM path."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=14, calibrate=syn.edges_window, net_stem_width=width, yolo_stem_width=width)
    _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 6000, B, W, H, seed=23), plain=True, log=name + "_events_only")


@pytest.mark.parametrize("name,width", [("dagr-m", 0.75), ("dagr-n", 0.25)])
def test_dagr_m_and_n_with_image_branch(name, width):
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=15, calibrate=syn.uniform_window, use_image=True, img_net="resnet18",
                             net_stem_width=width, yolo_stem_width=width)
    image = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        _compare(args, model, sd, W, H, B, *_events(syn.uniform_window, 5000, B, W, H, seed=29), image=image, plain=True,
                 log=name + "_resnet18")


def test_ncaltech_geometry_one_scale_100_classes():
    """config/dagr-l-ncaltech.yaml shape: 240x180 (r = 3, square-ish tap window), num_scales = 1,
    100 classes (N = 100 predictor GEMM), batch 1."""
    W, H, B = 240, 180, 1
    args, model, sd = _setup(W, H, B, seed=7, net_stem_width=1.0, yolo_stem_width=1.0, num_scales=1,
                             dataset="ncaltech101")
    _compare_one_scale(args, model, sd, W, H, B, *_events(syn.uniform_window, 6000, B, W, H, seed=19))


def test_one_scale_b3_shared_cells_keep_the_highest_node():
    """num_scales = 1 at B = 3 with 101 predictor channels: every sample's t = 1.0 cluster (QUIRK-1) shares a level-4
    cell with a regular node, and at this size torch's own CPU index_put stops being sequential -- oracle/ops.py:to_dense
    and csrc/dense.hip:k_dense_winner both define the survivor as the highest node index (parity sweep seed 2054)."""
    W, H, B = 240, 180, 3
    args, model, sd = _setup(W, H, B, seed=2054, num_scales=1, dataset="ncaltech101")
    _compare_one_scale(args, model, sd, W, H, B, *_events(syn.uniform_window, 8975, B, W, H, seed=2054 * 7 + 1))


def _decoded_err(eng, out_h, out_o, err=None):
    """Decoded outputs (dagr.py:306-312): the sigmoids directly; the box terms with the decode undone -- xy = (logit +
    grid) * stride cancels where logit ~ -grid, w, h = exp(logit) * stride turns an absolute logit error into a relative
    one -- so both are held to the tolerance in the logit domain."""
    oh, oo_ = out_h.cpu(), out_o
    grid, stride = eng.grid_cache.cpu(), eng.stride_cache.cpu()
    un = lambda o: torch.cat([o[..., :2] / stride - grid, torch.log(o[..., 2:4] / stride)], -1)
    err = err or _err
    uh, uo = un(oh), un(oo_)
    # a box logit beyond fp32's exp range (> 88.7: random weights on millions of events) decodes to +inf; the raw logits
    # themselves were compared above (head_dense), so such entries are not compared again here
    # (a logit within the tolerance of 88.72 can overflow on one side only: an entry that is infinite on either side is left
    # to the head_dense comparison)
    same_inf = torch.isinf(uh) | torch.isinf(uo)
    assert float(same_inf.float().mean()) < 0.05, "too many overflowing box logits to call the decoded comparison meaningful"
    uh, uo = torch.where(same_inf, torch.zeros_like(uh), uh), torch.where(same_inf, torch.zeros_like(uo), uo)
    return max(err(uh, uo), err(oh[..., 4:], oo_[..., 4:]))


def _compare_one_scale(args, model, sd, W, H, B, x, y, t, p, b, pos):
    dev = torch.device("cuda:0")
    eng = model.engine()
    out_h = eng.forward_raw(torch.from_numpy(pos).to(dev), torch.from_numpy(p.astype(np.float32)).view(-1, 1).to(dev),
                            torch.from_numpy(b).to(dev))
    eng.check_status()
    out_o, _ = om.forward_events(sd, args, H, W, x, y, t, p, b, B, exact_pos_mean=True)
    assert out_h.shape == out_o.shape == (B, 35, 105)
    rel = _decoded_err(eng, out_h, out_o)
    assert rel < TOL, f"decoded outputs differ by {rel}"


def test_coarse_edge_bitmap_and_generic_paths_agree():
    """pool1's coarse edges: the per-voxel 5x5 bitmap path and the generic per-edge set insertion give the same
    CSR: on a window without t == 1.0 events, on one whose last events sit at t == 1.0 as the dataset makes them
    (QUIRK-1: their in-edges land in the bitmaps of the slot one sample plane up), and on one where every event does."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=4)
    dev = torch.device("cuda:0")
    eng = model.engine()
    x, y, t, p, b, _ = _events(syn.edges_window, 9000, B, W, H, seed=11)
    last = np.flatnonzero(np.diff(np.concatenate([b, [B]])) != 0)      # last event of every sample
    for with_leak in (0, 1, 2):
        tt = np.minimum(t, 999999)
        if with_leak == 1:
            tt[last] = 1000000                                            # pos[:, 2] == 1.0 (QUIRK-1)
        elif with_leak == 2:
            tt[:] = 1000000                                               # every node is a t == 1.0 node
        pp = syn.format_data_np(x, y, tt, W, H)
        assert (pp[:, 2].max() >= 1.0) == (with_leak > 0)
        snaps = []
        for fast in (True, False):
            eng.fast_coarse_edges = fast
            tr = {}
            eng.forward_raw(torch.from_numpy(pp).to(dev), torch.from_numpy(p.astype(np.float32)).view(-1, 1).to(dev),
                            torch.from_numpy(b).to(dev), trace=tr)
            eng.check_status()
            snaps.append(tr["pool1"])
        eng.fast_coarse_edges = True
        for key in ("rowptr", "col", "code"):
            assert torch.equal(snaps[0][key], snaps[1][key]), f"pool1 {key} differs (leak={with_leak})"
        assert snaps[0]["col"].numel() > 1000


@pytest.mark.parametrize("img_net", ["resnet18", "resnet50"])
def test_image_branch_inference_copy_matches_the_modules(img_net):
    """The engine's inference copy of the image branch (BN folded, channels-last, 1x1 convs as GEMMs with the ReLU in
    the epilogue, one-pass residual joins) against the plain eval-mode modules it was derived from."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=8, use_image=True, img_net=img_net)
    eng = model.engine()
    image = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        feats, cnn_out = eng._image_branch(image)
        feats_ref, outs_ref = model.backbone.net(image)
        outs_ref = outs_ref[-eng.num_scales:]
        resized = [torch.nn.functional.interpolate(f, o) for f, o in zip(outs_ref, eng.out_sizes)]
        cnn_ref = model.head.cnn_head(resized)
    for a, b in zip(feats, feats_ref):
        scale = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 2e-4 * scale
    for k in cnn_ref:
        for a, b in zip(cnn_out[k], cnn_ref[k]):
            scale = max(1.0, float(b.abs().max()))
            assert float((a - b).abs().max()) <= 2e-4 * scale


# ---------------------------------------------------------------------------------------------------------------
# The configurations the numbers are quoted on (VERDICT r1 "weak" #1): stage-by-stage against the oracle at full
# size.  The CPU oracle needs ~4 s per 100 k events (C graph builder + torch-CPU convs), so these take a minute each.
def _bench_image(B, H, W, seed):
    # the very generator bench.py draws its resident frames from (slot 0, rank 0)
    return torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(seed)).cuda()


def test_bench_workload_dagr_s_resnet50_vga_b8_100k():
    """bench.py's default step (BASELINE config 2 on the synthetic 640x480 stream): dagr-s + --use_image --img_net
    resnet50, B = 8 windows x 100 k S-uniform events, seeds 1234.. (bench.py slot 0)."""
    W, H, B = 640, 480, 8
    args, model, sd = _setup(W, H, B, seed=0, calibrate=syn.uniform_window, use_image=True, img_net="resnet50")
    with torch.no_grad():
        _compare(args, model, sd, W, H, B, *_events(syn.uniform_window, 100000, B, W, H, seed=1234),
                 image=_bench_image(B, H, W, 77), plain=True, log="bench_workload_dagr_s_resnet50_vga_b8_100k")


def test_bench_workload_events_only_vga_b8_100k():
    """bench.py --events-only / the `events_only` leg of the default line (BASELINE config 1 shape at B = 8)."""
    W, H, B = 640, 480, 8
    args, model, sd = _setup(W, H, B, seed=0, calibrate=syn.uniform_window)
    _compare(args, model, sd, W, H, B, *_events(syn.uniform_window, 100000, B, W, H, seed=1234), plain=True,
             log="bench_workload_events_only_vga_b8_100k")


def test_s_dsec_geometry_resnet50_b8_50k_edges():
    """SURVEY 8(d) S-dsec: the geometry the reference runs DSEC at (320x215, r = 4), N = 50 k per window, B = 8,
    S-edges (saturates K = 16, stresses the FIFO depth), dagr-s + resnet50 (BASELINE config 2)."""
    W, H, B = 320, 215, 8
    args, model, sd = _setup(W, H, B, seed=9, calibrate=syn.edges_window, use_image=True, img_net="resnet50")
    with torch.no_grad():
        _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 50000, B, W, H, seed=2234),
                 image=_bench_image(B, H, W, 78), plain=True, log="s_dsec_geometry_resnet50_b8_50k_edges")


def test_dagr_l_resnet50_b8():
    """BASELINE config 4: dagr-l (128-channel levels) + --use_image --img_net resnet50, batch 8, DSEC geometry."""
    W, H, B = 320, 215, 8
    args, model, sd = _setup(W, H, B, seed=10, calibrate=syn.edges_window, use_image=True, img_net="resnet50",
                             net_stem_width=1.0, yolo_stem_width=1.0)
    with torch.no_grad():
        _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 30000, B, W, H, seed=3234),
                 image=_bench_image(B, H, W, 79), plain=True, log="dagr_l_resnet50_b8")


def test_dagr_l_resnet50_vga_b8_100k():
    """BASELINE config 4 at the size ``tools/config_probe.py`` reports it (profiles/*_config_probe.jsonl): dagr-l + --use_image
    --img_net resnet50, 640x480, B = 8 x 100 k S-uniform events -- the deep, wide levels under the bench's own stream."""
    W, H, B = 640, 480, 8
    args, model, sd = _setup(W, H, B, seed=10, calibrate=syn.uniform_window, use_image=True, img_net="resnet50",
                             net_stem_width=1.0, yolo_stem_width=1.0)
    with torch.no_grad():
        _compare(args, model, sd, W, H, B, *_events(syn.uniform_window, 100000, B, W, H, seed=1234),
                 image=_bench_image(B, H, W, 80), plain=True, log="dagr_l_resnet50_vga_b8_100k")


def _last_log(name):
    import json
    import os
    path = os.environ.get("DAGR_PARITY_LOG") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                             "gpurun_out", "parity_stage_errors.jsonl")
    recs = [json.loads(line) for line in open(path)]
    return [r for r in recs if r["case"] == name][-1]


def test_vga_edges_b8_100k_whole_engine():
    """S-edges at the BASELINE size (640x480, B = 8 x 100 k) through the whole engine: the stream the latency table
    reports next to S-uniform.  Its event-dense neighbourhoods leave the row kernel (> 320 candidates: deferred to
    k_search_dense, ev_graph.cu:48-78 semantics) and its voxels hold thousands of members."""
    W, H, B = 640, 480, 8
    args, model, sd = _setup(W, H, B, seed=0, calibrate=syn.edges_window)
    name = "vga_edges_events_only_b8_100k"
    _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 100000, B, W, H, seed=1234), plain=True, log=name)
    assert _last_log(name)["paths"]["deferred"] > 0, "the dense-neighbourhood path did not run"
    assert _last_log(name)["paths"]["ring_limited"] > 0, "no neighbourhood was answered from its inner rings"


@pytest.mark.parametrize("stream,n", [("uniform", 200000), ("uniform", 400000), ("edges", 200000), ("edges", 400000)])
def test_vga_b1_dense_windows(stream, n):
    """N = 200 k / 400 k events in ONE 50 ms window (the right end of bench.py's latency table), both streams: graph
    indices exact, features 1e-4 (1 + |b|).  These windows are the ones that leave the fast paths: neighbourhoods beyond
    320 candidates, pixels beyond the FIFO depth (ev_graph.cu:201-211)."""
    W, H, B = 640, 480, 1
    gen = syn.uniform_window if stream == "uniform" else syn.edges_window
    args, model, sd = _setup(W, H, B, seed=3, calibrate=gen)
    name = f"vga_b1_{stream}_{n // 1000}k"
    _compare(args, model, sd, W, H, B, *_events(gen, n, B, W, H, seed=4234), plain=True, log=name)
    paths = _last_log(name)["paths"]
    if stream == "edges" or n >= 400000:
        assert paths["deferred"] > 0, "the dense-neighbourhood path did not run"
    assert paths["pool1_global_path"] > 0          # the window's t == 1.0 event (QUIRK-1) at least


@pytest.mark.parametrize("stream,n", [("edges", 200000), ("uniform", 400000)])
def test_vga_b8_dense_windows(stream, n):
    """The B = 8 columns of bench.py's latency table beyond 100 k events per window (1.6 M events per step): the same
    stage-by-stage comparison as the B = 1 cases above, eight sample planes at once -- the 8 x 200 k S-edges column and the
    largest one, 8 x 400 k S-uniform (3.2 M events: the CPU oracle takes two minutes on it)."""
    W, H, B = 640, 480, 8
    gen = syn.uniform_window if stream == "uniform" else syn.edges_window
    args, model, sd = _setup(W, H, B, seed=3, calibrate=gen)
    name = f"vga_b8_{stream}_{n // 1000}k"
    _compare(args, model, sd, W, H, B, *_events(gen, n, B, W, H, seed=4234), plain=True, log=name)
    paths = _last_log(name)["paths"]
    assert paths["deferred"] > 0, "the dense-neighbourhood path did not run"
    if stream == "uniform":
        assert paths["ring_limited"] > 0, "no neighbourhood was answered from its inner rings"


def test_bench_workload_dagr_s_resnet50_vga_b8_100k_edges():
    """The `image_resnet50` x S-edges column of the latency table at the bench size: dagr-s + --use_image --img_net
    resnet50, 640x480, B = 8 x 100 k S-edges events."""
    W, H, B = 640, 480, 8
    args, model, sd = _setup(W, H, B, seed=0, calibrate=syn.edges_window, use_image=True, img_net="resnet50")
    with torch.no_grad():
        _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 100000, B, W, H, seed=4234),
                 image=_bench_image(B, H, W, 77), plain=True, log="dagr_s_resnet50_vga_b8_100k_edges")


@pytest.mark.parametrize("stream", ["uniform", "edges"])
def test_full_size_pooled_positions_against_the_fp32_sequential_form(stream):
    """The full-size cases above compare pooled positions with the exact-mean form of the oracle.  The form pinned to the
    reference's own code is the fp32 sequential sum; on voxels with hundreds of members the two differ in the last bits
    of a mean that is then floored to the pixel grid.  This case makes that deviation a number: the engine's rounded xy
    of the 8 x 100 k window batch against BOTH forms -- identical to the exact form, and the clusters on which the fp32
    sequential form lands on the neighbouring pixel are counted and logged (a handful of ~18 k)."""
    from oracle import graph as og
    from oracle import ops as oo
    W, H, B = 640, 480, 8
    args, model, sd = _setup(W, H, B, seed=0)
    gen = syn.uniform_window if stream == "uniform" else syn.edges_window
    x, y, t, p, b, pos = _events(gen, 100000, B, W, H, seed=1234)
    dev = torch.device("cuda:0")
    eng = model.engine()
    tr = {}
    eng.forward_raw(torch.from_numpy(pos).to(dev), torch.from_numpy(p.astype(np.float32)).view(-1, 1).to(dev),
                    torch.from_numpy(b).to(dev), trace=tr)
    eng.check_status()
    got = tr["pool1"]["pos"].cpu()
    nc = om.NetConstants(args, H, W)
    post = torch.from_numpy(pos)
    batch = torch.from_numpy(b.astype(np.int64))
    no_edges = torch.zeros((2, 0), dtype=torch.int64)
    dummy = torch.zeros((len(x), 1))
    exact = oo.pooling(nc.pools[0], dummy, post, batch, no_edges, exact_mean=True)[1]
    seq32 = oo.pooling(nc.pools[0], dummy, post, batch, no_edges, exact_mean=False)[1]
    assert got.shape == exact.shape
    assert torch.equal(got[:, :2], exact[:, :2])
    flips = int((seq32[:, :2] != exact[:, :2]).any(1).sum())
    dmax = float(((seq32[:, :2] - exact[:, :2]).abs() * torch.tensor([W, H])).max())       # in pixels, per axis
    _log(f"pool1_positions_vs_fp32_sequential_{stream}_vga_b8_100k",
         dict(clusters=int(exact.shape[0]), clusters_where_fp32_sequential_floors_to_another_pixel=flips,
              largest_difference_px=round(dmax, 3)))
    assert flips <= 16 and dmax <= 1.001, (flips, dmax)       # a rounding-order effect: never more than the next pixel


def test_round_to_pixel_near_tie_follows_the_exact_mean():
    """Pooled positions are cluster means floored to the pixel grid (pooling.py:47-49,67,86).  The reference sums with
    float atomics (order-dependent), the oracle sequentially in fp32, the engine exactly (64-bit fixed point): on a
    voxel whose mean lands within fp32 noise of a pixel boundary the three may legitimately differ.  The engine's
    contract: the reference's fp32 formula applied to the correctly-rounded exact mean.  Constructed case: 313 events
    in one voxel with sum(x) = 312 (mod 313), i.e. frac(mean_x * W + 1e-5 * W) within 1e-5 of an integer."""
    from oracle import ops as oo
    W, H, B = 320, 215, 1
    args, model, sd = _setup(W, H, B, seed=11)
    n = 313
    rng = np.random.default_rng(0)
    for target in (312, 311, 0, 1):       # residues around the boundary (and two safe ones)
        x = rng.integers(8, 12, n)        # one 5.7-px-wide level-1 voxel column: x in [8, 11]
        k = 0
        while int(x.sum()) % n != target and k < n:     # nudge single events inside the voxel until the residue fits
            if x[k] < 11:
                x[k] += 1
            k += 1
        assert int(x.sum()) % n == target and x.min() >= 6 and x.max() <= 11
        y = np.full(n, 3, np.int64)
        t = np.sort(rng.integers(960000, 1000000, n)); t[-1] = 1000000 - 1
        p = np.ones(n, np.int8); b = np.zeros(n, np.int64)
        pos = syn.format_data_np(x, y, t, W, H)
        dev = torch.device("cuda:0")
        eng = model.engine()
        tr = {}
        eng.forward_raw(torch.from_numpy(pos).to(dev), torch.from_numpy(p.astype(np.float32)).view(-1, 1).to(dev),
                        torch.from_numpy(b).to(dev), trace=tr)
        eng.check_status()
        got = tr["pool1"]["pos"].cpu()
        assert got.shape[0] == 1
        mean = torch.from_numpy(pos.astype(np.float64).mean(0).astype(np.float32))      # correctly-rounded exact mean
        want_xy = oo.round_to_pixel(mean[:2].view(1, 2), 1 / torch.Tensor([[W, H]]))
        assert torch.equal(got[:, :2], want_xy), (target, got[:, :2], want_xy)
        assert abs(float(got[0, 2]) - float(mean[2])) < 1e-7


def _dev_window(gen, n, B, W, H, seed):
    dev = torch.device("cuda:0")
    x, y, t, p, b, pos = _events(gen, n, B, W, H, seed=seed)
    return (torch.from_numpy(pos).to(dev), torch.from_numpy(p.astype(np.float32)).view(-1, 1).to(dev),
            torch.from_numpy(b).to(dev))


def test_window_graph_replay_matches_eager_launches():
    """Latency mode: forward_raw stages the caller's window with one launch and replays the WHOLE window -- graph build,
    level 0, pooling, tail, heads, decode -- as one captured HIP graph whose launches are sized for the engine's event
    capacity and bounded by device-side counts.  Same kernels, same order per buffer: the outputs are bit-identical to
    the launch-by-launch (trace) path, for windows of DIFFERENT sizes through the same captured graph, an empty window
    included."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=12)
    dev = torch.device("cuda:0")
    eng = model.engine().set_low_latency(True)
    wins = [_dev_window(syn.edges_window, n, B, W, H, seed) for n, seed in ((4000, 41), (2500, 43), (6000, 45), (1, 47))]
    wins.append((torch.zeros((0, 3), device=dev), torch.zeros((0, 1), device=dev), torch.zeros((0,), dtype=torch.int64, device=dev)))
    eager = [eng.forward_raw(*w, trace={}).clone() for w in wins]
    got = []
    for rep in range(3):
        for k, w in enumerate(wins):
            got.append((k, eng.forward_raw(*w)))
    assert eng._wg is not None, "the window was not captured"
    eng.check_status()
    for k, o in got:
        assert torch.equal(o, eager[k]), k
    # a window beyond the capacity grows the buffers and re-captures
    cap0 = eng.max_events
    big = _dev_window(syn.uniform_window, cap0 // B + 500, B, W, H, seed=49)
    want = eng.forward_raw(*big, trace={}).clone()
    for rep in range(4):
        assert torch.equal(eng.forward_raw(*big), want)
    assert eng.max_events > cap0 and eng._wg is not None
    assert torch.equal(eng.forward_raw(*wins[0]), eager[0])


def test_detections_come_out_of_the_captured_window():
    """Latency mode: ``forward_detections`` replays forward + post-processing (confidence mask, class-offset NMS,
    model/utils.py:61-110) as ONE captured graph -- det / n_keep bit-identical to the launch-by-launch forward followed by
    ``postprocess_device``, for windows of different sizes through the same graph, after a change of the thresholds
    (re-capture), and for asynchronous updates through the captured tail."""
    from dagr_amd.model.utils import postprocess_device
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=12)
    eng = model.engine().set_low_latency(True)
    wins = [_dev_window(syn.edges_window, n, B, W, H, seed) for n, seed in ((4000, 41), (2500, 43), (6000, 45))]

    def want(w, conf, nms):
        o = eng.forward_raw(*w, trace={})
        det, nk = postprocess_device(o, eng.num_classes, conf, nms, H, W)
        return det.clone(), nk.clone()
    for conf, nms in ((0.001, 0.65), (0.05, 0.5)):
        model.conf_threshold, model.nms_threshold = conf, nms
        ref = [want(w, conf, nms) for w in wins]
        for rep in range(3):
            for k, w in enumerate(wins):
                det, nk = eng.forward_detections(*w)
                assert torch.equal(nk, ref[k][1]), (conf, rep, k)
                for b in range(B):
                    n = int(nk[b])
                    assert torch.equal(det[b, :n], ref[k][0][b, :n]), (conf, rep, k, b)
        assert eng._wg is not None and eng._post_fresh, "the window (with its post-processing) was not captured"
        assert int(ref[0][1].sum()) > 0
    # asynchronous updates: the captured tail ends with the post-processing too
    model.conf_threshold, model.nms_threshold = 0.001, 0.65
    upd = [_dev_window(syn.edges_window, 300, B, W, H, s) for s in (61, 62, 63)]
    eng.tail_graph = False
    eng.forward_raw(*wins[0])
    ref = []
    for u in upd:
        o = eng.forward_append(*u)
        det, nk = postprocess_device(o, eng.num_classes, 0.001, 0.65, H, W)
        ref.append((det.clone(), nk.clone()))
    eng.tail_graph = True
    eng.forward_raw(*wins[0])
    for k, u in enumerate(upd):
        det, nk = eng.forward_detections(*u, append=True)
        assert torch.equal(nk, ref[k][1])
        for b in range(B):
            assert torch.equal(det[b, :int(nk[b])], ref[k][0][b, :int(nk[b])])
    eng.check_status()
    # throughput mode (no captured graphs): the heads' last launch post-processes every image all the same
    from dagr_amd.engine import WindowEngine
    eng2 = WindowEngine(model).set_low_latency(False)
    assert not eng2.window_graph and not eng2.tail_graph
    for k, w in enumerate(wins):
        o = eng2.forward_raw(*w).clone()
        want_det, want_nk = postprocess_device(o, eng2.num_classes, 0.001, 0.65, H, W)
        det, nk = eng2.forward_detections(*w)
        assert torch.equal(nk, want_nk)
        for b in range(B):
            assert torch.equal(det[b, :int(nk[b])], want_det[b, :int(nk[b])])
        assert torch.equal(eng2.forward_raw(*w), o)            # the decoded outputs are written as before


def test_window_graph_with_the_image_branch():
    """--use_image: the dense branch (ResNet + CNN head on PyTorch-ROCm) sits inside the captured window too, on a static
    frame buffer.  Replayed windows (different frames and window sizes through the same graph) equal the launch-by-launch
    path to the library kernels' rounding: MIOpen may pick another solver between its first and later calls, and the
    library GEMMs behind the 1x1 convolutions may split K with atomics (low bits differ from run to run, eager or not)."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=13, use_image=True, img_net="resnet18")
    eng = model.engine().set_low_latency(True)
    wins = [_dev_window(syn.uniform_window, n, B, W, H, seed) for n, seed in ((3000, 51), (5000, 53))]
    imgs = [torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(s)).cuda() for s in (7, 8)]
    with torch.no_grad():
        eager = [eng.forward_raw(*w, image=im, trace={}).clone() for w, im in zip(wins, imgs)]
        runs = [[eng.forward_raw(*wins[k], image=imgs[k]) for k in range(2)] for rep in range(5)]
    assert eng._wg is not None
    eng.check_status()
    for k in range(2):
        for rep in range(5):
            assert _decoded_err(eng, runs[rep][k], eager[k].cpu()) < 1e-4, (rep, k)
    assert _decoded_err(eng, runs[-1][0], runs[-1][1].cpu()) > 1e-3      # the two windows are different windows


def test_pipelined_image_window_samples_every_map_after_its_event():
    """In a captured --use_image window the image branch runs on a stream of its own and the graph levels start when
    THEIR feature map exists: every sampler must be ordered behind the event of the map it reads (a trunk
    forward that recorded no per-map event let the graph levels read the maps without a dependency).  Same outputs as
    the launch-by-launch engine to the library kernels' rounding, and every sampled map had its event."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=13, use_image=True, img_net="resnet18")
    win = _dev_window(syn.uniform_window, 4000, B, W, H, 51)
    img = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(7)).cuda()
    with torch.no_grad():
        want = model.engine().forward_raw(*win, image=img, trace={}).clone()
        from dagr_amd.engine import WindowEngine
        eng = WindowEngine(model).set_low_latency(True)
        seen = []
        sample0 = eng._sample

        def spy(*a, **k):
            seen.append(eng._feat_ready is not None and id(a[5]) in eng._feat_ready)
            return sample0(*a, **k)
        eng._sample = spy
        runs = [eng.forward_raw(*win, image=img).clone() for _ in range(5)]
    assert eng._wg is not None and seen and all(seen), seen
    eng.check_status()
    for r in runs:
        assert _decoded_err(eng, r, want.cpu()) < 1e-4


def test_tail_graph_replay_matches_eager_launches():
    """The asynchronous update (forward_append) replays everything after pool1 as one captured HIP graph (head scale 1
    beside pool4 / layer5 / head scale 2): bit-identical to the launch-by-launch path."""
    W, H, B = 320, 215, 2
    args, model, sd = _setup(W, H, B, seed=12)
    eng = model.engine().set_low_latency(True)
    w0 = _dev_window(syn.edges_window, 4000, B, W, H, 41)
    upd = [_dev_window(syn.edges_window, 300, B, W, H, s) for s in (61, 62, 63, 64)]
    eng.tail_graph = False
    eng.forward_raw(*w0)
    eager = [eng.forward_append(*u).clone() for u in upd]
    eng.tail_graph = True
    eng.forward_raw(*w0)
    got = [eng.forward_append(*u).clone() for u in upd]
    assert eng._graph is not None, "the tail was not captured"
    eng.check_status()
    for a_, b_ in zip(got, eager):
        assert torch.equal(a_, b_)
