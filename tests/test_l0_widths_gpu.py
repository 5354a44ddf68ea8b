"""The event level at 8 and 32 channels (``--base_width`` 0.25 / 1.0: Net's ``int(base_width * 32)``) through the engine:
stage-by-stage parity with the CPU oracle, the tiled level-0 conv against a float64 evaluation, asynchronous updates,
graph capture, and the refusal of every other width.  The comparison machinery and the model builders are those of
tests/test_engine_gpu.py and tests/test_async_update_gpu.py."""
import ctypes
import functools
import gc

import numpy as np
import pytest
import torch

from oracle import ops as oo
from dagr_amd.utils import synthetic as syn
from tests.test_async_update_gpu import _dev, _level1, _model
from tests.test_engine_gpu import _compare, _events, _setup

pytestmark = pytest.mark.gpu
WIDTHS = [0.25, 1.0]          # cout0 = 8, 32


@pytest.fixture(autouse=True)
def _no_garbage_left_behind():
    """Models and engines sit in reference cycles (model <-> engine) and own streams and captured HIP graphs.  They are
    collected here, between tests, and not by a collection that happens to start inside a later test's stream capture."""
    yield
    torch.cuda.synchronize()
    gc.collect()


@pytest.fixture(autouse=True, scope="module")
def _drop_the_shared_models():
    yield
    _calibrated.cache_clear()
    torch.cuda.synchronize()
    gc.collect()


@functools.lru_cache(maxsize=None)
def _calibrated(W, H, B, stream, seed, base_width, **over):
    gen = syn.edges_window if stream == "edges" else syn.uniform_window
    args, model, sd = _setup(W, H, B, seed=seed, calibrate=gen, base_width=base_width, **over)
    assert model.engine().cout0 == int(base_width * 32) and model.engine().l0_tiles
    return args, model, sd


# ----------------------------------------------------------------------------------------------- 1. engine == oracle
@pytest.mark.parametrize("bw", WIDTHS)
def test_edges_b2_rows_of_full_degree(bw):
    """320x215 (3x5 tap window), B = 2 x 3000 on the edges stream: rows of degree 16.  (6000 nodes fill their 16-node tiles;
    the ragged last tile is the 500-, 1500- and 3-event cases'.)"""
    W, H, B = 320, 215, 2
    args, model, sd = _calibrated(W, H, B, "edges", 40, bw)
    ev = _events(syn.edges_window, 3000, B, W, H, seed=41)
    _compare(args, model, sd, W, H, B, *ev, plain=True)
    assert int(model.engine().deg[:len(ev[0])].max()) == 16


@pytest.mark.parametrize("bw", WIDTHS)
def test_ncaltech_geometry_b1_the_other_tap_window(bw):
    W, H, B = 240, 180, 1
    args, model, sd = _calibrated(W, H, B, "uniform", 42, bw)
    assert model.engine().win0 != _calibrated(320, 215, 2, "edges", 40, bw)[1].engine().win0
    assert 500 % 16 != 0                             # a ragged last tile
    _compare(args, model, sd, W, H, B, *_events(syn.uniform_window, 500, B, W, H, seed=43), plain=True)


@pytest.mark.parametrize("bw", WIDTHS)
def test_three_events_and_an_empty_window(bw):
    W, H, B = 320, 215, 2
    args, model, sd = _calibrated(W, H, B, "edges", 40, bw)
    x = np.array([10, 11, 300], np.int64); y = np.array([20, 20, 200], np.int64)
    t = np.array([999000, 1000000, 1000000], np.int64); p = np.array([1, -1, 1], np.int8); b = np.array([0, 0, 1], np.int64)
    _compare(args, model, sd, W, H, B, x, y, t, p, b, syn.format_data_np(x, y, t, W, H), plain=True)
    dev = torch.device("cuda:0")
    eng = model.engine()
    out = eng.forward_raw(torch.zeros((0, 3), device=dev), torch.zeros((0, 1), device=dev),
                          torch.zeros((0,), dtype=torch.int64, device=dev))
    eng.check_status()
    assert out.shape == (B, 175, 7)
    assert torch.allclose(out[..., 4:], torch.full_like(out[..., 4:], 0.5))      # decode of all-zero maps


@pytest.mark.parametrize("bw", WIDTHS)
def test_use_image_resnet18_hp0_is_h2_then_image_features(bw):
    """--use_image: the level-0 feature map has cout0 channels too (11 / 35-channel first conv and skip), and hp0 is
    [h2 (cout0) | 64 image features] -- pool1's rows, compared with the oracle's."""
    W, H, B = 320, 215, 1
    args, model, sd = _calibrated(W, H, B, "edges", 44, bw, use_image=True, img_net="resnet18")
    eng = model.engine()
    assert eng.hp0.shape[1] == eng.cout0 + eng.feat_ch[1] and eng.feat_ch[0] == eng.cout0
    image = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 1500, B, W, H, seed=45), image=image, plain=True)


def test_wide_stem_reads_a_32_channel_level():
    W, H, B = 320, 215, 2
    args, model, sd = _calibrated(W, H, B, "edges", 46, 1.0, net_stem_width=1.0)
    assert model.engine().packs[0][0].cin == 32 + 2
    _compare(args, model, sd, W, H, B, *_events(syn.edges_window, 3000, B, W, H, seed=47), plain=True)


# ----------------------------------------------------------------------------------------------- 2. the kernel alone
def _window(L, r, den):
    lo, cnt = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.dagr_spline_tap_window(r, den, ctypes.byref(lo), ctypes.byref(cnt)) == 0
    return (min(lo.value, 2), 3) if cnt.value <= 3 else (0, 5)


KERNEL_CASES = [  # N, cout, (cmain, cextra), cskip, r, (den_x, den_y), relu
    (2001, c, blocks, cskip, r, den, relu)
    for c in (8, 32)
    for blocks, cskip, relu in (((0, 3), 0, True), ((c, 0), 3, True), ((c, 3), 0, True), ((c, 0), c + 3, False))
    for r, den in ((7, (32.0, 24.0)), (4, (20.0, 20.0)))     # 3x5 and 3x3 tap windows
] + [(17, 32, (32, 0), 35, 4, (20.0, 13.4375), True), (1, 8, (8, 0), 11, 4, (20.0, 13.4375), True)]


@pytest.mark.parametrize("N,cout,cm_ce,cskip,r,den,relu", KERNEL_CASES)
def test_tiles_match_float64_at_8_and_32_columns(N, cout, cm_ce, cskip, r, den, relu):
    """tests/test_conv_l0_tiles_gpu.py::test_tiles_match_float64's evaluation (float64, the oracle's spline basis, all 25
    taps) and its tolerance (1e-4 of the output scale) with the output width a parameter; rows of degree 0 and 16."""
    from dagr_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    cm, ce = cm_ce
    cin = cm + ce
    ldx = (cin + 3) // 4 * 4
    lds = (cskip + 3) // 4 * 4 if cskip else 0
    rng = np.random.default_rng(N * 7 + cin + cskip + cout)
    K, S = 16, 2 * r + 1
    deg = rng.integers(1, K + 1, size=N).astype(np.int32)
    deg[rng.integers(0, N, size=max(1, N // 10))] = K
    if N > 2:
        deg[1], deg[2] = 0, K
    src = rng.integers(0, N, size=(N, K)).astype(np.int32)
    src[:, 0] = np.arange(N)
    code = rng.integers(0, S * S, size=(N, K)).astype(np.int16)
    code[:, 0] = r * S + r
    x = rng.standard_normal((N, ldx)).astype(np.float32)
    xs = rng.standard_normal((N, max(lds, 1))).astype(np.float32)
    W = (rng.standard_normal((25, cin, cout)) * 0.3).astype(np.float32)
    root = (rng.standard_normal((cin, cout)) * 0.3).astype(np.float32)
    wskip = (rng.standard_normal((cskip, cout)) * 0.3).astype(np.float32)
    shift = rng.standard_normal(cout).astype(np.float32)
    (wx0, tx), (wy0, ty) = _window(L, r, den[0]), _window(L, r, den[1])
    rows = [W[(wx0 + a) + 5 * (wy0 + b)] for b in range(ty) for a in range(tx)] + [root] + ([wskip] if cskip else [])
    wpack = np.concatenate(rows, 0).astype(np.float32)
    dst = np.repeat(np.arange(N), deg)
    slot = np.concatenate([np.arange(d) for d in deg])
    e_src, e_code = src[dst, slot], code[dst, slot].astype(np.int64)
    ix, iy = e_code // S, e_code % S
    pseudo = torch.stack([torch.from_numpy((ix - r).astype(np.float32)) / np.float32(den[0]) + 0.5,
                          torch.from_numpy((iy - r).astype(np.float32)) / np.float32(den[1]) + 0.5], 1)
    basis, index = oo.spline_basis(pseudo)
    A = np.zeros((N, 25, cin), dtype=np.float64)
    xj = x[e_src, :cin].astype(np.float64)
    for s in range(4):
        np.add.at(A, (dst, index[:, s].numpy()), basis[:, s].numpy().astype(np.float64)[:, None] * xj)
    want = A.reshape(N, -1) @ W.reshape(25 * cin, cout).astype(np.float64) + x[:, :cin].astype(np.float64) @ root
    if cskip:
        want = want + xs[:, :cskip].astype(np.float64) @ wskip
    want = want + shift
    if relu:
        want = np.maximum(want, 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_src, d_code, d_deg, d_x, d_xs, d_w, d_s = T(src), T(code), T(deg), T(x), T(xs), T(wpack), T(shift)
    ldo = cout + 4                                   # (the columns behind the row's cout stay untouched)
    out = torch.full((N, ldo), float("nan"), device=dev)
    _lib.check(L.dagr_spline_conv_l0_tiles_w(cout, cm, ce, cskip, wx0, tx, wy0, ty, r, r, den[0], den[1], N, K, P(d_src),
                                             P(d_code), P(d_deg), P(d_x), ldx, P(d_xs) if cskip else None, lds, P(d_w),
                                             P(d_s), 1 if relu else 0, P(out), ldo, None, _lib.cur_stream(dev)), "l0_tiles_w")
    torch.cuda.synchronize()
    assert torch.isnan(out[:, cout:]).all()
    got = out[:, :cout].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    print(f"cout={cout} cm,ce={cm_ce} cskip={cskip} r={r}: err={err:.3e}")
    assert err < 1e-4, err


def test_the_width_entry_points_refuse_other_widths_and_combinations():
    from dagr_amd import _lib
    L = _lib.lib()
    z = torch.zeros((256, 64), device="cuda:0")
    zi = torch.zeros((64, 16), dtype=torch.int32, device="cuda:0")
    P = _lib.ptr
    call = lambda cout, cm, ce, cs: L.dagr_spline_conv_l0_tiles_w(cout, cm, ce, cs, 1, 3, 0, 5, 4, 4, 20.0, 13.4375, 16, 16,
                                                                  P(zi), P(zi), P(zi), P(z), 64, P(z), 64, P(z), P(z), 1,
                                                                  P(z), 64, None, None)
    assert call(24, 0, 3, 0) == -4          # DAGR_ERR_UNSUPPORTED
    assert call(32, 16, 0, 3) == -4         # the main block follows the width
    assert call(8, 8, 0, 3) == 0 and call(16, 16, 0, 3) == 0
    # an offset domain whose tap rows do not fit the kernel's LDS is refused, not launched
    assert L.dagr_spline_conv_l0_tiles_w(32, 32, 0, 3, 1, 3, 0, 5, 60, 60, 20.0, 13.4375, 16, 16, P(zi), P(zi), P(zi), P(z), 64,
                                         P(z), 64, P(z), P(z), 1, P(z), 64, None, None) == -1      # DAGR_ERR_INVALID_ARG
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- 3. asynchronous updates
@pytest.mark.parametrize("bw", WIDTHS)
def test_updates_of_1_10_100_events_equal_one_window(bw):
    W, H, B = 320, 215, 1
    args, model = _model(W, H, B, seed=3, base_width=bw)
    eng = model.engine()
    x, y, t, p = syn.edges_window(2111, W, H, seed=91)
    pos, feat, batch = _dev(x, y, t, p, np.zeros(2111, np.int64), W, H)
    cuts = [0, 2000, 2001, 2011, 2111]
    with torch.no_grad():
        eng.set_low_latency(False)
        eng.forward_raw(pos[:2000], feat[:2000], batch[:2000])
        assert eng.can_append()
        for lo, hi in zip(cuts[1:-1], cuts[2:]):
            out_async = eng.forward_append(pos[lo:hi], feat[lo:hi], batch[lo:hi]).clone()
        eng.check_status()
        assert eng._n_rows == 2111 and eng._async_on
        lvl_async = _level1(eng)
        out_full = eng.forward_raw(pos, feat, batch).clone()
        eng.check_status()
        lvl_full = _level1(eng)
    assert lvl_async["n"] == lvl_full["n"] and lvl_async["e"] == lvl_full["e"] and lvl_full["x"].shape[1] >= int(bw * 32) + 2
    for k in ("x", "pos", "batch", "rowptr", "col", "code"):
        assert torch.equal(lvl_async[k], lvl_full[k]), k
    assert torch.equal(out_async, out_full)


@pytest.mark.parametrize("bw", WIDTHS)
def test_reset_false_asynchronous_synchronous_and_one_window_agree(bw):
    from dagr_amd.asynchronous import make_model_asynchronous, make_model_synchronous
    from dagr_amd.data import Batch, Data
    from dagr_amd.utils.buffers import format_data
    W, H, B = 320, 215, 1
    args, model = _model(W, H, B, seed=5, base_width=bw)
    x, y, t, p = syn.edges_window(2111, W, H, seed=92)

    def batch_of(lo, hi):
        d = Data(x=torch.from_numpy(p[lo:hi].reshape(-1, 1)), pos=torch.from_numpy(np.stack([x[lo:hi], y[lo:hi]], -1)),
                 t=torch.from_numpy(t[lo:hi]), width=W, height=H, time_window=1000000)
        return format_data(Batch.from_data_list([d]).cuda())

    cuts = [0, 2000, 2001, 2011, 2111]
    outs = {}
    with torch.no_grad():
        for mode, convert in (("asynchronous", make_model_asynchronous), ("synchronous", make_model_synchronous)):
            convert(model)
            for k in range(len(cuts) - 1):
                det, = model(batch_of(cuts[k], cuts[k + 1]), reset=(k == 0), return_targets=False)
            outs[mode] = [{k: v.clone() for k, v in d.items()} for d in det]
        make_model_asynchronous(model)
        full, = model(batch_of(0, 2111), reset=True, return_targets=False)
    for a, s_, f in zip(outs["asynchronous"], outs["synchronous"], full):
        for key in ("boxes", "scores", "labels"):
            assert torch.equal(a[key], s_[key]), key
            assert torch.equal(a[key], f[key]), key


# ----------------------------------------------------------------------------------------------- 4. graph capture
@pytest.mark.parametrize("bw", WIDTHS)
def test_captured_window_and_tail_graphs_replay_the_launches_bit_for_bit(bw):
    W, H, B = 320, 215, 2
    args, model = _model(W, H, B, seed=8, base_width=bw)
    eng = model.engine()
    wins = []
    for n, seed in ((3000, 61), (1100, 62)):         # two window sizes on one capture
        x, y, t, p, b = syn.batch_windows(syn.edges_window, n, B, W, H, seed=seed)
        wins.append(_dev(x, y, t, p, b, W, H))
    with torch.no_grad():
        eng.set_low_latency(False)
        ref = [eng.forward_raw(*w).clone() for w in wins]
        eng.check_status()
        eng.set_low_latency(True)                    # the whole window as one graph (captured by the third call)
        for _ in range(3):
            got_a = eng.forward_raw(*wins[0]).clone()
        assert eng._wg is not None
        got_b = eng.forward_raw(*wins[1]).clone()
        got_a2 = eng.forward_raw(*wins[0]).clone()
        eng.check_status()
        assert torch.equal(got_a, ref[0]) and torch.equal(got_b, ref[1]) and torch.equal(got_a2, ref[0])
        eng.window_graph = False                     # level 0 launch by launch, everything behind pool1 replayed
        for _ in range(3):
            tail_a = eng.forward_raw(*wins[0]).clone()
        assert eng._graph is not None
        tail_b = eng.forward_raw(*wins[1]).clone()
        eng.check_status()
        assert torch.equal(tail_a, ref[0]) and torch.equal(tail_b, ref[1])


# ----------------------------------------------------------------------------------------------- 5. refusal
def test_other_widths_are_refused_by_name():
    args, model = _model(320, 215, 1, seed=9, base_width=0.75)      # cout0 = 24
    with pytest.raises(NotImplementedError, match="8, 16, 32"):
        model.engine()
