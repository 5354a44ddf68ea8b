"""The heads' last launch through the C ABI: dagr_heads_finish, dagr_heads_finish_detect, dagr_decode_heads (csrc/nms.hip)
and dagr_to_dense (csrc/dense.hip) against a numpy restatement kept here:

  cell   = trunc(float32(pos) / float32(voxel)); among the nodes below ``*n_ptr`` the highest index wins a cell
  logit  = the winner's predictor value (0 for an empty cell) + the CNN head's logit           (one fp32 add)
  decode = xy: (logit + cell) * stride; wh: exp(logit) * stride; objectness / classes: 1 / (1 + exp(-logit))

Bars: the ``dense`` by-product, dagr_to_dense and the decoded x, y are BIT-EQUAL to numpy float32.  w, h and the sigmoids
are held to a float64 evaluation within ``4 * 2^-23 * |want|``: the device code is ``expf`` (documented to 1 ulp) followed
by one or two correctly rounded operations, about 3 ulp.  Measured on the MI355X over all cases here, logits
in [-10, 10] included: w, h at most 0.95 ulp, sigmoids at most 1.00 ulp (every test prints its own maxima).
dagr_decode_heads on the by-product and dagr_heads_finish_detect's ``out`` are bit-equal to dagr_heads_finish's ``out``;
its detections are bit-equal to dagr_postprocess on that ``out`` and follow tests/test_postprocess_paths_gpu.py's rules
against the oracle."""
import ctypes

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from tests import nms_cases as nc

pytestmark = pytest.mark.gpu

F32 = np.float32
ULP = 2.0 ** -23
ENGINE = [(10, 14, F32(1 / 7) / F32(2), F32(1 / 5) / F32(2), 22.0), (5, 7, F32(1 / 7), F32(1 / 5), 43.0)]     # 320 x 215
LARGE = [(20, 24, F32(1 / 24), F32(1 / 20), 16.0), (10, 12, F32(1 / 12), F32(1 / 10), 32.0)]                # A = 600
CLASS_OFFSET = 641.0


def _make_scale(rng, geom, B, CH, cnn, ld_extra, empty_image, live_oob, spread):
    """One head scale's host arrays.  Live nodes: several per cell (QUIRK-1 duplicates: about half as many distinct cells
    as nodes), some exactly on a cell boundary, none in ``empty_image``; the rows from ``n_live`` to ``n_max`` hold
    positions and samples outside the map and must be ignored.  ``live_oob``: one live node outside the map."""
    Hc, Wc, vx, vy, stride = geom
    n_live = 3 * B * Hc * Wc // 4
    n_max = n_live + 37
    images = [b for b in range(B) if b != empty_image]
    cells = rng.integers(0, max(1, Hc * Wc // 2), n_live) * 2 % (Hc * Wc)
    cells[: Hc * Wc // 4] = rng.integers(0, Hc * Wc, Hc * Wc // 4)
    cy, cx = cells // Wc, cells % Wc
    u = rng.uniform(0.05, 0.95, (n_live, 2))
    u[::7] = 0.0                                              # exactly float32(k * voxel): whichever cell fp32 says
    pos = np.zeros((n_max, 3), F32)
    pos[:n_live, 0] = ((cx + u[:, 0]) * np.float64(vx)).astype(F32)
    pos[:n_live, 1] = ((cy + u[:, 1]) * np.float64(vy)).astype(F32)
    pos[:n_live, 2] = rng.uniform(0, 1, n_live)
    batch = np.zeros(n_max, np.int32)
    batch[:n_live] = rng.choice(images, n_live)
    pos[n_live:, :2] = 5.0
    batch[n_live::2] = B + 3
    if live_oob:
        pos[n_live // 2, 0] = 1.5
    ld = CH + ld_extra
    pred = rng.uniform(-spread, spread, (n_max, ld)).astype(F32)
    if spread < 5:                                            # boxes of 4 - 5 strides next to their cells: they overlap
        pred[:, :2] = rng.uniform(-0.5, 0.5, (n_max, 2))
        pred[:, 2:4] = rng.uniform(1.4, 1.6, (n_max, 2))
    maps = None
    if cnn:
        amp = 0.25 if spread < 5 else 4.0
        maps = [rng.uniform(-amp, amp, (B, c, Hc, Wc)).astype(F32) for c in (4, 1, CH - 5)]
    return dict(geom=geom, n_live=n_live, n_max=n_max, pos=pos, batch=batch, pred=pred, ld=ld, cnn=maps, layout=cnn)


def _make(geoms, B, C, cnn=None, ld_extra=0, empty_image=None, live_oob=False, seed=0, spread=3.0):
    rng = np.random.default_rng(seed)
    return [_make_scale(rng, g, B, 5 + C, cnn, ld_extra, empty_image, live_oob and i == 0, spread) for i, g in enumerate(geoms)]


def _reference(scales, B, CH):
    """(events-only maps, fused logit maps, out32 with exact x / y, out64 float64 evaluation, status)."""
    ev_maps, maps, outs32, outs64, status = [], [], [], [], 0
    for s in scales:
        Hc, Wc, vx, vy, stride = s["geom"]
        n = s["n_live"]
        cx = np.trunc(s["pos"][:n, 0] / F32(vx)).astype(np.int64)         # fp32 division
        cy = np.trunc(s["pos"][:n, 1] / F32(vy)).astype(np.int64)
        ev = np.zeros((B, CH, Hc, Wc), F32)
        for i in range(n):                                                 # ascending: the highest index stays
            b = int(s["batch"][i])
            if not (0 <= cx[i] < Wc and 0 <= cy[i] < Hc and 0 <= b < B):
                status |= 1
                continue
            ev[b, :, cy[i], cx[i]] = s["pred"][i, :CH]
        logit = ev if s["cnn"] is None else ev + np.concatenate(s["cnn"], axis=1)
        assert logit.dtype == F32 and np.abs(logit).max() <= 10.0
        grid_y, grid_x = np.meshgrid(np.arange(Hc, dtype=F32), np.arange(Wc, dtype=F32), indexing="ij")
        o32 = np.zeros((B, CH, Hc, Wc), F32)
        o32[:, 0] = (logit[:, 0] + grid_x) * F32(stride)
        o32[:, 1] = (logit[:, 1] + grid_y) * F32(stride)
        l64 = logit.astype(np.float64)
        o64 = o32.astype(np.float64)
        o64[:, 2:4] = np.exp(l64[:, 2:4]) * stride
        o64[:, 4:] = 1.0 / (1.0 + np.exp(-l64[:, 4:]))
        ev_maps.append(ev)
        maps.append(logit)
        outs32.append(o32.reshape(B, CH, -1).transpose(0, 2, 1))
        outs64.append(o64.reshape(B, CH, -1).transpose(0, 2, 1))
    return ev_maps, maps, np.concatenate(outs32, 1), np.concatenate(outs64, 1), status


class _Device:
    """The scales on the device as dagr_head_scale structs (the tensors are kept alive here)."""

    def __init__(self, scales, B, CH, dense=True, use_n_ptr=True):
        self.keep, self.hs, self.dense = [], [], []
        dev = torch.device("cuda")

        def up(a):
            t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self.keep.append(t)
            return t
        for s in scales:
            Hc, Wc, vx, vy, stride = s["geom"]
            # without n_ptr the kernel takes n_max rows: hand it the live ones only
            n_ptr = up(np.array([s["n_live"], 0], np.int32)) if use_n_ptr else None
            hs = _lib.HeadScale(n_ptr=n_ptr.data_ptr() if use_n_ptr else None, n_max=s["n_max"] if use_n_ptr else s["n_live"],
                                pred=up(s["pred"]).data_ptr(), ld=s["ld"], pos=up(s["pos"]).data_ptr(),
                                batch=up(s["batch"]).data_ptr(), vx=float(vx), vy=float(vy), stride=float(stride), Hc=Hc, Wc=Wc)
            if s["cnn"] is not None:
                for k, m in enumerate(s["cnn"]):
                    t = up(m)
                    if s["layout"] == "nhwc":
                        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # same values, channels-last strides
                        self.keep.append(t)
                        assert t.stride(1) == 1 or t.shape[1] == 1
                    hs.cnn[k] = t.data_ptr()
                    for j in range(4):
                        hs.cnn_stride[k][j] = int(t.stride(j))
            if dense:
                d = torch.full((B, CH, Hc, Wc), float("nan"), dtype=torch.float32, device=dev)
                self.dense.append(d)
                hs.dense = d.data_ptr()
            self.hs.append(hs)
        self.A = sum(s["geom"][0] * s["geom"][1] for s in scales)
        self.B, self.CH, self.dev = B, CH, dev
        self.s0 = ctypes.byref(self.hs[0])
        self.s1 = ctypes.byref(self.hs[1]) if len(self.hs) > 1 else None

    def finish(self):
        out = torch.full((self.B, self.A, self.CH), float("nan"), dtype=torch.float32, device=self.dev)
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        _lib.check(_lib.lib().dagr_heads_finish(self.s0, self.s1, self.B, self.CH, _lib.ptr(out), _lib.ptr(status),
                                                _lib.cur_stream(self.dev)), "heads_finish")
        torch.cuda.synchronize()
        return out, int(status.item())

    def finish_detect(self, conf, iou):
        out = torch.full((self.B, self.A, self.CH), float("nan"), dtype=torch.float32, device=self.dev)
        det = torch.full((self.B, self.A, 6), float("nan"), dtype=torch.float32, device=self.dev)
        n_keep = torch.full((self.B,), -1, dtype=torch.int32, device=self.dev)
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        _lib.check(_lib.lib().dagr_heads_finish_detect(self.s0, self.s1, self.B, self.CH, _lib.ptr(out), _lib.ptr(status),
                                                       float(conf), float(iou), CLASS_OFFSET, _lib.ptr(det), _lib.ptr(n_keep),
                                                       _lib.cur_stream(self.dev)), "heads_finish_detect")
        torch.cuda.synchronize()
        return out, det, n_keep, int(status.item())


def _ulp(got, want):
    """max |got - want| / (2^-23 |want|) over float64 ``want`` (never 0 here: exp and sigmoid of a finite logit)."""
    return float(np.max(np.abs(got.astype(np.float64) - want) / (ULP * np.abs(want))))


def _check_out(got, out32, out64, what):
    got = got.cpu().numpy()
    assert np.array_equal(got[..., :2].view(np.int32), out32[..., :2].view(np.int32)), f"{what}: decoded x, y differ in bits"
    wh, sg = _ulp(got[..., 2:4], out64[..., 2:4]), _ulp(got[..., 4:], out64[..., 4:])
    print(f"{what}: w, h within {wh:.2f} ulp, sigmoids within {sg:.2f} ulp of the float64 evaluation")
    bad = np.abs(got.astype(np.float64) - out64) > 4 * ULP * np.abs(out64)
    bad[..., :2] = False
    assert not bad.any(), (f"{what}: {int(bad.sum())} decoded values beyond 4 ulp, first at (b, a, ch) = "
                           f"{tuple(int(v) for v in np.argwhere(bad)[0])}: got {got[bad][0]!r}, want {out64[bad][0]!r}")
    return wh, sg


CASES = [
    # geometry, B, C, CNN logits, ld - channels, image without a node, dense by-product, n_ptr
    ("engine", ENGINE, 1, 2, None, 0, None, True, True),
    ("engine", ENGINE, 3, 2, "nchw", 3, 1, True, True),
    ("engine", ENGINE, 8, 2, "nhwc", 0, 5, True, True),
    ("engine", ENGINE, 8, 2, None, 0, 0, False, True),
    ("engine", ENGINE, 3, 8, "nhwc", 5, 2, False, False),
    ("one scale", ENGINE[:1], 1, 1, "nchw", 0, None, True, True),
    ("one scale", ENGINE[1:], 8, 3, None, 2, 7, True, False),
    ("large", LARGE, 1, 2, "nhwc", 0, None, True, True),
    ("large", LARGE, 3, 3, None, 1, 0, True, True),
    ("large", LARGE, 8, 1, "nchw", 0, 3, False, True),
]
_IDS = [f"{c[0]}-B{c[2]}-C{c[3]}-{c[4] or 'events'}-ld+{c[5]}-empty{c[6]}-{'dense' if c[7] else 'nodense'}-"
        f"{'nptr' if c[8] else 'nmax'}" for c in CASES]


@pytest.mark.parametrize("name,geoms,B,C,cnn,ld_extra,empty,dense,use_n_ptr", CASES, ids=_IDS)
def test_heads_finish_against_numpy(name, geoms, B, C, cnn, ld_extra, empty, dense, use_n_ptr):
    CH = 5 + C
    scales = _make(geoms, B, C, cnn, ld_extra, empty, seed=B * 100 + C)
    ev_maps, maps, out32, out64, status = _reference(scales, B, CH)
    assert status == 0
    d = _Device(scales, B, CH, dense=dense, use_n_ptr=use_n_ptr)
    out, st = d.finish()
    assert st == 0, "rows past *n_ptr hold positions outside the map: they must be ignored"
    _check_out(out, out32, out64, name)
    if dense:
        for i, m in enumerate(maps):
            assert np.array_equal(d.dense[i].cpu().numpy().view(np.int32), m.view(np.int32)), f"dense by-product, scale {i}"
        # dagr_decode_heads on the by-product: the same decode, bit for bit
        again = torch.full_like(out, float("nan"))
        d1 = d.dense[1] if len(d.dense) > 1 else None
        g1 = geoms[1] if len(geoms) > 1 else (0, 0, 0, 0, 0.0)
        _lib.check(_lib.lib().dagr_decode_heads(_lib.ptr(d.dense[0]), geoms[0][0], geoms[0][1], float(geoms[0][4]), _lib.ptr(d1),
                                                g1[0], g1[1], float(g1[4]), B, CH, _lib.ptr(again), _lib.cur_stream(d.dev)),
                   "decode_heads")
        torch.cuda.synchronize()
        assert torch.equal(nc.bits(again), nc.bits(out)), "dagr_decode_heads differs from dagr_heads_finish"
    # dagr_to_dense of every scale: the events-only maps
    for i, s in enumerate(scales):
        Hc, Wc, vx, vy, _ = s["geom"]
        t = [torch.from_numpy(s[k]).cuda() for k in ("pred", "pos", "batch")]
        n_ptr = torch.tensor([s["n_live"], 0], dtype=torch.int32, device="cuda")
        scratch = torch.zeros(B * Hc * Wc, dtype=torch.int32, device="cuda")
        got = torch.full((B, CH, Hc, Wc), float("nan"), dtype=torch.float32, device="cuda")
        status_t = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib().dagr_to_dense(_lib.ptr(n_ptr), s["n_max"], _lib.ptr(t[0]), s["ld"], CH, _lib.ptr(t[1]),
                                            _lib.ptr(t[2]), float(vx), float(vy), B, Hc, Wc, _lib.ptr(scratch), _lib.ptr(got),
                                            _lib.ptr(status_t), _lib.cur_stream(got.device)), "to_dense")
        torch.cuda.synchronize()
        assert int(status_t.item()) == 0
        assert np.array_equal(got.cpu().numpy().view(np.int32), ev_maps[i].view(np.int32)), f"dagr_to_dense, scale {i}"


@pytest.mark.parametrize("geoms", [ENGINE, LARGE], ids=["engine", "large"])
def test_one_live_node_outside_the_map_sets_status_and_changes_nothing_else(geoms):
    B, C = 3, 2
    CH = 5 + C
    scales = _make(geoms, B, C, "nchw", 0, None, live_oob=True, seed=11)
    _, maps, out32, out64, status = _reference(scales, B, CH)
    assert status == 1
    d = _Device(scales, B, CH)
    out, st = d.finish()
    assert st & 1
    _check_out(out, out32, out64, "one live node outside")
    for i, m in enumerate(maps):
        assert np.array_equal(d.dense[i].cpu().numpy().view(np.int32), m.view(np.int32))
    s = scales[0]
    Hc, Wc, vx, vy, _ = s["geom"]
    t = [torch.from_numpy(s[k]).cuda() for k in ("pred", "pos", "batch")]
    n_ptr = torch.tensor([s["n_live"], 0], dtype=torch.int32, device="cuda")
    scratch = torch.zeros(B * Hc * Wc, dtype=torch.int32, device="cuda")
    got = torch.full((B, CH, Hc, Wc), float("nan"), dtype=torch.float32, device="cuda")
    status_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().dagr_to_dense(_lib.ptr(n_ptr), s["n_max"], _lib.ptr(t[0]), s["ld"], CH, _lib.ptr(t[1]), _lib.ptr(t[2]),
                                        float(vx), float(vy), B, Hc, Wc, _lib.ptr(scratch), _lib.ptr(got), _lib.ptr(status_t),
                                        _lib.cur_stream(got.device)), "to_dense")
    torch.cuda.synchronize()
    assert int(status_t.item()) & 1
    ev = _reference(scales, B, CH)[0][0]
    assert np.array_equal(got.cpu().numpy().view(np.int32), ev.view(np.int32))


@pytest.mark.parametrize("geoms", [ENGINE, LARGE], ids=["engine", "large"])
def test_decode_error_in_ulp(geoms):
    """Logits over the whole of [-10, 10] (predictor +-6, CNN +-4), where neither exp nor the sigmoid saturates: the
    measured maxima, in ulp of the float64 value, are printed and held to 4."""
    B, C = 8, 3
    CH = 5 + C
    scales = _make(geoms, B, C, "nhwc", 0, None, seed=3, spread=6.0)
    _, _, out32, out64, _ = _reference(scales, B, CH)
    out, st = _Device(scales, B, CH, dense=False).finish()
    assert st == 0
    wh, sg = _check_out(out, out32, out64, f"logits in [-10, 10], A = {out.shape[1]}")
    assert wh <= 4.0 and sg <= 4.0


def _postprocess(out, C, conf, iou):
    B, A, _ = out.shape
    det = torch.full((B, A, 6), float("nan"), dtype=torch.float32, device=out.device)
    n_keep = torch.full((B,), -1, dtype=torch.int32, device=out.device)
    _lib.check(_lib.lib().dagr_postprocess(_lib.ptr(out), B, A, C, float(conf), float(iou), CLASS_OFFSET, _lib.ptr(det),
                                           _lib.ptr(n_keep), _lib.cur_stream(out.device)), "postprocess")
    torch.cuda.synchronize()
    return det, n_keep


DETECT = [("engine", ENGINE, 1, 2, None, None), ("engine", ENGINE, 8, 2, "nhwc", 5), ("one scale", ENGINE[:1], 3, 3, "nchw", 1),
          ("large", LARGE, 1, 2, "nchw", None), ("large", LARGE, 3, 3, None, 0), ("large", LARGE, 8, 1, "nhwc", 3)]


@pytest.mark.parametrize("name,geoms,B,C,cnn,empty", DETECT,
                         ids=[f"{c[0]}-B{c[2]}-C{c[3]}-{c[4] or 'events'}-empty{c[5]}" for c in DETECT])
def test_heads_finish_detect(name, geoms, B, C, cnn, empty):
    """The in-launch post-processing (A = 175: rank sort + masks; A = 600: bitonic network + barrier loop).

    * ``out`` is dagr_heads_finish's, bit for bit; ``det[:n_keep]`` / ``n_keep`` are dagr_postprocess's on that ``out``, bit
      for bit, and the oracle's on that ``out`` under test_postprocess_paths_gpu's rules (equal n_keep / anchors / labels,
      bit-equal score and box);
    * against the oracle on the NUMPY ``out`` (whose w, h and sigmoids differ from the device's by a few ulp): the same
      anchors with the same labels survive.  That needs room in the case itself, checked on the numpy side alone: no
      candidate pair within 1e-5 of the IoU threshold and no anchor within 1e-5 of the confidence threshold (4 ulp on
      the inputs move an IoU or a score by less than 2e-6 relative)."""
    CH = 5 + C
    conf, iou = 0.05, 0.5
    scales = _make(geoms, B, C, cnn, 0, empty, seed=B * 10 + C + 1)
    _, _, out32, out64, _ = _reference(scales, B, CH)
    d = _Device(scales, B, CH)
    out_plain, _ = d.finish()
    out, det, n_keep, st = d.finish_detect(conf, iou)
    assert st == 0
    assert torch.equal(nc.bits(out), nc.bits(out_plain))
    det2, n_keep2 = _postprocess(out, C, conf, iou)
    assert torch.equal(n_keep, n_keep2)
    out_c, det_c = out.cpu(), det.cpu()
    want_np = out64.astype(F32)
    want_np[..., :2] = out32[..., :2]
    want_np = torch.from_numpy(want_np)
    for b in range(B):
        n = int(n_keep[b])
        assert torch.equal(nc.bits(det[b, :n]), nc.bits(det2[b, :n])), f"image {b}: in-launch rows differ from dagr_postprocess"
        assert nc.min_iou_margin(nc.offset_boxes(*_cand(out_c[b], C, conf)).numpy(), iou) >= nc.MARGIN, "case too close"
        nc.check_rows(det_c[b], n, out_c[b], C, f"{name}, image {b}", conf, iou, class_offset=CLASS_OFFSET)
        # the numpy side
        boxes, score, label, masked = nc.rows_of(want_np[b], C)
        assert float((masked - conf).abs().min()) >= 1e-5, "case too close to the confidence threshold"
        assert nc.min_iou_margin(nc.offset_boxes(*_cand(want_np[b], C, conf)).numpy(), iou) >= 1e-5, "case too close"
        want_anchors = nc.expected_anchors(want_np[b], C, conf, iou, CLASS_OFFSET)
        dev_anchors = nc.expected_anchors(out_c[b], C, conf, iou, CLASS_OFFSET)      # (== the device rows, just checked)
        assert sorted(dev_anchors.tolist()) == sorted(want_anchors.tolist()), f"{name}, image {b}: survivors differ from numpy's"
        _, _, label_dev, _ = nc.rows_of(out_c[b], C)
        assert torch.equal(label_dev, label)
        assert 0 < n <= d.A
    if empty is not None and cnn is None:
        # an image without a node and without CNN logits: all logits 0, boxes of one stride at the grid -- disjoint, all kept
        assert int(n_keep[empty]) == d.A
    assert int(n_keep.min()) < d.A, "no suppression happened in any image"


def _cand(pred, C, conf):
    boxes, _, label, masked = nc.rows_of(pred, C)
    cand = masked >= conf
    return boxes[cand], label[cand], CLASS_OFFSET
