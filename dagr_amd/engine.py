"""WindowEngine -- sequences the HIP kernels of libdagr_hip for one batch of event windows.

Mirrors the control flow of ``Net.forward`` (src/dagr/model/networks/net.py:108-190) and the eval
branch of ``GNNHead.forward`` (src/dagr/model/networks/dagr.py:192-236,283-312), but every graph
level lives in pre-sized device buffers with device-side node/edge counts, so a window runs without
host synchronisation: graph build -> fused level-0 convs -> voxel pooling -> (tap aggregation +
GEMM) per pooled conv -> dense head maps.  PyTorch supplies memory and the stream only.
"""
import contextlib
import ctypes
import gc
import types

import numpy as np
import torch

from . import _lib
from .graph.ev_graph import WindowGraphBuilder

# convs whose rows are wider than the fused kernel's LDS tile run it in passes over the edges on levels of at most this
# many node slots (it pays on small levels only); larger levels take tap aggregation + GEMM as two launches
FUSED_PASSES_MAX_NODES = 1600

# level-0 widths the engine's kernels exist for: Net's int(base_width * 32) (csrc/conv_l0_tiles.hip)
L0_WIDTHS = (8, 16, 32)


def _l0_block(c):
    """Split a level-0 row of ``c`` channels into the tiled kernel's (main block, extras): the block is 0, 8, 16 or 32."""
    cm = max(b for b in (0,) + L0_WIDTHS if b <= c)
    return cm, c - cm


def _f32(v):
    """Value of ``v`` (python float or 0-dim tensor) as the fp32 torch would compute with."""
    return float(torch.as_tensor(v, dtype=torch.float32))


def _same_domain(a, b):
    return (a["rx"], a["ry"], a["den_x"], a["den_y"]) == (b["rx"], b["ry"], b["den_x"], b["den_y"]) \
        and torch.equal(a["remap"], b["remap"])


def _bn_affine(bn):
    m = bn.module
    scale = (m.weight / torch.sqrt(m.running_var + m.eps)).detach().float()
    shift = (m.bias - m.running_mean * scale).detach().float()
    return scale, shift



@contextlib.contextmanager
def _capture(graph):
    """``torch.cuda.graph`` with Python's cyclic collector paused for the length of the capture.  Entering the context
    collects everything that is garbage already; a collection that starts in the middle of the capture would run
    finalizers (of objects a previous engine left in a cycle, of temporaries of the body) that may call into the HIP runtime
    while the stream is capturing -- one ad-hoc ordering of the GPU test files aborted inside a captured tail that way."""
    was_enabled = gc.isenabled()
    with torch.cuda.graph(graph):
        gc.disable()
        try:
            yield
        finally:
            if was_enabled:
                gc.enable()

class _ConvPack:
    """Packed weights of one fused contraction: Wm[K, N], bias[N] (BN folded), plus shape info."""

    def __init__(self, cin, cskip, Wm, bias, relu):
        self.K, self.N = Wm.shape
        self.ldw = (self.N + 7) // 8 * 8      # zero-padded columns: rows stay 32-byte aligned for the MFMA GEMM
        if self.ldw != self.N:
            Wm = torch.cat([Wm, torch.zeros((self.K, self.ldw - self.N), dtype=Wm.dtype, device=Wm.device)], 1)
        self.cin, self.cskip, self.Wm, self.bias, self.relu = cin, cskip, Wm.contiguous(), bias.contiguous(), relu
        # MFMA operand order for dagr_spline_conv_fused: Wq[c][g][l][j] = W[16g + 4j + (l>>4)][16c + (l&15)]
        K16, N16 = (self.K + 15) // 16 * 16, (self.N + 15) // 16 * 16
        Wp = torch.zeros((K16, N16), dtype=Wm.dtype, device=Wm.device)
        Wp[: self.K, : self.N] = Wm[:, : self.N]
        # [g, j, kk, c, nn] -> [c, g, kk, nn, j]  (lane l = 16 kk + nn)
        self.Wq = Wp.view(K16 // 16, 4, 4, N16 // 16, 16).permute(3, 0, 2, 4, 1).contiguous()


def _pack_generic(convs, norms, skip=None, relu=True, device="cuda"):
    """Columns of several convs that read the same input are concatenated (N = sum of couts).
    rows: [25*cin taps (kx + 5*ky major, then input channel) | cin root | cskip skip]."""
    cols, biases = [], []
    cin = convs[0].in_channels
    for conv, norm in zip(convs, norms):
        W = conv.weight.detach().float()            # [25, cin, cout]
        root = conv.lin.weight.detach().float()     # [cout, cin]
        cout = W.shape[2]
        if norm is not None:
            scale, shift = _bn_affine(norm)
        else:
            scale, shift = torch.ones(cout, device=W.device), torch.zeros(cout, device=W.device)
        if conv.bias is not None:
            shift = shift + conv.bias.detach().float() * scale
        block = torch.cat([W.reshape(25 * cin, cout), root.t()], 0) * scale.view(1, -1)
        if skip is not None:
            lin, norm_skip = skip
            s_scale, s_shift = _bn_affine(norm_skip)
            block = torch.cat([block, lin.mlp.weight.detach().float().t() * s_scale.view(1, -1)], 0)
            shift = shift + s_shift
        cols.append(block)
        biases.append(shift)
    cskip = skip[0].mlp.in_features if skip is not None else 0
    return _ConvPack(cin, cskip, torch.cat(cols, 1).to(device), torch.cat(biases).to(device), relu)


def _pack_l0(conv, norm, win, skip=None, device="cuda", cols_in=None, cols_skip=None):
    """Level-0 packing: rows [(a + tx*b)*cin + i | root | skip] x cout over the tx x ty tap window.
    ``cols_in`` / ``cols_skip``: reference channel behind every column of the input / skip-input rows as the engine
    lays them out (identity when None)."""
    win_x, tx, win_y, ty = win
    W = conv.weight.detach().float()
    cin, cout = W.shape[1], W.shape[2]
    if cout not in L0_WIDTHS:
        raise NotImplementedError(f"the level-0 kernels exist for {', '.join(map(str, L0_WIDTHS))} output channels "
                                  f"(base_width = 0.25, 0.5, 1.0), not {cout}")
    cols_in = list(range(cin)) if cols_in is None else list(cols_in)
    scale, shift = _bn_affine(norm)
    rows = []
    for b in range(ty):
        for a in range(tx):
            rows.append(W[(win_x + a) + 5 * (win_y + b)][cols_in] * scale.view(1, -1))
    rows.append(conv.lin.weight.detach().float().t()[cols_in] * scale.view(1, -1))
    cskip = 0
    if skip is not None:
        lin, norm_skip = skip
        s_scale, s_shift = _bn_affine(norm_skip)
        ws = lin.mlp.weight.detach().float().t()
        if cols_skip is not None:
            ws = ws[list(cols_skip)]
        rows.append(ws * s_scale.view(1, -1))
        shift = shift + s_shift
        cskip = lin.mlp.in_features
    return cin, cskip, torch.cat(rows, 0).contiguous().to(device), shift.contiguous().to(device)


class _Conv1x1Gemm(torch.nn.Module):
    """A folded 1x1 Conv2d of the channels-last image branch as one GEMM ([B*H*W, Cin] x [Cin, Cout] + bias):
    hipBLASLt's fp32 GEMM is ~25 % faster than MIOpen's implicit-GEMM kernels on these shapes
    (tools/conv1x1_bench.py).  Output stays channels-last (a permuted view of the NHWC result)."""

    def __init__(self, conv, relu=False):
        super().__init__()
        cout, cin = conv.weight.shape[:2]
        self.stride = conv.stride[0]
        self.relu = relu       # ReLU in the GEMM epilogue (hipBLASLt) instead of a separate pass
        self.register_buffer("wt", conv.weight.detach().reshape(cout, cin).t().contiguous())
        self.register_buffer("b", conv.bias.detach().clone() if conv.bias is not None else torch.zeros(cout, device=conv.weight.device))
        self.planes = None     # the weights as three bf16 planes (_split_pack), where _split_min_rows selects the layer
        self.path = None       # "split" / "library": what the last forward ran

    def forward(self, x, residual=None):
        """``residual`` (a channels-last map of the output's shape): relu(conv(x) + bias + residual) in ONE library GEMM
        (dagr_gemm_epilogue: hipBLASLt with beta = 1 on the residual, bias and ReLU in the epilogue) -- the join of a
        bottleneck (net_img.py:47-48) without a pass of its own."""
        N = self.wt.shape[1]
        r = None if residual is None else residual.permute(0, 2, 3, 1)
        if self.planes is not None:
            y = _split_conv(x, self.planes, 1, self.stride, N, self.b, r, self.relu or r is not None)
            if y is not None:
                self.path = "split"
                return y
        self.path = "library"
        if self.stride != 1:
            x = x[:, :, ::self.stride, ::self.stride]
        B, C, H, W = x.shape
        a = x.permute(0, 2, 3, 1).reshape(-1, C)
        if _LT["ok"] and a.is_cuda and a.dtype == torch.float32 and a.stride(1) == 1 \
                and (r is None or (r.is_contiguous() and tuple(r.shape) == (B, H, W, N))):
            # every 1x1 conv of the branch through the same entry: bias (+ residual) (+ ReLU) in the GEMM's epilogue, the
            # library kernel picked by timing its candidates on this shape once (dagr_gemm_epilogue)
            y = torch.empty((a.shape[0], N), dtype=torch.float32, device=a.device)
            ws = _lt_workspace(a.device)
            act = 1 if (self.relu or r is not None) else 0
            rc = _lib.lib().dagr_gemm_epilogue(_lib.ptr(a), a.shape[0], C, a.stride(0), _lib.ptr(self.wt), N,
                                               _lib.ptr(self.b), _lib.ptr(r), N, act, _lib.ptr(y), N, _lib.ptr(ws),
                                               ws.numel(), _lib.cur_stream(a.device))
            if rc == 0:
                return y.view(B, H, W, -1).permute(0, 3, 1, 2)
            _LT["ok"] = False      # the library has no kernel for this epilogue here: torch's GEMM (+ a join pass) from now on
        if residual is not None:
            y = torch.addmm(self.b, a, self.wt).view(B, H, W, -1).permute(0, 3, 1, 2)
            return _add_relu_(y, residual)
        y = torch._addmm_activation(self.b, a, self.wt) if self.relu else torch.addmm(self.b, a, self.wt)
        return y.view(B, H, W, -1).permute(0, 3, 1, 2)


_LT = {"ok": True, "ws": {}}


def _lt_workspace(device):
    """Scratch for the library GEMMs of ``dagr_gemm_epilogue`` (allocated once per device, before any capture)."""
    key = str(device)
    if key not in _LT["ws"]:
        _LT["ws"][key] = torch.empty(int(_lib.lib().dagr_gemm_epilogue_workspace_bytes()), dtype=torch.uint8, device=device)
    return _LT["ws"][key]


def _split_min_rows(K, N, taps):
    """The selection rule of the split-bf16 MFMA kernel (csrc/gemm_split_bf16.hip): the fewest output rows M = B * Ho * Wo
    from which a convolution with K input channels (per tap), N output channels and ``taps`` in (1, 9) runs on it instead
    of the library, or None where the library keeps the layer at every size.  Written line for line from the measured table
    profiles/split_bf16_shapes.md (B = 8 at 640 x 480, and the B = 2, 320 x 215 rows): a class is in only where the kernel
    beat the library by more than the run-to-run spread of the medians.  No timing at run time: the same shapes take the
    same path in every run.  Where a class was measured at ONE row count only, the bound below is that row count: a
    "measured size only" bound, NOT a crossover -- nothing is known about the class below it.
      1x1, K 128..256, N >= 128: won at every M measured, 560 to 153 600 (14 - 65 % faster).
      1x1, K 257..512, N >= 256: won at every M measured, 2 400 to 38 400 (12 - 15 %).  N = 128: won at 38 400 (38.8 against
        43.6 us), measured size only.
      1x1, K = 1024, N = 512 (layer4.0.conv1): won at 9 600 (68.2 against 78.4 us), measured size only.  K = 1024, N = 2048
        (layer4.0.downsample, read in place with stride 2): re-measured in profiles/split_bf16_loop.md, 71.3 - 71.8 against
        88.0 - 88.9 us in two tables (spreads up to 2.6), admitted at 2 400 rows, measured size only.  K = 1024, N = 256
        (layer3.1-5.conv1): too near the library until the kernel's addressing left the K loop; re-measured in
        profiles/split_bf16_addressing.md, 39.1 - 39.6 against 42.6 - 42.7 us in two tables (spreads up to 0.6), admitted at
        9 600 rows, measured size only.  2 400 x 2048 x 512 still loses (47.4 - 47.8 against 41.9 - 42.6 us).
      1x1 of layer1 (64 -> 64, 256 -> 64, 64 -> 256): won at 153 600 (12 - 27 %), measured size only.
      1x1 with K < 64 or N < 64 (the narrow dconvs): not measured, not selected.
      3x3 stride 1: C = 128 won at M = 38 400 (30 %); the bound stays at 32 768, where the image branch's own tests hold
        it (at 2 160 the 32 x 64 tile now wins too, 21.8 against 28.0 us; not admitted).  C = 64 won at 153 600 (35 %) and
        C = 256 at 9 600 (23 %), both measured size only.  C = 512 ties at 2 400 (112.0 - 112.9 against 114.0 us, spreads of 4)
        with the tile the kernel picks; the eight-wave tile, which it does not pick for a 3x3, ran in 107.8 - 108.4."""
    if taps == 1:
        if K < 64 or N < 64:
            return None
        if K < 128 or N < 128:
            return 153600 if (K, N) in ((64, 64), (256, 64), (64, 256)) else None
        if K <= 256:
            return 512
        if K <= 512:
            return 2400 if N >= 256 else 38400
        return {(1024, 256): 9600, (1024, 512): 9600, (1024, 2048): 2400}.get((K, N))
    if taps == 9 and K == N:
        return {64: 153600, 128: 32768, 256: 9600}.get(K)
    return None


def _split_pack(wt):
    """Wt[K, N] (fp32, dense, on the device) as the kernel's three bf16 planes; once per layer, at folding time."""
    L = _lib.lib()
    K, N = wt.shape
    nbytes = int(L.dagr_gemm_split_bf16_packed_bytes(K, N))
    if nbytes == 0 or not wt.is_cuda:
        return None
    out = torch.empty(nbytes, dtype=torch.uint8, device=wt.device)
    _lib.check(L.dagr_gemm_split_bf16_pack(_lib.ptr(wt), K, N, _lib.ptr(out), nbytes, _lib.cur_stream(wt.device)),
               "gemm_split_bf16_pack")
    return out


def _split_conv(x, planes, taps, stride, N, bias, r, relu):
    """act(conv(x) + bias (+ r)) of a channels-last map on the split-bf16 kernel: a 1x1 with ``stride`` (read in place) or
    a 3x3 / stride 1 / pad 1.  ``r``: the residual as an NHWC tensor.  Returns the channels-last result, or None where the
    rule or the layout leaves the layer to the library; a failing launch raises."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = B * Ho * Wo
    rows = _split_min_rows(C, N, taps)
    xn = x.permute(0, 2, 3, 1)
    if rows is None or M < rows or not (x.is_cuda and x.dtype == torch.float32 and xn.is_contiguous()) \
            or (r is not None and not (r.is_contiguous() and tuple(r.shape) == (B, Ho, Wo, N))):
        return None
    # the kernel addresses the map through one buffer descriptor with 32-bit offsets and refuses a view of 2^31 bytes or
    # more (a 3x3's starts W + 1 pixels in front of the map); such a map stays with the library
    if ((B * H * W - 1 + (W + 1 if taps == 9 else 0)) * C + C) * 4 >= 1 << 31:
        return None
    y = torch.empty((B, Ho, Wo, N), dtype=torch.float32, device=x.device)
    L, st = _lib.lib(), _lib.cur_stream(x.device)
    if taps == 1:
        rc = L.dagr_gemm_split_bf16(_lib.ptr(xn), M, C, C, _lib.ptr(planes), N, _lib.ptr(bias), _lib.ptr(r), N, int(relu),
                                    _lib.ptr(y), N, B, H, W, stride, 0, st)
    else:
        rc = L.dagr_conv3x3_split_bf16(_lib.ptr(xn), B, H, W, C, C, _lib.ptr(planes), N, _lib.ptr(bias), _lib.ptr(r), N,
                                       int(relu), _lib.ptr(y), N, 0, st)
    _lib.check(rc, "gemm_split_bf16")
    return y.permute(0, 3, 1, 2)


def _gemmify_1x1(module):
    for name, child in list(module.named_children()):
        if isinstance(child, torch.nn.Conv2d) and child.kernel_size == (1, 1) and child.groups == 1 \
                and child.padding == (0, 0) and child.stride[0] == child.stride[1]:
            setattr(module, name, _Conv1x1Gemm(child))
        else:
            _gemmify_1x1(child)


def _add_relu_(y, z):
    """y = relu(y + z) in place, one pass (dagr_add_relu) when both maps share one dense layout."""
    if y.is_cuda and y.dtype == torch.float32 and z.dtype == torch.float32 and y.shape == z.shape \
            and y.stride() == z.stride() and y.data_ptr() % 16 == 0 and z.data_ptr() % 16 == 0 \
            and (y.is_contiguous() or y.is_contiguous(memory_format=torch.channels_last)):
        _lib.check(_lib.lib().dagr_add_relu(_lib.ptr(y), _lib.ptr(z), y.numel(), _lib.cur_stream(y.device)), "add_relu")
        return y
    return torch.relu_(y.add_(z))


def _bias_relu_(y, bias):
    """y = relu(y + bias[c]) in place, one pass (dagr_bias_relu) on a channels-last map."""
    C = y.shape[1]
    if y.is_cuda and y.dtype == torch.float32 and C % 4 == 0 and y.is_contiguous(memory_format=torch.channels_last) \
            and y.data_ptr() % 16 == 0 and bias.data_ptr() % 16 == 0:
        _lib.check(_lib.lib().dagr_bias_relu(_lib.ptr(y), _lib.ptr(bias), y.numel(), C, _lib.cur_stream(y.device)),
                   "bias_relu")
        return y
    return torch.relu_(y.add_(bias.view(1, -1, 1, 1)))


def _baseconv_forward(m, x):
    """yolox BaseConv.forward of the inference copy: bias-free conv, then folded-BN bias + SiLU in one pass."""
    y = m.conv(x)
    b = m._bias
    C = y.shape[1]
    if y.is_cuda and y.dtype == torch.float32 and C % 4 == 0 and y.is_contiguous(memory_format=torch.channels_last) \
            and y.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0:
        _lib.check(_lib.lib().dagr_bias_silu(_lib.ptr(y), _lib.ptr(b), y.numel(), C, _lib.cur_stream(y.device)),
                   "bias_silu")
        return y
    return torch.nn.functional.silu(y.add_(b.view(1, -1, 1, 1)), inplace=True)


def _conv_bias_relu(blk, name, x):
    """relu(conv(x) + bias): spatial convs of the inference copy run bias-free (MIOpen would add the bias in a pass of
    its own) and get bias + ReLU in one pass; the 1x1 GEMMs keep their epilogue.  (MIOpen's own conv + bias + ReLU fusion
    plan, aten::miopen_convolution_relu, was measured in round 5: it falls to a naive kernel on these fp32 NHWC shapes --
    260 ms per B = 8 forward instead of 4.7; profiles/r5_conv_phases.md.)"""
    conv = getattr(blk, name)
    b = getattr(blk, "_" + name + "_bias", None)
    planes = getattr(conv, "_split_planes", None)
    if planes is not None:          # a stride-1 3x3 the rule selects: bias + ReLU in the kernel's epilogue
        out = _split_conv(x, planes, 9, 1, conv.out_channels, b, None, True)
        if out is not None:
            conv._split_path = "split"
            return out
    if isinstance(conv, torch.nn.Conv2d):
        conv._split_path = "library"
    out = conv(x)
    if b is not None:
        return _bias_relu_(out, b)
    if getattr(conv, "relu", False):
        return out
    return blk.relu(out)


def _bottleneck_forward(blk, x):
    """Bottleneck.forward (net_img.py:43-48) of the folded inference copy: conv1's ReLU rides in its GEMM
    epilogue, the residual join is one pass."""
    identity = x if blk.downsample is None else blk.downsample(x)
    out = _conv_bias_relu(blk, "conv1", x)
    out = _conv_bias_relu(blk, "conv2", out)
    if isinstance(blk.conv3, _Conv1x1Gemm):
        return blk.conv3(out, residual=identity)      # relu(conv3 + bias + identity): one GEMM
    return _add_relu_(blk.conv3(out), identity)


def _resnet_features_forward(net, x, emit=None):
    """ResNet.forward_features (net_img.py:80-88) of the inference copy: bn1 -> relu -> maxpool after the raw conv1
    output (which the reference taps) in one pass over the largest activation map of the network.  ``emit(name, map)`` is
    called as soon as a stage's output exists (the engine's pipelined window starts a graph level when ITS map is ready)."""
    emit = emit or (lambda name, t: None)
    c1 = net.conv1(x)
    emit("conv1", c1)
    mp = net.maxpool
    ok = (c1.is_cuda and c1.dtype == torch.float32 and c1.is_contiguous(memory_format=torch.channels_last)
          and c1.shape[1] % 4 == 0 and mp.kernel_size == 3 and mp.stride == 2 and mp.padding == 1
          and mp.dilation == 1 and not mp.ceil_mode)
    if ok:
        B, C, H, W = c1.shape
        scale, shift = net._stem_affine
        y = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=c1.dtype, device=c1.device,
                        memory_format=torch.channels_last)
        _lib.check(_lib.lib().dagr_bn_relu_maxpool(_lib.ptr(c1), B, H, W, C, _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y),
                                                   _lib.cur_stream(c1.device)), "bn_relu_maxpool")
    else:
        y = net.maxpool(net.relu(net.bn1(c1)))
    l1 = net.layer1(y)
    emit("layer1", l1)
    l2 = net.layer2(l1)
    emit("layer2", l2)
    l3 = net.layer3(l2)
    emit("layer3", l3)
    l4 = net.layer4(l3)
    emit("layer4", l4)
    return dict(conv1=c1, layer1=l1, layer2=l2, layer3=l3, layer4=l4)


def _basicblock_forward(blk, x):
    identity = x if blk.downsample is None else blk.downsample(x)
    out = _conv_bias_relu(blk, "conv1", x)
    return _add_relu_(blk.conv2(out), identity)


def flicker_map_bytes(B, sensor_w, sensor_h):
    """The bytes at the front of a ``dagr_stream_flicker`` state that hold its per-pixel maps (include/dagr_hip.h): t_edge
    and t_pass, int64, each rounded up to 256 bytes, then the packed int32 words."""
    pixels = B * sensor_w * sensor_h
    return 2 * (-(-8 * pixels // 256) * 256) + 4 * pixels


def flicker_maps_from_state(state, B, sensor_w, sensor_h):
    """The per-pixel maps of a ``dagr_stream_flicker`` state (a uint8 device tensor) unpacked into the named arrays of
    ``dagr.streaming.flicker_definition``, each ``[B, sensor_h, sensor_w]`` (copies; synchronises)."""
    pixels, shape = B * sensor_w * sensor_h, (B, sensor_h, sensor_w)
    stride = -(-8 * pixels // 256) * 256
    t_edge = state[:8 * pixels].view(torch.int64).cpu().numpy().reshape(shape)
    t_pass = state[stride:stride + 8 * pixels].view(torch.int64).cpu().numpy().reshape(shape)
    word = state[2 * stride:2 * stride + 4 * pixels].view(torch.int32).cpu().numpy().reshape(shape)
    polarity = np.array([0, 1, -1, 0], np.int8)         # a polarity field: 0 none yet, 1 +1, 2 -1
    return dict(t_edge=t_edge, last_p=polarity[(word >> 9) & 3], count=(word & 0xff).astype(np.int32),
                blocking=((word >> 8) & 1).astype(bool), t_pass=t_pass, p_pass=polarity[(word >> 11) & 3])


def _state_buffer(device, entry, *sizes):
    """An uninitialised device buffer of the bytes ``entry(*sizes)`` asks for (a ``dagr_*_bytes`` entry, by name); sizes it
    refuses (0) are raised under its name."""
    nbytes = getattr(_lib.lib(), entry)(*sizes)
    if nbytes == 0:
        raise RuntimeError(f"{entry}({', '.join(str(v) for v in sizes)}): out of range")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


class _PushStage:
    """One stage a stream's pushes pass through: the entry ``dagr_<entry>`` on a state of the family ``dagr_<family>``
    (``_bytes``, ``_reset``), which holds the stage's maps in its first ``carried`` bytes and behind them the scratch of a
    largest push.  Owns the state, the push size ``cap`` it is sized for, the five output tensors ``out`` (xy, t, p, batch,
    count) and the device-side ``counters`` the entry adds to.  ``geometry`` is what ``_bytes`` / ``_reset`` take between
    ``B`` and the push size, ``rule`` what the entry takes between the push size and the push; ``out_rows(cap)`` the rows of
    the outputs (default: ``cap``)."""

    def __init__(self, B, device, status, family, entry, geometry, carried, rule, counters=(), out_rows=None):
        self.B, self.device, self.status = B, device, status
        self.family, self.entry, self.geometry, self.carried = family, entry, tuple(geometry), int(carried)
        self.rule, self.counters, self.out_rows = tuple(rule), list(counters), out_rows or (lambda cap: cap)
        self.state, self.cap, self.out = None, 0, None

    def grow(self, n):
        """State and outputs for pushes of ``n`` rows; the maps are carried over."""
        if n <= self.cap:
            return
        new = _state_buffer(self.device, f"dagr_{self.family}_bytes", self.B, *self.geometry, n)
        old, self.state, self.cap = self.state, new, n
        self.reset(counters=False)
        if old is not None:
            new[:self.carried].copy_(old[:self.carried])
        rows, dev = self.out_rows(n), self.device
        if self.out is None or rows != int(self.out[1].shape[0]):
            self.out = (torch.empty((rows, 2), dtype=torch.int16, device=dev), torch.empty((rows,), dtype=torch.int64, device=dev),
                        torch.empty((rows,), dtype=torch.int8, device=dev), torch.empty((rows,), dtype=torch.int32, device=dev),
                        torch.zeros((1,), dtype=torch.int32, device=dev))

    def reset(self, counters=True):
        """The maps as new; with ``counters``, nothing counted."""
        reset = getattr(_lib.lib(), f"dagr_{self.family}_reset")
        _lib.check(reset(_lib.ptr(self.state), self.state.numel(), self.B, *self.geometry, self.cap,
                         _lib.cur_stream(self.device)), self.family + "_reset")
        for c in self.counters if counters else ():
            c.zero_()

    def run(self, n, push):
        """The entry on a push of ``n`` rows (``push``: its arguments between the rule and the outputs); returns ``out``."""
        if n > self.cap:
            self.grow(max(n, 2 * self.cap))
        P = _lib.ptr
        _lib.check(getattr(_lib.lib(), "dagr_" + self.entry)(
            P(self.state), self.state.numel(), self.B, self.cap, *self.rule, *push, *(P(o) for o in self.out),
            *(P(c) for c in self.counters), P(self.status), _lib.cur_stream(self.device)), self.entry)
        return self.out

    def carried_bytes(self):
        return self.state[:self.carried]


class StreamState:
    """Device-side state of one event stream (``dagr_stream_stage``): the raw events of the running window in two sets
    written alternately, the lanes' bounds and reference instants, the stream's status word, the per-lane counts of the
    last step -- and what the host knows of the window's size, which is an upper bound until a count has been read.
    Owned by the stream (``dagr.streaming.EventStream``), handed to ``WindowEngine.forward_stream`` on every step: the
    engine keeps no pointer into it, so a buffer that grew leaves nothing stale; an engine rebuilt with a smaller
    capacity than the stream's is grown to it on the stream's next step.

    A stream of raw sensor events (``enable_front``) also owns the front's state (``dagr_stream_downsample``): the lanes'
    change maps and the scratch of a largest push, grown with the push size, and the survivors' buffers.  The host's bound
    is then "last count read + RAW events pushed since".

    A filtering stream (``enable_denoise``) owns the noise filter's state (``dagr_stream_denoise``): the lanes' int64 stamp
    maps and the scratch of a largest push, grown with the push size, the survivors' buffers, and ``lane_filtered``, which
    accumulates on the device what the filter removed.  Its bound counts the UNFILTERED events pushed.

    A stream with the anti-flicker / trail filters (``enable_flicker``) owns their state (``dagr_stream_flicker``): the
    lanes' per-pixel maps and the scratch of a largest push, grown with the push size, the survivors' buffers, and
    ``lane_suppressed`` int64 [2, B], what the flicker and the trail stage removed.  It runs in front of the noise filter.

    A decoding stream (``enable_decode``) owns the decoder's state (``dagr_stream_decode``): the lanes' decoder states and
    the scratch of a largest push of words, the decoded events' buffers, and ``lane_decoded``, the cumulative counters.  The
    host never learns how many events a push decoded: its bound grows by ``decode_rows(n_words)`` per push.

    A capped stream (``max_lane_events = N``, ``dagr_stream_stage_capped``) keeps the newest ``N`` events of every lane at
    most: no window exceeds ``B * N``, which bounds the host's bound too, and ``lane_dropped`` accumulates on the device
    what the count rule removed.

    A tracking stream (``enable_track``) owns the tracker's state (``dagr_stream_track``): the lanes' track slots,
    ``lane_untracked``, and the step's ``track_ids`` / ``track_hits``.  With a motion model (``enable_track(...,
    motion=)``) the state is ``dagr_stream_track_cv``'s, which also holds the velocities, and the stream owns the step's
    ``track_boxes`` / ``track_vel`` and the lanes' coast lists, allocated once.  With a second association round
    (``enable_track(..., rescue=)``) the step ends with the ``_rescue`` entry of either, on the same state, and the stream
    owns ``lane_rescued``.

    A scoring stream (``enable_score``, on a tracking stream) owns the scorer's state (``dagr_stream_score``): the lanes'
    object tables and counters, allocated next to the tracker's, and the ``gt_match`` / ``gt_flags`` of the last scored
    step.  A step launches nothing for it: ``run_score`` is the one launch, on the last step's device arrays.

    An identity stream (``enable_identity``, on a scoring stream) owns the identity state (``dagr_stream_identity``): the
    lanes' track tables and overlap counts, and the assignment's workspace.  ``run_score`` then makes a second launch behind
    the scorer's on the same arrays, still without a host wait; ``run_identity_solve`` is ``dagr_stream_identity_solve``.

    A HOTA stream (``enable_hota``, on an identity stream) owns HOTA's state (``dagr_stream_hota``): the alignment tables,
    the log of the labelled instants, the last solve's counts, and the solve's workspace.  ``run_score`` then makes a third
    launch behind the identity step's; ``run_hota_solve`` is ``dagr_stream_hota_solve``.

    A drawing stream (``enable_render``) owns the picture's state (``dagr_stream_render``): the per-pixel maps, the output
    frames, a status word of its own and -- with trails, on a tracking stream -- the rings of the slots' last centres
    (``dagr_stream_trail``).  A step with trails makes one more launch behind the tracker's (``run_trail``); ``run_render``
    is the picture, on the last step's device arrays, whenever it is asked for."""

    def __init__(self, batch_size, window_us, device, max_lane_events=None):
        self.B, self.window_us, self.device = int(batch_size), int(window_us), torch.device(device)
        self.max_lane_events = None if max_lane_events is None else int(max_lane_events)
        self.lane_dropped = torch.zeros((self.B,), dtype=torch.int64, device=self.device)
        self.cap = 0
        self.state = None
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.lane_count = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self.image = None                     # the frame in force, fp32 [B, 3, H, W] (--use_image)
        self.frame_new = True                 # a frame has arrived since the stream's last frame body
        self.frame_steps = self.held_steps = 0      # bodies run (forward_stream)
        # the counts come back with every step, into pinned memory; the host reads them only after a synchronisation it
        # makes anyway (the detections' read-back)
        self._host = torch.zeros((self.B,), dtype=torch.int32).pin_memory()
        self._known = np.zeros((self.B,), np.int64)     # the last counts read
        self._since = 0                                 # events pushed since
        self._fresh = True                              # _known belongs to the last step staged
        self.stages = {}                                # the enabled push stages (_PushStage), under their options' names:
        self.front = None                               # (fx, fy, W_in, H_in, W, H) of a downsampling stream
        self.noise, self.lane_filtered = None, None     # (W_in, H_in, denoise_us or 0, refractory_us or 0) of a filtering stream
        self.flick, self.lane_suppressed = None, None   # (W_in, H_in, min_period, max_period, start, stop, max_count, trail_us)
        self.words, self.lane_decoded = None, None      # (format, W_in, H_in, max_decoded or None) of a decoding stream
        self.track = None                               # the options of a tracking stream (dagr.streaming._track_options)
        self.track_state, self.lane_untracked, self.track_ids, self.track_hits = None, None, None, None
        self.motion = None                              # the options of its motion model (dagr.streaming._motion_options)
        self.track_boxes, self.track_vel, self.coast = None, None, None
        self.rescue, self.lane_rescued = None, None     # the options of its second round (dagr.streaming._rescue_options)
        self.assign, self.assign_ws = None, None        # "optimal": dagr_stream_track_optimal and its workspace
        self.score = None                               # the options of its scorer (dagr.streaming._score_options)
        self.score_state, self.gt_match, self.gt_flags = None, None, None
        self._last_det, self._scored = None, False      # the last step's (det, n_keep); whether run_score has had them
        self.identity = None                            # the options of its IDF1 state (dagr.streaming._identity_options)
        self.identity_state, self.identity_ws, self.obj_track, self.identity_result = None, None, None, None
        self.hota = None                                # the options of its HOTA state (dagr.streaming._hota_options)
        self.hota_state, self.hota_ws = None, None
        self._t_ref = None                              # (state pointer, capacity, where its t_ref[B] lives)
        self.labels = None                              # the options of its label store (dagr.streaming._label_options)
        self.labels_state, self.gt_labels = None, None  # the store; the last labelled step's (gt_box, gt_label, gt_id, n_gt)
        self._stepped, self._labelled = False, False    # a step since construction / reset(); whether run_labels has had it
        self.map, self.map_classes = None, None         # the options of its mAP log (dagr.streaming._map_options)
        self.map_state, self.map_plan, self._map_sizes = None, None, None
        self._map_det, self._mapped = None, False       # the last step's (det, n_keep); whether run_map_log has had them
        self.render = None                              # the options of its picture (dagr.streaming._render_options)
        self.render_size, self.render_colors, self.render_ws, self.render_flags, self.render_out = None, None, None, None, None
        self.trail_rings, self._render_det = None, None # the trail rings; the last step's (det, n_keep) for run_render

    def stepped(self):
        """``forward_stream`` has staged a step: ``run_labels`` may run at its ``t_ref``, once."""
        self._stepped, self._labelled = True, False

    def _t_ref_where(self):
        """Where the step's reference instants ``t_ref[B]`` live inside the stream state (``dagr_stream_t_ref``), looked
        up again only when the state has grown."""
        if self._t_ref is None or self._t_ref[:2] != (self.state.data_ptr(), self.cap):
            where = _lib.lib().dagr_stream_t_ref(_lib.ptr(self.state), self.B, self.cap)
            if not where:
                raise RuntimeError(f"dagr_stream_t_ref(B = {self.B}, capacity = {self.cap}): out of range")
            self._t_ref = (self.state.data_ptr(), self.cap, ctypes.c_void_p(where))
        return self._t_ref[2]

    # ------------------------------------------------------------------------------------ labels at every step
    def enable_labels(self, options):
        """The stream keeps labelled keyframes and ``run_labels`` interpolates them to a step's ``t_ref``
        (``dagr_stream_labels_push`` / ``dagr_stream_labels_at``): ``options`` as ``dagr.streaming._label_options`` returns
        them.  Allocates the lanes' rings, empty, and the step's ground-truth tensors."""
        self.labels = dict(options)
        K, R, dev = self.labels["max_keyframes"], self.labels["max_rows"], self.device
        self.labels_state = _state_buffer(dev, "dagr_stream_labels_bytes", self.B, K, R)
        self.gt_labels = (torch.zeros((self.B, R, 4), dtype=torch.float32, device=dev),
                          torch.zeros((self.B, R), dtype=torch.int32, device=dev),
                          torch.zeros((self.B, R), dtype=torch.int64, device=dev),
                          torch.full((self.B,), -1, dtype=torch.int32, device=dev))
        self._reset_labels()

    def _reset_labels(self):
        """No keyframe, zero counters; the last step has no labels any more."""
        _lib.check(_lib.lib().dagr_stream_labels_reset(_lib.ptr(self.labels_state), self.labels_state.numel(), self.B,
                                                       self.labels["max_keyframes"], self.labels["max_rows"],
                                                       _lib.cur_stream(self.device)), "stream_labels_reset")
        self._stepped, self._labelled = False, False

    def push_labels(self, t, n, xywh, label, id):
        """``dagr_stream_labels_push``: ``F`` keyframes a lane from contiguous device tensors ``t`` int64 [B, F], ``n`` int32
        [B, F], ``xywh`` fp64 [B, F, max_rows, 4], ``label`` int32 [B, F, max_rows], ``id`` int64 [B, F, max_rows]: one
        launch, no host wait."""
        if self.labels is None:
            raise RuntimeError("this stream keeps no labels (labels=): it has no push_labels")
        B, F, R = self.B, int(t.shape[1]), self.labels["max_rows"]
        for v, dtype, shape, name in ((t, torch.int64, (B, F), "t"), (n, torch.int32, (B, F), "n"),
                                      (xywh, torch.float64, (B, F, R, 4), "xywh"), (label, torch.int32, (B, F, R), "label"),
                                      (id, torch.int64, (B, F, R), "id")):
            if v.dtype != dtype or tuple(v.shape) != shape or not v.is_contiguous() or v.device != self.device:
                raise RuntimeError(f"push_labels: {name} must be a contiguous {dtype} {list(shape)} on {self.device}")
        P = _lib.ptr
        _lib.check(_lib.lib().dagr_stream_labels_push(P(self.labels_state), self.labels_state.numel(), B,
                                                      self.labels["max_keyframes"], R, F, P(t), P(n), P(xywh), P(label), P(id),
                                                      _lib.cur_stream(self.device)), "stream_labels_push")

    def run_labels(self):
        """``dagr_stream_labels_at`` at the LAST step's ``t_ref``, at most once per step: ``(gt_box fp32 [B, max_rows, 4],
        gt_label int32 [B, max_rows], gt_id int64 [B, max_rows], n_gt int32 [B])``, valid until the next step.  One launch,
        no host wait."""
        if self.labels is None:
            raise RuntimeError("this stream keeps no labels (labels=): it has no labels_step")
        if not self._stepped:
            raise RuntimeError("labels_step: the stream has made no step since its construction / reset(): there is no "
                               "instant to interpolate to")
        if not self._labelled:
            P, o, nan = _lib.ptr, self.labels, float("nan")
            _lib.check(_lib.lib().dagr_stream_labels_at(
                P(self.labels_state), self.labels_state.numel(), self.B, o["max_keyframes"], o["max_rows"],
                self._t_ref_where(), o["max_gap_us"] or 0, nan if o["min_height"] is None else o["min_height"],
                nan if o["min_diag"] is None else o["min_diag"], *(P(v) for v in self.gt_labels),
                _lib.cur_stream(self.device)), "stream_labels_at")
            self._labelled = True
        return self.gt_labels

    def label_words(self):
        """The lanes' words read back: int64 [B, DAGR_LABELS_WORDS] -- keyframes, head, refused, cut_rows, overwritten,
        labelled, outside, gap --, the layout include/dagr_hip.h documents (a copy; synchronises)."""
        if self.labels is None:
            raise RuntimeError("this stream keeps no labels (labels=): it has no counters")
        W = _lib.DEFINES["DAGR_LABELS_WORDS"]
        return self.labels_state[:8 * W * self.B].view(torch.int64).cpu().numpy().reshape(self.B, W)

    # ------------------------------------------------------------------------------------ mAP over every step
    def enable_map(self, options, n_classes):
        """``run_map_log`` appends a step's detections and ground truth to the lanes' logs (``dagr_stream_map_log``) and
        ``run_map_plan`` builds the COCO job list from them (``dagr_stream_map_plan``): ``options`` as
        ``dagr.streaming._map_options`` returns them.  The log is allocated by the first ``run_map_log``, which knows the
        rows per lane ``A`` and the ground truth's ``G``, the plan's arrays by the first ``run_map_plan``; nothing is
        allocated after that.  Both are sized from the capacities: about ``64 * B * max_images * max_dets`` bytes together
        (the log keeps 24 bytes a detection row, the plan 40; its column arrays add 32 for each of the first 100 rows a
        class) -- with ``max_dets = None`` and an engine of 4096 rows a lane that is 2.6 GB at B = 8 and 1200 images."""
        self.map, self.map_classes = dict(options), int(n_classes)

    def map_sizes(self):
        """``(B, max_images, G, max_dets)`` of the allocated log, or None before the first ``run_map_log``."""
        return None if self.map_state is None else (self.B,) + self._map_sizes

    def _empty_map_log(self):
        """``dagr_stream_map_reset``: an empty log, zero counters."""
        _lib.check(_lib.lib().dagr_stream_map_reset(_lib.ptr(self.map_state), self.map_state.numel(), *self.map_sizes(),
                                                    _lib.cur_stream(self.device)), "stream_map_reset")

    def _reset_map(self):
        """An empty log, zero counters; the last step cannot be logged any more."""
        if self.map_state is not None:
            self._empty_map_log()
        self._map_det, self._mapped = None, False

    def run_map_log(self, gt_box, gt_label, n_gt):
        """``dagr_stream_map_log`` on the LAST step's ``det`` / ``n_keep`` at its ``t_ref`` against device tensors ``gt_box``
        fp32 [B, G, 4], ``gt_label`` int32 [B, G] and ``n_gt`` int32 [B]: one launch, no host wait, once per step."""
        if self.map is None:
            raise RuntimeError("this stream keeps no mAP log (map=): it has no map_step")
        if self._map_det is None:
            raise RuntimeError("map_step: the stream has made no step since its construction / reset(): there is nothing "
                               "to log")
        if self._mapped:
            raise RuntimeError("map_step: the last step has been logged already (one map_step per step)")
        det, n_keep = self._map_det
        A, G = int(det.shape[1]), int(gt_box.shape[1])
        if self.map_state is None:
            D = A if self.map["max_dets"] is None else self.map["max_dets"]
            self._map_sizes = (self.map["max_images"], G, D)
            self.map_state = _state_buffer(self.device, "dagr_stream_map_bytes", self.B, *self._map_sizes)
            self._empty_map_log()
        if G != self._map_sizes[1]:
            raise ValueError(f"map_step: gt_box has {G} rows a lane, the stream's log was sized for {self._map_sizes[1]} by its "
                             "first map_step")
        P = _lib.ptr
        _lib.check(_lib.lib().dagr_stream_map_log(P(self.map_state), self.map_state.numel(), *self.map_sizes(), P(det),
                                                  P(n_keep), A, P(gt_box), P(gt_label), P(n_gt), self._t_ref_where(),
                                                  _lib.cur_stream(self.device)), "stream_map_log")
        self._mapped = True

    def run_map_plan(self):
        """``dagr_stream_map_plan`` on the log so far (no host wait): the ``StreamMapPlan`` (utils/coco_eval.py) that holds
        the result, its arrays allocated by the first call; None while nothing has been logged."""
        if self.map is None:
            raise RuntimeError("this stream keeps no mAP log (map=): it has no map")
        if self.map_state is None:
            return None
        if self.map_plan is None:
            from .utils.coco_eval import StreamMapPlan
            self.map_plan = StreamMapPlan(*self.map_sizes(), self.map_classes, self.device)
        self.map_plan.run(self.map_state)
        return self.map_plan

    MAP_SECTIONS = (("t", np.int64, 8, ()), ("n_gt", np.int32, 4, ()), ("n_dt", np.int32, 4, ()),
                    ("gt_box", np.float32, 4, ("G", 4)), ("gt_label", np.int32, 4, ("G",)), ("det", np.float32, 4, ("D", 6)))

    def map_words(self, log=False):
        """The lanes' words read back: int64 [B, DAGR_MAP_WORDS] -- images, dropped_images, cut_dets, unlabelled, empty
        (zeros before the first ``run_map_log``); with ``log`` also the dict of the log's arrays in the layout
        include/dagr_hip.h documents (copies; synchronises)."""
        if self.map is None:
            raise RuntimeError("this stream keeps no mAP log (map=): it has no counters")
        W = _lib.DEFINES["DAGR_MAP_WORDS"]
        if self.map_state is None:
            return (np.zeros((self.B, W), np.int64), None) if log else np.zeros((self.B, W), np.int64)
        if not log:
            return self.map_state[:8 * W * self.B].view(torch.int64).cpu().numpy().reshape(self.B, W)
        host = self.map_state.cpu().numpy()
        B, I, G, D = self.map_sizes()
        at, out = -(-8 * W * B // 16) * 16, {}
        for name, dtype, size, tail in self.MAP_SECTIONS:
            shape = (B, I) + tuple(dict(G=G, D=D).get(v, v) for v in tail)
            nbytes = int(np.prod(shape)) * size
            out[name] = host[at:at + nbytes].view(dtype).reshape(shape).copy()
            at += -(-nbytes // 16) * 16
        return host[:8 * W * B].view(np.int64).reshape(B, W).copy(), out

    # ------------------------------------------------------------------------------------ track ids
    # the slots' arrays in the order the state holds them over [B, max_tracks]: (name, dtype, width); next_id[B] follows
    TRACK_FIELDS = (("id", torch.int64, 1), ("t_last", torch.int64, 1), ("box", torch.float32, 4), ("vel", torch.float32, 4),
                    ("label", torch.int32, 1), ("hits", torch.int32, 1))

    def enable_track(self, options, motion=None, rescue=None, assign=None):
        """Every step ends with ``dagr_stream_track``: ``options`` as ``dagr.streaming._track_options`` returns them.
        Allocates the lanes' slots, empty, and ``lane_untracked``.  With ``motion`` (as ``_motion_options`` returns it)
        the step ends with ``dagr_stream_track_cv`` instead, on a state of that layout, and the coast lists are allocated.
        With ``rescue`` (as ``_rescue_options`` returns it) the step ends with the ``_rescue`` entry of the one or the
        other, on the same state -- ``_bytes`` and ``_reset`` are the family's --, and ``lane_rescued`` is allocated.
        With ``assign`` (as ``_assign_options`` returns it: ``"optimal"``) the step ends with ``dagr_stream_track_optimal``
        instead of any of the four, on the same state again, and its workspace is allocated."""
        self.track, self.motion = dict(options), None if motion is None else dict(motion)
        self.rescue = None if rescue is None else dict(rescue)
        self.assign = assign
        # the family of entry points dagr_<family>, dagr_<family>_bytes, dagr_<family>_reset, chosen here once -- as a
        # name: every call looks its function up on the library
        self._track_family = "stream_track" if motion is None else "stream_track_cv"
        M, dev = self.track["max_tracks"], self.device
        self.track_state = _state_buffer(dev, f"dagr_{self._track_family}_bytes", self.B, M)
        self.lane_untracked = torch.zeros((self.B,), dtype=torch.int64, device=dev)
        if rescue is not None:
            self.lane_rescued = torch.zeros((self.B,), dtype=torch.int64, device=dev)
        if assign is not None:
            self.assign_ws = _state_buffer(dev, "dagr_stream_track_optimal_bytes", self.B, M)
        if motion is not None:
            self.coast = (torch.zeros((self.B,), dtype=torch.int32, device=dev),            # n_coast
                          torch.zeros((self.B, M), dtype=torch.int64, device=dev),          # coast_id
                          torch.zeros((self.B, M, 4), dtype=torch.float32, device=dev),     # coast_box
                          torch.zeros((self.B, M), dtype=torch.int32, device=dev),          # coast_label
                          torch.zeros((self.B, M), dtype=torch.int64, device=dev))          # coast_age_us
        self._reset_track()

    def _track_fn(self, suffix=""):
        return getattr(_lib.lib(), "dagr_" + self._track_family + suffix)

    def _reset_track(self):
        """Every slot free, ``next_id = 1``, nothing untracked, nothing coasting."""
        _lib.check(self._track_fn("_reset")(_lib.ptr(self.track_state), self.track_state.numel(), self.B, self.track["max_tracks"],
                                            _lib.cur_stream(self.device)), self._track_family + "_reset")
        self.lane_untracked.zero_()
        if self.rescue is not None:
            self.lane_rescued.zero_()
        if self.motion is not None:
            self.coast[0].zero_()

    def run_track(self, det, n_keep):
        """``dagr_stream_track`` on a step's detections, at the reference instants the step's staging left in the stream
        state: ``track_ids`` int64 [B, A] and ``track_hits`` int32 [B, A], valid until the next step.  With a motion model
        ``dagr_stream_track_cv`` instead, never both: it also leaves ``track_boxes`` / ``track_vel`` and the coast lists.
        With a second round the one launch is the ``_rescue`` entry of either, which also adds to ``lane_rescued``.  With
        ``assign`` the one launch is ``dagr_stream_track_optimal``, whose flags say which of the four it stands for."""
        B, A = int(det.shape[0]), int(det.shape[1])
        if B != self.B or det.dtype != torch.float32 or not det.is_contiguous() or n_keep.dtype != torch.int32:
            raise RuntimeError(f"run_track: det must be contiguous fp32 [{self.B}, A, 6] and n_keep int32 [{self.B}]")
        if self.track_ids is None or tuple(self.track_ids.shape) != (B, A):
            self.track_ids = torch.zeros((B, A), dtype=torch.int64, device=self.device)
            self.track_hits = torch.zeros((B, A), dtype=torch.int32, device=self.device)
            if self.motion is not None:
                self.track_boxes = torch.zeros((B, A, 4), dtype=torch.float32, device=self.device)
                self.track_vel = torch.zeros((B, A, 4), dtype=torch.float32, device=self.device)
        P, o = _lib.ptr, self.track
        self._t_ref_where()
        gains, outputs = [], []             # what dagr_stream_track_cv takes in addition, in their places
        if self.motion is not None:
            n_coast, c_id, c_box, c_label, c_age = self.coast
            gains = [self.motion["alpha"], self.motion["beta"]]
            outputs = [P(self.track_boxes), P(self.track_vel), P(c_id), P(c_box), P(c_label), P(c_age), P(n_coast)]
        suffix, second = "", []             # what the _rescue entries take in addition, behind `untracked`
        if self.rescue is not None:
            suffix, second = "_rescue", [self.rescue["low_score"], self.rescue["iou"], P(self.lane_rescued)]
        if self.assign is not None:
            self._run_track_optimal(det, n_keep, A)
            return
        _lib.check(self._track_fn(suffix)(P(self.track_state), self.track_state.numel(), self.B, o["max_tracks"], o["iou"],
                                          o["max_age_us"], o["min_score"], *gains, P(det), P(n_keep), A, self._t_ref[2],
                                          P(self.track_ids), P(self.track_hits), *outputs, P(self.lane_untracked), *second,
                                          _lib.cur_stream(self.device)), self._track_family + suffix)
        self._last_det, self._scored = (det, n_keep), False

    def _run_track_optimal(self, det, n_keep, A):
        """``run_track``'s one launch with ``assign``: the arguments of ``dagr_stream_track_cv_rescue``, NULL / 0 where a
        flag is clear, then the flags and the workspace."""
        L, P, o, D = _lib.lib(), _lib.ptr, self.track, _lib.DEFINES
        flags, gains, outputs, second = 0, [0.0, 0.0], [None] * 7, [0.0, 0.0, None]
        if self.motion is not None:
            n_coast, c_id, c_box, c_label, c_age = self.coast
            flags |= D["DAGR_TRACK_OPTIMAL_MOTION"]
            gains = [self.motion["alpha"], self.motion["beta"]]
            outputs = [P(self.track_boxes), P(self.track_vel), P(c_id), P(c_box), P(c_label), P(c_age), P(n_coast)]
        if self.rescue is not None:
            flags |= D["DAGR_TRACK_OPTIMAL_RESCUE"]
            second = [self.rescue["low_score"], self.rescue["iou"], P(self.lane_rescued)]
        _lib.check(L.dagr_stream_track_optimal(P(self.track_state), self.track_state.numel(), self.B, o["max_tracks"], o["iou"],
                                               o["max_age_us"], o["min_score"], *gains, P(det), P(n_keep), A, self._t_ref[2],
                                               P(self.track_ids), P(self.track_hits), *outputs, P(self.lane_untracked),
                                               *second, flags, P(self.assign_ws), self.assign_ws.numel(),
                                               _lib.cur_stream(self.device)), "stream_track_optimal")
        self._last_det, self._scored = (det, n_keep), False

    # ------------------------------------------------------------------------------------ scoring the tracks
    def enable_score(self, options):
        """``run_score`` scores a step's track ids against labelled boxes (``dagr_stream_score``): ``options`` as
        ``dagr.streaming._score_options`` returns them, on a stream that tracks.  Allocates the lanes' tables, empty."""
        if self.track is None:
            raise RuntimeError("enable_score: the stream does not track (enable_track comes first)")
        self.score = dict(options)
        self.score_state = _state_buffer(self.device, "dagr_stream_score_bytes", self.B, self.score["max_objects"])
        self._reset_score()

    def _reset_score(self):
        """Empty tables, zero counters; the last step cannot be scored any more."""
        _lib.check(_lib.lib().dagr_stream_score_reset(_lib.ptr(self.score_state), self.score_state.numel(), self.B,
                                                      self.score["max_objects"], _lib.cur_stream(self.device)),
                   "stream_score_reset")
        self._last_det, self._scored = None, False

    def run_score(self, gt_box, gt_label, gt_id, n_gt):
        """``dagr_stream_score`` on the LAST step's ``det`` / ``n_keep`` / ``track_ids`` (``track_boxes`` with
        ``boxes="track"``) against device tensors ``gt_box`` fp32 [B, G, 4], ``gt_label`` int32 [B, G], ``gt_id`` int64
        [B, G] and ``n_gt`` int32 [B]: one launch, no host wait.  Leaves ``gt_match`` int64 [B, G] / ``gt_flags`` int32
        [B, G], valid until the next call."""
        if self.score is None:
            raise RuntimeError("this stream does not score (score=): it has no score_step")
        if self._last_det is None:
            raise RuntimeError("score_step: the stream has made no step since its construction / reset(): there is nothing "
                               "to score")
        if self._scored:
            raise RuntimeError("score_step: the last step has been scored already (one score_step per step)")
        det, n_keep = self._last_det
        B, A, G = self.B, int(det.shape[1]), int(gt_box.shape[1])
        if self.gt_match is None or tuple(self.gt_match.shape) != (B, G):
            self.gt_match = torch.zeros((B, G), dtype=torch.int64, device=self.device)
            self.gt_flags = torch.zeros((B, G), dtype=torch.int32, device=self.device)
        P, o = _lib.ptr, self.score
        boxes = P(self.track_boxes) if o["boxes"] == "track" else None
        _lib.check(_lib.lib().dagr_stream_score(P(self.score_state), self.score_state.numel(), B, o["max_objects"], o["iou"],
                                                P(det), P(n_keep), A, P(self.track_ids), boxes, P(gt_box), P(gt_label),
                                                P(gt_id), P(n_gt), G, P(self.gt_match), P(self.gt_flags),
                                                _lib.cur_stream(self.device)), "stream_score")
        self._scored = True
        if self.identity is not None:              # the second launch, behind the scorer's on the same arrays
            T = self.identity["max_tracks"]
            _lib.check(_lib.lib().dagr_stream_identity(P(self.identity_state), self.identity_state.numel(), B, o["max_objects"],
                                                       T, o["iou"], P(self.score_state), self.score_state.numel(), P(det),
                                                       P(n_keep), A, P(self.track_ids), boxes, P(gt_box), P(gt_label), P(gt_id),
                                                       P(n_gt), G, P(self.gt_match), _lib.cur_stream(self.device)),
                       "stream_identity")
        if self.hota is not None:                  # the third launch, behind the identity step's on the same arrays
            _lib.check(_lib.lib().dagr_stream_hota(P(self.hota_state), self.hota_state.numel(), B, o["max_objects"],
                                                   self.identity["max_tracks"], self.hota["max_instants"],
                                                   P(self.identity_state), self.identity_state.numel(), P(self.score_state),
                                                   self.score_state.numel(), P(det), P(n_keep), A, P(self.track_ids), boxes,
                                                   P(gt_box), P(gt_label), P(gt_id), P(n_gt), G, P(self.gt_match),
                                                   _lib.cur_stream(self.device)), "stream_hota")
        return self.gt_match, self.gt_flags

    # ------------------------------------------------------------------------------------ IDF1 behind the scorer
    def enable_identity(self, options):
        """``run_score`` also counts the overlaps of object identities with track ids (``dagr_stream_identity``):
        ``options`` as ``dagr.streaming._identity_options`` returns them, on a stream that scores.  Allocates the lanes'
        tables, empty, and the workspace of the solve."""
        if self.score is None:
            raise RuntimeError("enable_identity: the stream does not score (enable_score comes first)")
        self.identity = dict(options)
        M, T = self.score["max_objects"], self.identity["max_tracks"]
        self.identity_state = _state_buffer(self.device, "dagr_stream_identity_bytes", self.B, M, T)
        self.identity_ws = _state_buffer(self.device, "dagr_assign_workspace_bytes", self.B, M, T)
        self.obj_track = torch.zeros((self.B, M), dtype=torch.int64, device=self.device)
        self.identity_result = torch.zeros((self.B, _lib.DEFINES["DAGR_IDENTITY_RESULT_WORDS"]), dtype=torch.int64,
                                           device=self.device)
        self._reset_identity()

    def _reset_identity(self):
        _lib.check(_lib.lib().dagr_stream_identity_reset(_lib.ptr(self.identity_state), self.identity_state.numel(), self.B,
                                                         self.score["max_objects"], self.identity["max_tracks"],
                                                         _lib.cur_stream(self.device)), "stream_identity_reset")

    def run_identity_solve(self):
        """``dagr_stream_identity_solve`` on the counts so far: one launch; returns the device tensors ``(result int64
        [B, 9], obj_track int64 [B, max_objects])``, valid until the next call."""
        if self.identity is None:
            raise RuntimeError("this stream keeps no identity state (identity=): it has no IDF1")
        P = _lib.ptr
        _lib.check(_lib.lib().dagr_stream_identity_solve(P(self.identity_state), self.identity_state.numel(), self.B,
                                                         self.score["max_objects"], self.identity["max_tracks"],
                                                         P(self.obj_track), P(self.identity_result), P(self.identity_ws),
                                                         self.identity_ws.numel(), _lib.cur_stream(self.device)),
                   "stream_identity_solve")
        return self.identity_result, self.obj_track

    def identity_words(self):
        """The state read back through the layout include/dagr_hip.h documents: ``dict(track_id int64 [B, T], track_len int64
        [B, T], obj_len int64 [B, M], words int64 [B, 8], overlap int32 [B, M, T], obj_col int32 [B, M])`` (copies;
        synchronises)."""
        if self.identity is None:
            raise RuntimeError("this stream keeps no identity state (identity=): it has no tables")
        B, M, T = self.B, self.score["max_objects"], self.identity["max_tracks"]
        raw = self.identity_state.cpu().numpy()
        n64 = 2 * B * T + B * M + 8 * B
        q, r = raw[:8 * n64].view(np.int64), raw[8 * n64:8 * n64 + 4 * (B * M * T + B * M)].view(np.int32)
        return dict(track_id=q[:B * T].reshape(B, T), track_len=q[B * T:2 * B * T].reshape(B, T),
                    obj_len=q[2 * B * T:2 * B * T + B * M].reshape(B, M), words=q[2 * B * T + B * M:].reshape(B, 8),
                    overlap=r[:B * M * T].reshape(B, M, T), obj_col=r[B * M * T:].reshape(B, M))

    # ------------------------------------------------------------------------------------ HOTA behind the identity step
    HOTA_THRESHOLDS = _lib.DEFINES["DAGR_HOTA_THRESHOLDS"]

    def enable_hota(self, options):
        """``run_score`` also runs HOTA's pass 1 and appends the labelled instant to the lanes' logs (``dagr_stream_hota``):
        ``options`` as ``dagr.streaming._hota_options`` returns them, on a stream that keeps the identity state.  Allocates
        the state, empty, and the workspace of the solve; refuses by name a state above ``DAGR_HOTA_MAX_STATE_BYTES``."""
        if self.identity is None:
            raise RuntimeError("enable_hota: the stream keeps no identity state (enable_identity comes first)")
        L, M, T, I = _lib.lib(), self.score["max_objects"], self.identity["max_tracks"], int(options["max_instants"])
        nbytes, limit = L.dagr_stream_hota_bytes(self.B, M, T, I), _lib.DEFINES["DAGR_HOTA_MAX_STATE_BYTES"]
        if nbytes > limit:
            raise ValueError(f"hota: batch_size = {self.B}, score max_objects = {M}, identity max_tracks = {T} and hota "
                             f"max_instants = {I} need a state of {nbytes} bytes, above DAGR_HOTA_MAX_STATE_BYTES = {limit} "
                             f"(the log takes {24 * _lib.DEFINES['DAGR_HOTA_LOG_ENTRIES']} bytes an instant and lane, the 19 "
                             f"mc tables {76 * M * T} bytes a lane): lower max_instants, max_objects or max_tracks")
        state = _state_buffer(self.device, "dagr_stream_hota_bytes", self.B, M, T, I)
        self.hota_ws = _state_buffer(self.device, "dagr_stream_hota_workspace_bytes", self.B, M, T, I)
        self.hota, self.hota_state = dict(options), state
        self._reset_hota()

    def _reset_hota(self):
        _lib.check(_lib.lib().dagr_stream_hota_reset(_lib.ptr(self.hota_state), self.hota_state.numel(), self.B,
                                                     self.score["max_objects"], self.identity["max_tracks"],
                                                     self.hota["max_instants"], _lib.cur_stream(self.device)),
                   "stream_hota_reset")

    def run_hota_solve(self):
        """``dagr_stream_hota_solve`` on the log so far: the replay and the fp64 sums, left in the state (no host wait)."""
        if self.hota is None:
            raise RuntimeError("this stream keeps no HOTA state (hota=): it has no HOTA")
        P = _lib.ptr
        _lib.check(_lib.lib().dagr_stream_hota_solve(P(self.hota_state), self.hota_state.numel(), self.B,
                                                     self.score["max_objects"], self.identity["max_tracks"],
                                                     self.hota["max_instants"], P(self.hota_ws), self.hota_ws.numel(),
                                                     _lib.cur_stream(self.device)), "stream_hota_solve")

    def hota_sections(self):
        """Where the arrays of the HOTA state lie, by the layout include/dagr_hip.h documents: ``{name: (byte offset, numpy
        dtype, shape)}``, each array at the next multiple of 16 bytes behind the one before it."""
        B, M, T, I = self.B, self.score["max_objects"], self.identity["max_tracks"], self.hota["max_instants"]
        K, E = self.HOTA_THRESHOLDS, _lib.DEFINES["DAGR_HOTA_LOG_ENTRIES"]
        out, at = {}, 0
        for name, dtype, shape in (("pmc", np.int64, (B, M, T)), ("gc", np.int64, (B, M)), ("tc", np.int64, (B, T)),
                                   ("words", np.int64, (B, 4)), ("count", np.int64, (B, K, 4)), ("sums", np.float64, (B, K, 3)),
                                   ("log_box", np.float32, (B, I, E, 4)), ("log_n", np.int32, (B, I, 2)),
                                   ("log_index", np.int32, (B, I, E)), ("log_label", np.int32, (B, I, E)),
                                   ("mc", np.int32, (B, K, M, T))):
            out[name] = (at, dtype, shape)
            at += -(-int(np.prod(shape)) * np.dtype(dtype).itemsize // 16) * 16
        return out

    def hota_words(self, names):
        """The named arrays of the HOTA state read back (``hota_sections``; copies; synchronises)."""
        if self.hota is None:
            raise RuntimeError("this stream keeps no HOTA state (hota=): it has no tables")
        sections, out = self.hota_sections(), {}
        for name in names:
            at, dtype, shape = sections[name]
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            out[name] = self.hota_state[at:at + nbytes].cpu().numpy().view(dtype).reshape(shape)
        return out

    def score_words(self):
        """The state read back: ``(table int64 [8, B, max_objects] -- id, last_hyp, prev_hyp, seen_step, present, tracked,
        switches, frags --, words int64 [B, 16])``, the layout include/dagr_hip.h documents (copies; synchronises)."""
        if self.score is None:
            raise RuntimeError("this stream does not score (score=): it has no counters and no objects")
        n = self.B * self.score["max_objects"]
        raw = self.score_state.view(torch.int64).cpu().numpy()
        return raw[:8 * n].reshape(8, self.B, self.score["max_objects"]), raw[8 * n:].reshape(self.B, 16)

    def untracked(self):
        """Per-lane eligible rows that got no track id, int64 [B] (synchronises)."""
        if self.track is None:
            raise RuntimeError("this stream does not track (track=): it has no untracked count")
        return self.lane_untracked.cpu().numpy()

    def rescued(self):
        """Per-lane matches of the second association round, int64 [B] (synchronises)."""
        if self.rescue is None:
            raise RuntimeError("this stream has no second association round (rescue=): it has no rescued count")
        return self.lane_rescued.cpu().numpy()

    def track_slots(self):
        """The lanes' slots read back as ``(id int64, t_last int64, box fp32[., 4], label int32, hits int32)`` over
        ``[B, max_tracks]`` and ``next_id int64 [B]`` -- the layout include/dagr_hip.h documents (copies; synchronises).
        With a motion model ``vel fp32[., 4]`` follows ``box``: seven arrays."""
        if self.track is None:
            raise RuntimeError("this stream does not track (track=): it has no tracks")
        B, M = self.B, self.track["max_tracks"]
        out, at = [], 0
        for name, dtype, width in self.TRACK_FIELDS:
            if name == "vel" and self.motion is None:               # dagr_stream_track_cv's layout only
                continue
            size = B * M * width * torch.empty((), dtype=dtype).element_size()
            out.append(self.track_state[at:at + size].view(dtype).view((B, M) if width == 1 else (B, M, width)).cpu().numpy())
            at += size
        return (*out, self.track_state[at:at + 8 * B].view(torch.int64).cpu().numpy())

    def coast_device(self):
        """``(n_coast, coast_id, coast_box, coast_label, coast_age_us)`` of the last step, the device tensors."""
        if self.motion is None:
            raise RuntimeError("this stream has no motion model (motion=): nothing coasts")
        return self.coast

    # ------------------------------------------------------------------------------------ the picture
    def enable_render(self, options, width, height):
        """``run_render`` paints the lanes' frames (``dagr_stream_render``): ``options`` as
        ``dagr.streaming._render_options`` returns them (``colors`` a uint8 ``[n, 3]`` array), ``width`` x ``height`` the
        engine's.  Allocates the per-pixel maps (zero), the output, the status word and -- ``trail > 0``, after
        ``enable_track`` -- the trail rings, empty; a step then ends with ``dagr_stream_trail`` (``run_trail``).  Nothing
        is allocated after this."""
        self.render = dict(options)
        self.render_size = (int(width), int(height))
        dev = self.device
        if (self.render["trail"] > 0 or self.render["ids"]) and self.track is None:
            raise RuntimeError("enable_render: trails and id plates need the tracker (enable_track first)")
        self.render_colors = torch.from_numpy(np.ascontiguousarray(self.render["colors"], dtype=np.uint8)).to(dev)
        self.render_ws = _state_buffer(dev, "dagr_stream_render_workspace_bytes", self.B, height, width)
        self.render_flags = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.render_out = torch.zeros((self.B, height, width, 3), dtype=torch.uint8, device=dev)
        if self.render["trail"] > 0:
            self.trail_rings = _state_buffer(dev, "dagr_stream_trail_bytes", self.B, self.track["max_tracks"],
                                             self.render["trail"])
        self._reset_render()

    def _reset_render(self):
        """Zero maps, a clear status word, empty rings, and no step to draw."""
        self.render_ws.zero_()
        self.render_flags.zero_()
        self._render_det = None
        if self.trail_rings is not None:
            _lib.check(_lib.lib().dagr_stream_trail_reset(_lib.ptr(self.trail_rings), self.trail_rings.numel(), self.B,
                                                          self.track["max_tracks"], self.render["trail"],
                                                          _lib.cur_stream(self.device)), "stream_trail_reset")

    def run_trail(self):
        """``dagr_stream_trail`` on the slots the step's tracker launch left, at the step's ``t_ref``: one launch, no host
        wait (``run_track`` has looked ``t_ref`` up)."""
        _lib.check(_lib.lib().dagr_stream_trail(_lib.ptr(self.trail_rings), self.trail_rings.numel(), self.B,
                                                self.track["max_tracks"], self.render["trail"], _lib.ptr(self.track_state),
                                                self.track_state.numel(), self._t_ref[2], _lib.cur_stream(self.device)),
                   "stream_trail")

    def run_render(self, base=None, base_stride=0, out=None):
        """``dagr_stream_render`` on the last step's device arrays -- the resident events, ``det`` / ``n_keep``, the track
        ids, the rings --, or on nothing but ``base`` before the first step: uint8 ``[B, H, W, 3]`` (``out``, default the
        stream's own), valid until the next call.  Three launches at most, no host wait."""
        if self.render is None:
            raise RuntimeError("this stream draws nothing (render=): it has no render_step")
        o, P = self.render, _lib.ptr
        out = self.render_out if out is None else out
        W, H = self.render_size
        det, n_keep = self._render_det if self._render_det is not None else (None, None)
        drawn = det is not None
        _lib.check(_lib.lib().dagr_stream_render(
            P(self.state) if drawn else None, self.B, self.cap, -1 if o["event_window_us"] is None else o["event_window_us"],
            o["alpha"], P(det), P(n_keep), int(det.shape[1]) if drawn else 0,
            P(self.track_ids) if drawn and self.track is not None else None,
            P(self.trail_rings), self.track["max_tracks"] if self.trail_rings is not None else 0, o["trail"], o["linewidth"],
            1 if o["ids"] else 0, o["id_scale"], P(self.render_colors), int(self.render_colors.shape[0]), P(base), base_stride,
            P(out), H, W, P(self.render_flags), P(self.render_ws), self.render_ws.numel(), _lib.cur_stream(self.device)),
            "stream_render")
        return out

    def trail_arrays(self):
        """The rings read back as ``(id int64 [B, M], count int32 [B, M], pt int32 [B, M, trail, 2])``, the layout
        include/dagr_hip.h documents (copies; synchronises)."""
        if self.trail_rings is None:
            raise RuntimeError("this stream keeps no trails (render= with trail > 0): it has no rings")
        n, T = self.B * self.track["max_tracks"], self.render["trail"]
        shape = (self.B, self.track["max_tracks"])
        r = self.trail_rings
        return (r[:8 * n].view(torch.int64).view(shape).cpu().numpy(), r[8 * n:12 * n].view(torch.int32).view(shape).cpu().numpy(),
                r[12 * n:12 * n + 8 * n * T].view(torch.int32).view(*shape, T, 2).cpu().numpy())

    # ------------------------------------------------------------------------------------ the push stages
    def _enable(self, name, *description, **more):
        """The stage ``name`` (as its option tuple is called), with the scratch of a push of 4096 rows to begin with."""
        self.stages[name] = _PushStage(self.B, self.device, self.status, *description, **more)
        self.stages[name].grow(4096)

    def _push(self, name, xy, t, p, batch, n=None):
        """A push of events (their first ``n`` rows; None: all) through the stage ``name``: ``(xy, t, p, batch int32, count
        int32[1])`` of the survivors, on the device, valid until the next push."""
        n, P = int(t.shape[0]) if n is None else n, _lib.ptr
        return self.stages[name].run(n, (P(xy), P(t), P(p), P(batch), 1 if batch.dtype == torch.int64 else 0, n))

    # ------------------------------------------------------------------------------------ sensor noise
    def enable_denoise(self, sensor_w, sensor_h, denoise_us=None, refractory_us=None):
        """Pushes go through ``dagr_stream_denoise`` first: a ``sensor_w x sensor_h`` stamp map per lane, ``denoise_us`` /
        ``refractory_us`` positive or None (off; not both)."""
        if denoise_us is None and refractory_us is None:
            raise ValueError("enable_denoise: denoise_us and refractory_us are both None")
        self.noise = (int(sensor_w), int(sensor_h), int(denoise_us or 0), int(refractory_us or 0))
        self.lane_filtered = torch.zeros((self.B,), dtype=torch.int64, device=self.device)
        self._enable("noise", "stream_denoise", "stream_denoise", self.noise[:2], 8 * self.B * self.noise[0] * self.noise[1],
                     self.noise, [self.lane_filtered])

    def denoise(self, xy, t, p, batch):
        """``dagr_stream_denoise`` on a push (``_push``); rows from the count up to the push's size are lane-less (lane -1
        at pixel (0, 0))."""
        return self._push("noise", xy, t, p, batch)

    def filtered(self):
        """Per-lane events the noise filter has removed, int64 [B]; zeros without the filter (synchronises)."""
        if self.noise is None:
            torch.cuda.current_stream(self.device).synchronize()
            return np.zeros((self.B,), np.int64)
        return self.lane_filtered.cpu().numpy()

    def last_stamps(self):
        """The lanes' stamp maps int64[B, sensor_h, sensor_w], never = INT64_MIN (a copy; synchronises)."""
        if self.noise is None:
            raise RuntimeError("this stream does not filter noise (denoise_us / refractory_us): it has no stamp maps")
        sensor_w, sensor_h = self.noise[:2]
        return self.stages["noise"].carried_bytes().view(torch.int64).view(self.B, sensor_h, sensor_w).cpu().numpy()

    # ------------------------------------------------------------------------------------ flicker and trails
    def enable_flicker(self, sensor_w, sensor_h, flicker=None, trail_us=None):
        """Pushes go through ``dagr_stream_flicker`` in front of the noise filter: per-pixel state over a ``sensor_w x
        sensor_h`` sensor per lane; ``flicker`` as ``dagr.streaming._flicker_options`` returns it or None (off),
        ``trail_us`` positive or None (off; not both)."""
        if flicker is None and trail_us is None:
            raise ValueError("enable_flicker: flicker and trail_us are both None")
        periods, thresholds = (0, 0), (0, 0, 0)
        if flicker is not None:
            from .streaming import flicker_periods
            periods = flicker_periods(flicker)
            thresholds = (int(flicker["start"]), int(flicker["stop"]), int(flicker["max_count"]))
        self.flick = (int(sensor_w), int(sensor_h), *periods, *thresholds, int(trail_us or 0))
        self.lane_suppressed = torch.zeros((2, self.B), dtype=torch.int64, device=self.device)      # flicker, trail
        self._enable("flick", "stream_flicker", "stream_flicker", self.flick[:2], flicker_map_bytes(self.B, *self.flick[:2]),
                     self.flick, [self.lane_suppressed[0], self.lane_suppressed[1]])

    def flicker(self, xy, t, p, batch):
        """``dagr_stream_flicker`` on a push (``_push``); rows from the count up to the push's size are lane-less (lane -1
        at pixel (0, 0))."""
        return self._push("flick", xy, t, p, batch)

    def suppressed(self):
        """Per-lane events the flicker stage and the trail stage have removed, ``(int64 [B], int64 [B])``; zeros without the
        filter (synchronises)."""
        if self.flick is None:
            torch.cuda.current_stream(self.device).synchronize()
            return np.zeros((self.B,), np.int64), np.zeros((self.B,), np.int64)
        both = self.lane_suppressed.cpu().numpy()
        return both[0].copy(), both[1].copy()

    def flicker_maps(self):
        """The per-pixel state as ``dagr.streaming.flicker_definition`` names it (``flicker_maps_from_state``; copies;
        synchronises)."""
        if self.flick is None:
            raise RuntimeError("this stream has no flicker / trail filter (flicker / trail_us): it has no per-pixel state")
        return flicker_maps_from_state(self.stages["flick"].state, self.B, *self.flick[:2])

    # ------------------------------------------------------------------------------------ camera words
    def enable_decode(self, format, sensor_w, sensor_h, max_decoded=None, t_base=None):
        """Pushes carry camera words, which ``dagr_stream_decode`` turns into events first: ``format`` is
        ``DAGR_DECODE_EVT2`` / ``DAGR_DECODE_EVT3``, ``max_decoded`` the rows of the output buffers (None: the worst case of
        the largest push so far, ``events_per_word`` each), ``t_base`` int64 [B] on the host or None."""
        self.words = (int(format), int(sensor_w), int(sensor_h), None if max_decoded is None else int(max_decoded))
        self.words_per = 12 if int(format) == _lib.DEFINES["DAGR_DECODE_EVT3"] else 1
        self.words_t_base = None if t_base is None else torch.as_tensor(np.asarray(t_base, np.int64)).to(self.device)
        self.lane_decoded = torch.zeros((self.B, 4), dtype=torch.int64, device=self.device)
        # the state is sized by the words of a push, the decoded events' buffers by what those can decode
        per, most = self.words_per, self.words[3]
        self._enable("words", "stream_decode", "stream_decode", (), 64 * self.B, self.words[:3], [self.lane_decoded],
                     out_rows=lambda n: per * n if most is None else most)

    def decode(self, words, word_end, t_base=None):
        """``dagr_stream_decode`` on a push of words (``words`` uint16 / uint32 bits, ``word_end`` int64 [B], both on the
        device): ``(xy, t, p, batch int32, count int32[1])`` of the decoded events, valid until the next push.  The arrays
        have ``max_out = decode_rows(n_words)`` rows; those from the count up are lane-less (lane -1 at pixel (0, 0))."""
        n, P = int(words.shape[0]), _lib.ptr
        t_base = self.words_t_base if t_base is None else t_base
        rows = max(self.decode_rows(n), 1)
        o = self.stages["words"].run(n, (P(words) if n else None, P(word_end), n, P(t_base), rows))
        return o[0][:rows], o[1][:rows], o[2][:rows], o[3][:rows], o[4]

    def decode_rows(self, n_words):
        """What a push of ``n_words`` words can decode at the most: the host's bound of the window grows by this."""
        worst = self.words_per * int(n_words)
        return worst if self.words[3] is None else min(self.words[3], worst)

    def decode_counts(self):
        """The decoder's cumulative counters int64 [B, 4]: decoded, unsynced, outside, skipped (a copy; synchronises)."""
        if self.words is None:
            raise RuntimeError("this stream does not decode camera words (decode=): it has no decoder counters")
        return self.lane_decoded.cpu().numpy()

    def decode_state(self):
        """The lanes' decoder states int64 [B, 8]: high, low, loops, y, base_x, pol, synced, 0 (a copy; synchronises)."""
        if self.words is None:
            raise RuntimeError("this stream does not decode camera words (decode=): it has no decoder state")
        return self.stages["words"].carried_bytes().view(torch.int64).view(self.B, 8).cpu().numpy()

    # ------------------------------------------------------------------------------------ raw sensor events
    def enable_front(self, fx, fy, sensor_w, sensor_h, width, height):
        """Pushes carry raw events of a ``sensor_w x sensor_h`` sensor, downsampled ``fx x fy`` on the device."""
        self.front = tuple(int(v) for v in (fx, fy, sensor_w, sensor_h, width, height))
        cells_w, cells_h = self._cells()
        self._enable("front", "stream_front", "stream_downsample", (cells_w, cells_h), 4 * self.B * cells_w * cells_h,
                     self.front)

    def _cells(self):
        fx, fy, sensor_w, sensor_h = self.front[:4]
        return sensor_w // fx, sensor_h // fy

    def downsample(self, xy, t, p, batch):
        """``dagr_stream_downsample`` on a raw push (``_push``)."""
        return self._push("front", xy, t, p, batch)

    def change_maps(self):
        """The lanes' change maps fp32[B, cells_h, cells_w] (a copy; synchronises)."""
        if self.front is None:
            raise RuntimeError("this stream does not downsample: it has no change maps")
        cells_w, cells_h = self._cells()
        return self.stages["front"].carried_bytes().view(torch.float32).view(self.B, cells_h, cells_w).cpu().numpy()

    def _alloc(self, cap):
        return _state_buffer(self.device, "dagr_stream_state_bytes", self.B, cap)

    def reset(self):
        if self.state is not None:
            _lib.check(_lib.lib().dagr_stream_reset(_lib.ptr(self.state), self.B, self.cap, _lib.cur_stream(self.device)),
                       "stream_reset")
        for stage in self.stages.values():
            stage.reset()
        if self.track_state is not None:
            self._reset_track()
        if self.score_state is not None:
            self._reset_score()
        if self.identity_state is not None:
            self._reset_identity()
        if self.hota_state is not None:
            self._reset_hota()
        if self.labels_state is not None:
            self._reset_labels()
        if self.map is not None:
            self._reset_map()
        if self.render is not None:
            self._reset_render()
        self._stepped, self._labelled = False, False
        self.status.zero_()
        self.lane_count.zero_()
        self.lane_dropped.zero_()
        torch.cuda.current_stream(self.device).synchronize()       # (a count copy may still be on its way)
        self._host.zero_()
        self._known, self._since, self._fresh = np.zeros((self.B,), np.int64), 0, True
        self.frame_steps = self.held_steps = 0
        self.frame_new = True                 # the frame in force stays; the next step runs it through the branch again

    def write_frames(self, frames, lanes, fx, fy, width, height, bgr):
        """``dagr_stream_frame``: raw frames (uint8 [n, H_f, W_f, 3] on the device; rows may be padded) into the named
        lanes (int32 [n] on the device) of the frame in force; the other lanes keep theirs (zeros before their first).
        Counts as a new frame for the whole batch."""
        if self.image is None or tuple(self.image.shape) != (self.B, 3, height, width):
            self.image = torch.zeros((self.B, 3, height, width), dtype=torch.float32, device=self.device)
        n, frame_h, frame_w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        img = self.image
        _lib.check(_lib.lib().dagr_stream_frame(
            _lib.ptr(frames), frames.stride(0), frames.stride(1), n, _lib.ptr(lanes), frame_w, frame_h, fx, fy, width, height,
            1 if bgr else 0, _lib.ptr(img), self.B, img.stride(0), img.stride(1), img.stride(2), img.stride(3),
            _lib.ptr(self.status), _lib.cur_stream(self.device)), "stream_frame")
        self.frame_new = True

    def grow(self, cap):
        """Raw sets of ``cap`` events; the resident events are copied over on the device."""
        if cap <= self.cap:
            return
        new = self._alloc(cap)
        L, stream = _lib.lib(), _lib.cur_stream(self.device)
        if self.state is None:
            _lib.check(L.dagr_stream_reset(_lib.ptr(new), self.B, cap, stream), "stream_reset")
        else:
            _lib.check(L.dagr_stream_grow(_lib.ptr(self.state), self.cap, _lib.ptr(new), cap, self.B, stream), "stream_grow")
        self.state, self.cap = new, cap

    def read_counts(self):
        """The stream has just been drained: the last step's counts are in the pinned buffer."""
        self._known, self._since, self._fresh = self._host.numpy().astype(np.int64), 0, True

    def bound(self):
        """Upper bound of the resident count: the last count read plus every event pushed since -- and, with a cap,
        ``B * max_lane_events``."""
        bound = int(self._known.sum()) + self._since
        return bound if self.max_lane_events is None else min(bound, self.B * self.max_lane_events)

    def dropped(self):
        """Per-lane events the count rule has removed, int64 [B] (synchronises)."""
        return self.lane_dropped.cpu().numpy()

    def counts_known(self):
        """Per-lane counts of the last step if they have been read, else None."""
        return self._known.copy() if self._fresh else None

    def _pushed_now(self, n_new):
        self._since += int(n_new)
        self._fresh = False
        self._host.copy_(self.lane_count, non_blocking=True)


class _Level:
    """Device buffers of one pooled graph level (capacity T = gx*gy*(B+1) nodes)."""

    def __init__(self, T, cin, cout, device, cf_next=0):
        self.T = T
        self.e_cap = T * 64
        i32 = dict(dtype=torch.int32, device=device)
        f32 = dict(dtype=torch.float32, device=device)
        # pooled features + pos[:, :2]; row stride padded to 16 bytes (the tiled conv reads 16-byte channel quads)
        self.x = torch.zeros((T, (cin + 3) // 4 * 4), **f32)
        self.pos = torch.zeros((T, 3), **f32)
        self.batch = torch.zeros((T,), **i32)
        self.rowptr = torch.zeros((T + 2,), **i32)
        self.col = torch.zeros((self.e_cap,), **i32)
        self.code = torch.zeros((self.e_cap,), **i32)
        self.counts = torch.zeros((2,), **i32)       # [n_nodes, n_edges]
        self.cluster = torch.zeros((T,), **i32)      # scratch for the next pooling
        self.h1 = torch.zeros((T, cout), **f32)
        # Layer output h2 = hp[:, :cout]; with --use_image the image features sampled at this level's
        # nodes are written into hp[:, cout:] (sampling_skip, net.py:142,155,171) and hp is what gets pooled
        self.hp = torch.zeros((T, cout + cf_next), **f32)
        self.cout = cout


class WindowEngine:
    def __init__(self, model, max_events=1 << 17, device="cuda"):
        self.model = model
        self.device = torch.device(device)
        args = model.args
        bb, head = model.backbone, model.head
        self.args = args
        self.B = int(args.batch_size)
        self.W, self.H = int(model.width), int(model.height)
        self.time_window = int(getattr(args, "time_window_us", 1000000))
        self.num_classes = bb.num_classes
        self.num_scales = int(args.num_scales)
        self.use_image = bool(args.use_image)
        self.no_events = bool(getattr(args, "no_events", False))
        # channels of the image features concatenated before Layer k (net.py:47-50): [16,64,s,s,s]
        self.feat_ch = list(bb.net.feature_channels) if self.use_image else [0] * 5
        if self.use_image:   # channels-last image branch: its feature maps are then read as [B,h,w,C] rows
            bb.net.to(memory_format=torch.channels_last)
            head.cnn_head.to(memory_format=torch.channels_last)
        if bb.conv_block1.conv_block1.conv.lut_domain is None:
            model.cache_luts(width=self.W, height=self.H, radius=args.radius)
            model._engine = self
        self.L = _lib.lib()
        if self.L.dagr_device_count() < 1:
            raise RuntimeError("dagr_amd: no HIP device visible; the event-graph path has no CPU fallback")
        self._keep = []
        self._cnn_out = None
        self._img_stream = None
        self._feat_ready = None                 # pipelined window: event per feature map (keyed by the map's id)
        # detection post-processing captured with the window / tail graph (forward_detections): thresholds it was captured
        # with, its static outputs, and whether the last forward ran it
        self._post_key = None
        self._det = self._n_keep = None
        self._wg_post = self._graph_post = (None, None)
        self._post_fresh = False
        self._cnn_ready = None
        self._net_f = self._cnn_f = None
        self._tail_jobs = None
        self._inputs_gathered = False
        # level-0 pooling on the graph builder's offset codes (bitmap coarse edges); False: the generic coarse-edge path
        self.fast_coarse_edges = True
        self._pool_accumulated = [False] * 4
        # The stream (StreamState) whose last frame body left the maps ``_img_feats`` / ``_cnn_out`` now hold, or None:
        # forward_stream runs the held body -- the window without the image branch -- only for that stream, and everything
        # that rewrites the maps' memory or replaces them clears it.
        self._held_for = None
        self._hg = self._hg_out = self._wg_maps = None   # the held body's captured graph; the maps _wg's capture allocated
        self._hg_post = (None, None)
        self._hg_warm = 0
        # Latency mode (one window batch at a time, e.g. DAGR.forward): head scale 1 runs beside pool4 / layer5 / head scale
        # 2 and everything after pool1 is replayed as one HIP graph -- the host issues one launch instead of ~70.  When
        # several engines keep the GPU full on their own streams (bench.py's throughput rigs) both cost throughput
        # (measured, events-only, 3 engines: 696 M events/s plain, 620 M with the side stream, 594 M with graph replay),
        # so such callers switch it off with set_low_latency(False).
        self.set_low_latency(True)
        self._head_stream = self._head_join = self._graph = self._graph_out = None
        self._graph_warm = 0
        self._wg = self._wg_out = None       # the whole window as one captured HIP graph (latency mode)
        self._wg_warm = 0
        self._dev_mode = False               # stages bound by the device-side event / node counts (inside the capture)
        self.in_image = None
        self._async_on = False
        self._app = None
        self._n_rows = 0
        self._N = 0                  # events of the resident window (0: none yet)
        self._stream_pending = None  # the stream whose step is the resident window, until its count has been read
        self._prepare(bb, head)
        self.max_events = 0
        self._alloc_events(int(max_events))

    # ------------------------------------------------------------------------------------ plan
    def _prepare(self, bb, head):
        dev = self.device
        L = self.L
        stream = _lib.cur_stream(dev)
        layers = [bb.conv_block1, bb.layer2, bb.layer3, bb.layer4, bb.layer5]
        pools = [bb.pool1, bb.pool2, bb.pool3, bb.pool4]
        self.dom = [layer.conv_block1.conv.lut_domain for layer in layers]
        # ---- level 0
        d0 = self.dom[0]
        if d0["rx"] != d0["ry"]:
            raise NotImplementedError("level 0 expects a square search radius (ev_tgn.py:29 derives it from the width)")
        win = []
        for r, den in ((d0["rx"], d0["den_x"]), (d0["ry"], d0["den_y"])):
            lo, cnt = ctypes.c_int32(0), ctypes.c_int32(0)
            _lib.check(L.dagr_spline_tap_window(r, den, ctypes.byref(lo), ctypes.byref(cnt)), "tap_window")
            if cnt.value <= 3:      # 3-tap window (clamped into the 5-tap kernel), else all 5 taps
                win += [min(lo.value, 2), 3]
            else:
                win += [0, 5]
        self.win0 = tuple(win)      # (win_x, tx, win_y, ty)
        self.ntaps0 = win[1] * win[3]
        ntp = (self.ntaps0 + 3) // 4 * 4
        self.ncodes0 = (2 * d0["rx"] + 1) * (2 * d0["ry"] + 1)
        self.tab0 = torch.zeros((self.ncodes0, ntp), dtype=torch.float32, device=dev)
        bad = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.check(L.dagr_spline_l0_table(d0["rx"], d0["ry"], d0["den_x"], d0["den_y"], win[0], win[1], win[2], win[3],
                                          _lib.ptr(self.tab0), _lib.ptr(bad), stream), "l0_table")
        if int(bad.item()) != 0:
            raise RuntimeError("level-0 offset table: an offset needs a kernel tap outside the chosen window")
        l0 = layers[0]
        # Input row of level 0.  Reference channel order (net.py:118,124-125): [polarity | image feats | pos_xy].  The
        # tiled kernel (csrc/conv_l0_tiles.hip) reads a main block of cout0 channels as 16-byte (8-byte: cout0 = 8) pieces,
        # so with --use_image the row is laid out [cout0 image feats | polarity | pos_xy | pad] (80 B at 16); events-only
        # [polarity | pos_xy | pad] (16 B).
        c0 = 1 + self.feat_ch[0] + 2
        self.cout0 = int(l0.conv_block1.conv.weight.shape[2])     # Net: int(base_width * 32)
        self.l0_tiles = ((win[1], win[3]) in ((3, 3), (3, 5), (5, 3)) and int(self.args.max_neighbors) == 16
                         and self.feat_ch[0] in (0, self.cout0))
        if self.cout0 != 16 and not self.l0_tiles:
            raise NotImplementedError("level-0 widths other than 16 run on the tiled level-0 conv only (16 neighbours, "
                                      "3x3 / 3x5 / 5x3 tap window); supported widths: " + ", ".join(map(str, L0_WIDTHS)))
        if self.l0_tiles:
            nf = self.feat_ch[0]
            self.x0_cols = list(range(1, 1 + nf)) + [0, 1 + nf, 2 + nf]      # reference channel of every x0 column
            self.x0_ld = (c0 + 3) // 4 * 4
            self.x0_feat_col, self.x0_img_col, self.x0_pos_col = nf, 0, nf + 1
        else:
            self.x0_cols = list(range(c0))
            self.x0_ld = c0
            self.x0_feat_col, self.x0_img_col, self.x0_pos_col = 0, 1, c0 - 2
        self.l0_conv1 = _pack_l0(l0.conv_block1.conv, l0.conv_block1.norm, self.win0, device=dev, cols_in=self.x0_cols)
        self.l0_conv2 = _pack_l0(l0.conv_block2.conv, l0.conv_block2.norm, self.win0,
                                 skip=(l0.conv_block2.lin, l0.conv_block2.norm_skip), device=dev,
                                 cols_skip=self.x0_cols)
        # (main block, extras) of both convs' input rows, looked up per launch
        self._l0_blocks = {p[0]: _l0_block(p[0]) for p in (self.l0_conv1, self.l0_conv2)}
        # ---- pooled levels 1..4
        self.packs = []
        for layer in layers[1:]:
            c1 = _pack_generic([layer.conv_block1.conv], [layer.conv_block1.norm], device=dev)
            c2 = _pack_generic([layer.conv_block2.conv], [layer.conv_block2.norm],
                               skip=(layer.conv_block2.lin, layer.conv_block2.norm_skip), device=dev)
            self.packs.append((c1, c2))
        # ---- poolings
        self.pool_desc, self.pool_ws, self.levels = [], [], []
        B = self.B
        chans = [l.out_channel for l in layers]
        fch = self.feat_ch
        for k, pool in enumerate(pools):
            vs = pool.voxel_size.detach().float().cpu()
            end = torch.Tensor([0.9999999, 0.9999999])
            g = ((end - 0) / vs[:2]).to(torch.int64) + 1            # grid_cluster num_voxels
            nd = self.dom[k + 1]
            remap = nd["remap"]
            desc = _lib.PoolDesc(batch_size=B, channels=chans[k] + fch[k + 1], gx=int(g[0]), gy=int(g[1]), vx=float(vs[0]),
                                 vy=float(vs[1]), inv_w=float(pool.wh_inv[0, 0]), inv_h=float(pool.wh_inv[0, 1]),
                                 two_max=_f32(2 * pool.transform.max), r00=float(remap[0, 0]),
                                 r02=float(remap[0, 2]), r11=float(remap[1, 1]), r12=float(remap[1, 2]),
                                 rx=nd["rx"], ry=nd["ry"], aggr=0 if pool.aggr == "max" else 1, append_pos=1,
                                 # --keep_temporal_ordering (pooling.py:69-72): the kernels drop the coarse edges that do
                                 # not point forward in time (one launch more per pooling step; every path and capture)
                                 keep_order=1 if getattr(pool, "keep_temporal_ordering", False) else 0)
            nbytes = L.dagr_pool_workspace_bytes(ctypes.byref(desc))
            if nbytes == 0:
                raise RuntimeError("libdagr_hip: " + L.dagr_last_error().decode())
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(L.dagr_pool_workspace_init(ctypes.byref(desc), _lib.ptr(ws), nbytes, stream), "pool_ws_init")
            self.pool_desc.append(desc)
            self.pool_ws.append(ws)
            T = int(g[0]) * int(g[1]) * (B + 1)
            self.levels.append(_Level(T, chans[k] + fch[k + 1] + 2, chans[k + 1], dev,
                                      cf_next=fch[k + 2] if k + 2 < 5 else 0))
        # voxel -> first pixel tables for the level-0 pooling (same fp32 division as grid_cluster)
        vs = pools[0].voxel_size.detach().float().cpu()
        d = self.pool_desc[0]
        cellx = ((torch.arange(self.W).float() / self.W) / vs[0]).to(torch.int64)
        celly = ((torch.arange(self.H).float() / self.H) / vs[1]).to(torch.int64)
        self.xlo = torch.searchsorted(cellx, torch.arange(d.gx + 1)).to(torch.int32).to(dev)
        self.ylo = torch.searchsorted(celly, torch.arange(d.gy + 1)).to(torch.int32).to(dev)
        # ---- head
        self.head_packs, self.head_dom = [], []
        first_level = 5 - self.num_scales   # levels feeding scale 1..num_scales (3,4 or 4)
        self.head_levels = list(range(first_level, 5))
        for s in range(1, self.num_scales + 1):
            g = lambda n: getattr(head, n + str(s))
            stem = _pack_generic([g("stem").conv], [g("stem").norm], device=dev)
            cr = _pack_generic([g("cls_conv").conv, g("reg_conv").conv], [g("cls_conv").norm, g("reg_conv").norm],
                               device=dev)
            cls = _pack_generic([g("cls_pred")], [None], relu=False, device=dev)
            ro = _pack_generic([g("reg_pred"), g("obj_pred")], [None, None], relu=False, device=dev)
            self.head_packs.append((stem, cr, cls, ro))
            # DAGR.cache_luts ties the table to the head's name ("1" -> pool3, "2" -> pool4), whatever level it
            # consumes (dagr.py:52-72): the convs of head s are evaluated on THEIR domain
            hd = g("stem").conv.lut_domain
            for n in ("cls_conv", "reg_conv"):
                assert _same_domain(getattr(head, n + str(s)).conv.lut_domain, hd)
            for n in ("cls_pred", "reg_pred", "obj_pred"):
                assert _same_domain(getattr(head, n + str(s)).lut_domain, hd)
            self.head_dom.append(hd)
        self.n_reg = head.stem1.conv.out_channels
        osz = bb.get_output_sizes()[-self.num_scales:]
        self.out_sizes = osz                                   # [[H,W], ...]
        self.strides = list(bb.strides)
        self.head_vox = [pools[2].voxel_size[:2].detach().float().cpu(), pools[3].voxel_size[:2].detach().float().cpu()][-self.num_scales:]
        # scratch for the head / aggregation
        lda_max = 0
        for k, (c1, c2) in enumerate(self.packs):
            lda_max = max(lda_max, self.levels[k].T * (max(c1.K, c2.K) + 3))
        for i, lvl in enumerate(self.head_levels):
            for p in self.head_packs[i]:
                lda_max = max(lda_max, self.levels[lvl - 1].T * (p.K + 3))
        self.A = torch.zeros((lda_max,), dtype=torch.float32, device=dev)
        # second scratch for head scale 1 when it overlaps layer5 on a side stream (only the unfused convs touch it)
        lda2 = max([self.levels[self.head_levels[0] - 1].T * (p.K + 3) for p in self.head_packs[0]])
        self.A2 = torch.zeros((lda2 if self.num_scales > 1 else 1,), dtype=torch.float32, device=dev)
        self.head_buf = []
        for i, lvl in enumerate(self.head_levels):
            T = self.levels[lvl - 1].T
            Hc, Wc = self.out_sizes[i]
            self.head_buf.append(dict(
                stem=torch.zeros((T, self.n_reg), dtype=torch.float32, device=dev),
                cr=torch.zeros((T, 2 * self.n_reg), dtype=torch.float32, device=dev),
                pred=torch.zeros((T, 5 + self.num_classes), dtype=torch.float32, device=dev),
                dense=torch.zeros((self.B, 5 + self.num_classes, Hc, Wc), dtype=torch.float32, device=dev)))
        self.status = torch.zeros((4,), dtype=torch.int32, device=dev)
        # a head whose table domain is not its input level's (num_scales = 1: head "1" on out4 with the pool3
        # table) gets its own LUT coordinates (dagr_pool_recode)
        self.head_code = []
        for i, lvl in enumerate(self.head_levels):
            same = _same_domain(self.head_dom[i], self.dom[lvl])
            self.head_code.append(None if same else torch.zeros_like(self.levels[lvl - 1].code))
        # grid / stride cache of decode_outputs (model/utils.py:119-134)
        grids, strides = [], []
        for (hs, ws_), stride in zip(self.out_sizes, self.strides):
            yv, xv = torch.meshgrid(torch.arange(hs), torch.arange(ws_), indexing="ij")
            grid = torch.stack((xv, yv), 2).view(1, -1, 2)
            grids.append(grid)
            strides.append(torch.full((1, grid.shape[1], 1), stride))
        self.grid_cache = torch.cat(grids, dim=1).float().to(dev)
        self.stride_cache = torch.cat(strides, dim=1).float().to(dev)

    def set_low_latency(self, on):
        self.overlap_heads = self.tail_graph = bool(on)
        # the WHOLE window (image branch, graph build, level 0, tail, heads, decode) as one HIP graph: every launch is sized
        # for the engine's event capacity and bounded by counts that live in device memory
        self.window_graph = bool(on)
        self._held_for = None                # the other mode's frame body keeps its maps elsewhere
        return self

    def _drop_window_graph(self):
        """Forget the captured window -- both bodies, and the maps the frame body's capture allocated -- and with it any
        hold on a frame's maps: the next window runs eagerly (two warm-up runs) and is captured anew."""
        self._wg = self._wg_out = None
        self._wg_warm = 0
        self._hg = self._hg_out = self._wg_maps = None
        self._hg_warm = 0
        self._held_for = None

    def _alloc_events(self, n):
        if n <= self.max_events:
            return
        dev = self.device
        n = max(n, 1024)
        self.max_events = n
        bb = self.model.backbone
        tgn = bb.events_to_graph
        self.graph = tgn.window_builder(self.W, self.H, self.time_window, self.B, dev, max_events=n)
        K = self.graph.K
        self.nbr_src = torch.zeros((n, K), dtype=torch.int32, device=dev)
        self.nbr_code = torch.zeros((n, K), dtype=torch.int16, device=dev)
        self.deg = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.h1 = torch.zeros((n, self.cout0), dtype=torch.float32, device=dev)
        self.hp0 = torch.zeros((n, self.cout0 + self.feat_ch[1]), dtype=torch.float32, device=dev)  # [h2 | image feats]
        self.x0buf = torch.zeros((n, self.x0_ld), dtype=torch.float32, device=dev)
        self.cluster0 = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.pos_n = torch.zeros((n, 3), dtype=torch.float32, device=dev)     # node (slot) order
        self.batch_n = torch.zeros((n,), dtype=torch.int32, device=dev)
        # static inputs of the captured window (latency mode): the caller's events are staged here by one launch
        self.in_pos = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        self.in_feat = torch.zeros((n,), dtype=torch.float32, device=dev)
        self.in_batch = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.n_dev = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._drop_window_graph()            # captured on the old buffers
        self.rows_cap = n
        self._async_on = False
        self._app = None

    # ---------------------------------------------------------------------- asynchronous operation
    _ROW_ARRAYS = ("nbr_src", "nbr_code", "deg", "h1", "hp0", "x0buf", "cluster0", "pos_n", "batch_n")

    def _grow_rows(self, rows):
        """More level-0 rows WITHOUT losing the resident window (the asynchronous state lives in these arrays)."""
        if rows <= self.rows_cap:
            return
        cap = max(rows, self.rows_cap + self.rows_cap // 2)
        for name in self._ROW_ARRAYS:
            old = getattr(self, name)
            new = torch.zeros((cap,) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
            new[:old.shape[0]] = old
            setattr(self, name, new)
        if self._app is not None:
            for name in ("next", "xytb", "batch_ev"):
                old = self._app[name]
                new = torch.zeros((cap,) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
                new[:old.shape[0]] = old
                self._app[name] = new
        self.rows_cap = cap

    def can_append(self):
        """Whether ``forward_append`` can attach events to the resident window: the incremental path runs on the tiled
        level-0 conv and keeps pool1's coarse edges as cell bitmaps (search radius <= two voxels, dagr_pool_l0_stream),
        and it needs a window of THIS engine to attach to.  ``DAGR.forward(reset=False)`` re-evaluates the running
        window otherwise (``make_model_synchronous``'s path)."""
        if not self.l0_tiles or self.no_events or self._N <= 0 or self.B >= 30:
            return False
        d, g = self.pool_desc[0], self.graph.params
        cell_w, cell_h = int(np.floor(np.float32(d.vx) * np.float32(g["width"]))), int(np.floor(np.float32(d.vy) * np.float32(g["height"])))
        return g["max_neighbors"] <= 16 and g["radius"] <= 2 * min(cell_w, cell_h) and g["width"] <= 4096

    def async_begin(self):
        """Turn the resident window (the last ``forward_raw``) into the state of an asynchronous run: per-pixel chains for
        the events to come (empty), the sample index by event id, and pool1's accumulators resident in their own
        workspace (dagr_pool_l0_stream).  Called by the first ``forward_append`` after a window."""
        L, P = self.L, _lib.ptr
        dev = self.device
        n0 = self._N
        if n0 == 0:
            raise RuntimeError("asynchronous update without a window: call forward_raw (reset=True) first")
        self._grow_rows(n0 + max(4096, n0 // 4))
        npix = self.B * self.H * self.W
        if self._app is None or self._app["head"].shape[0] != npix:
            nbytes = L.dagr_pool_workspace_bytes(ctypes.byref(self.pool_desc[0]))
            self._app = dict(head=torch.empty((npix,), dtype=torch.int32, device=dev),
                             next=torch.zeros((self.rows_cap,), dtype=torch.int32, device=dev),
                             xytb=torch.zeros((self.rows_cap, 4), dtype=torch.int32, device=dev),
                             batch_ev=torch.zeros((self.rows_cap,), dtype=torch.int32, device=dev),
                             status=torch.zeros((4,), dtype=torch.int32, device=dev),
                             pool_ws=torch.empty(nbytes, dtype=torch.uint8, device=dev))
        a = self._app
        for name in ("next", "xytb", "batch_ev"):
            if a[name].shape[0] < self.rows_cap:
                a[name] = torch.zeros((self.rows_cap,) + tuple(a[name].shape[1:]), dtype=a[name].dtype, device=dev)
        a.pop("args", None)                  # the argument block of dagr_async_update is rebuilt for this window
        a["head"].fill_(-1)
        a["status"].zero_()
        a["batch_ev"][:n0] = self._batch.to(torch.int32)
        self._n_rows = n0
        self._async_on = True
        self._pool1_stream(rebuild=True, first=n0, n=0)

    def _pool1_stream(self, rebuild, first, n):
        L, P = self.L, _lib.ptr
        g, a, l1, d = self.graph, self._app, self.levels[0], self.pool_desc[0]
        _lib.check(L.dagr_pool_l0_stream(ctypes.byref(d), P(a["pool_ws"]), 1 if rebuild else 0, ctypes.byref(g.desc),
                                         P(g.workspace), P(self.xlo), P(self.ylo), P(self.hp0), self.hp0.shape[1],
                                         P(self.pos_n), P(a["batch_ev"]), self._N, first, n, P(self.nbr_src),
                                         P(self.nbr_code), P(self.deg), P(l1.x), l1.x.shape[1], 0, P(l1.pos), P(l1.batch),
                                         P(l1.counts), P(l1.rowptr), P(l1.col), P(l1.code),
                                         ctypes.c_void_p(l1.counts.data_ptr() + 4), l1.e_cap,
                                         _lib.cur_stream(self.device)), "pool_l0_stream")

    def _conv_l0_rows(self, pack, first, n, x, ldx, xskip, ldskip, out, ldo):
        L, P = self.L, _lib.ptr
        cin, cskip, w, s = pack
        d0 = self.dom[0]
        wx, tx, wy, ty = self.win0
        cm, ce = self._l0_blocks[cin]
        _lib.check(L.dagr_spline_conv_l0_tiles_rows_w(self.cout0, cm, ce, cskip, wx, tx, wy, ty, d0["rx"], d0["ry"],
                                                      d0["den_x"], d0["den_y"], first, n, self.graph.K, P(self.nbr_src),
                                                      P(self.nbr_code), P(self.deg), x, ldx, xskip, ldskip, P(w), P(s), 1, out,
                                                      ldo, None, _lib.cur_stream(self.device)), "conv_l0_tiles_rows")

    def _async_call(self, a, first, n, pos, feat, batch, stream):
        """Fill / refresh the argument block of ``dagr_async_update`` and issue the update."""
        P = lambda t: None if t is None else t.data_ptr()
        u = a.get("args")
        g, l1, d0 = self.graph, self.levels[0], self.dom[0]
        if u is None or a.get("args_rows_cap") != self.rows_cap:
            u = _lib.AsyncUpdateArgs()
            u.gdesc, u.graph_ws = ctypes.pointer(g.desc), P(g.workspace)
            u.app_head, u.app_next, u.app_xytb = P(a["head"]), P(a["next"]), P(a["xytb"])
            u.capacity = a["next"].shape[0]
            u.nbr_src, u.nbr_code, u.deg, u.status = P(self.nbr_src), P(self.nbr_code), P(self.deg), P(a["status"])
            u.pos_nodes, u.batch_nodes, u.batch_events = P(self.pos_n), P(self.batch_n), P(a["batch_ev"])
            u.x0, u.ldx0, u.col_feat, u.col_pos = P(self.x0buf), self.x0_ld, self.x0_feat_col, self.x0_pos_col
            u.win_x, u.tx, u.win_y, u.ty = self.win0
            u.rx, u.ry, u.den_x, u.den_y = d0["rx"], d0["ry"], d0["den_x"], d0["den_y"]
            cin1, _, w1, s1 = self.l0_conv1
            _, _, w2, s2 = self.l0_conv2
            u.cin1, u.w1, u.s1, u.h1, u.ldh1 = cin1, P(w1), P(s1), P(self.h1), self.cout0
            u.w2, u.s2, u.hp0, u.ldhp0 = P(w2), P(s2), P(self.hp0), self.hp0.shape[1]
            u.pdesc, u.pool_ws, u.xlo, u.ylo = ctypes.pointer(self.pool_desc[0]), P(a["pool_ws"]), P(self.xlo), P(self.ylo)
            u.x_out, u.ldo, u.pos_out, u.batch_out = P(l1.x), l1.x.shape[1], P(l1.pos), P(l1.batch)
            u.n_out, u.rowptr_out, u.col_out, u.code_out = P(l1.counts), P(l1.rowptr), P(l1.col), P(l1.code)
            u.e_out, u.e_cap = l1.counts.data_ptr() + 4, l1.e_cap
            a["args"], a["args_rows_cap"] = u, self.rows_cap
        u.n_static, u.first_id, u.n_new = self._N, first, n
        u.pos, u.feat, u.batch = P(pos), P(feat), P(batch)
        u.batch_is_int64 = 1 if (batch is not None and batch.dtype == torch.int64) else 0
        _lib.check(self.L.dagr_async_update_w(ctypes.byref(u), self.cout0, stream), "async_update")

    def forward_append(self, pos, feat, batch, static_out=False):
        """``reset=False``: the n events of a micro-batch attach to the resident window (EV_TGN.forward, ev_tgn.py:45-56).
        Edges point from older to newer events, so the window's level-0 rows stand; the update
          1. links the events into their pixels' chains and searches their in-edges (dagr_async_graph_append),
          2. computes conv_block1 on the n new rows only (dagr_spline_conv_l0_tiles_rows),
          3. adds the rows to pool1's resident accumulators and re-emits level 1 (dagr_pool_l0_stream),
          4. runs the fixed-size part (levels 1-4, heads, decode) as a window does.
        Output = what ``forward_raw`` gives on all events so far, bit for bit (same kernels per row; order-free
        accumulators).  pos fp32[n,3] normalised as format_data does, feat fp32[n,1], batch int32/int64[n]."""
        if not self.l0_tiles:
            raise NotImplementedError("asynchronous updates run on the tiled level-0 conv (16 neighbours, 3x3/3x5 tap window)")
        L, P = self.L, _lib.ptr
        if not self._async_on:
            self.async_begin()
        n = int(pos.shape[0])
        a = self._app
        first = self._n_rows
        stream = _lib.cur_stream(self.device)
        if n:
            self._grow_rows(first + n)
            a = self._app
            pos = pos.float().contiguous()
            feat = feat.float().reshape(-1).contiguous()
            batch = batch.contiguous()
        if not self.use_image:
            # events-only: graph append + both level-0 convs on the new rows + pool1's resident accumulators as ONE native
            # call (dagr_async_update): same kernels, no host time between their launches
            self._async_call(a, first, n, pos if n else None, feat if n else None, batch if n else None, stream)
            self._n_rows = first + n
        else:
            if n:
                b64 = 1 if batch.dtype == torch.int64 else 0
                g = self.graph
                _lib.check(L.dagr_async_graph_append(ctypes.byref(g.desc), P(g.workspace), self._N, first, P(a["head"]),
                                                     P(a["next"]), P(a["xytb"]), a["next"].shape[0], P(pos), 0, P(batch), b64,
                                                     n, P(self.nbr_src), P(self.nbr_code), P(self.deg), P(a["status"]), P(feat),
                                                     P(self.pos_n), P(self.batch_n), P(a["batch_ev"]), P(self.x0buf),
                                                     self.x0_ld, self.x0_feat_col, self.x0_pos_col, stream),
                           "async_graph_append")
                rows = slice(first, first + n)
                self._sample(None, n, self.pos_n[rows], self.batch_n[rows], 0, self._img_feats[0], self.x0buf[rows],
                             self.x0_img_col)
                c = self.cout0
                self._conv_l0_rows(self.l0_conv1, first, n, P(self.x0buf), self.x0_ld, None, 0, P(self.h1), c)
                self._conv_l0_rows(self.l0_conv2, first, n, P(self.h1), c, P(self.x0buf), self.x0_ld, P(self.hp0),
                                   self.hp0.shape[1])
                self._sample(None, n, self.pos_n[rows], self.batch_n[rows], 0, self._img_feats[1], self.hp0[rows], c)
                self._n_rows = first + n
            self._pool1_stream(rebuild=False, first=first, n=n)
        if self.tail_graph and not self.use_image:
            return self._replay_tail(static_out)
        return self._tail_and_head()

    # ------------------------------------------------------------------------------- kernels
    def _conv_generic(self, lvl, pack, x, ldx, xskip, ldskip, out, ldo, dom, stream, code=None, scratch=None):
        L = self.L
        P = _lib.ptr
        code = lvl.code if code is None else code
        scratch = self.A if scratch is None else scratch
        passes = L.dagr_spline_conv_fused_passes(pack.cin, pack.cskip)
        if passes == 1 or (passes > 1 and lvl.T <= FUSED_PASSES_MAX_NODES):
            # tap aggregation + contraction in one launch (A tile lives in LDS; rows wider than the tile in passes over
            # the edges, which pays on small levels only: tools/microbench/head_ab.hip)
            _lib.check(L.dagr_spline_conv_fused(P(lvl.counts), lvl.T, P(lvl.rowptr), P(lvl.col), P(code), x, ldx,
                                                pack.cin, xskip, ldskip, pack.cskip, dom["rx"], dom["ry"], dom["den_x"],
                                                dom["den_y"], P(pack.Wq), P(pack.bias), out, ldo, pack.N,
                                                1 if pack.relu else 0, stream), "spline_conv_fused")
            return
        lda = (pack.K + 3) // 4 * 4    # 16-byte aligned rows for the MFMA GEMM's float4 loads
        _lib.check(L.dagr_spline_tap_aggregate(P(lvl.counts), lvl.T, P(lvl.rowptr), P(lvl.col), P(code),
                                               x, ldx, pack.cin, xskip, ldskip, pack.cskip, dom["rx"], dom["ry"],
                                               dom["den_x"], dom["den_y"], P(scratch), lda, stream), "tap_aggregate")
        _lib.check(L.dagr_gemm_bias_act(P(lvl.counts), lvl.T, P(scratch), lda, P(pack.Wm), pack.ldw, P(pack.bias),
                                        out, ldo, pack.K, pack.N, 1 if pack.relu else 0, stream), "gemm")

    # -------------------------------------------------------------------------------- stages
    def stage_graph(self, pos, batch, feat=None):
        """events -> neighbour lists (EV_TGN.forward, layers/ev_tgn.py:39-58).  With ``feat`` (the events' features) the
        build's last launch also writes the node-ordered level-0 inputs (``stage_l0_input`` then only samples the image
        features): one launch less per window."""
        N = int(pos.shape[0])
        self._alloc_events(N)
        self._N = N
        self._pos, self._batch = pos, batch
        self._nbr = (self.nbr_src[:N], self.nbr_code[:N], self.deg[:N])
        inputs = None
        if feat is not None and pos.dtype == torch.float32:
            self._feat_flat = feat.float().reshape(-1).contiguous()      # (kept alive until the launch has run)
            inputs = _lib.L0Inputs(feat=self._feat_flat.data_ptr(), pos_nodes=self.pos_n.data_ptr(),
                                   batch_nodes=self.batch_n.data_ptr(), x0=self.x0buf.data_ptr(), ldx0=self.x0_ld,
                                   col_feat=self.x0_feat_col, col_pos=self.x0_pos_col)
        self.graph.build(pos, batch, out=self._nbr, n_dev=self.n_dev if self._dev_mode else None, inputs=inputs)
        self._inputs_gathered = inputs is not None
        self._n_rows = N              # a new window: the asynchronous state of the previous one is gone
        self._async_on = False

    def _nptr(self):
        """``n_ptr`` of the level-0 kernels: the builder's device-side node count inside a captured window, else NULL (the
        host passes the exact count)."""
        return self.graph.node_count_ptr() if self._dev_mode else None

    def _sample(self, n_ptr, n_max, pos, batch, b64, fmap, out, coff):
        """sample_features (net.py:193-221) of one channels-last feature map into out[:, coff:coff+C]."""
        if self._feat_ready is not None:            # pipelined window: the map comes from the image branch's stream
            ready = self._feat_ready.get(id(fmap))
            if ready is None:
                raise RuntimeError("pipelined window: a sampled feature map has no ready-event (the image branch did not "
                                   "announce it) -- reading it would race with the image stream")
            torch.cuda.current_stream(self.device).wait_event(ready)
        Bf, C, h, w = fmap.shape
        nhwc = fmap.permute(0, 2, 3, 1)
        if not nhwc.is_contiguous():
            nhwc = nhwc.contiguous()
        self._keep.append(nhwc)
        _lib.check(self.L.dagr_sample_features(n_ptr, n_max, _lib.ptr(pos), _lib.ptr(batch), b64, _lib.ptr(nhwc), Bf, h,
                                               w, C, self.W, self.H, _lib.ptr(out), out.shape[1], coff,
                                               _lib.cur_stream(self.device)), "sample_features")

    def _fold_image_branch(self):
        """Inference copy of the image branch with every Conv2d+BatchNorm2d(eval) pair folded into one
        conv (torch.nn.utils.fusion.fuse_conv_bn_eval): the BN passes over the 640x480 activations are
        pure HBM traffic.  The stem conv1 stays unfolded: the reference taps its raw output
        (feature_layers=["conv1", ...], net.py:47).  Parameters of the original modules are untouched."""
        import copy
        from torch.nn.utils.fusion import fuse_conv_bn_eval
        bb, head = self.model.backbone, self.model.head
        net = copy.deepcopy(bb.net).eval()
        cnn = copy.deepcopy(head.cnn_head).eval()

        def fold_block(blk):
            for ci, bi in (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3")):
                if hasattr(blk, ci):
                    setattr(blk, ci, fuse_conv_bn_eval(getattr(blk, ci), getattr(blk, bi)))
                    setattr(blk, bi, torch.nn.Identity())
            if blk.downsample is not None:
                blk.downsample = torch.nn.Sequential(fuse_conv_bn_eval(blk.downsample[0], blk.downsample[1]))
        for name in ("layer1", "layer2", "layer3", "layer4"):
            for blk in getattr(net.module, name):
                fold_block(blk)
        for m in cnn.modules():
            if hasattr(m, "conv") and hasattr(m, "bn") and isinstance(m.bn, torch.nn.BatchNorm2d):
                m.conv = fuse_conv_bn_eval(m.conv, m.bn)
                m.bn = torch.nn.Identity()
                if isinstance(getattr(m, "act", None), torch.nn.SiLU) and m.conv.bias is not None:
                    m._bias = m.conv.bias.detach().clone().contiguous()
                    m.conv.bias = None
                    m.forward = types.MethodType(_baseconv_forward, m)
        net = net.to(memory_format=torch.channels_last)
        cnn = cnn.to(memory_format=torch.channels_last)
        for blkname in ("layer1", "layer2", "layer3", "layer4"):
            _gemmify_1x1(getattr(net.module, blkname))
            for blk in getattr(net.module, blkname):
                relu_convs = ("conv1", "conv2") if hasattr(blk, "conv3") else ("conv1",)
                for cname in relu_convs:
                    conv = getattr(blk, cname)
                    if isinstance(conv, _Conv1x1Gemm):
                        conv.relu = True                      # ReLU in the GEMM's epilogue
                    elif isinstance(conv, torch.nn.Conv2d) and conv.bias is not None:
                        setattr(blk, "_" + cname + "_bias", conv.bias.detach().clone().contiguous())
                        conv.bias = None                      # bias + ReLU in one pass after the conv
                        if conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) \
                                and conv.dilation == (1, 1) and conv.groups == 1 \
                                and _split_min_rows(conv.in_channels, conv.out_channels, 9) is not None:
                            # K runs over (tap, channel): row (3 ky + kx) C + c of Wt[9 C, N]
                            conv._split_planes = _split_pack(conv.weight.detach().permute(2, 3, 1, 0).reshape(
                                9 * conv.in_channels, conv.out_channels).contiguous())
                for m in blk.modules():
                    if isinstance(m, _Conv1x1Gemm) and _split_min_rows(m.wt.shape[0], m.wt.shape[1], 1) is not None:
                        m.planes = _split_pack(m.wt)          # the three bf16 planes, once per layer
                blk.forward = types.MethodType(_bottleneck_forward if hasattr(blk, "conv3") else _basicblock_forward,
                                               blk)
        bn = net.module.bn1
        scale = (bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)).contiguous()
        shift = (bn.bias.detach().float() - bn.running_mean.detach().float() * scale).contiguous()
        net.module._stem_affine = (scale, shift)
        net.module.forward_features = types.MethodType(_resnet_features_forward, net.module)
        _gemmify_1x1(net.feature_dconv)
        _gemmify_1x1(net.output_dconv)
        # the dconvs are 1x1 GEMMs like the trunk's: the same rule selects them (feature_dconv[1], 256 -> 64 on the layer1
        # map, is the shape of layer1.1-2.conv1; output_dconv[0], 1024 -> 256 on the layer3 map, that of layer3.1-5.conv1)
        for dconvs in (net.feature_dconv, net.output_dconv):
            for m in dconvs.modules():
                if isinstance(m, _Conv1x1Gemm) and _split_min_rows(m.wt.shape[0], m.wt.shape[1], 1) is not None:
                    m.planes = _split_pack(m.wt)
        self._net_f, self._cnn_f = net, cnn

    def image_branch_paths(self):
        """Which kernel every folded convolution of the ResNet trunk ran in the last image branch: name -> "split" (the
        split-bf16 MFMA kernel) or "library" (hipBLASLt / MIOpen); layers that have not run yet are left out."""
        if self._net_f is None:
            return {}
        out = {}
        for name, m in self._net_f.named_modules():
            path = m.path if isinstance(m, _Conv1x1Gemm) else getattr(m, "_split_path", None)
            if path is not None:
                out[name] = path
        return out

    def _image_branch(self, image, on_feature=None):
        """``on_feature(j, map)``: called when feature map j (feature_layers[j] through its 1x1 dconv) has been issued --
        HookModule.forward (net_img.py:137-145) applies the dconvs after the whole trunk; here each one follows its layer."""
        if self._net_f is None:
            self._fold_image_branch()
        bb, head = types.SimpleNamespace(net=self._net_f), types.SimpleNamespace(cnn_head=self._cnn_f)
        x = image.contiguous(memory_format=torch.channels_last)
        net = self._net_f
        if on_feature is not None:
            feats = [None] * len(net.feature_layers)

            def emit(name, t):
                if name in net.feature_layers:
                    j = net.feature_layers.index(name)
                    feats[j] = net.feature_dconv[j](t) if len(net.feature_dconv) > 0 else t
                    on_feature(j, feats[j])
            d = _resnet_features_forward(net.module, x, emit)
            outs = [d[l] for l in net.output_layers]
            if len(net.output_dconv) > 0:
                outs = [dconv(o) for o, dconv in zip(outs, net.output_dconv)]
        else:
            feats, outs = bb.net(x)
        outs = outs[-self.num_scales:]
        resized = [torch.nn.functional.interpolate(f, o) for f, o in zip(outs, self.out_sizes)]
        return feats, head.cnn_head(resized)

    def stage_image(self, image):
        """HookModule + CNNHead on PyTorch-ROCm (net.py:110, dagr.py:205-206)."""
        self._keep = []
        self._held_for = None
        self._img_feats, self._cnn_out = self._image_branch(image)

    def image_async(self, image, stream=None):
        """Start the image branch of a *future* window batch on a side stream and return a handle for
        ``forward_raw(..., image_handle=h)``.  Windows are independent, and a frame is available before
        the 50 ms of events that follow it, so the dense CNN of batch i+1 can share the GPU with the
        gather-bound event path of batch i."""
        cur = torch.cuda.current_stream(self.device)
        if stream is not None:
            self._img_stream = stream
        if self._img_stream is None:
            self._img_stream = torch.cuda.Stream(self.device)
        s = self._img_stream
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            feats, cnn_out = self._image_branch(image)
            ev = torch.cuda.Event()
            ev.record(s)
        return feats, cnn_out, ev

    def image_handle_from(self, feats, cnn_out):
        """A handle for ``forward_raw(..., image_handle=h)`` / ``forward_detections`` from maps the caller holds (the
        feature maps and CNN-head outputs of an image branch, e.g. clones of ``EventStream.held_maps()``), ready as of the
        current stream."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return list(feats), cnn_out, ev

    def held_maps(self, st):
        """The live ``(feats, cnn_out)`` tensors the stream ``st``'s next held step would read, or None when its next
        step is a frame body (no hold, an invalidated hold, or a frame the branch has not seen yet)."""
        if not self.use_image or self._held_for is not st or st.frame_new:
            return None
        return self._img_feats, self._cnn_out

    def _consume_image_handle(self, handle):
        feats, cnn_out, ev = handle
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        for t in list(feats) + [o for v in cnn_out.values() for o in v]:
            t.record_stream(cur)   # allocated on the side stream, read on this one
        self._keep = []
        self._held_for = None
        self._img_feats, self._cnn_out = feats, cnn_out

    def stage_l0_input(self, feat):
        """Level-0 inputs in node order: x = cat(x, [image feats,] pos[:, :2]) (net.py:118,124-125)."""
        N = self._N
        x0 = self.x0buf[:N]
        g = self.graph
        if not self._inputs_gathered:
            f = feat.float().reshape(-1).contiguous()
            _lib.check(self.L.dagr_graph_gather_inputs(ctypes.byref(g.desc), _lib.ptr(g.workspace), _lib.ptr(self._pos),
                                                       _lib.ptr(f), N, _lib.ptr(self.pos_n), _lib.ptr(self.batch_n),
                                                       _lib.ptr(x0), self.x0_ld, self.x0_feat_col, self.x0_pos_col,
                                                       _lib.cur_stream(self.device)), "graph_gather_inputs")
        if self.use_image:
            self._sample(self._nptr(), N, self.pos_n, self.batch_n, 0, self._img_feats[0], x0, self.x0_img_col)
        self._x0 = x0

    def _conv_l0(self, pack, x, ldx, xskip, ldskip, out, ldo):
        L, P = self.L, _lib.ptr
        nbr_src, nbr_code, deg = self._nbr
        cin, cskip, w, s = pack
        d0 = self.dom[0]
        wx, tx, wy, ty = self.win0
        stream = _lib.cur_stream(self.device)
        if self.l0_tiles:
            cm, ce = self._l0_blocks[cin]
            _lib.check(L.dagr_spline_conv_l0_tiles_w(self.cout0, cm, ce, cskip, wx, tx, wy, ty, d0["rx"], d0["ry"],
                                                     d0["den_x"], d0["den_y"], self._N, self.graph.K, P(nbr_src), P(nbr_code),
                                                     P(deg), x, ldx, xskip, ldskip, P(w), P(s), 1, out, ldo, self._nptr(),
                                                     stream), "conv_l0_tiles")
        else:
            _lib.check(L.dagr_spline_conv_l0(cin, cskip, self.ntaps0, self._N, self.graph.K, self.ncodes0, P(nbr_src),
                                             P(nbr_code), P(deg), x, ldx, xskip, ldskip, P(self.tab0), P(w), P(s), 1,
                                             out, ldo, stream), "conv_l0")

    def stage_l0_conv1(self):
        """conv_block1.conv_block1: SplineConv(3|cout0+3 -> cout0)+BN+ReLU (conv.py:23-28); cout0 = 16 by default."""
        P = _lib.ptr
        assert self.l0_conv1[0] == len(self.x0_cols)
        self._conv_l0(self.l0_conv1, P(self._x0), self.x0_ld, None, 0, P(self.h1), self.cout0)

    def stage_l0_conv2(self, sample=True):
        """conv_block1.conv_block2: SplineConv(cout0->cout0)+BN + skip Linear+BN, ReLU (conv.py:47-56);
        with --use_image followed by sampling_skip(image_feat[1]) (net.py:129)."""
        P = _lib.ptr
        self._conv_l0(self.l0_conv2, P(self.h1), self.cout0, P(self._x0), self.x0_ld, P(self.hp0), self.hp0.shape[1])
        if self.use_image and sample:
            self._sample(self._nptr(), self._N, self.pos_n, self.batch_n, 0, self._img_feats[1], self.hp0[:self._N],
                         self.cout0)

    def stage_l0_sample1(self):
        """sampling_skip(image_feat[1]) (net.py:129) alone: the level-0 nodes' features of the second map into
        hp0[:, cout0:]."""
        self._sample(None, self._N, self.pos_n, self.batch_n, 0, self._img_feats[1], self.hp0[:self._N], self.cout0)

    def stage_pool1(self):
        """pool1 (net.py:131) on the event graph."""
        L, P = self.L, _lib.ptr
        g = self.graph
        nbr_src, nbr_code, deg = self._nbr
        l1 = self.levels[0]
        d = self.pool_desc[0]
        b64 = 1 if self._batch.dtype == torch.int64 else 0
        _lib.check(L.dagr_pool_l0(ctypes.byref(d), P(self.pool_ws[0]), ctypes.byref(g.desc), P(g.workspace),
                                  P(self.xlo), P(self.ylo), P(self.hp0), self.hp0.shape[1], P(self.pos_n),
                                  P(self.batch_n), P(self._batch), b64, self._N, P(nbr_src),
                                  P(nbr_code) if self.fast_coarse_edges else None, P(deg), P(self.cluster0), P(l1.x),
                                  l1.x.shape[1], 0, P(l1.pos), P(l1.batch), P(l1.counts), P(l1.rowptr), P(l1.col),
                                  P(l1.code), ctypes.c_void_p(l1.counts.data_ptr() + 4), l1.e_cap,
                                  _lib.cur_stream(self.device)), "pool_l0")

    def pool1_accumulate_again(self):
        """pool1's accumulation kernel alone on the resident window (measurement: bench.py); follow with ``stage_pool1``."""
        L, P = self.L, _lib.ptr
        g = self.graph
        nbr_src, nbr_code, deg = self._nbr
        _lib.check(L.dagr_pool_l0_accumulate(ctypes.byref(self.pool_desc[0]), P(self.pool_ws[0]), ctypes.byref(g.desc),
                                             P(g.workspace), P(self.xlo), P(self.ylo), P(self.hp0), self.hp0.shape[1],
                                             P(self.pos_n), self._N, P(nbr_src),
                                             P(nbr_code) if self.fast_coarse_edges else None, P(deg),
                                             _lib.cur_stream(self.device)), "pool_l0_accumulate")

    def _stage_level(self, k, trace=None):
        """Layer k+2 on pooled level k+1 (conv pair), then -- for k < 3 -- [sampling_skip] + pool k+2 (net.py:137-184)."""
        L, P = self.L, _lib.ptr
        stream = _lib.cur_stream(self.device)
        lvl = self.levels[k]
        c1, c2 = self.packs[k]
        dom = self.dom[k + 1]
        ldx = lvl.x.shape[1]
        self._conv_generic(lvl, c1, P(lvl.x), ldx, None, 0, P(lvl.h1), c1.N, dom, stream)
        ldh = lvl.hp.shape[1]
        # events-only levels that are pooled next: launch (A) of that pooling (merge of every node into its cluster's
        # accumulators, coarse-edge sets) rides in this conv's epilogue -- one launch less per level
        fuse_pool = (k < 3 and not self.use_image and L.dagr_spline_conv_fused_passes(c2.cin, c2.cskip) == 1
                     and self.pool_desc[k + 1].channels == c2.N)
        self._pool_accumulated[k] = fuse_pool
        if fuse_pool:
            d = self.pool_desc[k + 1]
            _lib.check(L.dagr_spline_conv_fused_pool(P(lvl.counts), lvl.T, P(lvl.rowptr), P(lvl.col), P(lvl.code), P(lvl.h1),
                                                     c1.N, c2.cin, P(lvl.x), ldx, c2.cskip, dom["rx"], dom["ry"],
                                                     dom["den_x"], dom["den_y"], P(c2.Wq), P(c2.bias), P(lvl.hp), ldh, c2.N,
                                                     1 if c2.relu else 0, ctypes.byref(d), P(self.pool_ws[k + 1]), P(lvl.pos),
                                                     P(lvl.batch), P(lvl.cluster), stream), "spline_conv_fused_pool")
        else:
            self._conv_generic(lvl, c2, P(lvl.h1), c1.N, P(lvl.x), ldx, P(lvl.hp), ldh, dom, stream)
        if trace is not None:
            trace[f"pool{k + 1}"] = self._level_snapshot(lvl, lvl.x)
            trace[f"layer{k + 2}"] = self._level_snapshot(lvl, lvl.hp[:, :lvl.cout])

    def _stage_pool(self, k):
        """[sampling_skip(image_feat[k+2])] + pool k+2: level k+1 -> level k+2 (net.py:142-146,155-159,171-175)."""
        L, P = self.L, _lib.ptr
        stream = _lib.cur_stream(self.device)
        lvl, nxt = self.levels[k], self.levels[k + 1]
        ldh = lvl.hp.shape[1]
        if self.use_image:
            self._sample(P(lvl.counts), lvl.T, lvl.pos, lvl.batch, 0, self._img_feats[k + 2], lvl.hp, lvl.cout)
        d = self.pool_desc[k + 1]
        # (n_max = 0: the accumulation already happened in the conv's epilogue -- scan + emit only)
        _lib.check(L.dagr_pool_csr(ctypes.byref(d), P(self.pool_ws[k + 1]), P(lvl.counts),
                                   0 if self._pool_accumulated[k] else lvl.T, P(lvl.hp),
                                   ldh, P(lvl.pos), P(lvl.batch), P(lvl.rowptr), P(lvl.col),
                                   P(lvl.cluster), P(nxt.x), nxt.x.shape[1], 0, P(nxt.pos), P(nxt.batch),
                                   P(nxt.counts), P(nxt.rowptr), P(nxt.col), P(nxt.code),
                                   ctypes.c_void_p(nxt.counts.data_ptr() + 4), nxt.e_cap, stream), "pool_csr")

    def stage_tail(self, trace=None):
        """layer2..layer5 with pool2..pool4 (net.py:137-184)."""
        for k in range(4):
            self._stage_level(k, trace)
            if k < 3:
                self._stage_pool(k)

    def _head_recode(self, i):
        """Edge codes of head scale i's graph in the head convs' own offset domain, when that differs from the level's
        (num_scales = 1: the head's table covers pool3's domain, dagr.py:52-62)."""
        code = self.head_code[i]
        if code is None:
            return
        L, P = self.L, _lib.ptr
        lvln = self.head_levels[i]
        lvl = self.levels[lvln - 1]
        dom = self.head_dom[i]
        rm = dom["remap"]
        _lib.check(L.dagr_pool_recode(P(lvl.counts), lvl.T, P(lvl.rowptr), P(lvl.col), P(lvl.pos),
                                      self.pool_desc[lvln - 1].two_max, float(rm[0, 0]), float(rm[0, 2]),
                                      float(rm[1, 1]), float(rm[1, 2]), dom["rx"], dom["ry"], P(code),
                                      lvl.e_cap, ctypes.c_void_p(self.status.data_ptr() + 4), _lib.cur_stream(self.device)),
                   "pool_recode")

    def _conv_job(self, lvl, pack, x, ldx, xskip, ldskip, out, ldo, dom, code=None):
        """One entry of a multi-job launch: the arguments ``_conv_generic`` would pass (device addresses as ints)."""
        code = lvl.code if code is None else code
        return _lib.ConvJob(n_nodes_ptr=lvl.counts.data_ptr(), n_nodes_max=lvl.T, rowptr=lvl.rowptr.data_ptr(),
                            col=lvl.col.data_ptr(), code=code.data_ptr(), x=x, ldx=ldx, cin=pack.cin, xskip=xskip,
                            ldskip=ldskip, cskip=pack.cskip, rx=dom["rx"], ry=dom["ry"], den_x=dom["den_x"],
                            den_y=dom["den_y"], Wq=pack.Wq.data_ptr(), bias=pack.bias.data_ptr(), C=out, ldc=ldo, N=pack.N,
                            relu=1 if pack.relu else 0)

    def _build_tail_jobs(self):
        """Launch plan of layer5 + both head scales when both exist (net.py:166-186, dagr.py:179-236): head scale 1 needs
        level 3 only, so its convs share the launches of pool4's consumers --
            [layer5.conv1 | stem_1]  [layer5.conv2 | cls_conv,reg_conv_1]  [stem_2 | reg,obj_pred_1 | cls_pred_1]
            [cls_conv,reg_conv_2]  [reg,obj_pred_2 | cls_pred_2]
        five launches where the stream fork ran eight (three of them beside the others, + a fork and a join).  None when
        a conv of the plan needs the pass form (dagr-m / dagr-l heads) or a single scale exists."""
        L = self.L
        if not (len(self.head_levels) == 2 and self.head_levels[0] == 3):
            return None
        c1, c2 = self.packs[3]
        packs = [c1, c2] + [p for hp in self.head_packs for p in hp]
        if any(L.dagr_spline_conv_fused_passes(p.cin, p.cskip) != 1 for p in packs):
            return None
        nr = self.n_reg
        lvl4 = self.levels[3]
        dom4 = self.dom[4]
        ldx4, ldh4 = lvl4.x.shape[1], lvl4.hp.shape[1]
        layer5 = [self._conv_job(lvl4, c1, lvl4.x.data_ptr(), ldx4, None, 0, lvl4.h1.data_ptr(), c1.N, dom4),
                  self._conv_job(lvl4, c2, lvl4.h1.data_ptr(), c1.N, lvl4.x.data_ptr(), ldx4, lvl4.hp.data_ptr(), ldh4, dom4)]
        heads = []
        for i in range(2):
            lvl = self.levels[self.head_levels[i] - 1]
            stem, cr, cls, ro = self.head_packs[i]
            hb, dom, code = self.head_buf[i], self.head_dom[i], self.head_code[i]
            pred = hb["pred"]
            npred = pred.shape[1]
            heads.append([
                [self._conv_job(lvl, stem, lvl.hp.data_ptr(), lvl.hp.shape[1], None, 0, hb["stem"].data_ptr(), nr, dom, code)],
                [self._conv_job(lvl, cr, hb["stem"].data_ptr(), nr, None, 0, hb["cr"].data_ptr(), 2 * nr, dom, code)],
                # pred columns: [reg(4) | obj(1) | cls(num_classes)] = order of collect_outputs (dagr.py:300-302)
                [self._conv_job(lvl, ro, hb["cr"].data_ptr() + 4 * nr, 2 * nr, None, 0, pred.data_ptr(), npred, dom, code),
                 self._conv_job(lvl, cls, hb["cr"].data_ptr(), 2 * nr, None, 0, pred.data_ptr() + 4 * 5, npred, dom, code)]])
        plan = [[layer5[0]] + heads[0][0], [layer5[1]] + heads[0][1], heads[1][0] + heads[0][2], heads[1][1], heads[1][2]]
        return [((_lib.ConvJob * len(jobs))(*jobs), len(jobs)) for jobs in plan]

    def _stage_level5_and_heads(self):
        """layer5 and both head scales by the launch plan of ``_build_tail_jobs``."""
        stream = _lib.cur_stream(self.device)
        self._pool_accumulated[3] = False
        for i in range(2):
            self._head_recode(i)
        for arr, count in self._tail_jobs:
            _lib.check(self.L.dagr_spline_conv_fused_multi(arr, count, stream), "spline_conv_fused_multi")

    def _stage_head_scale(self, i, scratch=None):
        """GNNHead.process_feature of scale i (dagr.py:179-190): stem, cls_conv | reg_conv (one launch, shared input),
        then reg_pred | obj_pred on the reg half and cls_pred on the cls half of that row as the two jobs of ONE paired
        launch (dagr_spline_conv_fused_pair) -> the scale's predictor rows."""
        L, P = self.L, _lib.ptr
        stream = _lib.cur_stream(self.device)
        lvln = self.head_levels[i]
        lvl = self.levels[lvln - 1]
        stem, cr, cls, ro = self.head_packs[i]
        hb = self.head_buf[i]
        dom = self.head_dom[i]
        code = self.head_code[i]
        self._head_recode(i)
        nr = self.n_reg
        self._conv_generic(lvl, stem, P(lvl.hp), lvl.hp.shape[1], None, 0, P(hb["stem"]), nr, dom, stream, code, scratch)
        self._conv_generic(lvl, cr, P(hb["stem"]), nr, None, 0, P(hb["cr"]), 2 * nr, dom, stream, code, scratch)
        pred = hb["pred"]
        npred = pred.shape[1]
        # pred columns: [reg(4) | obj(1) | cls(num_classes)] = order of collect_outputs (dagr.py:300-302)
        x_reg, x_cls = ctypes.c_void_p(hb["cr"].data_ptr() + 4 * nr), P(hb["cr"])
        o_reg, o_cls = P(pred), ctypes.c_void_p(pred.data_ptr() + 4 * 5)
        if L.dagr_spline_conv_fused_passes(ro.cin, 0) >= 1 and \
                (L.dagr_spline_conv_fused_passes(ro.cin, 0) == 1 or lvl.T <= FUSED_PASSES_MAX_NODES):
            kcode = lvl.code if code is None else code
            _lib.check(L.dagr_spline_conv_fused_pair(P(lvl.counts), lvl.T, P(lvl.rowptr), P(lvl.col), P(kcode), 2 * nr, ro.cin,
                                                     dom["rx"], dom["ry"], dom["den_x"], dom["den_y"], npred, 0, x_reg,
                                                     P(ro.Wq), P(ro.bias), o_reg, ro.N, x_cls, P(cls.Wq), P(cls.bias), o_cls,
                                                     cls.N, stream), "spline_conv_fused_pair")
        else:
            self._conv_generic(lvl, ro, x_reg, 2 * nr, None, 0, o_reg, npred, dom, stream, code, scratch)
            self._conv_generic(lvl, cls, x_cls, 2 * nr, None, 0, o_cls, npred, dom, stream, code, scratch)
        return pred

    def _heads_finish(self):
        """to_dense of every scale (spline_conv.py:80-107) + the CNN head's logits (dagr.py:219-222,230-234) +
        collect_outputs / decode_outputs (dagr.py:283-312): one launch (dagr_heads_finish).  The fused logit maps land in
        ``head_buf[i]["dense"]`` as a by-product (traces, tests)."""
        P = _lib.ptr
        if self._cnn_ready is not None:             # pipelined window: the CNN head ran beside the graph levels
            torch.cuda.current_stream(self.device).wait_event(self._cnn_ready)
            self._cnn_ready = None
            self._feat_ready = None
        scales = []
        for i, lvln in enumerate(self.head_levels):
            lvl, hb = self.levels[lvln - 1], self.head_buf[i]
            Hc, Wc = self.out_sizes[i]
            vox = self.head_vox[i]
            hs = _lib.HeadScale(n_ptr=lvl.counts.data_ptr(), n_max=lvl.T, pred=hb["pred"].data_ptr(), ld=hb["pred"].shape[1],
                                pos=lvl.pos.data_ptr(), batch=lvl.batch.data_ptr(), vx=float(vox[0]), vy=float(vox[1]),
                                stride=float(self.strides[i]), Hc=int(Hc), Wc=int(Wc), dense=hb["dense"].data_ptr())
            if self._cnn_out is not None:
                for k, name in enumerate(("reg_output", "obj_output", "cls_output")):
                    t = self._cnn_out[name][i]
                    hs.cnn[k] = t.data_ptr()
                    for j in range(4):
                        hs.cnn_stride[k][j] = int(t.stride(j))
            scales.append(hs)
        A = sum(int(h) * int(w) for h, w in self.out_sizes)
        CH = 5 + self.num_classes
        out = torch.empty((self.B, A, CH), dtype=torch.float32, device=self.device)
        s0, s1 = ctypes.byref(scales[0]), ctypes.byref(scales[1]) if len(scales) > 1 else None
        if self._post_key is not None:
            # a caller wants detections (forward_detections): every image's post-processing runs inside the same launch,
            # right behind its decode (dagr_heads_finish_detect) -- fresh buffers per call (inside a capture they belong
            # to the graph and are remembered with it)
            self._det = torch.empty((self.B, A, 6), dtype=torch.float32, device=self.device)
            self._n_keep = torch.empty((self.B,), dtype=torch.int32, device=self.device)
            conf, nms = self._post_key
            _lib.check(self.L.dagr_heads_finish_detect(s0, s1, self.B, CH, P(out), P(self.status), conf, nms,
                                                       float(max(self.W, self.H) + 1), P(self._det), P(self._n_keep),
                                                       _lib.cur_stream(self.device)), "heads_finish_detect")
            self._post_fresh = True
        else:
            _lib.check(self.L.dagr_heads_finish(s0, s1, self.B, CH, P(out), P(self.status), _lib.cur_stream(self.device)),
                       "heads_finish")
        self._fused_dense = [hb["dense"] for hb in self.head_buf]
        return out

    def stage_head(self):
        """GNNHead.process_feature per scale, then to_dense + fusion + decode in one launch (dagr.py:179-236,283-312)."""
        for i in range(len(self.head_levels)):
            self._stage_head_scale(i)
        return self._heads_finish()

    def _tail_and_head(self, trace=None):
        """Levels 1..4 and both head scales with the dependency structure the graph has: head scale 1 only needs level 3
        (out3), so it runs on a side stream next to pool4 -> layer5 -> head scale 2 (net.py:166-186, dagr.py:213-236);
        then to_dense + image-logit fusion + decode of both scales in one launch.  Returns the decoded outputs."""
        first = self.head_levels[0]                  # 3 when both scales exist, 4 with num_scales = 1
        if trace is None:
            if self._tail_jobs is None:
                self._tail_jobs = self._build_tail_jobs() or False
            if self._tail_jobs:
                for k in range(3):
                    self._stage_level(k)
                    self._stage_pool(k)
                self._stage_level5_and_heads()
                return self._heads_finish()
        done = [False] * len(self.head_levels)
        cur = torch.cuda.current_stream(self.device)
        forked = False
        for k in range(4):
            self._stage_level(k, trace)
            if k + 1 == first and first == 3 and trace is None and self.overlap_heads:
                if self._head_stream is None:
                    self._head_stream = torch.cuda.Stream(self.device)
                ev = torch.cuda.Event()
                ev.record(cur)
                self._head_stream.wait_event(ev)
                with torch.cuda.stream(self._head_stream):
                    self._stage_head_scale(0, scratch=self.A2)
                    done[0] = True
                    self._head_join = torch.cuda.Event()
                    self._head_join.record(self._head_stream)
                forked = True
            if k < 3:
                self._stage_pool(k)
        for i in range(len(self.head_levels)):
            if not done[i]:
                self._stage_head_scale(i)
        if forked:
            cur.wait_event(self._head_join)
        return self._heads_finish()

    def _post_launch(self, out):
        """``postprocess_network_output`` (model/utils.py:61-110; dagr.py:94-95) of the decoded outputs for the paths that do
        not end in ``_heads_finish`` (``--no_events``: the image branch's own maps); everywhere else the heads' launch has
        already run it (dagr_heads_finish_detect).  Only when a caller asked for detections (forward_detections)."""
        if self._post_key is None or self._post_fresh:     # (nobody asked / the heads' own launch already did it)
            return
        B, A, C = out.shape
        self._det = torch.empty((B, A, 6), dtype=torch.float32, device=self.device)
        self._n_keep = torch.empty((B,), dtype=torch.int32, device=self.device)
        conf, nms = self._post_key
        _lib.check(self.L.dagr_postprocess(_lib.ptr(out), B, A, int(self.num_classes), conf, nms,
                                           float(max(self.W, self.H) + 1), _lib.ptr(self._det), _lib.ptr(self._n_keep),
                                           _lib.cur_stream(self.device)), "postprocess")
        self._post_fresh = True

    def forward_detections(self, pos, feat, batch, image=None, append=False, image_handle=None):
        """One window (``append``: one asynchronous update) through forward + post-processing: ``(det[B, A, 6], n_keep[B])``
        as ``model.utils.postprocess_device`` returns them, valid until the engine's next call.  In latency mode the
        post-processing is part of the captured graph: no launch, and no host time, between the heads and the NMS.
        ``image_handle``: as ``forward_raw`` takes it (the window then runs launch by launch)."""
        from .model.utils import postprocess_device
        key = (float(self.model.conf_threshold), float(self.model.nms_threshold))
        if key != self._post_key:                   # (re)capture with these thresholds
            self._post_key = key
            self._drop_window_graph()
            self._graph = None
            self._graph_warm = 0
        self._post_fresh = False
        if append:
            out = self.forward_append(pos, feat, batch, static_out=True)
        else:
            out = self.forward_raw(pos, feat, batch, image=image, image_handle=image_handle, static_out=True)
        if self._post_fresh:
            return self._det, self._n_keep
        return postprocess_device(out, self.num_classes, key[0], key[1], self.H, self.W)

    def forward_raw(self, pos, feat, batch, image=None, trace=None, image_handle=None, static_out=False):
        """pos fp32[N,3] normalised (format_data), feat fp32[N,1], batch int32/int64[N] on the device;
        image fp32[B,3,H,W] in [0,1] when the model was built with --use_image.
        Returns decoded head outputs [B, n_anchors, 5+num_classes] (GNNHead.forward eval).
        ``static_out``: the caller consumes the outputs before the engine's next window (``DAGR.forward`` post-processes
        them at once), so a captured window may hand out its own output buffer instead of a copy."""
        if trace is None and image_handle is None and self.window_graph and self.l0_tiles and not self.no_events \
                and (image is not None or not self.use_image):
            return self._forward_window_graph(pos, feat, batch, image, static_out)
        self._cnn_out = None
        if self.use_image:
            if image_handle is not None:
                self._consume_image_handle(image_handle)
            elif image is None:
                raise RuntimeError("model was built with --use_image: an image batch is required")
            else:
                self.stage_image(image)
        if self.no_events:
            # GNNHead.forward eval, dagr.py:283-284: the image branch's own outputs (dagr.py:207-212); the reference
            # still runs the event path and throws its maps away -- here it is skipped
            c = self._cnn_out
            return self._decode_maps([torch.cat([c["reg_output"][k], c["obj_output"][k], c["cls_output"][k]], 1)
                                      for k in range(self.num_scales)])
        self.stage_graph(pos.contiguous(), batch.contiguous(), feat)
        self.stage_l0_input(feat)
        self.stage_l0_conv1()
        self.stage_l0_conv2()
        if trace is not None:
            trace["nbr"] = tuple(t.clone() for t in self._nbr)
            _, ev_slot = self.graph.node_order(self._N)     # traces are reported in event order
            ev_slot = ev_slot.long()
            trace["layer1"] = self.hp0[:self._N, :self.cout0][ev_slot].clone()
            if self.use_image:
                back = [self.x0_cols.index(k) for k in range(len(self.x0_cols))]   # reference channel order
                trace["x0"] = self._x0[ev_slot][:, back].clone()
        self.stage_pool1()
        if trace is None and self.tail_graph and not self.use_image:
            return self._replay_tail(static_out)
        out = self._tail_and_head(trace)
        if trace is not None:
            trace["head_dense"] = [o.clone() for o in self._fused_dense]
        return out

    def _forward_static(self, held=False):
        """One window on the engine's static input buffers with every launch sized for the event capacity and bounded by
        the device-side counts: the body of the captured window graph (and of its eager warm-up runs).

        ``held`` (``--use_image``): the held body -- the same launch sequence without the fork for the image branch.
        Every ``_sample`` call and ``_heads_finish`` read the feature maps and CNN-head outputs the last frame body left
        in ``_img_feats`` / ``_cnn_out``; it waits on none of that body's events (they belong to another capture, and
        replays on one stream are ordered)."""
        self._dev_mode = True
        try:
            if held:
                self._feat_ready = self._cnn_ready = None
                self.stage_graph(self.in_pos, self.in_batch, self.in_feat)
            elif self.use_image:
                self._held_for = None                 # the maps are rewritten: whoever runs this body takes the hold anew
                self._cnn_out = None
                # the graph build needs nothing from the frame: it runs beside the image branch (a fork inside the captured
                # window; the level-0 input rows are the first stage that needs both)
                cur = torch.cuda.current_stream(self.device)
                if self._head_stream is None:
                    self._head_stream = torch.cuda.Stream(self.device)
                fork = torch.cuda.Event()
                fork.record(cur)
                self._head_stream.wait_event(fork)
                with torch.cuda.stream(self._head_stream):
                    self.stage_graph(self.in_pos, self.in_batch, self.in_feat)
                    join = torch.cuda.Event()
                    join.record(self._head_stream)
                # The graph levels do not wait for the whole image branch: level k samples feature map k (+ 1), which
                # exists as soon as ResNet stage k has run (net.py:110-184: the reference calls the CNN first, but its
                # outputs are consumed level by level).  The branch gets a stream of its own and records an event per
                # map; a B = 1 window is two chains of small dependent kernels, and the shorter one (the graph levels,
                # ~0.4 ms) now runs UNDER the longer one (the CNN, ~1.3 ms) instead of after it.
                if self._img_stream is None:
                    self._img_stream = torch.cuda.Stream(self.device)
                s_img = self._img_stream
                s_img.wait_event(fork)
                self._feat_ready = {}
                self._keep = []
                with torch.cuda.stream(s_img):
                    def on_feature(j, fmap):
                        ev = torch.cuda.Event()
                        ev.record(s_img)
                        self._feat_ready[id(fmap)] = ev
                        fmap.record_stream(cur)
                    self._img_feats, self._cnn_out = self._image_branch(self.in_image, on_feature)
                    for v in self._cnn_out.values():
                        for o in v:
                            o.record_stream(cur)
                    self._cnn_ready = torch.cuda.Event()
                    self._cnn_ready.record(s_img)
                cur.wait_event(join)
            else:
                self._cnn_out = None
                self.stage_graph(self.in_pos, self.in_batch, self.in_feat)
            self.stage_l0_input(self.in_feat)
            self.stage_l0_conv1()
            self.stage_l0_conv2()
            self.stage_pool1()
            out = self._tail_and_head()
            self._post_launch(out)
            return out
        finally:
            self._dev_mode = False

    def _capture_window(self):
        """Capture the frame body (the full window) as ``_wg`` and replay it once; the feature maps and CNN-head outputs its
        capture allocated stay referenced for as long as either captured body lives (the held body reads them)."""
        cg = torch.cuda.CUDAGraph()
        with _capture(cg):
            out = self._forward_static()
        self._wg, self._wg_out, self._wg_post = cg, out, (self._det, self._n_keep)
        self._wg_maps = (self._img_feats, self._cnn_out) if self.use_image else None
        cg.replay()
        return out

    def _replay_window(self):
        """Replay the captured frame body: its outputs, its post-processing buffers and (``--use_image``) its maps are the
        engine's current ones again."""
        self._wg.replay()
        self._det, self._n_keep = self._wg_post
        if self._wg_maps is not None:
            self._img_feats, self._cnn_out = self._wg_maps
        return self._wg_out

    def _held_window(self):
        """The held body in latency mode: a second captured graph beside ``_wg``, on the maps ``_wg``'s capture allocated
        and with output and post-processing buffers of its own.  It is captured only while ``_wg`` exists (after one eager
        run, as every capture here); until then -- the frame body's own warm-up runs -- the held body runs launch by
        launch on the maps the last eager frame body left."""
        if self._wg is None or self._wg_maps is None or self._img_feats is not self._wg_maps[0]:
            return self._forward_static(held=True)
        if self._hg is None:
            if self._hg_warm < 1:
                self._hg_warm += 1
                return self._forward_static(held=True)
            cg = torch.cuda.CUDAGraph()
            with _capture(cg):
                out = self._forward_static(held=True)
            self._hg, self._hg_out, self._hg_post = cg, out, (self._det, self._n_keep)
            cg.replay()
            return out
        self._hg.replay()
        self._det, self._n_keep = self._hg_post
        self._post_fresh = True
        return self._hg_out

    def _forward_window_graph(self, pos, feat, batch, image, static_out=False):
        """Latency mode: the caller's window is staged into the static buffers by ONE launch (which also writes the event
        count to device memory); everything else -- image branch, graph build, level 0, pooled levels, heads, decode: ~45
        launches events-only, several hundred with the ResNet-50 branch -- is one replayed HIP graph.  Until round 4 only the
        part after pool1 was captured and the image model not at all (the host issued every MIOpen launch of a window)."""
        L, P = self.L, _lib.ptr
        N = int(pos.shape[0])
        if N > self.max_events:
            self._alloc_events(max(N, 2 * self.max_events))
        pos = pos.float().contiguous()
        feat = feat.float().reshape(-1).contiguous()
        batch = batch.contiguous()
        g = self.graph
        _lib.check(L.dagr_stage_window(ctypes.byref(g.desc), P(g.workspace), P(pos), P(feat), P(batch),
                                       1 if batch.dtype == torch.int64 else 0, N, P(self.in_pos), P(self.in_feat),
                                       P(self.in_batch), P(self.n_dev), _lib.cur_stream(self.device)), "stage_window")
        self._held_for = None                        # this window's frame body rewrites the maps a stream may hold
        if self.use_image:
            if self.in_image is None or self.in_image.shape != image.shape:
                self.in_image = torch.empty(tuple(image.shape), dtype=torch.float32, device=self.device)
                self._drop_window_graph()
            self.in_image.copy_(image)
        if self._wg is None:
            if self._wg_warm < 2:                    # lazy one-time work (kernel attributes, MIOpen's search) stays eager
                self._wg_warm += 1
                out = self._forward_static()
            else:
                out = self._capture_window()
        else:
            out = self._replay_window()
            self._post_fresh = self._post_key is not None
        # the resident window (what check_status / an asynchronous update / the probes look at): the actual count
        self._N = N
        self._n_rows = N
        self._async_on = False
        self._pos, self._batch = self.in_pos[:N], self.in_batch[:N]
        self._nbr = (self.nbr_src[:N], self.nbr_code[:N], self.deg[:N])
        self._x0 = self.x0buf[:N]
        return out if static_out else out.clone()   # the graph's output buffer is rewritten by the next window

    def forward_stream(self, st, xy, t, p, batch, t_now=None, image=None, words=None, word_end=None):
        """One step of an event stream (``StreamState`` ``st``): ``_forward_window_graph`` with ``dagr_stream_stage`` in
        place of ``dagr_stage_window``.  The new raw events (``xy`` int16[n,2], ``t`` int64[n] absolute us, ``p`` int8[n],
        ``batch`` int32/int64[n] sorted lanes, ``t_now`` int64[B] or None; all on the device) join the window kept in
        ``st``; two launches write the next window into the static input buffers and its count to device memory, and
        the window runs on them -- the captured graph in latency mode, the same body launch by launch otherwise.  No host
        synchronisation: the host knows an upper bound of the window's size only (``st.bound()``), which is what the
        buffers are sized by.
        The push passes through the stages the stream has enabled, in this order: the decoder (``st.words``; the push is
        then ``words``, the camera's words as int16 / int32 bit patterns, and ``word_end`` int64 [B], the cumulative end of
        every lane's run, in place of the events), the flicker / trail filters (``st.flick``), the noise filter
        (``st.noise``) and the downsampling front (``st.front``).  Each takes ALL rows handed on -- those behind the count
        of the stage in front are lane-less -- and leaves its survivors and their count on the device.  The staging entry
        follows from the chain: ``dagr_stream_stage_dev_clock`` behind the decoder (the decoded push and its device-side
        count are the clock), ``dagr_stream_stage_dev`` behind any other stage (the push itself is the clock),
        ``dagr_stream_stage`` with none; ``_capped`` with ``st.max_lane_events = N``, whose windows never exceed ``B * N``,
        which the buffers meet once -- no growth and no re-capture after the first step.  The host's bound of a decoding
        stream grows by ``st.decode_rows(n_words)`` per step, so one that is never read back should be capped.
        A tracking stream (``st.track``) ends the step with ``dagr_stream_track`` on the step's detections and the reference
        instants the staging left: one plain launch on the same stream, outside the captured graphs, so every mode and
        body is covered without a re-capture; ``st.track_ids`` / ``st.track_hits`` hold the result.  With a motion model
        (``st.motion``) that launch is ``dagr_stream_track_cv``, which also leaves ``st.track_boxes`` / ``st.track_vel`` and the
        coast lists.  A drawing stream with trails (``st.trail_rings``) makes one more plain launch right behind it,
        ``dagr_stream_trail``.
        Returns ``(out, (det, n_keep))``, both valid until the engine's next call.

        ``--use_image``: the window has two bodies.  The frame body runs the image branch on the stream's frame
        (``st.image``; ``image=`` replaces it) and leaves its feature maps and CNN-head outputs; the held body samples
        those and skips the branch.  A step runs the held body only if the stream has had no new frame since its last
        frame body and nothing has rewritten the maps since (``_held_for``); ``st.frame_steps`` / ``st.held_steps`` count
        the bodies.  Either way the step returns what ``reset=True`` gives on the window with the frame in force."""
        from .model.utils import postprocess_device
        if not self.l0_tiles or self.no_events:
            raise RuntimeError("forward_stream runs the captured window's body: it needs the tiled level-0 conv "
                               "(l0_tiles) and the event path (no --no_events)")
        L, P = self.L, _lib.ptr
        decoding = st.words is not None
        if decoding != (words is not None):
            raise RuntimeError("forward_stream: a decoding stream takes words= / word_end=, any other stream events")
        # a decoding stream: the rows the decoder writes, of which the device alone knows how many are events
        n_new = st.decode_rows(int(words.shape[0])) if decoding else int(t.shape[0])
        N = st.max_lane_events
        if N is None:
            need = max(st.bound() + n_new, st.cap)   # (a stream that grew on another engine keeps its capacity)
            if need > self.max_events:
                self._alloc_events(max(need, 2 * self.max_events))   # (re-captures, as a large window does)
        else:       # a capped stream: no window exceeds B * N, whatever is pushed -- a constant, met on the first step
            need = max(self.B * N, st.cap)
            if need > self.max_events:
                self._alloc_events(need)
        if st.state is None or need > st.cap:
            st.grow(self.max_events)
        if self.use_image:
            if image is not None:
                st.image = image.to(device=self.device, dtype=torch.float32).clone()
                st.frame_new = True                  # (contents are not compared)
            if st.image is None:
                raise RuntimeError("model was built with --use_image: the stream needs a frame (image= or frame=) on its "
                                   "first step")
            if self.in_image is None or self.in_image.shape != st.image.shape:
                self.in_image = torch.empty(tuple(st.image.shape), dtype=torch.float32, device=self.device)
                self._drop_window_graph()
        key = (float(self.model.conf_threshold), float(self.model.nms_threshold))
        if key != self._post_key:                   # (re)capture with these thresholds
            self._post_key = key
            self._drop_window_graph()
            self._graph = None
            self._graph_warm = 0
        self._post_fresh = False
        # Which body this step runs: the held body if and only if the stream has had no new frame since its last frame body
        # AND nothing has rewritten or replaced the maps since (_held_for: cleared by every other frame body, capture,
        # re-allocation and threshold change).  In doubt the frame body runs: that is only a needless image branch.
        held = self.use_image and self._held_for is st and not st.frame_new
        if self.use_image and not held:
            self.in_image.copy_(st.image)
        g = self.graph
        outputs = (P(self.in_pos), P(self.in_feat), P(self.in_batch), P(self.n_dev), P(st.lane_count), P(st.status),
                   _lib.cur_stream(self.device))
        cap_args = () if N is None else (N, P(st.lane_dropped))
        # every stage sees the same sensor: the front's, or without one the engine's
        sensor = (self.W, self.H) if st.front is None else st.front[2:4]
        filters = [f for f in (st.flick, st.noise) if f is not None]
        if decoding and any(s[:2] != sensor for s in (st.words[1:3], *filters)):
            raise RuntimeError(f"the stream decodes a {st.words[1]} x {st.words[2]} sensor, its fronts take "
                               f"{sensor[0]} x {sensor[1]} pixels")
        for filt in () if decoding else filters:
            if filt[:2] != sensor:
                raise RuntimeError(f"the stream filters a {filt[0]} x {filt[1]} sensor, its pushes carry "
                                   f"{sensor[0]} x {sensor[1]} pixels")
        if st.front is not None and st.front[4:] != (self.W, self.H):
            raise RuntimeError(f"the stream downsamples to {st.front[4]} x {st.front[5]}, the engine runs {self.W} x {self.H}")
        # the source rows, which are also the clock: the decoded push with its count on the device, or the push itself
        source = st.decode(words, word_end) if decoding else (xy, t, p, batch, None)
        rows = int(source[1].shape[0])
        if decoding:
            clock = (P(source[1]), P(source[3]), 0, P(source[4]), rows)
        else:
            clock = (P(t), P(batch), 1 if batch.dtype == torch.int64 else 0, rows)
        # flicker / trail in front of the noise filter (flicker would support noise there), the front last; each on all rows,
        # of which those behind the count of the stage in front are lane-less: they meet no state and integrate nowhere
        last = source
        for name in ("flick", "noise", "front"):
            if name in st.stages:
                last = st._push(name, *last[:4], n=rows)
        if decoding or last is not source:      # the survivors and their count are on the device (a cap counts survivors)
            kind = "stream_stage_dev_clock" if decoding else "stream_stage_dev"
            push = (*(P(v) for v in last), rows, *clock)
        else:
            kind, push = "stream_stage", (P(xy), P(t), P(p), P(batch), *clock[2:])
        stage = getattr(L, "dagr_" + kind + ("" if N is None else "_capped"))
        _lib.check(stage(ctypes.byref(g.desc), P(g.workspace), P(st.state), self.B, st.cap, *push, P(t_now), st.window_us,
                         *cap_args, *outputs), kind)
        if not self.window_graph:                    # throughput mode: the body of the captured window, launch by launch
            out = self._forward_static(held)
        elif held:
            out = self._held_window()
        elif self._wg is None:
            if self._wg_warm < 2:
                self._wg_warm += 1
                out = self._forward_static()
            else:
                out = self._capture_window()
        else:
            out = self._replay_window()
            self._post_fresh = True
        if held:
            st.held_steps += 1
        else:
            st.frame_steps += 1
            if self.use_image:                       # the maps are this stream's frame now
                self._held_for, st.frame_new = st, False
        st._pushed_now(n_new)
        # the resident window is this step's, but its size is on the device: nothing may attach to it (can_append) until
        # the count has been read (stream_counted)
        self._N = self._n_rows = 0
        self._async_on = False
        self._pos = self._batch = None
        self._stream_pending = st
        det = (self._det, self._n_keep) if self._post_fresh else \
            postprocess_device(out, self.num_classes, key[0], key[1], self.H, self.W)
        st.stepped()
        if st.track is not None:                     # a plain launch behind the window, captured or not: the track ids
            st.run_track(*det)
        if st.map is not None:                       # logged on request (run_map_log): a step launches nothing for it
            st._map_det, st._mapped = det, False
        if st.render is not None:                    # the picture is made on request (run_render); the trails follow every step
            st._render_det = det
            if st.trail_rings is not None:
                st.run_trail()
        return out, det

    def stream_counted(self, st):
        """The stream has been drained (the detections' read-back): take the last step's counts, and if that step is still
        the engine's resident window, describe it as ``_forward_window_graph`` describes a caller's."""
        st.read_counts()
        if self._stream_pending is st and self._pos is None and st.counts_known() is not None:
            N = int(st.counts_known().sum())
            self._N = self._n_rows = N
            self._pos, self._batch = self.in_pos[:N], self.in_batch[:N]
            self._nbr = (self.nbr_src[:N], self.nbr_code[:N], self.deg[:N])
            self._x0 = self.x0buf[:N]
        self._stream_pending = None

    def _replay_tail(self, static_out=False):
        """Everything after pool1 has launch shapes that do not depend on the window (node / edge counts stay on the
        device): ~70 small dependent launches, captured once as a HIP graph and replayed -- the host then issues ONE
        launch for them, which is what bounds single-window latency at small N.  (Events-only: with --use_image the tail
        samples this window's freshly allocated feature maps.)"""
        if self._graph is None:
            if self._graph_warm < 2:                 # lazy one-time work (function attributes, allocator) stays eager
                self._graph_warm += 1
                out = self._tail_and_head()
                self._post_launch(out)
                return out
            g = torch.cuda.CUDAGraph()
            with _capture(g):
                out = self._tail_and_head()
                self._post_launch(out)
            self._graph, self._graph_out, self._graph_post = g, out, (self._det, self._n_keep)
        self._graph.replay()
        self._det, self._n_keep = self._graph_post
        self._post_fresh = self._post_key is not None
        return self._graph_out if static_out else self._graph_out.clone()   # rewritten by the next window

    def _decode_maps(self, dense_maps):
        """collect_outputs + decode_outputs (dagr.py:283-312) in one launch (dagr_decode_heads)."""
        P = _lib.ptr
        d = [m.contiguous() for m in dense_maps]
        self._keep_maps = d
        CH = d[0].shape[1]
        A = sum(m.shape[2] * m.shape[3] for m in d)
        out = torch.empty((self.B, A, CH), dtype=torch.float32, device=self.device)
        second = d[1] if len(d) > 1 else None
        _lib.check(self.L.dagr_decode_heads(P(d[0]), d[0].shape[2], d[0].shape[3], float(self.strides[0]), P(second),
                                            second.shape[2] if second is not None else 0,
                                            second.shape[3] if second is not None else 0,
                                            float(self.strides[1]) if second is not None else 0.0, self.B, CH, P(out),
                                            _lib.cur_stream(self.device)), "decode_heads")
        return out

    def _level_snapshot(self, lvl, x):
        n, e = [int(v) for v in lvl.counts.tolist()]
        return dict(x=x[:n].clone(), pos=lvl.pos[:n].clone(), batch=lvl.batch[:n].clone(),
                    rowptr=lvl.rowptr[:n + 1].clone(), col=lvl.col[:e].clone(), code=lvl.code[:e].clone())

    def l0_kernel_names(self):
        """Kernel (as rocprofv3 prints it) behind each level-0 conv stage, for bench.py's roofline line."""
        c0 = 3 + self.feat_ch[0]
        nt = self.ntaps0
        if self.l0_tiles:
            tx, ty = self.win0[1], self.win0[3]
            cm, ce = _l0_block(c0)
            c = self.cout0
            if c != 16:     # the other widths are instantiations of the width-parametrised template
                return {"l0_conv1": f"k_conv_l0_tiles_w<{c}, {cm}, {ce}, 0, {tx}, {ty}>",
                        "l0_conv2": f"k_conv_l0_tiles_w<{c}, {c}, 0, {c0}, {tx}, {ty}>"}
            return {"l0_conv1": f"k_conv_l0_tiles<{cm}, {c0 - cm}, 0, {tx}, {ty}>",
                    "l0_conv2": f"k_conv_l0_tiles<16, 0, {c0}, {tx}, {ty}>"}
        return {"l0_conv1": f"k_conv_l0<{c0}, 0, {nt}>", "l0_conv2": f"k_conv_l0<16, {c0}, {nt}>"}

    def check_status(self):
        """Raise if any kernel flagged an inconsistency (synchronises)."""
        ne, fl = self.graph.status()
        if fl:
            raise RuntimeError(f"graph builder flagged {fl:#x} (events outside the sensor / batch range)")
        for k, (d, ws) in enumerate(zip(self.pool_desc, self.pool_ws)):
            f = ctypes.c_int32(0)
            _lib.check(self.L.dagr_pool_status(ctypes.byref(d), _lib.ptr(ws), ctypes.byref(f),
                                               _lib.cur_stream(self.device)), "pool_status")
            if f.value:
                raise RuntimeError(f"pool{k + 1} flagged {f.value:#x}")
        if self._async_on:
            if int(self._app["status"][0]):
                raise RuntimeError("asynchronous update: event outside the sensor / batch range")
            f = ctypes.c_int32(0)
            _lib.check(self.L.dagr_pool_status(ctypes.byref(self.pool_desc[0]), _lib.ptr(self._app["pool_ws"]),
                                               ctypes.byref(f), _lib.cur_stream(self.device)), "pool_status")
            if f.value:
                raise RuntimeError(f"pool1 (asynchronous accumulators) flagged {f.value:#x}")
        st = self.status.tolist()
        if st[0]:
            raise RuntimeError("to_dense: node outside the output map")
        if st[1]:
            raise RuntimeError("head: LUT coordinate outside the head's table (dagr_pool_recode)")

    def check_batch(self, data):
        """Host-side validation of a batch against the engine's constants (no device read-back)."""
        ng = getattr(data, "num_graphs", None)
        if ng is not None and int(ng) > self.B:
            raise RuntimeError(f"batch of {int(ng)} windows, but the model was built with batch_size = {self.B}")
        geo = getattr(data, "_geometry", None)          # python ints stashed by the collation (data/__init__.py)
        for k, (name, want) in enumerate((("width", self.W), ("height", self.H), ("time_window", self.time_window))):
            v = geo[k] if geo is not None else getattr(data, name, None)
            if v is not None and not (torch.is_tensor(v) and v.is_cuda):   # no device read-back on the hot path
                v = int(v[0]) if hasattr(v, "__len__") else int(v)
                if v != want:
                    raise RuntimeError(f"data.{name} = {v}, but the model was built for {want}")

    def forward_detections_data(self, data):
        """``forward_detections`` on ``DAGR.forward``'s input contract."""
        batch = data.batch if getattr(data, "batch", None) is not None else \
            torch.zeros(data.pos.shape[0], dtype=torch.int64, device=data.pos.device)
        self.check_batch(data)
        return self.forward_detections(data.pos.float(), data.x.float(), batch, image=getattr(data, "image", None))

    def forward_data(self, data, static_out=False):
        """``DAGR.forward`` input contract: ``data`` after ``format_data`` (pos fp32[N,3] normalised,
        x fp32[N,1], batch)."""
        batch = data.batch if getattr(data, "batch", None) is not None else \
            torch.zeros(data.pos.shape[0], dtype=torch.int64, device=data.pos.device)
        self.check_batch(data)
        return self.forward_raw(data.pos.float(), data.x.float(), batch, image=getattr(data, "image", None),
                                static_out=static_out)
