"""Per-shape timing of the image branch's compute-bound convolutions at B = 8, 640x480: the library path the engine ran
before (dagr_gemm_epilogue for the 1x1 convs; the library 3x3 conv + dagr_bias_relu) against the split-bf16 MFMA kernel
(dagr_gemm_split_bf16 / dagr_conv3x3_split_bf16), each with bias + ReLU.

HIP events around every launch, `--warm` untimed launches, the median of `--iters`; the whole measurement of a shape is
repeated `--rounds` times and the spread of the medians (max - min) is printed beside the first: a path wins a shape only
by more than that spread.  Prints a markdown table (TF/s: 2 M K N / time; the split columns are fp32-equivalent TF/s,
against the 417 TF-equivalent ceiling of six bf16 MFMAs per product; the split times are every variant of
dagr_gemm_split_bf16_variant / dagr_conv3x3_split_bf16_variant, rows x columns, "w8" on eight waves, each as first median
(spread of its medians); "auto" is what tile 0 of the first entry points chooses).

    python tools/split_gemm_bench.py [--md OUT.md] [--only 1x1|3x3]
"""
import argparse
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd import _lib  # noqa: E402

# (M, K, N, note) of the 1x1 convs of layers 1-4 (M = B * H * W at the conv's output resolution, B = 8)
GEMMS = [(153600, 64, 64, "layer1.0.conv1"), (153600, 256, 64, "layer1.1-2.conv1"), (153600, 64, 256, "layer1.*.conv3, layer1.0.downsample"),
         (153600, 256, 128, "layer2.0.conv1"),
         (38400, 512, 128, "layer2.1-3.conv1"), (38400, 128, 512, "layer2.*.conv3"), (38400, 256, 512, "layer2.0.downsample"),
         (38400, 512, 256, "layer3.0.conv1"), (9600, 1024, 256, "layer3.1-5.conv1"), (9600, 256, 1024, "layer3.*.conv3"),
         (9600, 512, 1024, "layer3.0.downsample"),
         (9600, 1024, 512, "layer4.0.conv1"), (2400, 2048, 512, "layer4.1-2.conv1"), (2400, 512, 2048, "layer4.*.conv3"),
         (2400, 1024, 2048, "layer4.0.downsample")]
# the same layers at B = 2, 320 x 215 (the size of the engine tests): where the rule's lower bound on M comes from
GEMMS += [(8640, 256, 128, "B=2 320x215 layer2.0.conv1"), (2160, 128, 512, "B=2 320x215 layer2.*.conv3"),
          (560, 256, 1024, "B=2 320x215 layer3.*.conv3")]
# stride-2 1x1 (downsample) convs read in place: (B, H, W, K, N) of the INPUT map
STRIDED = [(8, 120, 160, 256, 512, "layer2.0.downsample /2"), (8, 60, 80, 512, 1024, "layer3.0.downsample /2"),
           (8, 30, 40, 1024, 2048, "layer4.0.downsample /2"), (2, 54, 80, 256, 512, "B=2 320x215 layer2.0.downsample /2"),
           (2, 27, 40, 512, 1024, "B=2 320x215 layer3.0.downsample /2")]
# stride-1 3x3 convs: (H, W, C)
CONVS = [(8, 120, 160, 64, "layer1.*.conv2"), (8, 60, 80, 128, "layer2.1-3.conv2"), (8, 30, 40, 256, "layer3.1-5.conv2"),
         (8, 15, 20, 512, "layer4.1-2.conv2"), (2, 27, 40, 128, "B=2 320x215 layer2.1-3.conv2")]


VARIANTS = [(name[len("DAGR_SPLIT_"):].lower(), code) for name, code in sorted(_lib.DEFINES.items(), key=lambda kv: kv[1])
            if name.startswith("DAGR_SPLIT_") and name != "DAGR_SPLIT_VARIANT_LAST"]


def all_tiles(split_fn):
    return [(name, split_fn(code)) for name, code in VARIANTS] + [("auto", split_fn(0))]


def time_us(fn, warm, iters):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3


def pack(wt):
    """Wt[K, N] fp32 -> the kernel's three bf16 planes."""
    L = _lib.lib()
    K, N = wt.shape
    nbytes = L.dagr_gemm_split_bf16_packed_bytes(K, N)
    assert nbytes > 0, (K, N)
    out = torch.empty(nbytes, dtype=torch.uint8, device=wt.device)
    _lib.check(L.dagr_gemm_split_bf16_pack(_lib.ptr(wt), K, N, _lib.ptr(out), nbytes, _lib.cur_stream(wt.device)), "pack")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["1x1", "3x3"], default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    torch.manual_seed(0)
    torch.backends.cudnn.benchmark = True
    ws = torch.empty(int(L.dagr_gemm_epilogue_workspace_bytes()), dtype=torch.uint8, device=dev)
    rows = ["| shape | layer | library us | TF/s | of 157.3 | split us (spread): " + " / ".join(n for n, _ in VARIANTS) + " / auto | best us | "
            "TF-eq/s | of 417 | spread lib / best us | max diff / max ref |", "|---|---|---|---|---|---|---|---|---|---|---|"]

    def measure(name, note, flop, lib_fn, split_fns, y_lib, y_split):
        lib = [time_us(lib_fn, a.warm, a.iters) for _ in range(a.rounds)]
        best, firsts = None, []
        for tile, fn in split_fns:
            t = [time_us(fn, a.warm, a.iters) for _ in range(a.rounds)]
            firsts.append(f"{t[0]:.1f} ({max(t) - min(t):.1f})")
            if tile != "auto" and (best is None or t[0] < best[1][0]):
                best = (tile, t)
        tile, sp = best
        split_fns[[t for t, _ in split_fns].index(tile)][1]()
        lib_fn()
        torch.cuda.synchronize()
        diff = ((y_lib - y_split).abs().max() / y_lib.abs().max()).item()
        tl, tsp = flop / lib[0] / 1e6, flop / sp[0] / 1e6
        all_tiles = " / ".join(firsts)
        rows.append(f"| {name} | {note} | {lib[0]:.1f} | {tl:.1f} | {tl / 157.3:.2f} | {all_tiles} | {sp[0]:.1f} ({tile}) | {tsp:.1f} | "
                    f"{tsp / 417:.2f} | {max(lib) - min(lib):.1f} / {max(sp) - min(sp):.1f} | {diff:.1e} |")
        print(rows[-1], flush=True)

    def st():
        return _lib.cur_stream(dev)

    if a.only in (None, "1x1"):
        for M, K, N, note in GEMMS:
            A = torch.relu(torch.randn(M, K, device=dev))
            wt = torch.randn(K, N, device=dev) * (2.0 / K) ** 0.5
            bias = torch.randn(N, device=dev) * 0.1
            wp = pack(wt)
            y0, y1 = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)

            def lib_fn():
                _lib.check(L.dagr_gemm_epilogue(_lib.ptr(A), M, K, K, _lib.ptr(wt), N, _lib.ptr(bias), None, N, 1, _lib.ptr(y0),
                                                N, _lib.ptr(ws), ws.numel(), st()), "gemm_epilogue")

            def split_fn(tile):
                return lambda: _lib.check(L.dagr_gemm_split_bf16_variant(_lib.ptr(A), M, K, K, _lib.ptr(wp), N, _lib.ptr(bias), None,
                                                                         N, 1, _lib.ptr(y1), N, 0, 0, 0, 1, tile, st()), "gemm_split")
            measure(f"{M} x {K} x {N}", note, 2.0 * M * K * N, lib_fn, all_tiles(split_fn), y0, y1)
            del A, wt, wp, y0, y1
        for B, H, W, K, N, note in STRIDED:
            x = torch.relu(torch.randn(B, H, W, K, device=dev))
            wt = torch.randn(K, N, device=dev) * (2.0 / K) ** 0.5
            bias = torch.randn(N, device=dev) * 0.1
            wp = pack(wt)
            Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            M = B * Ho * Wo
            y0, y1 = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)

            def lib_fn():
                xs = x[:, ::2, ::2, :].reshape(-1, K)          # the copy the engine's library path makes
                _lib.check(L.dagr_gemm_epilogue(_lib.ptr(xs), M, K, K, _lib.ptr(wt), N, _lib.ptr(bias), None, N, 0, _lib.ptr(y0),
                                                N, _lib.ptr(ws), ws.numel(), st()), "gemm_epilogue")

            def split_fn(tile):
                return lambda: _lib.check(L.dagr_gemm_split_bf16_variant(_lib.ptr(x), M, K, K, _lib.ptr(wp), N, _lib.ptr(bias), None,
                                                                         N, 0, _lib.ptr(y1), N, B, H, W, 2, tile, st()), "gemm_split")
            measure(f"{M} x {K} x {N} (/2 of {H}x{W})", note, 2.0 * M * K * N, lib_fn,
                    all_tiles(split_fn), y0, y1)
            del x, wt, wp, y0, y1
    if a.only in (None, "3x3"):
        for B, H, W, C, note in CONVS:
            x = torch.relu(torch.randn(B, C, H, W, device=dev)).contiguous(memory_format=torch.channels_last)
            w = (torch.randn(C, C, 3, 3, device=dev) * (2.0 / (9 * C)) ** 0.5).contiguous(memory_format=torch.channels_last)
            bias = torch.randn(C, device=dev) * 0.1
            wp = pack(w.permute(2, 3, 1, 0).reshape(9 * C, C).contiguous())
            M = B * H * W
            y1 = torch.empty(M, C, device=dev)
            hold = {}

            def lib_fn():
                y = torch.nn.functional.conv2d(x, w, None, 1, 1)
                _lib.check(L.dagr_bias_relu(_lib.ptr(y), _lib.ptr(bias), y.numel(), C, st()), "bias_relu")
                hold["y"] = y

            def split_fn(tile):
                return lambda: _lib.check(L.dagr_conv3x3_split_bf16_variant(_lib.ptr(x), B, H, W, C, C, _lib.ptr(wp), C, _lib.ptr(bias),
                                                                            None, C, 1, _lib.ptr(y1), C, tile, st()), "conv3x3_split")
            lib_fn()
            y0 = hold["y"].permute(0, 2, 3, 1).reshape(M, C)
            # (every lib_fn() makes a new map from the same operands; the first one is what the split result is set against)
            measure(f"3x3 {H}x{W} C={C} (M {M}, K {9 * C}, N {C})", note, 2.0 * M * 9 * C * C, lib_fn,
                    all_tiles(split_fn), y0, y1)
            del x, w, wp, y1
    text = "\n".join(rows) + "\n"
    if a.md:
        with open(a.md, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
