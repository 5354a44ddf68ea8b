"""The split-bf16 kernel on three representative shapes of the image branch, for a counter run:

    rocprofv3 --kernel-trace --pmc <counters> --output-format csv -d OUT -- python tools/split_gemm_pmc.py --variants 3,5
    python tools/pmc_dispatches.py OUT/.../*_counter_collection.csv k_gemm_split

Launches, in this order, every shape with every variant `--reps` times (bias + ReLU, as tools/split_gemm_bench.py), and
prints one line per launch, so the n-th k_gemm_split dispatch of the counter file is the n-th line printed here."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd import _lib  # noqa: E402
from tools.split_gemm_bench import pack  # noqa: E402

GEMMS = [(38400, 512, 256), (9600, 256, 1024)]
CONVS = [(8, 30, 40, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="3")
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    variants = [int(v) for v in a.variants.split(",")]
    dev = torch.device("cuda:0")
    L = _lib.lib()
    st = _lib.cur_stream(dev)
    torch.manual_seed(0)
    for M, K, N in GEMMS:
        A = torch.relu(torch.randn(M, K, device=dev))
        wp = pack(torch.randn(K, N, device=dev) * (2.0 / K) ** 0.5)
        bias = torch.randn(N, device=dev) * 0.1
        y = torch.empty(M, N, device=dev)
        for v in variants:
            for _ in range(a.reps):
                _lib.check(L.dagr_gemm_split_bf16_variant(_lib.ptr(A), M, K, K, _lib.ptr(wp), N, _lib.ptr(bias), None, N, 1,
                                                          _lib.ptr(y), N, 0, 0, 0, 1, v, st), "gemm_split")
                print(f"{M} x {K} x {N} variant {v}")
        torch.cuda.synchronize()
    for B, H, W, C in CONVS:
        x = torch.relu(torch.randn(B, H, W, C, device=dev))
        wp = pack(torch.randn(9 * C, C, device=dev) * (2.0 / (9 * C)) ** 0.5)
        bias = torch.randn(C, device=dev) * 0.1
        y = torch.empty(B * H * W, C, device=dev)
        for v in variants:
            for _ in range(a.reps):
                _lib.check(L.dagr_conv3x3_split_bf16_variant(_lib.ptr(x), B, H, W, C, C, _lib.ptr(wp), C, _lib.ptr(bias), None, C, 1,
                                                             _lib.ptr(y), C, v, st), "conv3x3_split")
                print(f"3x3 {H}x{W} C={C} variant {v}")
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
