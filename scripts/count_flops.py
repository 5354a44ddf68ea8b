#!/usr/bin/env python
"""Twin of the reference's ``scripts/count_flops.py``: FLOPs per layer of DAGR in the reference's asynchronous scheme,
averaged over the test windows (``evaluate_flops`` per batch, running mean through ``DictBuffer``), written to
``<output_directory>/flops_per_layer.pth`` after every batch.  The reference's command line is taken as it is
(readme.md:119-125; its ``config/eagr-s-dsec.yaml`` is not shipped by the reference -- ``dagr-s-dsec.yaml`` is used):

  python scripts/count_flops.py --config config/dagr-s-dsec.yaml --checkpoint data/dagr_s_50.pth --batch_size 8 \\
         --dataset_directory $DSEC_ROOT --output_directory $LOG_DIR --dense

Counted on the device (dagr/asynchronous/flops.py): the init pass (``--dense``, log index 0).  Without ``--dense`` the
reference reports the update pass, whose count is not implemented yet: the script stops with that error.  Without
``--dataset_directory`` the windows are the synthetic stand-in stream; a ``--dataset_directory`` that cannot be read is
an error."""
import sys

import torch

import _common as C
from dagr.asynchronous.evaluate_flops import evaluate_flops
from dagr.utils.buffers import DictBuffer, format_data


def main(argv=None):
    def more(p):
        p.add_argument("--check_consistency", action="store_true")
        p.add_argument("--dense", action="store_true")
    a = C.flags(__doc__, argv, extra=more)
    if a.dataset_directory is not None and not C.real_data_available(a):
        raise SystemExit(f"--dataset_directory {a.dataset_directory} cannot be read")
    torch.manual_seed(42)
    dev = torch.device("cuda")
    ds, loader = C.dataset_and_loader(a, 1, 0)
    args, model = C.build_model(a, ds, dev)
    model.eval()
    buffer = DictBuffer()
    a.output_directory.mkdir(parents=True, exist_ok=True)
    out = a.output_directory / "flops_per_layer.pth"
    for data in loader:
        data = format_data(data.to(dev))
        res = evaluate_flops(model, data, check_consistency=a.check_consistency, return_all_samples=True,
                             dense=a.dense)
        if res is None:
            continue
        buffer.update(res["flops_per_layer"])
        buffer.save(out)
        print(f"Total FLOPS {sum(buffer.compute().values())}", flush=True)
    total = sum(buffer.compute().values()) if buffer.compute() is not None else 0
    print(total)
    return out


if __name__ == "__main__":
    try:
        main()
    except NotImplementedError as e:
        print(f"count_flops: {e}", file=sys.stderr)
        sys.exit(2)
