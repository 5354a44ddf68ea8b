#!/usr/bin/env python
"""tools/order_probe.py -- cost of --keep_temporal_ordering in the window engine (dagr_pool_desc.keep_order).

Times one window (events only, dagr-s, 640x480, S-uniform) at B = 1 x 25 k and B = 8 x 100 k events: the engine
unflagged, the engine flagged (latency mode: one captured window graph), and the flagged model's module path
(DAGR.forward_modules, host-side filter).  Device-event p50 over the repeats; one JSON line per case.  Run it under
``rocprofv3 --kernel-trace --stats -- python tools/order_probe.py`` for the kernel names and counts per window."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import model as om  # noqa: E402
from dagr_amd.data import Batch, Data  # noqa: E402
from dagr_amd.model.networks.dagr import DAGR  # noqa: E402
from dagr_amd.utils import synthetic as syn  # noqa: E402
from dagr_amd.utils.buffers import format_data  # noqa: E402
from dagr_amd.utils.testing_weights import randomize_  # noqa: E402

W, H = 640, 480
REPS = int(os.environ.get("REPS", "40"))
dev = torch.device("cuda:0")


def p50(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main():
    torch.manual_seed(0)
    for B, n in ((1, 25000), (8, 100000)):
        args = om.default_args(batch_size=B, keep_temporal_ordering=True)
        model = randomize_(DAGR(args, height=H, width=W), seed=0).eval().cuda()
        model.cache_luts(width=W, height=H, radius=args.radius)
        x, y, t, p, b = syn.batch_windows(syn.uniform_window, n, B, W, H, seed=1234)
        pos = torch.from_numpy(syn.format_data_np(x, y, t, W, H)).to(dev)
        feat = torch.from_numpy(p.astype(np.float32)).view(-1, 1).to(dev)
        bt = torch.from_numpy(b).to(dev)
        samples = []
        for s in range(B):
            m = b == s
            samples.append(Data(x=torch.from_numpy(p[m].reshape(-1, 1).astype(np.float32)),
                                pos=torch.from_numpy(np.stack([x[m], y[m]], -1)), t=torch.from_numpy(t[m]), width=W,
                                height=H, time_window=1000000))
        with torch.no_grad():
            for flag in (False, True):
                for pl in (model.backbone.pool1, model.backbone.pool2, model.backbone.pool3, model.backbone.pool4):
                    pl.keep_temporal_ordering = flag
                eng = model.engine().set_low_latency(True)
                assert all(d.keep_order == int(flag) for d in eng.pool_desc)
                for _ in range(5):
                    eng.forward_raw(pos, feat, bt)
                torch.cuda.synchronize()
                us = p50(lambda: eng.forward_raw(pos, feat, bt), REPS)
                eng.check_status()
                print(json.dumps(dict(B=B, events_per_sample=n, path="engine", keep_order=flag, p50_us=round(us, 1))),
                      flush=True)
            model.forward_modules(format_data(Batch.from_data_list(samples).cuda()), reset=True)
            us = p50(lambda: model.forward_modules(format_data(Batch.from_data_list(samples).cuda()), reset=True), max(3, REPS // 8))
            print(json.dumps(dict(B=B, events_per_sample=n, path="module", keep_order=True, p50_us=round(us, 1))),
                  flush=True)


if __name__ == "__main__":
    main()
