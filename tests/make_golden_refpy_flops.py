#!/usr/bin/env python
"""Golden FLOP counts of the reference's OWN asynchronous package, executed on CPU.

The reference measures DAGR's cost in asynchronous mode with ``scripts/count_flops.py`` (readme.md:115-125): that script
runs ``evaluate_flops`` (``src/dagr/asynchronous/evaluate_flops.py:82-165``) on ``make_model_asynchronous(model,
log_flops=True)``.  Here that code runs unmodified over tests/refpy_fakes.py plus the stand-ins below, which the
asynchronous package needs on top of the model's:

  * ``torch_scatter.scatter_max`` / ``scatter_sum`` with ``out=`` (the incremental updates write into resident rows);
  * ``MessagePassing.aggregate`` of the ``SplineConv`` stand-in (sum);
  * ``Data.clone`` (a copy of every tensor attribute, as PyG's) and ``Batch.to_data_list`` (one ``Data`` per sample), and
    ``None`` for PyG's ``Data`` properties (``x``, ``pos``, ``batch``, ``edge_index``, ...) that a graph does not hold;
  * ``asy_tools``: the reference's masked row operators (``asynchronous/asy_tools/main.cu``), served by the oracle's
    numpy restatements (oracle/asy.py);
  * ``torch_geometric.nn.norm.BatchNorm`` and ``torch_geometric.nn.conv.GCNConv`` (imported, type-checked, not run).

Written: tests/golden/ref_py_flops.json -- per case the events, the seed of the weights, the model overrides, and the
per-sample and averaged ``flops_per_layer`` dicts (keys as the reference names them) for ``dense=False`` (the update
pass, log index 1) and ``dense=True`` (the init pass, log index 0).  Also the ``FLOPS_FLAGS()`` namespace of the readme's
``count_flops`` line.  That line names ``config/eagr-s-dsec.yaml``, which the reference does not ship: the golden is made
with ``config/dagr-s-dsec.yaml`` instead.

``--use_image``: the reference's ``evaluate_flops`` runs with the image branch over these stand-ins (the image of each
sample goes with both parts of ``split_data``); the ``s_img18_b1`` case covers it (resnet18; the frame is re-drawn from
the weights' seed, as in tests/make_golden_refpy_model.py, and not stored).

The last two cases pin where the update's event lands: ``s_newvoxel_b1`` moves the last event to a pixel whose pool1
voxel no earlier event occupies, ``s_oldvoxel_b1`` onto the pixel of an earlier event.

Run: python tests/make_golden_refpy_flops.py   (build container only)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name, W, H, events per sample, B, stream, seed of the weights, seed of the events, model overrides
CASES = [
    ("s_uniform_b2", 320, 215, 600, 2, "uniform", 31, 101, {}),
    ("s_edges_b2", 320, 215, 600, 2, "edges", 32, 102, {}),
    ("l_edges_b1", 240, 180, 500, 1, "edges", 33, 103, dict(net_stem_width=1.0, yolo_stem_width=1.0)),
    ("s_img18_b1", 320, 215, 400, 1, "edges", 34, 104, dict(use_image=True, img_net="resnet18")),
    ("s_newvoxel_b1", 320, 215, 300, 1, "uniform", 35, 105, {}),
    ("s_oldvoxel_b1", 320, 215, 300, 1, "uniform", 36, 106, {}),
]
# the readme's count_flops line (readme.md:119-125); eagr-s-dsec.yaml is not shipped: dagr-s-dsec.yaml is used
COUNT_FLOPS_LINE = ["--config", "config/dagr-s-dsec.yaml", "--use_image", "--img_net", "resnet50",
                    "--checkpoint", "data/dagr_s_50.pth", "--batch_size", "8", "--dataset_directory", "/DSEC_ROOT",
                    "--output_directory", "/LOG_DIR"]


def install_async_fakes():
    """The stand-ins the reference's asynchronous package needs beyond tests/refpy_fakes.py."""
    import refpy_fakes as rf
    from oracle import asy as oasy

    def _clone(self):
        out = type(self).__new__(type(self))
        out.__dict__.update({k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.__dict__.items()})
        return out

    def _to_data_list(self):
        out = []
        for s in range(int(self.num_graphs)):
            m = self.batch == s
            d = rf.Data(pos=self.pos[m], x=self.x[m], time_window=self.time_window[s:s + 1],
                        width=self.width[s:s + 1], height=self.height[s:s + 1])
            if hasattr(self, "image"):
                d.image = self.image[s:s + 1]
            out.append(d)
        return out

    def _from_data_list(lst):
        d = lst[0]
        d.batch = torch.zeros(len(d.x), dtype=torch.long)
        d.num_graphs = 1
        return d

    rf.Data.clone = _clone
    for key in ("x", "edge_index", "edge_attr", "y", "pos", "batch", "face", "edge_weight", "time"):
        setattr(rf.Data, key, None)           # PyG's Data properties: None when the attribute is absent
    rf.Data.to_data_list = _to_data_list
    rf.Batch.from_data_list = staticmethod(_from_data_list)

    def scatter_max(src, index, dim=0, out=None, dim_size=None):
        assert dim == 0
        n = int(index.max()) + 1 if dim_size is None else int(dim_size)
        if out is None:
            out = torch.full((n,) + tuple(src.shape[1:]), -torch.inf, dtype=src.dtype)
        arg = torch.full(out.shape, src.shape[0], dtype=torch.long)
        if src.numel() > 0:
            idx = index.view(-1, *([1] * (src.dim() - 1))).expand_as(src)
            out.scatter_reduce_(0, idx, src, reduce="amax", include_self=True)
        # argmax: the first member whose value equals the maximum (only the max pool's cache reads it)
        for i in range(src.shape[0]):
            hit = (src[i] == out[index[i]]) & (arg[index[i]] == src.shape[0])
            arg[index[i]][hit] = i
        return out, arg

    def scatter_sum(src, index, dim=0, out=None, dim_size=None):
        assert dim == 0
        if out is None:
            n = int(index.max()) + 1 if dim_size is None else int(dim_size)
            out = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype)
        if src.numel() > 0:
            out.index_add_(0, index, src)
        return out

    rf._module("torch_scatter", scatter_max=scatter_max, scatter_sum=scatter_sum)
    # MessagePassing.aggregate (aggr = sum), which the asynchronous conv calls directly (conv.py:15)
    rf.SplineConv.aggregate = lambda self, inputs, index, ptr=None, dim_size=None: scatter_sum(
        inputs, index, dim=0, dim_size=dim_size)

    def _np(t):
        return t.detach().numpy()

    def masked_isdiff(indices, x_new, x_old, atol, rtol):
        # main.cu:112-139 called as masked_isdiff(idx, new, old, ...): returns the surviving indices
        _, kept = oasy.masked_isdiff(_np(indices), _np(x_old), _np(x_new), atol, rtol)
        return torch.from_numpy(kept.astype(np.int64))

    def masked_lin(idx, x_in, x_out, weight, bias, add):
        x_out.copy_(torch.from_numpy(oasy.masked_lin(_np(idx), _np(x_in), _np(x_out), _np(weight), _np(bias), add)))

    def masked_lin_no_bias(idx, x_in, x_out, weight, add):
        x_out.copy_(torch.from_numpy(oasy.masked_lin_no_bias(_np(idx), _np(x_in), _np(x_out), _np(weight), add)))

    def masked_inplace_BN(idx, x, x_out, mean, var, weight, bias, eps):
        x_out.copy_(torch.from_numpy(oasy.masked_inplace_BN(_np(idx), _np(x), _np(x_out), _np(mean), _np(var),
                                                            _np(weight), _np(bias), eps)))

    rf._module("asy_tools", masked_isdiff=masked_isdiff, masked_lin=masked_lin, masked_lin_no_bias=masked_lin_no_bias,
               masked_inplace_BN=masked_inplace_BN)
    rf._module("torch_geometric.nn.norm", BatchNorm=rf.BatchNorm)
    rf._module("torch_geometric.nn.conv")    # GCNConv: a placeholder class (conv.py:241 isinstance check)


def _window(W, H, n, B, stream, seed):
    from dagr_amd.utils import synthetic as syn
    gen = syn.uniform_window if stream == "uniform" else syn.edges_window
    return syn.batch_windows(gen, n, B, W, H, seed=seed)


def _batch(rf, x, y, t, p, b, W, H, B):
    from dagr_amd.utils import synthetic as syn
    return rf.Batch(x=torch.from_numpy(p.astype(np.float32)).view(-1, 1),
                    pos=torch.from_numpy(syn.format_data_np(x, y, t, W, H)), batch=torch.from_numpy(b),
                    width=torch.tensor([W] * B), height=torch.tensor([H] * B),
                    time_window=torch.tensor([1000000] * B), num_graphs=B)


def _place_last(name, x, y, W, H, args):
    """s_newvoxel / s_oldvoxel: the last event onto an empty pool1 voxel / onto an earlier event's pixel."""
    from oracle import model as om
    if "voxel" not in name:
        return
    if name.startswith("s_oldvoxel"):
        x[-1], y[-1] = x[0], y[0]
        return
    vs = om.compute_pooling_at_each_layer(args.pooling_dim_at_output, 4)[0].numpy()
    vox = lambda px, py: (int(np.float32(px / W) / vs[0]), int(np.float32(py / H) / vs[1]))
    used = {vox(a, b) for a, b in zip(x[:-1], y[:-1])}
    x[-1], y[-1] = next((px, py) for py in range(H) for px in range(W) if vox(px, py) not in used)


def run_case(rdagr, ref_eval, W, H, B, seed, over, ev):
    import refpy_fakes as rf
    from oracle import model as om
    from dagr_amd.model.networks.dagr import DAGR as MirrorDAGR
    from dagr_amd.utils.testing_weights import randomize_
    args = om.default_args(batch_size=B, **over)
    torch.manual_seed(seed)
    mirror = randomize_(MirrorDAGR(args, height=H, width=W), seed=seed).eval()
    res = {}
    for dense in (False, True):
        ref = rdagr.DAGR(argparse.Namespace(**vars(args)), height=H, width=W)
        ref.load_state_dict(mirror.state_dict(), strict=True)
        ref.eval()
        ref.cache_luts(width=W, height=H, radius=args.radius)
        data = _batch(rf, *ev, W, H, B)
        if getattr(args, "use_image", False):
            data.image = torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(seed)).float() / 255
        with torch.no_grad():
            out = ref_eval.evaluate_flops(ref, data, dense=dense, check_consistency=False, return_all_samples=True)
        res["dense" if dense else "update"] = {
            "flops_per_layer": {k: float(v) for k, v in out["flops_per_layer"].items()},
            "flops_per_layer_batch": [{k: int(v) for k, v in d.items()} for d in out["flops_per_layer_batch"]],
            "total_flops": float(out["total_flops"])}
    return res


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refpy_fakes
    refpy_fakes.install()
    install_async_fakes()
    refpy_fakes.use_reference_package("/root/reference/src")
    import importlib
    rdagr = importlib.import_module("dagr.model.networks.dagr")
    ref_eval = importlib.import_module("dagr.asynchronous.evaluate_flops")
    out = {"cases": {}}
    for name, W, H, n, B, stream, seed, ev_seed, over in CASES:
        x, y, t, p, b = _window(W, H, n, B, stream, ev_seed)
        from oracle import model as om
        _place_last(name, x, y, W, H, om.default_args(batch_size=B, **over))
        res = run_case(rdagr, ref_eval, W, H, B, seed, over, (x, y, t, p, b))
        out["cases"][name] = dict(W=W, H=H, B=B, stream=stream, seed=seed, overrides=over,
                                  events=dict(x=x.tolist(), y=y.tolist(), t=t.tolist(), p=p.tolist(), b=b.tolist()),
                                  **res)
        print(name, res["update"]["total_flops"], res["dense"]["total_flops"])

    # FLOPS_FLAGS() of the readme's count_flops line (args.py:82-101), run from the reference's root as the readme does
    rargs = importlib.import_module("dagr.utils.args")
    argv0, cwd0 = list(sys.argv), os.getcwd()
    os.chdir("/root/reference")
    sys.argv = ["count_flops.py"] + COUNT_FLOPS_LINE
    ns = rargs.FLOPS_FLAGS()
    sys.argv = argv0
    os.chdir(cwd0)
    out["flops_flags"] = {"argv": COUNT_FLOPS_LINE,
                          "namespace": {k: (str(v) if not isinstance(v, (int, float, bool, str)) else v)
                                        for k, v in vars(ns).items()}}

    path = os.path.join(os.environ.get("GOLDEN_OUT", os.path.join(ROOT, "tests", "golden")), "ref_py_flops.json")
    with open(path, "w") as f:
        json.dump(out, f, sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
