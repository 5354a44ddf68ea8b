"""``src/dagr/asynchronous/evaluate_flops.py`` on this stack: FLOPs per layer of DAGR in the reference's scheme.

Each sample of the batch is split as the reference splits it (``split_data(data, -1)``: every event but the last is the
initial window, the last event is the update), run as a batch of one, and its per-module log goes through the
reference's ``_filter_non_leaf_nodes`` and ``_merge_to_level_flops(level=3)``; the result is the mean over samples.
The counts come from the device (``dagr_async_flops``, see ``flops.py``).  ``dense=True`` reports the init pass (log
index 0); ``dense=False`` (the update pass, log index 1) raises ``NotImplementedError`` (``flops.UPDATE_NOT_COUNTED``).

``check_consistency``: the update's detections must equal those of one ``reset=True`` call on all events -- here bit
for bit (the reference allows 1e-3, evaluate_flops.py:139-147); a sample that fails is left out of the average, as
there."""
from collections import OrderedDict
from typing import List, Tuple

import torch

from . import make_model_asynchronous, make_model_synchronous
from .flops import UPDATE_NOT_COUNTED, logged_modules


class _Sample:
    """One sample in ``DAGR.forward``'s input contract (batch of one)."""

    def __init__(self, pos, x, width, height, time_window, image=None):
        self.pos, self.x = pos, x
        self.batch = torch.zeros(pos.shape[0], dtype=torch.long, device=pos.device)
        self.width, self.height, self.time_window = width, height, time_window
        self.num_graphs = 1
        if image is not None:
            self.image = image


def _samples(batch):
    """``Batch.to_data_list``: the events of every sample, in order."""
    b = batch.batch if getattr(batch, "batch", None) is not None else \
        torch.zeros(batch.pos.shape[0], dtype=torch.long, device=batch.pos.device)
    n = int(getattr(batch, "num_graphs", None) or (int(b.max()) + 1 if b.numel() else 0))
    image = getattr(batch, "image", None)
    out = []
    for s in range(n):
        m = b == s
        out.append(dict(pos=batch.pos[m], x=batch.x[m], image=None if image is None else image[s:s + 1]))
    return out


def split_data(sample, index: int) -> Tuple[dict, dict]:
    """evaluate_flops.py:10-24: events before / from ``index``; the image goes with both parts."""
    first = dict(pos=sample["pos"][:index], x=sample["x"][:index], image=sample["image"])
    second = dict(pos=sample["pos"][index:], x=sample["x"][index:], image=sample["image"])
    return first, second


def evaluate_flops(model, batch, dense=False, check_consistency=False, return_all_samples=False):
    """evaluate_flops.py:82-165, same return dict: ``flops_per_layer`` (mean over samples), ``total_flops`` and, with
    ``return_all_samples``, ``flops_per_layer_batch``.  ``None`` when no sample passed the consistency check."""
    if not dense:
        raise NotImplementedError(UPDATE_NOT_COUNTED)
    geo = [getattr(batch, k)[:1] if torch.is_tensor(getattr(batch, k)) else getattr(batch, k)
           for k in ("width", "height", "time_window")]
    flops_per_layer_batch = []
    for i, sample in enumerate(_samples(batch)):
        initial, new = split_data(sample, -1)
        ok = True
        if check_consistency:
            make_model_asynchronous(model)
            with torch.no_grad():
                whole = model.forward(_Sample(sample["pos"], sample["x"], *geo, image=sample["image"]), reset=True,
                                      return_targets=False)[0]
                model.forward(_Sample(initial["pos"], initial["x"], *geo, image=initial["image"]), reset=True,
                              return_targets=False)
                upd = model.forward(_Sample(new["pos"], new["x"], *geo), reset=False, return_targets=False)[0]
            ok = all(torch.equal(a, b) for a, b in zip(whole, upd)) and len(whole) == len(upd)
            if not ok:
                print(f"AssertionError(Failed at index {i}.)")

        model = make_model_asynchronous(model, log_flops=True)
        with torch.no_grad():
            model.forward(_Sample(initial["pos"], initial["x"], *geo, image=initial["image"]), reset=True,
                          return_targets=False)
        flops_per_layer = OrderedDict((name, m.asy_flops_log[0]) for name, m, _ in logged_modules(model)
                                      if len(m.asy_flops_log) > 0)
        flops_per_layer = _filter_non_leaf_nodes(flops_per_layer)
        flops_per_layer = _merge_to_level_flops(flops_per_layer, level=3)
        model = make_model_synchronous(model)
        if ok:
            flops_per_layer_batch.append(flops_per_layer)

    if len(flops_per_layer_batch) == 0:
        return None
    flops_per_layer = _merge_list_flops(flops_per_layer_batch)
    output = {"flops_per_layer": flops_per_layer, "total_flops": sum(flops_per_layer.values())}
    if return_all_samples:
        output["flops_per_layer_batch"] = flops_per_layer_batch
    return output


def _filter_non_leaf_nodes(flops_per_layer: OrderedDict) -> OrderedDict:
    """evaluate_flops.py:167-177 (a name that occurs inside another name is dropped -- a substring test, as there)."""
    drop = [q for q in flops_per_layer if any(q in n and q != n for n in flops_per_layer)]
    for q in drop:
        flops_per_layer.pop(q)
    return flops_per_layer


def _merge_to_level_flops(flops_per_layer: OrderedDict, level=2) -> OrderedDict:
    """evaluate_flops.py:179-191: sums over the names' first ``level`` components, in order of first appearance."""
    merged = OrderedDict()
    for name, flops in flops_per_layer.items():
        key = ".".join(name.split(".")[:level])
        merged[key] = merged.get(key, 0) + flops
    return merged


def _merge_list_flops(flops_per_layer_batch: List[OrderedDict]) -> OrderedDict:
    """evaluate_flops.py:193-194: the mean over samples, key by key."""
    n = len(flops_per_layer_batch)
    return OrderedDict((k, sum(f[k] for f in flops_per_layer_batch) / n) for k in flops_per_layer_batch[0])
