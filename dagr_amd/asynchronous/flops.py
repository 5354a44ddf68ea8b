"""FLOP accounting in the reference's scheme (``src/dagr/asynchronous/flops``, the ``asy_flops_log`` of its converted
modules), counted on the device by ``dagr_async_flops`` (csrc/async_flops.hip).

Which modules log, as ``asynchronous/__init__.py:41-110`` converts them: ``MySplineConv`` (``SplineConvToDense``
included), ``Pooling``, ``BatchNormData``, ``Cartesian`` and ``Linear`` are leaves; ``DAGR``, ``Net``, ``GNNHead``,
``Layer``, ``ConvBlock`` / ``ConvBlockWithSkip`` and ``EV_TGN`` (forward annotated with ``Data``) are converted
recursively and log the sum of their converted children; everything else (the image branch, YOLOX's dense towers)
is not converted and logs nothing.

Counted: the init pass (log index 0, ``evaluate_flops(..., dense=True)``), a closed form of every module's level node
and edge counts.  Not implemented yet: the update pass (log index 1), which counts the sets the reference's per-layer
incremental update touches (``graph_changed_nodes`` verdicts at levels >= 1, conv.py:94-227, max_pool.py:389-509).
Counting it needs the pre-update per-level state kept beside the engine's re-evaluation of levels >= 1 and a kernel that
rebuilds those sets; until then asking for it raises ``NotImplementedError``."""
import ctypes

import torch

from .. import _lib

# ``dagr_flops_module`` and the DAGR_FLOPS_* kinds, as include/dagr_hip.h declares them
FlopsModule = _lib.FlopsModule
ZERO, CONV, LINEAR, POOL, CARTESIAN = (_lib.ENUMS["DAGR_FLOPS_" + k] for k in ("ZERO", "CONV", "LINEAR", "POOL", "CARTESIAN"))

_LEAVES = ("MySplineConv", "SplineConvToDense", "Pooling", "BatchNormData", "Cartesian", "Linear")
_CONTAINERS = ("DAGR", "Net", "GNNHead", "Layer", "ConvBlock", "ConvBlockWithSkip", "EV_TGN")

UPDATE_NOT_COUNTED = ("the update pass's FLOP log (log index 1, evaluate_flops(dense=False); the reference's per-layer "
                      "incremental sets, asynchronous/conv.py:94-227, max_pool.py:389-509) is not implemented yet -- "
                      "only the init pass is counted: pass dense=True (count_flops.py --dense)")


def logged_modules(model):
    """``[(name, module, children names)]`` of every module the reference's converter gives an ``asy_flops_log``, in
    ``named_modules`` order; containers list their converted direct children."""
    out = []

    def walk(name, m):
        kids = []
        for k, c in m._modules.items():
            if c is None:
                continue
            cls = type(c).__name__
            if cls in _LEAVES:
                out.append((_join(name, k), c, None))
                kids.append(_join(name, k))
            elif cls in _CONTAINERS:
                walk(_join(name, k), c)
                kids.append(_join(name, k))
        out.append((name, m, kids))

    walk("", model)
    order = {n: i for i, (n, _) in enumerate(model.named_modules())}
    return sorted(out, key=lambda e: order[e[0]])


def _join(a, b):
    return f"{a}.{b}" if a else b


# second name component of every leaf -> graph level it runs on (a pooling: its input level); head modules map through
# the engine's head_levels (scale s feeds from head_levels[s - 1]).  An unknown name is an error, never a default.
_BACKBONE_LEVEL = {"conv_block1": 0, "edge_attrs": 0, "pool1": 0, "layer2": 1, "pool2": 1, "layer3": 2, "pool3": 2,
                   "layer4": 3, "pool4": 3, "layer5": 4}
_HEAD_SCALE = {f"{p}{s}": s for p in ("stem", "cls_conv", "reg_conv", "cls_pred", "reg_pred", "obj_pred") for s in (1, 2)}


def _level_of(name, eng):
    """Graph level a logged leaf module runs on (a pooling: its input level)."""
    parts = name.split(".")
    top = parts[1] if len(parts) > 1 else None
    if parts[0] == "backbone" and top in _BACKBONE_LEVEL:
        return _BACKBONE_LEVEL[top]
    if parts[0] == "head" and top in _HEAD_SCALE and _HEAD_SCALE[top] <= len(eng.head_levels):
        return eng.head_levels[_HEAD_SCALE[top] - 1]
    raise NotImplementedError(f"FLOP accounting: no graph level known for module {name!r}")


def descriptors(model, eng):
    """``dagr_flops_module`` rows of the leaves of ``logged_modules(model)`` (the containers are sums on the host)."""
    rows, names = [], []
    for name, m, kids in logged_modules(model):
        if kids is not None:
            continue
        cls = type(m).__name__
        lvl = _level_of(name, eng)
        if cls in ("MySplineConv", "SplineConvToDense"):
            d = FlopsModule(CONV, lvl, m.in_channels, m.out_channels, 1 if getattr(m, "lin", None) is not None else 0,
                            1 if getattr(m, "bias", None) is not None else 0)
        elif cls == "Linear":
            d = FlopsModule(LINEAR, lvl, m.mlp.in_features, m.mlp.out_features, 0, 0)
        elif cls == "Pooling":
            d = FlopsModule(POOL, lvl, int(eng.pool_desc[lvl].channels), 0, 0, 0)
        elif cls == "Cartesian":
            d = FlopsModule(CARTESIAN, lvl, 0, 0, 0, 0)
        else:                                       # BatchNormData
            d = FlopsModule(ZERO, lvl, 0, 0, 0, 0)
        rows.append(d)
        names.append(name)
    return names, rows


class Accountant:
    """Per-engine plan: the module table on the device and the int64 output; ``count()`` runs ``dagr_async_flops``
    on the resident window and reads every count back once."""

    def __init__(self, model, eng):
        self.eng = eng
        self.entries = logged_modules(model)
        self.leaf_names, rows = descriptors(model, eng)
        table = (FlopsModule * max(1, len(rows)))(*rows)
        host = torch.frombuffer(bytearray(bytes(table)), dtype=torch.int32)
        self.mods = host.to(eng.device)
        self.mods_ptr = ctypes.cast(_lib.ptr(self.mods), ctypes.POINTER(FlopsModule))      # the table on the device
        self.out = torch.zeros(len(rows), dtype=torch.int64, device=eng.device)

    def count(self):
        eng, L, P = self.eng, self.eng.L, _lib.ptr
        if eng._N <= 0:
            raise RuntimeError("FLOP accounting: no resident window")
        deg = eng._nbr[2]
        lv = eng.levels
        _lib.check(L.dagr_async_flops(P(deg), int(eng._N), P(lv[0].counts), P(lv[1].counts), P(lv[2].counts),
                                      P(lv[3].counts), self.mods_ptr, len(self.leaf_names), P(self.out),
                                      _lib.cur_stream(eng.device)), "async_flops")
        leaf = dict(zip(self.leaf_names, self.out.tolist()))
        flops = {}
        for name, _, kids in reversed(self.entries):      # children come after their container in named_modules
            flops[name] = leaf[name] if kids is None else sum(flops[k] for k in kids)
        return flops
