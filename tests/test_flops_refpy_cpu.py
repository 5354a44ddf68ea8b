"""FLOP accounting in the reference's scheme, host side: the FLOPS_FLAGS namespace of the readme's count_flops line, the
modules that log and the keys evaluate_flops reports, against tests/golden/ref_py_flops.json (made by the reference's
own evaluate_flops, tests/make_golden_refpy_flops.py)."""
import json
import os
from collections import OrderedDict

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_py_flops.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_flops_flags_of_the_readme_line():
    from dagr.utils.args import FLOPS_FLAGS
    g = _golden()["flops_flags"]
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        ns = FLOPS_FLAGS(g["argv"])
    finally:
        os.chdir(cwd)
    got = {k: (str(v) if not isinstance(v, (int, float, bool, str)) else v) for k, v in vars(ns).items()}
    assert got == g["namespace"]


@pytest.mark.parametrize("case", sorted(_golden()["cases"]))
def test_logged_modules_and_merged_keys(case):
    from oracle import model as om
    from dagr_amd.asynchronous.evaluate_flops import _filter_non_leaf_nodes, _merge_to_level_flops
    from dagr_amd.asynchronous.flops import logged_modules
    from dagr_amd.model.networks.dagr import DAGR
    c = _golden()["cases"][case]
    args = om.default_args(batch_size=c["B"], **c["overrides"])
    model = DAGR(args, height=c["H"], width=c["W"])
    names = OrderedDict((n, 0) for n, _, _ in logged_modules(model))
    keys = list(_merge_to_level_flops(_filter_non_leaf_nodes(names), level=3))
    for mode in ("update", "dense"):
        assert sorted(keys) == sorted(c[mode]["flops_per_layer"])
        for d in c[mode]["flops_per_layer_batch"]:
            assert sorted(keys) == sorted(d)


def test_make_model_asynchronous_logs_flops_of_dagr():
    from oracle import model as om
    from dagr.asynchronous import make_model_asynchronous, make_model_synchronous
    from dagr_amd.model.networks.dagr import DAGR
    model = DAGR(om.default_args(batch_size=1), height=215, width=320)
    assert make_model_asynchronous(model, log_flops=True) is model
    assert model.asy_flops_log == [] and model.backbone.pool1.asy_flops_log == []
    assert model.head.stem1.conv.asy_flops_log == []
    make_model_synchronous(model)
    assert model.backbone.pool1.asy_flops_log == [] and not model._log_flops
    with pytest.raises(NotImplementedError):
        make_model_asynchronous(torch.nn.Linear(1, 1), log_flops=True)


def test_evaluate_flops_importable_under_reference_path():
    import dagr.asynchronous.evaluate_flops as ef
    import dagr_amd.asynchronous.evaluate_flops as own
    assert ef is own and callable(ef.evaluate_flops)


@pytest.mark.parametrize("case", sorted(_golden()["cases"]))
def test_every_logged_leaf_has_a_graph_level(case):
    """The level table covers every leaf the converter logs; a name outside it is an error, not level 0."""
    import types
    from oracle import model as om
    from dagr_amd.asynchronous.flops import _level_of, logged_modules
    from dagr_amd.model.networks.dagr import DAGR
    c = _golden()["cases"][case]
    args = om.default_args(batch_size=c["B"], **c["overrides"])
    model = DAGR(args, height=c["H"], width=c["W"])
    eng = types.SimpleNamespace(head_levels=list(range(5 - int(args.num_scales), 5)))
    levels = {n: _level_of(n, eng) for n, _, kids in logged_modules(model) if kids is None}
    assert levels["backbone.conv_block1.conv_block1.conv"] == 0 and levels["backbone.pool1"] == 0
    assert levels["backbone.layer5.conv_block2.conv"] == 4 and levels["head.stem1.conv"] == eng.head_levels[0]
    with pytest.raises(NotImplementedError):
        _level_of("backbone.layer6.conv_block1.conv", eng)
