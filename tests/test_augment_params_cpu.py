"""CPU suite: ``DeviceAugmentations.draw`` consumes torch's global RNG exactly as the host training chain does (so both
chains make the same random decisions under one seed), the out-of-scope configuration is refused, and the training script
takes ``--augment_on_device`` without changing the namespaces the reference's command lines parse to."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ARGS = types.SimpleNamespace(aug_p_flip=0.5, aug_zoom=1.5, aug_trans=0.1)
W, H = 240, 180


def _sample(seed, n=400):
    from dagr_amd.data.utils import to_data
    r = np.random.default_rng(seed)
    return to_data(x=r.integers(0, W, n), y=r.integers(0, H, n), t=np.sort(r.integers(0, 10 ** 6, n)),
                   p=r.choice(np.array([-1, 1], np.int8), n), bbox=np.array([[30, 40, 60, 50, 1, 1]], np.float32),
                   width=W, height=H, time_window=1000000)


def _chains():
    from dagr_amd.data.augment import Augmentations, init_transforms
    aug = Augmentations(ARGS)
    init_transforms(aug.transform_training.transforms, H, W)
    dev = aug.transform_training_device
    dev.init(H, W)
    return aug, dev


@pytest.mark.parametrize("n", [1, 5])
def test_draw_leaves_the_rng_where_the_host_chain_leaves_it(n):
    aug, dev = _chains()
    hits = set()
    for seed in range(64):
        torch.manual_seed(seed)
        for k in range(n):
            aug.transform_training(_sample(seed * 7 + k))
        want = torch.get_rng_state()
        torch.manual_seed(seed)
        params = dev.draw(n)
        assert torch.equal(torch.get_rng_state(), want), seed
        assert len(params) == n and params.dtype.itemsize == 36
        hits.update((int(r["flip"]), int(r["crop_on"])) for r in params)
    assert hits == {(0, 0), (0, 1), (1, 0), (1, 1)}        # the seeds reach every branch that draws differently


def test_draw_makes_the_host_chains_decisions():
    """The records themselves, against what the host transforms do to a probe sample under the same seed: a one-event
    sample at the centre keeps its place under the zoom, so the shift can be read off; the zoom off a second event."""
    from dagr_amd.data.utils import to_data
    aug, dev = _chains()
    for seed in range(32):
        torch.manual_seed(seed)
        rec = dev.draw(1)[0]
        assert 1 <= rec["zoom"] <= 1.5 and abs(int(rec["move"][0])) <= 24 and abs(int(rec["move"][1])) <= 18
        if rec["crop_on"]:
            assert (rec["crop_hi"] - rec["crop_lo"]).tolist() == [180, 135] and (rec["crop_lo"] >= 0).all()
            assert rec["crop_hi"][0] <= W and rec["crop_hi"][1] <= H
        # the centre pixel (120, 90) is a fixed point of flip-free zoom; with a flip it becomes 119
        d = to_data(x=np.array([W // 2]), y=np.array([H // 2]), t=np.array([5]), p=np.array([1], np.int8), width=W, height=H,
                    time_window=1000000)
        torch.manual_seed(seed)
        o = aug.transform_training(d)
        x0 = W - 1 - W // 2 if rec["flip"] else W // 2
        inside = (not rec["crop_on"]) or (rec["crop_lo"][0] <= x0 <= rec["crop_hi"][0]
                                          and rec["crop_lo"][1] <= H // 2 <= rec["crop_hi"][1])
        assert len(o.pos) == (1 if inside else 0)
        if inside:
            zx = int(np.float32(np.float32(x0 - W // 2) * rec["zoom"]) + np.float32(W // 2))
            assert o.pos[0].tolist() == [zx + int(rec["move"][0]), H // 2 + int(rec["move"][1])]


def test_loader_batches_draw_per_sample_whatever_the_rank():
    """A shuffling DataLoader hands every batch the seeds it gives the host chain per sample, a function of (seed, epoch,
    sample) alone.  Records drawn from them: two ranks' slices together are the single process's batch (not one record
    set repeated on every rank), they differ between samples and epochs, they equal what the host chain inside the loader
    decides for that sample, and the global RNG stream is neither used nor moved."""
    from dagr_amd.data import DataLoader
    from dagr_amd.data.synthetic_data import SyntheticObjects
    aug, dev = _chains()

    def loader(shard, transform=None):
        return DataLoader(SyntheticObjects(32, 300, seed=7, transform=transform), batch_size=8, shuffle=True, drop_last=True,
                          follow_batch=["bbox"], shard=shard, seed=42)

    def records(ld):
        out = []
        for batch in ld:
            assert len(batch._sample_seeds) == batch.num_graphs
            out.append(dev.draw(batch.num_graphs, batch._sample_seeds))
        return out

    torch.manual_seed(5)
    state = torch.get_rng_state()
    whole, r0, r1 = loader(None), loader((0, 2)), loader((1, 2))
    for epoch in range(2):
        full, a, b = records(whole), records(r0), records(r1)
        assert len(full) == 4 and all(len(x) == 4 for x in a + b)
        for f, x, y in zip(full, a, b):
            assert np.concatenate([x, y]).tobytes() == f.tobytes()
            assert x.tobytes() != y.tobytes()                      # the ranks do not repeat one set of records
        flat = np.concatenate(full)
        assert len({r.tobytes() for r in flat}) == len(flat)       # every sample its own record
        if epoch == 0:
            first = flat
        else:
            assert flat.tobytes() != first.tobytes()
    assert torch.equal(torch.get_rng_state(), state)
    # the host chain inside the loader makes the same decisions: a flipped sample's box is mirrored, the shift moves it
    for hb, db in zip(loader(None, aug.transform_training), loader(None)):
        rec = dev.draw(db.num_graphs, db._sample_seeds)
        for k in range(db.num_graphs):
            if rec[k]["crop_on"]:
                continue
            x, w = float(db.bbox[k, 0]), float(db.bbox[k, 2])
            x = W - 1 - (x + w) if rec[k]["flip"] else x
            want = (x - W // 2) * float(rec[k]["zoom"]) + W // 2 + int(rec[k]["move"][0])
            if 0 < want < W - 1:
                assert abs(float(hb.bbox[k, 0]) - want) < 1e-3, (k, rec[k])
        break
    with pytest.raises(ValueError):
        dev.draw(3, [1, 2])
    # a batch that no shuffling loader made has no seeds: its records come from the global stream
    assert not hasattr(next(iter(DataLoader(SyntheticObjects(8, 300), batch_size=4))), "_sample_seeds")


def test_zoom_below_one_is_refused_and_names_the_host_chain():
    from dagr_amd.data.augment import Augmentations, DeviceAugmentations
    bad = types.SimpleNamespace(aug_p_flip=0.5, aug_zoom=0.8, aug_trans=0.1)
    with pytest.raises(ValueError, match="transform_training"):
        DeviceAugmentations(bad)
    aug = Augmentations(bad)                   # the host chain still takes it
    with pytest.raises(ValueError):
        aug.transform_training_device
    assert DeviceAugmentations(types.SimpleNamespace(aug_p_flip=0.5, aug_zoom=1, aug_trans=0.1)) is not None


def test_a_host_batch_is_refused():
    from dagr_amd.data import Batch
    _, dev = _chains()
    with pytest.raises(RuntimeError, match="GPU"):
        dev(Batch.from_data_list([_sample(0), _sample(1)], follow_batch=["bbox"]))


def test_reexported_under_the_reference_import_path():
    from dagr.data.augment import DeviceAugmentations as A
    from dagr_amd.data.augment import DeviceAugmentations as B
    assert A is B


def test_script_flag_is_opt_in_and_leaves_the_reference_namespaces_alone():
    import train_ncaltech101 as T
    from make_golden_refpy_flags import README_LINES
    a = T.flags(["--config", "config/dagr-l-ncaltech.yaml", "--augment_on_device", "--max_iters", "3"])
    assert a.augment_on_device is True and a.max_iters == 3
    assert not getattr(T.flags(["--config", "config/dagr-l-ncaltech.yaml"]), "augment_on_device", False)
    a = T.flags(["--augment_on_device"], preset="dsec")
    assert a.augment_on_device is True
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_py_flags.json")))
    import _common as C
    assert len(README_LINES) == 5
    for key, argv in README_LINES.items():
        script = key.split("@")[0]
        if script in ("run_test.py", "run_test_interframe.py"):
            mine = vars(C.flags("", list(argv)))
        else:
            mine = vars(T.flags(list(argv), preset="dsec" if script == "train_dsec.py" else "ncaltech101"))
        assert "augment_on_device" not in mine, key
        for k, v in gold[key].items():
            if k in ("config", "path"):
                assert k in mine
                continue
            got = mine[k]
            got = str(got) if not isinstance(got, (int, float, bool, str)) else got
            assert got == v and type(got) is type(v), (key, k, got, v)
