"""GPU suite: ``DeviceAugmentations`` (csrc/augment.hip) against the reference's own training chain (the ``aug<seed>_*`` arrays
of tests/golden/ref_py_data.npz, made by the reference's augment.py under fixed seeds) and, at full batch size, against this
repository's host chain, which tests/test_data_refpy.py holds to the same golden.  Events (positions, polarities, times,
segment bounds) and frames must be equal bit for bit; boxes within the 1e-4 the host chain's own golden test allows."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.data import Batch
from dagr_amd.data import augment as A
from dagr_amd.data.utils import to_data
from dagr_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "ref_py_data.npz"), allow_pickle=False)
ARGS = types.SimpleNamespace(aug_p_flip=0.5, aug_zoom=1.5, aug_trans=0.1)
FOLLOW = ["bbox", "bbox0"]

# 32 seeds for the full-size comparison.  The first ones were picked on the CPU from DeviceAugmentations.draw(8) so that, at
# both resolutions, some sample's crop window starts in row 0 (one chance in 45 resp. 120 per crop); the rest are 0..27.
SEEDS = [67, 68, 308, 387] + list(range(28))


def _chains(H, W):
    aug = A.Augmentations(ARGS)
    A.init_transforms(aug.transform_training.transforms, H, W)
    dev = aug.transform_training_device
    dev.init(H, W)
    return aug, dev


def _boxes(rng, n, W, H):
    b = np.zeros((n, 6), np.float32)
    b[:, 2], b[:, 3] = rng.uniform(5, W / 2, n), rng.uniform(5, H / 2, n)
    b[:, 0], b[:, 1] = rng.uniform(0, W - 1 - b[:, 2]), rng.uniform(0, H - 1 - b[:, 3])
    b[:, 4], b[:, 5] = rng.integers(0, 2, n), 1
    return b


def _samples(B, n_events, W, H, seed, image_dtype=None, boxes=True):
    out = []
    for b in range(B):
        rng = np.random.default_rng(1000 * seed + b)
        x, y, t, p = syn.uniform_window(n_events, W, H, seed=1000 * seed + b)
        bbox = _boxes(rng, (seed + b) % 7 if boxes else 0, W, H)
        d = to_data(x=x, y=y, t=t, p=p, bbox=bbox, width=W, height=H, time_window=1000000)
        if image_dtype is not None:
            d.bbox0 = d.bbox.clone()
            d.bbox0[:, :2] += 1.5
            img = torch.randint(0, 256, (1, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed * 64 + b))
            d.image = img if image_dtype == torch.uint8 else img.float() / 255.0
        out.append(d)
    return out


def _compare(host, out, B, what):
    """``host``: the per-sample results of the host chain; ``out``: the augmented device batch."""
    ptr = out._event_ptr.cpu().numpy()
    assert ptr[0] == 0 and ptr[B] == out.pos.shape[0] == out.x.shape[0] == out.t.shape[0] == out.batch.shape[0]
    pos, x, t, bvec = out.pos.cpu(), out.x.cpu(), out.t.cpu(), out.batch.cpu()
    for b, h in enumerate(host):
        s = slice(int(ptr[b]), int(ptr[b + 1]))
        assert pos[s].dtype == h.pos.dtype == torch.int16 and x.dtype == h.x.dtype and t.dtype == h.t.dtype
        assert torch.equal(pos[s], h.pos), (what, b, "pos")
        assert torch.equal(x[s], h.x) and torch.equal(t[s], h.t), (what, b, "x / t")
        assert bool((bvec[s] == b).all())
        if hasattr(h, "image"):
            img = out.image[b:b + 1].cpu()
            assert img.dtype == h.image.dtype and torch.equal(img, h.image), (what, b, "image")
        for name in ("bbox", "bbox0"):
            if hasattr(h, name):
                got = getattr(out, name).cpu()[getattr(out, name + "_batch").cpu() == b]
                want = getattr(h, name)
                assert got.shape == want.shape and got.dtype == want.dtype
                assert np.allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-4), (what, b, name)


def _host(aug, samples, seed):
    torch.manual_seed(seed)
    return [aug.transform_training(d.clone()) for d in samples]


def test_reference_goldens():
    """The base sample and the seeds of tests/test_data_refpy.py::test_training_augmentation_chain_under_fixed_seeds: the
    device chain reproduces the reference's own outputs."""
    aug, dev = _chains(180, 240)
    base = {k: G[f"aug_base_{k}"] for k in ("x", "y", "t", "p", "bbox")}
    seen = set()
    for seed in range(8):
        d = to_data(**{k: v.copy() for k, v in base.items()}, width=240, height=180, time_window=1000000)
        batch = Batch.from_data_list([d], follow_batch=FOLLOW).cuda()
        torch.manual_seed(seed)
        o = dev(batch)
        for k in ("pos", "x", "t"):
            got = getattr(o, k).cpu().numpy()
            assert got.dtype == G[f"aug{seed}_{k}"].dtype and np.array_equal(got, G[f"aug{seed}_{k}"]), (seed, k)
        assert np.allclose(o.bbox.cpu().numpy(), G[f"aug{seed}_bbox"], rtol=0, atol=1e-4), seed
        assert torch.equal(o.bbox_batch.cpu(), batch.bbox_batch.cpu())
        seen.add(len(o.pos))
    assert len(seen) > 3


@pytest.mark.parametrize("W,H", [(240, 180), (640, 480)])
@pytest.mark.parametrize("image_dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_full_size_batches_equal_the_host_chain(W, H, image_dtype):
    B, n_events = 8, 50000
    aug, dev = _chains(H, W)
    cover = set()
    for seed in SEEDS:
        samples = _samples(B, n_events, W, H, seed, image_dtype)
        host = _host(aug, samples, seed)
        after_host = torch.get_rng_state()
        torch.manual_seed(seed)
        for r in dev.draw(B):
            cover.add("flip" if r["flip"] else "no flip")
            cover.add("crop" if r["crop_on"] else "no crop")
            if r["crop_on"]:
                cover.add("crop from row 0" if r["crop_lo"][1] == 0 else "crop from a later row")
            if r["zoom"] > 1.2:
                cover.add("zoom > 1.2")
            for m in r["move"]:
                cover.add("shift > 0" if m > 0 else "shift < 0" if m < 0 else "no shift")
        batch = Batch.from_data_list(samples, follow_batch=FOLLOW).cuda()
        torch.manual_seed(seed)
        out = dev(batch)
        assert torch.equal(torch.get_rng_state(), after_host)
        _compare(host, out, B, (W, H, seed))
        assert sum(len(h.pos) for h in host) < B * n_events          # something was removed
    assert cover >= {"flip", "no flip", "crop", "no crop", "crop from row 0", "crop from a later row", "zoom > 1.2",
                     "shift > 0", "shift < 0"}, cover


def _params(B, **kw):
    p = np.zeros(B, dtype=A.AUG_PARAMS)
    p["zoom"] = 1.0
    for k, v in kw.items():
        p[k] = v
    return p


def test_edges_empty_sample_everything_leaves_no_boxes_explicit_params():
    W, H, B = 240, 180, 4
    aug, dev = _chains(H, W)
    samples = _samples(B, 3000, W, H, seed=3, image_dtype=torch.uint8)
    e = samples[1]                                                        # an empty sample in the middle of the batch
    e.pos, e.x, e.t = e.pos[:0], e.x[:0], e.t[:0]
    samples[2].bbox, samples[2].bbox0 = samples[2].bbox[:0], samples[2].bbox0[:0]      # a sample without boxes
    batch = Batch.from_data_list(samples, follow_batch=FOLLOW).cuda()
    for seed in (0, 1, 5):
        host = _host(aug, samples, seed)
        torch.manual_seed(seed)
        out = dev(batch)
        _compare(host, out, B, ("edges", seed))
        ptr = out._event_ptr.cpu().numpy()
        assert ptr[1] == ptr[2]
    # every event of sample 3 is shifted off the sensor; the others pass unchanged
    p = _params(B)
    p["move"][3] = (W, 0)
    out = dev(batch, p)
    ptr = out._event_ptr.cpu().numpy()
    n = [len(d.pos) for d in samples]
    assert ptr.tolist() == [0, n[0], n[0], n[0] + n[2], n[0] + n[2]]
    keep = torch.cat([samples[0].pos, samples[2].pos])
    assert torch.equal(out.pos.cpu(), keep) and torch.equal(out.image[:3].cpu(), batch.image[:3].cpu())
    assert int(out.image[3].max()) == 0
    # the same explicit records twice: identical outputs, and the global RNG is not touched
    torch.manual_seed(11)
    p = dev.draw(B)
    state = torch.get_rng_state()
    a, b = dev(batch, p), dev(batch, p)
    assert torch.equal(torch.get_rng_state(), state)
    for k in ("pos", "x", "t", "batch", "image", "bbox", "bbox0", "_event_ptr"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    # all samples empty
    for d in samples:
        d.pos, d.x, d.t = d.pos[:0], d.x[:0], d.t[:0]
    out = dev(Batch.from_data_list(samples, follow_batch=FOLLOW).cuda(), p)
    assert out.pos.shape == (0, 2) and out._event_ptr.cpu().tolist() == [0] * (B + 1)


def test_spatial_frame_crop_when_the_reference_quirk_is_switched_off(monkeypatch):
    W, H, B = 240, 180, 8
    monkeypatch.setattr(A, "REFERENCE_FRAME_CROP", False)
    aug, dev = _chains(H, W)
    crops = 0
    for seed in (67, 0, 1, 2):
        samples = _samples(B, 2000, W, H, seed, image_dtype=torch.uint8)
        host = _host(aug, samples, seed)
        torch.manual_seed(seed)
        crops += int(dev.draw(B)["crop_on"].sum())
        torch.manual_seed(seed)
        _compare(host, dev(Batch.from_data_list(samples, follow_batch=FOLLOW).cuda()), B, ("spatial", seed))
    assert crops >= 3


def test_int32_coordinates():
    W, H, B = 240, 180, 3
    aug, dev = _chains(H, W)
    samples = _samples(B, 5000, W, H, seed=9)
    host = _host(aug, samples, 4)
    batch = Batch.from_data_list(samples, follow_batch=FOLLOW).cuda()
    batch.pos = batch.pos.to(torch.int32)
    torch.manual_seed(4)
    _compare(host, dev(batch), B, "int32")
    batch.pos[7, 0] = 70000                      # not an int16: reported, not wrapped
    with pytest.raises(RuntimeError, match="int16"):
        dev(batch, _params(B))


class _Listed:
    """A dataset over prepared samples, with or without a transform (what the training script's datasets are to the loader)."""

    def __init__(self, samples, transform=None):
        self.samples, self.transform = samples, transform

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        d = self.samples[i].clone()
        return self.transform(d) if self.transform is not None else d


def test_batches_of_a_shuffling_loader_are_augmented_as_the_loader_would_have():
    """The training script's two ways: the host chain inside a shuffling DataLoader, or no transform there and the device
    chain on the collated batch.  Both seed a sample's random decisions from (seed, epoch, sample) alone, so they give the
    same batches -- in one process, and on every rank's slice of a data-parallel run; the global RNG stream is not used."""
    from dagr_amd.data import DataLoader
    W, H, n = 240, 180, 16
    aug, dev = _chains(H, W)
    samples = _samples(n, 4000, W, H, seed=2, image_dtype=torch.uint8)
    for shard in (None, (0, 2), (1, 2)):
        host_loader = DataLoader(_Listed(samples, aug.transform_training), batch_size=8, shuffle=True, follow_batch=FOLLOW,
                                 shard=shard, seed=42)
        dev_loader = DataLoader(_Listed(samples), batch_size=8, shuffle=True, follow_batch=FOLLOW, shard=shard, seed=42)
        for epoch in range(2):
            state = torch.get_rng_state()
            for hb, db in zip(host_loader, dev_loader):
                out = dev(db.cuda())
                B = hb.num_graphs
                assert B == (8 if shard is None else 4)
                for k in ("pos", "x", "t", "batch", "image"):
                    assert torch.equal(getattr(out, k).cpu(), getattr(hb, k)), (shard, epoch, k)
                for k in ("bbox", "bbox0"):
                    assert torch.equal(getattr(out, k + "_batch").cpu(), getattr(hb, k + "_batch"))
                    assert np.allclose(getattr(out, k).cpu().numpy(), getattr(hb, k).numpy(), rtol=0, atol=1e-4)
            assert torch.equal(torch.get_rng_state(), state)


def test_more_tiles_than_a_workgroup_sums_go_through_the_scan():
    """N beyond 2048 tiles of 2048 events: the per-tile counts are scanned between the two launches.  Against torch on
    the device: a flip, a crop window and a shift on one sample, nothing but the sensor test on the other."""
    W, H, B, N = 640, 480, 2, 2048 * 2048 + 12345
    _, dev = _chains(H, W)
    g = torch.Generator().manual_seed(0)
    pos = torch.stack([torch.randint(0, W, (N,), generator=g), torch.randint(0, H, (N,), generator=g)], 1).to(torch.int16)
    cut = 1234567
    batch = Batch(pos=pos, x=torch.randint(-1, 2, (N, 1), generator=g).to(torch.int8), t=torch.arange(N, dtype=torch.int32),
                  batch=(torch.arange(N) >= cut).long())
    batch._num_graphs = B
    p = _params(B)
    p["flip"][0], p["crop_on"][0], p["crop_lo"][0], p["crop_hi"][0], p["move"][0] = 1, 1, (100, 50), (500, 400), (-30, 7)
    out = dev(batch.cuda(), p)
    x, y = pos[:, 0].long(), pos[:, 1].long()
    first = torch.arange(N) < cut
    fx = W - 1 - x
    keep0 = first & (fx >= 100) & (fx <= 500) & (y >= 50) & (y <= 400) & (fx - 30 >= 0) & (y + 7 < H)
    keep = keep0 | ~first
    want = torch.where(first[:, None], torch.stack([fx - 30, y + 7], 1), pos.long())[keep].to(torch.int16)
    assert out._event_ptr.cpu().tolist() == [0, int(keep0.sum()), int(keep.sum())]
    assert torch.equal(out.pos.cpu(), want) and torch.equal(out.t.cpu(), batch.t[keep])
    assert torch.equal(out.x.cpu(), batch.x[keep]) and torch.equal(out.batch.cpu(), batch.batch[keep])


def test_status_word_reports_a_non_monotone_sample_ptr():
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    N, B, W, H = 5000, 3, 240, 180
    pos = torch.randint(0, 180, (N, 2), dtype=torch.int16, device=dev)
    t = torch.arange(N, dtype=torch.int32, device=dev)
    p = torch.ones(N, dtype=torch.int8, device=dev)
    par = torch.from_numpy(_params(B).view(np.int32).reshape(B, -1)).to(dev)
    ws_bytes = L.dagr_augment_workspace_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stream = _lib.cur_stream(dev)
    par_ptr = ctypes.cast(_lib.ptr(par), ctypes.POINTER(_lib.AugParams))

    def run(ptr_host):
        ptr = torch.tensor(ptr_host, dtype=torch.int32, device=dev)
        out_pos, out_t, out_p = torch.full_like(pos, -7), torch.full_like(t, -7), torch.full_like(p, -7)
        out_ptr = torch.full((B + 1,), -7, dtype=torch.int32, device=dev)
        status = torch.full((1,), 5, dtype=torch.int32, device=dev)
        _lib.check(L.dagr_augment_events(par_ptr, B, W, H, _lib.ptr(pos), 2, _lib.ptr(t), 4, _lib.ptr(p), 1,
                                         _lib.ptr(ptr), N, _lib.ptr(out_pos), _lib.ptr(out_t), _lib.ptr(out_p), None,
                                         _lib.ptr(out_ptr), _lib.ptr(status), _lib.ptr(ws), ws_bytes, stream))
        return out_pos, out_t, out_p, out_ptr, status

    out_pos, out_t, out_p, out_ptr, status = run([0, 2000, 3000, N])
    _lib.check(L.dagr_augment_status(_lib.ptr(status), stream))
    assert int(status) == 0 and out_ptr.tolist() == [0, 2000, 3000, N]
    assert torch.equal(out_pos, pos) and torch.equal(out_t, t)           # identity records: nothing moves
    for bad in ([0, 3000, 2000, N], [1, 2000, 3000, N], [0, 2000, 3000, N - 1], [0, -5, 3000, N], [0, 2000, N + 9, N]):
        out_pos, out_t, out_p, out_ptr, status = run(bad)
        with pytest.raises(RuntimeError, match="sample_ptr"):
            _lib.check(L.dagr_augment_status(_lib.ptr(status), stream), "augment_events")
        assert int(status) & 1 and out_ptr.tolist() == [0] * (B + 1)
        assert bool((out_pos == -7).all()) and bool((out_t == -7).all()) and bool((out_p == -7).all())   # nothing written
    # host-side argument checks never reach the device
    one = ctypes.c_void_p(16)
    par_one = ctypes.cast(one, ctypes.POINTER(_lib.AugParams))
    assert L.dagr_augment_events(par_one, B, W, H, one, 3, one, 4, one, 1, one, N, one, one, one, None, one, one, one,
                                 ws_bytes, None) != 0 and b"pos_width" in L.dagr_last_error()
    assert L.dagr_augment_frames(par_one, 1, 3, H, W, 2, 1, one, one, None) != 0 and b"elem_bytes" in L.dagr_last_error()


def test_train_script_with_augment_on_device(tmp_path):
    """scripts/train_ncaltech101.py --augment_on_device for three iterations on the synthetic stream, in a process of its
    own under a time limit: exit status 0 and a finite mean loss over the iterations."""
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_ncaltech101.py"), "--config", "config/dagr-l-ncaltech.yaml",
           "--augment_on_device", "--max_iters", "3", "--samples", "16", "--val_samples", "4", "--batch_size", "4",
           "--n_nodes", "3000", "--output_directory", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DAGR_FORCE_DDP")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("epoch 0: loss")]
    assert len(lines) == 1, r.stdout[-2000:]
    assert np.isfinite(float(lines[0].split()[3])), lines[0]
