"""The event / frame / box transforms of ``src/dagr/data/augment.py``: the test-time ``Crop([0, 0], [1, 1])`` (:115-145,
``Augmentations.transform_testing`` :282-285) and the training chain of ``Augmentations.__init__`` (:287-294): horizontal
flip (:90-112), random crop with probability 0.2 (:201-243), random zoom (:148-198), random translation (:246-279), then
the crop to the sensor.  All of them act on the per-sample ``Data`` BEFORE the graph exists (host side, integer pixel
coordinates), exactly where the reference applies them (the loaders' ``transform``)."""
import copy
import ctypes

import numpy as np
import torch

from .. import _lib


class Compose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, data):
        for t in self.transforms:
            data = t(data)
        return data


class Crop:
    """Keep what lies inside [min, max) (fractions of the sensor size until ``init`` turns them into pixels)."""

    def __init__(self, min, max):
        self.min, self.max = torch.as_tensor(min), torch.as_tensor(max)
        self._pixels = False

    def init(self, height, width):
        size = torch.tensor([width, height], dtype=torch.float32)
        self.min = (self.min.float() * size).clamp(min=0).int()
        self.max = torch.minimum((self.max.float() * size), size).int()
        self._pixels = True

    def __call__(self, data):
        if not self._pixels:
            self.init(int(data.height), int(data.width))
        x0, y0 = int(self.min[0]), int(self.min[1])
        x1, y1 = int(self.max[0]), int(self.max[1])
        keep = (data.pos[:, 0] >= x0) & (data.pos[:, 0] < x1) & (data.pos[:, 1] >= y0) & (data.pos[:, 1] < y1)
        if not bool(keep.all()):
            for name in ("pos", "x", "t"):
                v = getattr(data, name, None)
                if torch.is_tensor(v) and v.shape[0] == keep.shape[0]:
                    setattr(data, name, v[keep])
        if (x0, y0) != (0, 0):
            data.pos = data.pos - torch.tensor([x0, y0], dtype=data.pos.dtype)
        if hasattr(data, "image"):
            data.image = data.image[..., y0:y1, x0:x1]
        for name in ("bbox", "bbox0"):
            b = getattr(data, name, None)
            if b is not None and len(b):
                b = b.clone()
                bx1 = (b[:, 0] + b[:, 2]).clamp(x0, x1 - 1)
                by1 = (b[:, 1] + b[:, 3]).clamp(y0, y1 - 1)
                b[:, 0] = b[:, 0].clamp(x0, x1 - 1)
                b[:, 1] = b[:, 1].clamp(y0, y1 - 1)
                b[:, 2], b[:, 3] = bx1 - b[:, 0], by1 - b[:, 1]
                b[:, 0] -= x0
                b[:, 1] -= y0
                setattr(data, name, b)
        return data


def init_transforms(transforms, height, width):
    for t in transforms:
        if hasattr(t, "init"):
            t.init(height=height, width=width)


def _each_box_field(data):
    for name in ("bbox", "bbox0"):
        b = getattr(data, name, None)
        if b is not None and len(b):
            yield name, b


class RandomHFlip:
    """Mirror the sample about the vertical axis with probability p (augment.py:90-112)."""

    def __init__(self, p):
        self.p = float(p)

    def __call__(self, data):
        if float(torch.rand(1)) > self.p:
            return data
        W = int(data.width)
        data.pos = data.pos.clone()
        data.pos[:, 0] = W - 1 - data.pos[:, 0]
        if hasattr(data, "image"):
            data.image = torch.flip(data.image, dims=[-1]).contiguous()
        for name, b in _each_box_field(data):
            b = b.clone()
            b[:, 0] = W - 1 - (b[:, 0] + b[:, 2])
            setattr(data, name, b)
        return data


REFERENCE_FRAME_CROP = True      # see _keep_window


def _keep_window(data, lo, hi):
    """Events inside [lo, hi] (inclusive, as augment.py:39-51 keeps them), frame cropped as the reference does it (below),
    boxes clamped."""
    keep = ((data.pos >= lo) & (data.pos <= hi)).all(dim=1)
    for name in ("pos", "x", "t"):
        v = getattr(data, name, None)
        if torch.is_tensor(v) and v.shape[0] == keep.shape[0]:
            setattr(data, name, v[keep])
    x0, y0, x1, y1 = int(lo[0]), int(lo[1]), int(hi[0]), int(hi[1])
    if hasattr(data, "image"):
        img = data.image.clone()
        if REFERENCE_FRAME_CROP:
            # augment.py:51-58 as written: the four assignments index the FIRST TWO dimensions of the [1, 3, H, W] frame
            # (batch, channel), not rows and columns -- any window that does not start in row 0 blanks the whole frame,
            # one that starts in column c > 0 of row 0 blanks the first min(c, 3) channels.  Kept: a model trained here
            # sees the frames the reference's training loop shows it.  REFERENCE_FRAME_CROP = False blanks outside the
            # window, which is what the function's name promises.
            img[:y0, :] = 0
            img[y1:, :] = 0
            img[:, :x0] = 0
            img[:, x1:] = 0
        else:
            img[..., :y0, :] = 0
            img[..., y1:, :] = 0
            img[..., :, :x0] = 0
            img[..., :, x1:] = 0
        data.image = img
    for name, b in _each_box_field(data):
        b = b.clone()
        far = b[:, :2] + b[:, 2:4]
        near = torch.minimum(torch.maximum(b[:, :2], lo.to(b.dtype)), hi.to(b.dtype))
        far = torch.minimum(torch.maximum(far, lo.to(b.dtype)), hi.to(b.dtype))
        b[:, :2], b[:, 2:4] = near, far - near
        setattr(data, name, b)
    return data


class RandomCrop:
    """With probability p keep a random window of ``size`` (fractions of the sensor) and drop the rest (augment.py:201-243);
    coordinates are NOT shifted: the window stays where it was."""

    def __init__(self, size=(0.75, 0.75), dim=(0, 1), p=0.5):
        self.size, self.dim, self.p = torch.as_tensor(size, dtype=torch.float32), list(dim), float(p)
        self.left_max = None

    def init(self, height, width):
        full = torch.tensor([width, height], dtype=torch.float32)
        self.size = torch.minimum((self.size * full), full - 1).clamp(min=0).int()
        self.left_max = full.int() - self.size

    def __call__(self, data):
        if self.left_max is None:
            self.init(int(data.height), int(data.width))
        if float(torch.rand(1)) > self.p:
            return data
        left = (torch.rand(len(self.dim)) * self.left_max).to(torch.int16)
        return _keep_window(data, left, left + self.size.to(torch.int16))


def subsample_events(pos, polarity, zoom):
    """Events of a shrunk sample (zoom < 1): each event spreads p * bilinear weights over the 4 surrounding pixels of an
    accumulator; a pixel emits an event whenever its accumulated magnitude exceeds 1 / zoom^2 (augment.py:13-36, a
    sequential integrate-and-fire: inherently ordered, a plain loop here where the reference uses numba)."""
    thr = 1.0 / float(zoom) ** 2
    H = int(pos[:, 1].max()) + 2 if len(pos) else 1
    W = int(pos[:, 0].max()) + 2 if len(pos) else 1
    acc = np.zeros((H, W), dtype=np.float32)
    keep = np.zeros(len(pos), dtype=bool)
    out = np.array(pos, dtype=np.float32, copy=True)
    for i in range(len(pos)):
        x, y = float(pos[i, 0]), float(pos[i, 1])
        for xl, yl in ((int(x), int(y)), (int(x + 1), int(y)), (int(x), int(y + 1)), (int(x + 1), int(y + 1))):
            acc[yl, xl] += np.float32(float(polarity[i]) * (1 - abs(x - xl)) * (1 - abs(y - yl)))
            sign = 1 if acc[yl, xl] > 0 else -1
            if sign * acc[yl, xl] > thr:
                acc[yl, xl] -= sign * thr
                keep[i] = True
                out[i, 0], out[i, 1] = xl, yl
    return out, keep


class RandomZoom:
    """Scale the sample about the sensor centre by a factor drawn from ``zoom`` = [lo, hi] (augment.py:148-198): events
    move to ((p - c) * z + c) truncated to int16 (events pushed out of the sensor are removed by the final Crop), boxes
    scale with them; the frame is resized (nearest) and centre-cropped / centre-padded to the sensor."""

    def __init__(self, zoom, subsample=False):
        self.zoom, self.subsample = list(zoom), bool(subsample)

    def init(self, height, width):
        pass

    def __call__(self, data):
        # the factor is a float32 tensor expression in the reference (augment.py:174): same roundings here
        z = float(torch.rand(1) * (self.zoom[1] - self.zoom[0]) + self.zoom[0])
        W, H = int(data.width), int(data.height)
        cx, cy = W // 2, H // 2
        pos = data.pos.float()
        zx = ((pos[:, 0] - cx) * z + cx)
        zy = ((pos[:, 1] - cy) * z + cy)
        if self.subsample and z < 1:
            # augment.py:178-182: the zoomed coordinates are int16 before the integrate-and-fire pass sees them (the
            # bilinear weights collapse onto the truncated pixel; the other three pixels still get their threshold check)
            p, keep = subsample_events(torch.stack([zx, zy], 1).to(torch.int16).numpy().astype(np.float32),
                                       data.x.reshape(-1).numpy(), z)
            data.pos = torch.from_numpy(p[keep].astype("int16"))
            data.x = data.x[torch.from_numpy(keep)]
            if hasattr(data, "t") and torch.is_tensor(data.t):
                data.t = data.t[torch.from_numpy(keep)]
        else:
            data.pos = torch.stack([zx, zy], 1).to(torch.int16)
        if hasattr(data, "image"):
            w2, h2 = int(np.ceil(W * z)), int(np.ceil(H * z))
            img = torch.nn.functional.interpolate(data.image.float(), size=(h2, w2), mode="nearest").to(data.image.dtype)
            px, py = (w2 - W) // 2, (h2 - H) // 2
            if px >= 0:
                data.image = img[..., py:py + H, px:px + W].contiguous()
            else:
                bg = torch.zeros_like(data.image)
                bg[..., -py:-py + h2, -px:-px + w2] = img
                data.image = bg
        for name, b in _each_box_field(data):
            b = b.clone()
            b[:, 2:4] *= z
            b[:, 0] = (b[:, 0] - cx) * z + cx
            b[:, 1] = (b[:, 1] - cy) * z + cy
            setattr(data, name, b)
        return data


class RandomTranslate:
    """Shift the sample by a random whole number of pixels within +-size (fractions of the sensor, augment.py:246-279);
    what leaves the sensor is removed by the final Crop, the frame is padded with black."""

    def __init__(self, size):
        self.size = torch.as_tensor(size, dtype=torch.float32)[:2]
        self.px = None

    def init(self, height, width):
        full = torch.tensor([width, height], dtype=torch.float32)
        self.px = torch.minimum(self.size * full, full - 1).clamp(min=0).int()

    def __call__(self, data):
        if self.px is None:
            self.init(int(data.height), int(data.width))
        move = (self.px * (torch.rand(2) * 2 - 1)).to(torch.int16)
        data.pos = data.pos + move
        if hasattr(data, "image"):
            H, W = data.image.shape[-2:]
            mx, my = int(move[0]), int(move[1])
            out = torch.zeros_like(data.image)
            xs0, xs1 = max(0, -mx), min(W, W - mx)
            ys0, ys1 = max(0, -my), min(H, H - my)
            if xs1 > xs0 and ys1 > ys0:
                out[..., ys0 + my:ys1 + my, xs0 + mx:xs1 + mx] = data.image[..., ys0:ys1, xs0:xs1]
            data.image = out
        for name, b in _each_box_field(data):
            b = b.clone()
            b[:, :2] += move.to(b.dtype)
            setattr(data, name, b)
        return data


# ``dagr_aug_params`` (include/dagr_hip.h): one record per sample, drawn on the host, read by the kernels on the device
AUG_PARAMS = np.dtype(_lib.AugParams)


class DeviceAugmentations:
    """The training chain of ``Augmentations`` (flip, random crop, zoom, translate, crop to the sensor) applied to a
    collated ``Batch`` that is already on the device (``dagr_augment_events`` / ``_frames`` / ``_boxes``, csrc/augment.hip).
    The random numbers still come from torch's RNG on the host, drawn call for call as the host chain draws them for one
    sample after another, so under one seed both chains make the same decisions and leave the same RNG state.  A batch
    from a shuffling ``DataLoader`` carries the per-sample seeds the loader gives the host chain (``_sample_seeds``, a
    function of (seed, epoch, sample) alone); its records are drawn from those, each in a forked RNG scope: a sample is
    augmented the same way whatever the rank, the world size or the batch it arrives in, and as the host chain in the
    loader would have augmented it.

    ``RandomZoom(subsample=True)`` with a factor below 1 (a sequential integrate-and-fire pass over the events) has no
    device form: ``aug_zoom < 1`` raises here; use the host chain (``Augmentations(args).transform_training``) for it."""

    def __init__(self, args):
        if float(args.aug_zoom) < 1:
            raise ValueError(f"DeviceAugmentations: aug_zoom = {args.aug_zoom} < 1 needs RandomZoom's event subsampling, "
                             "which only the host chain (Augmentations.transform_training) implements")
        self.p_flip = float(args.aug_p_flip)
        self.zoom = [1, args.aug_zoom]
        # the host transforms own the pixel sizes (their ``init``): the same roundings by construction
        self._crop = RandomCrop([0.75, 0.75], p=0.2)
        self._translate = RandomTranslate([args.aug_trans, args.aug_trans, 0])
        self.height = self.width = None

    def init(self, height, width):
        self._crop.init(height, width)
        self._translate.init(height, width)
        self.height, self.width = int(height), int(width)

    def draw(self, n, seeds=None):
        """``n`` parameter records (numpy, dtype ``AUG_PARAMS``) from torch's global RNG: per sample ``rand(1)`` (flip),
        ``rand(1)`` (crop coin) and ``rand(2)`` only when it hits, ``rand(1)`` (zoom), ``rand(2)`` (shift) -- the calls, order,
        dtypes and roundings of RandomHFlip / RandomCrop / RandomZoom / RandomTranslate.  With ``seeds`` (n ints) record k
        is drawn after ``manual_seed(seeds[k])`` inside a forked RNG scope, as ``DataLoader._fetch`` runs the host chain;
        the global stream is then left untouched."""
        if self.width is None:
            raise RuntimeError("DeviceAugmentations.init(height, width) has not been called")
        if seeds is not None:
            if len(seeds) != int(n):
                raise ValueError(f"{len(seeds)} seeds for {n} records")
            out = np.zeros(int(n), dtype=AUG_PARAMS)
            for k, s in enumerate(seeds):
                with torch.random.fork_rng(devices=[]):
                    torch.manual_seed(int(s))
                    out[k] = self.draw(1)[0]
            return out
        out = np.zeros(int(n), dtype=AUG_PARAMS)
        size = self._crop.size.to(torch.int16)
        for rec in out:
            rec["flip"] = 0 if float(torch.rand(1)) > self.p_flip else 1
            if not float(torch.rand(1)) > self._crop.p:
                left = (torch.rand(len(self._crop.dim)) * self._crop.left_max).to(torch.int16)
                rec["crop_on"], rec["crop_lo"], rec["crop_hi"] = 1, left.numpy(), (left + size).numpy()
            rec["zoom"] = (torch.rand(1) * (self.zoom[1] - self.zoom[0]) + self.zoom[0]).numpy()[0]
            rec["move"] = (self._translate.px * (torch.rand(2) * 2 - 1)).to(torch.int16).numpy()
        return out

    def __call__(self, batch, params=None):
        """A new ``Batch`` with the fields of ``batch`` (``pos`` int16 / int32 ``[N, 2]`` pixels, ``x``, ``t``, ``batch``,
        optionally ``image`` ``[B, C, H, W]`` uint8 / fp32 and ``bbox`` / ``bbox0`` with their ``*_batch`` vectors), augmented;
        ``pos`` comes back int16 as from the host chain.  ``params``: records of ``draw`` (default: ``draw(B)`` now, from the
        batch's per-sample seeds when a shuffling ``DataLoader`` made it, else from the global RNG).
        Everything is queued on the current stream; the call synchronises once, to read ``out_ptr[B]`` (the number of
        surviving events, which sizes the outputs) together with the status word."""
        if self.width is None:
            geo = getattr(batch, "_geometry", None)
            if geo is None:
                raise RuntimeError("DeviceAugmentations.init(height, width) has not been called")
            self.init(geo[1], geo[0])
        W, H = self.width, self.height
        pos, t, x = batch.pos, batch.t, batch.x
        if not pos.is_cuda:
            raise RuntimeError("DeviceAugmentations works on a batch that is on the GPU (batch.cuda() first); the host "
                               "chain is Augmentations.transform_training")
        if pos.dtype not in (torch.int16, torch.int32) or pos.dim() != 2 or pos.shape[1] != 2:
            raise TypeError(f"pos must be int16 / int32 [N, 2] pixel coordinates, got {pos.dtype} {tuple(pos.shape)}")
        dev, N, B = pos.device, int(pos.shape[0]), int(batch.num_graphs)
        if t.shape[0] != N or x.shape[0] != N or x.numel() != N or t.numel() != N:
            raise ValueError("pos, x and t must describe the same N events, one value each")
        if t.element_size() not in (4, 8):
            raise TypeError(f"t must have 4- or 8-byte entries, got {t.dtype}")
        if params is None:
            params = self.draw(B, getattr(batch, "_sample_seeds", None))
        params = np.ascontiguousarray(params, dtype=AUG_PARAMS)
        if len(params) != B:
            raise ValueError(f"{len(params)} parameter records for a batch of {B} samples")
        par = torch.from_numpy(params.view(np.int32).reshape(B, -1)).to(dev, non_blocking=True)
        # the segment bounds from the (sorted) sample vector, on the device: no read-back, and right for any batch
        ptr = torch.searchsorted(batch.batch.contiguous(), torch.arange(B + 1, device=dev)).to(torch.int32)
        return self._run(batch, par, ptr, pos.contiguous(), t.contiguous(), x.contiguous(), B, W, H)

    def _run(self, batch, par, ptr, pos, t, x, B, W, H):
        L, dev, N = _lib.lib(), pos.device, int(pos.shape[0])
        stream = _lib.cur_stream(dev)
        par_ptr = ctypes.cast(_lib.ptr(par), ctypes.POINTER(_lib.AugParams))        # the records on the device
        out_pos, out_t, out_x = torch.empty((N, 2), dtype=torch.int16, device=dev), torch.empty_like(t), torch.empty_like(x)
        out_batch = torch.empty(N, dtype=torch.long, device=dev)
        meta = torch.empty(B + 2, dtype=torch.int32, device=dev)           # out_ptr[B + 1], then the status word
        status = meta[B + 1:]
        ws_bytes = L.dagr_augment_workspace_bytes(N)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.dagr_augment_events(par_ptr, B, W, H, _lib.ptr(pos), pos.element_size(), _lib.ptr(t),
                                             t.element_size(), _lib.ptr(x), x.element_size(), _lib.ptr(ptr), N,
                                             _lib.ptr(out_pos), _lib.ptr(out_t), _lib.ptr(out_x), _lib.ptr(out_batch),
                                             _lib.ptr(meta), _lib.ptr(status), _lib.ptr(ws), ws_bytes, stream),
                       "augment_events")
            out = copy.copy(batch)
            image = getattr(batch, "image", None)
            if torch.is_tensor(image):
                if image.dim() != 4 or image.shape[0] != B or tuple(image.shape[-2:]) != (H, W) \
                        or image.dtype not in (torch.uint8, torch.float32):
                    raise TypeError(f"image must be uint8 / float32 [{B}, C, {H}, {W}], got {image.dtype} {tuple(image.shape)}")
                image = image.contiguous()
                out.image = torch.empty_like(image)
                _lib.check(L.dagr_augment_frames(par_ptr, B, int(image.shape[1]), H, W, image.element_size(),
                                                 1 if REFERENCE_FRAME_CROP else 0, _lib.ptr(image), _lib.ptr(out.image),
                                                 stream), "augment_frames")
            for name in ("bbox", "bbox0"):
                b = getattr(batch, name, None)
                if not torch.is_tensor(b) or b.shape[0] == 0:
                    continue
                rows = b.to(torch.float32).contiguous()
                new = torch.empty_like(rows)
                _lib.check(L.dagr_augment_boxes(par_ptr, B, W, H, _lib.ptr(rows),
                                                _lib.ptr(getattr(batch, name + "_batch").to(torch.long).contiguous()),
                                                int(rows.shape[0]), int(rows.shape[1]), _lib.ptr(new), stream),
                           "augment_boxes")
                setattr(out, name, new.to(b.dtype))
            n_out, st = meta[B:].tolist()                                  # the one synchronisation of the call
            if st:
                _lib.check(L.dagr_augment_status(_lib.ptr(status), stream), "augment_events")
        out.pos, out.t, out.x, out.batch = out_pos[:n_out], out_t[:n_out], out_x[:n_out], out_batch[:n_out]
        out.__dict__["_event_ptr"] = meta[:B + 1]
        return out


class Augmentations:
    transform_testing = Compose([Crop([0, 0], [1, 1])])

    def __init__(self, args):
        """augment.py:287-294: the training chain, parameterised by ``aug_p_flip`` / ``aug_zoom`` / ``aug_trans``."""
        self._args = args
        self._device_chain = None
        self.transform_training = Compose([
            RandomHFlip(p=args.aug_p_flip),
            RandomCrop([0.75, 0.75], p=0.2),
            RandomZoom(zoom=[1, args.aug_zoom], subsample=True),
            RandomTranslate([args.aug_trans, args.aug_trans, 0]),
            Crop([0, 0], [1, 1]),
        ])

    @property
    def transform_training_device(self):
        """The same chain for a collated batch on the GPU (``DeviceAugmentations``; built on first use)."""
        if self._device_chain is None:
            self._device_chain = DeviceAugmentations(self._args)
        return self._device_chain
