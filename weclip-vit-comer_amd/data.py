"""Synthetic VOC-shaped input for the data-parallel step: per-rank seeded batches that
differ from step to step, resident on the device.

The reference's loader (datasets/voc.py:190-250 + datasets/transforms.py) decodes JPEGs on the host, rescales /
flips / crops with numpy + PIL and normalises with mean/std (transforms.py:8-15); its output per step is a float32
(B, 3, crop, crop) tensor of ~N(0,1) pixels plus the image-level class ids.  No dataset exists offline, so this
loader draws that output directly: a pool of `pool` distinct batches per rank (seed = f(base seed, rank)), cycled.
"""
import torch

from . import synth


class SyntheticVOCLoader:
    """Iterable of (images (B,3,S,S) f32 CUDA, label lists) -- `DistributedSampler`-like: rank r of `world` draws
    from its own seed stream, so no two ranks (and no two consecutive steps) see the same tensor.

    source="float": the pool holds ready normalised batches (what the parity tests feed).
    source="uint8": the pool holds uint8 (B, 375, 500, 3) "decoded JPEGs" on the device and every next() runs the
    device-side input pipeline (DeviceAugment: random rescale / flip / pad + crop / normalise, csrc/augment.hip) --
    the per-step work of the reference's loader, minus JPEG decoding, on the GPU and inside the timed step.
    source="seg": the fully supervised variant's input -- uint8 images plus uint8 ground-truth maps
    (synth.make_label_maps) on the device; every next() runs DeviceSegAugment (csrc/augment_seg.hip) and yields
    (images (B,3,S,S) f32, labels (B,S,S) int64), what SupervisedTrainStep takes."""

    def __init__(self, batch, size, classes_per_image=2, rank=0, world=1, seed=100, pool=4, device="cuda",
                 n_classes=20, source="float", src_hw=(375, 500)):
        self.batch, self.size, self.rank, self.world, self.source = batch, size, rank, world, source
        self.images, self.labels = [], []
        for j in range(pool):
            s = seed + 1000 * j + rank            # j = 0, rank = 0 is bench.py's historical batch (seed 100 / 7)
            if source in ("uint8", "seg"):
                f = synth.make_images(batch, src_hw[0], src_hw[1], seed=s)
                u8 = (f * 58.0 + 118.0).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
                self.images.append(u8.to(device))
            else:
                self.images.append(synth.make_images(batch, size, size, seed=s).to(device))
            if source == "seg":
                self.labels.append(synth.make_label_maps(batch, src_hw[0], src_hw[1], n_classes=n_classes + 1,
                                                         seed=7 + 1000 * j + rank).to(device))
            else:
                self.labels.append(synth.make_label_lists(batch, classes_per_image, n_classes=n_classes,
                                                          seed=7 + 1000 * j + rank))
        self.aug = DeviceAugment(crop_size=size, seed=seed + rank) if source == "uint8" else None
        if source == "seg":
            self.aug = DeviceSegAugment(crop_size=size, seed=seed + rank)
        self._i = 0

    def __len__(self):
        return len(self.images)

    def next(self):
        i = self._i % len(self.images)
        self._i += 1
        if self.source == "seg":
            return self.aug(self.images[i], self.labels[i])[:2]
        if self.aug is not None:
            return self.aug(self.images[i]), self.labels[i]
        return self.images[i], self.labels[i]

    def __iter__(self):
        while True:
            yield self.next()


MEAN = (123.675, 116.28, 103.53)       # datasets/transforms.py:8
STD = (58.395, 57.12, 57.375)


def _check_rescale(who, b, H, W, rh, rw):
    """Precondition of the Pillow tables (csrc/resample.h) for image b: (H, W) -> (rh, rw).  Raises, never poisons."""
    if rh < 1 or rw < 1 or H > 4 * rh or W > 4 * rw:
        raise RuntimeError(f"{who}: image {b} ({H}x{W} -> {rh}x{rw}): rescaled size must be >= 1 and "
                           "down-scaling at most 4x")


def _workspace(ws, n_ints, device):
    """`ws` if it holds n_ints int32 on `device`, else a new buffer that does."""
    if ws is None or ws.numel() < n_ints or ws.device != device:
        ws = torch.empty(n_ints, device=device, dtype=torch.int32)
    return ws


class DeviceAugment:
    """The reference's train-time augmentation (datasets/voc.py:108-143: random_scaling -> random_fliplr -> random_crop
    -> normalize_img -> CHW) with the random draws on the host and the pixel work in HIP kernels (csrc/augment.hip):
    uint8 (B,H,W,3) on the device in, float32 (B,3,crop,crop) normalised out, the rescale being Pillow's BILINEAR for
    8-bit images bit for bit (up- and down-scaling).  The host never touches a pixel, so the loader cannot serialise
    the step.

    The draws follow the reference's own sources and order per image -- `random.uniform` (scale, transforms.py:31),
    `random.random` (flip, :71), `np.random.randint` x 2 (pad offsets, :134-135), `random.randrange` x 2 (crop box,
    :143-146; without a label map the first box is taken) -- from private `random.Random(seed)` /
    `np.random.RandomState(seed)` instances, so a loader seeded like the reference's worker produces its crops."""

    def __init__(self, crop_size=512, rescale_range=(0.5, 2.0), fliplr=True, seed=0, mean=MEAN, std=STD, np_seed=None):
        import random
        import numpy as np
        self.crop, self.range, self.fliplr = int(crop_size), tuple(rescale_range) if rescale_range else None, bool(fliplr)
        self.py_rng = random.Random(seed)
        self.np_rng = np.random.RandomState(seed if np_seed is None else np_seed)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self._ws = None

    def draw_one(self, H, W):
        """(scale, flip, rh, rw, pad_y, pad_x, crop_y, crop_x) of one image."""
        s = self.py_rng.uniform(*self.range) if self.range else 1.0
        rh, rw = (int(s * H), int(s * W)) if self.range else (H, W)
        flip = int(self.py_rng.random() > 0.5) if self.fliplr else 0
        ch, cw = max(self.crop, rh), max(self.crop, rw)                  # canvas (transforms.py:123-124)
        pad_y, pad_x = int(self.np_rng.randint(ch - rh + 1)), int(self.np_rng.randint(cw - rw + 1))
        crop_y = self.py_rng.randrange(0, ch - self.crop + 1, 1)
        crop_x = self.py_rng.randrange(0, cw - self.crop + 1, 1)
        return s, flip, rh, rw, pad_y, pad_x, crop_y, crop_x

    @staticmethod
    def pack(draws):
        """List of draw_one() tuples -> int32 tensor (B, 8) in the kernel's record layout."""
        import numpy as np
        rec = np.zeros((len(draws), 8), np.int32)
        for b, d in enumerate(draws):
            rec[b, 0] = np.float32(d[0]).view(np.int32)
            rec[b, 1:] = d[1:]
        return torch.from_numpy(rec)

    def draw(self, B, H, W):
        """Host-side random parameters of one batch -> int32 tensor (B, 8) in the kernel's record layout."""
        return self.pack([self.draw_one(H, W) for _ in range(B)])

    def _buffers(self, B, device):
        """The output of one call, with the coefficient workspace grown to the batch."""
        import ctypes
        from . import _lib as L
        n = ctypes.c_long(0)
        L.lib().wc_augment_workspace_ints(B, self.crop, ctypes.byref(n))
        self._ws = _workspace(self._ws, n.value, device)
        return torch.empty(B, 3, self.crop, self.crop, device=device, dtype=torch.float32)

    def __call__(self, images_u8, params=None):
        """images_u8 (B,H,W,3) uint8 CUDA; params: a draw() result (default: a fresh draw).  -> (B,3,crop,crop) f32."""
        import ctypes
        from . import _lib as L
        L.require_gpu()
        B, H, W, C = images_u8.shape
        if C != 3 or images_u8.dtype != torch.uint8:
            raise RuntimeError("DeviceAugment expects uint8 (B, H, W, 3) images")
        if params is None:
            params = self.draw(B, H, W)
        if not params.is_cuda:
            rhw = params[:, 2:4]
            if int(rhw.min()) < 1 or H > 4 * int(rhw[:, 0].min()) or W > 4 * int(rhw[:, 1].min()):
                raise RuntimeError("DeviceAugment: rescaled size must be >= 1 and down-scaling at most 4x")
        p = params.pin_memory().to(images_u8.device, non_blocking=True) if not params.is_cuda else params
        out = self._buffers(B, images_u8.device)
        L.lib().wc_augment_normalize(L.ptr(images_u8.contiguous(), torch.uint8, "images"), L.ptr(p, torch.int32, "params"),
                                     L.ptr(out), L.ptr(self._ws, torch.int32), B, H, W, self.crop,
                                     (ctypes.c_float * 3)(*self.mean), (ctypes.c_float * 3)(*self.std), L.stream())
        return out

    def check_ragged(self, params, sizes):
        """Host-side precondition of the kernels for host-resident records and a list of (H, W): raises, never poisons."""
        for b, (H, W) in enumerate(sizes):
            _check_rescale("DeviceAugment", b, H, W, int(params[b, 2]), int(params[b, 3]))

    def ragged(self, src_u8, offsets, sizes, params):
        """A batch of images of different sizes (csrc/augment.hip, wc_augment_normalize_ragged): src_u8 flat uint8 CUDA, the
        images HWC back to back; offsets (B) int64 / sizes (B,2) int32 {H, W} / params (B,8) int32 CUDA tensors (views of one
        buffer are fine).  -> (B,3,crop,crop) f32 on the current stream; nothing synchronises with the host."""
        import ctypes
        from . import _lib as L
        L.require_gpu()
        B = int(offsets.shape[0])
        if src_u8.dtype != torch.uint8 or src_u8.dim() != 1 or tuple(sizes.shape) != (B, 2) or tuple(params.shape) != (B, 8):
            raise RuntimeError("DeviceAugment.ragged expects a flat uint8 source, (B) offsets, (B,2) sizes, (B,8) params")
        out = self._buffers(B, src_u8.device)
        L.lib().wc_augment_normalize_ragged(L.ptr(src_u8, torch.uint8, "src"), src_u8.numel(), L.ptr(offsets, torch.int64, "offsets"),
                                            L.ptr(sizes, torch.int32, "sizes"), L.ptr(params, torch.int32, "params"), L.ptr(out),
                                            L.ptr(self._ws, torch.int32), B, self.crop, (ctypes.c_float * 3)(*self.mean),
                                            (ctypes.c_float * 3)(*self.std), L.stream())
        return out

    @staticmethod
    def img_box(draw, crop):
        """`img_box` of random_crop (datasets/transforms.py:162-166) from one draw_one() tuple, int16 like the reference's."""
        import numpy as np
        _, _, rh, rw, pad_y, pad_x, crop_y, crop_x = draw
        return np.asarray([max(pad_y - crop_y, 0), min(crop_y + crop, pad_y + rh), max(pad_x - crop_x, 0),
                           min(crop_x + crop, pad_x + rw)], dtype=np.int16)


def normalize_u8(image_u8, label_u8=None, mean=MEAN, std=STD):
    """The aug=False path on the device (wc_normalize_u8): image (H,W,3) uint8 CUDA -> (3,H,W) f32 `normalize_img`
    (datasets/transforms.py:8-15, evaluated in double precision and rounded once, as numpy does for a uint8 image) and, if
    given, label (H,W) uint8 -> int64.  -> image or (image, label)."""
    import ctypes
    from . import _lib as L
    L.require_gpu()
    H, W, C = image_u8.shape
    if C != 3 or image_u8.dtype != torch.uint8:
        raise RuntimeError("normalize_u8 expects a uint8 (H, W, 3) image")
    if label_u8 is not None and (label_u8.dtype != torch.uint8 or tuple(label_u8.shape) != (H, W)):
        raise RuntimeError("normalize_u8 expects a uint8 (H, W) label map of the image's size")
    out = torch.empty(3, H, W, device=image_u8.device, dtype=torch.float32)
    lab = None if label_u8 is None else torch.empty(H, W, device=image_u8.device, dtype=torch.int64)
    L.lib().wc_normalize_u8(L.ptr(image_u8, torch.uint8, "image"), L.ptr(label_u8, torch.uint8, "label"), L.ptr(out),
                            L.ptr(lab, torch.int64, "label out"), H, W, (ctypes.c_double * 3)(*[float(v) for v in mean]),
                            (ctypes.c_double * 3)(*[float(v) for v in std]), L.stream())
    return out if lab is None else (out, lab)


class DeviceSegAugment:
    """The reference's label-aware train-time augmentation of the fully supervised variant (`VOC12SegDataset.__transforms`,
    datasets/voc.py:216-251: random_fliplr(image, label) -> PhotoMetricDistortion -> random_crop(image, label) ->
    normalize_img -> CHW; optionally random_scaling(image, label) first, which the reference has commented out, hence
    rescale_range=None) with the random draws on the host and all pixel work in HIP kernels (csrc/augment_seg.hip):
    uint8 (B,H,W,3) images and uint8 (B,H,W) label maps on the device in; float32 (B,3,crop,crop) image, int64
    (B,crop,crop) label (ignore_index in the padding) and int32 (B,4) img_box out.  The label-aware crop box
    (get_random_cropbox, transforms.py:137-156) is chosen on the device from `n_cand` host-drawn candidates and never
    returns to the host; `self.sel` (B,4) int32 {H_start, W_start, chosen candidate, accepted} of the last call stays on
    the device for inspection.

    Draw order per image, from private `random.Random(seed)` / `np.random.RandomState(seed)` instances, follows the
    reference's sources: [`random.uniform` (scale)] -> `random.random` (flip) -> the draws of
    PhotoMetricDistortion.__call__ (`np.random.randint(2)` gates, `random.uniform` amounts, `np.random.randint(-18, 18)`
    for hue, the `mode` draw) -> `np.random.randint` x 2 (pad) -> `random.randrange` x 2 per candidate.
    DELIBERATE DIFFERENCE: the reference stops drawing candidates at the first accepted one; that needs the histogram
    result on the host, so this pipeline always draws all `n_cand`.  The chosen box has the same distribution, but a
    seeded loader does not replay a reference worker's random stream past the first image.  Given the same candidate list
    the result is identical (tests/golden/seg_augment_ref.npz).

    Pinned to the unmodified reference code, exactly: flip, brightness, contrast, pad, crop-box selection, label handling,
    img_box, normalisation (and Pillow's BILINEAR / NEAREST when rescaling).  Saturation and hue go through OpenCV's 8-bit
    BGR<->HSV conversions, which are pinned to a restatement (tests/photo_ref.py), UNVERIFIED AGAINST REAL OPENCV."""

    N_CAND = 10                                                            # transforms.py:139

    def __init__(self, crop_size=512, rescale_range=None, fliplr=True, photometric=True, ignore_index=255, seed=0, mean=MEAN,
                 std=STD, np_seed=None, n_cand=N_CAND, brightness_delta=32, contrast_range=(0.5, 1.5),
                 saturation_range=(0.5, 1.5), hue_delta=18):
        import random
        import numpy as np
        self.crop, self.range, self.fliplr = int(crop_size), tuple(rescale_range) if rescale_range else None, bool(fliplr)
        self.photometric, self.ignore_index, self.n_cand = bool(photometric), int(ignore_index), int(n_cand)
        self.brightness_delta, self.contrast_range = brightness_delta, tuple(contrast_range)
        self.saturation_range, self.hue_delta = tuple(saturation_range), int(hue_delta)
        self.py_rng = random.Random(seed)
        self.np_rng = np.random.RandomState(seed if np_seed is None else np_seed)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.draw_names = []               # generator method names of the last draw_one(), in call order
        self._ws = None
        self.sel = None

    def _py(self, name, *a):
        self.draw_names.append(name)
        return getattr(self.py_rng, name)(*a)

    def _np(self, *a):
        self.draw_names.append("randint")
        return int(self.np_rng.randint(*a))

    def draw_one(self, H, W):
        """(scale, flip, rh, rw, pad_y, pad_x, photo, beta, alpha_c, alpha_s, hue, candidates) of one image; photo is the
        kernel's bit set (1 brightness, 2 contrast, 4 saturation, 8 hue, 16 mode), candidates a list of (H_start, W_start)."""
        self.draw_names = []
        s = self._py("uniform", *self.range) if self.range else 1.0
        rh, rw = (int(s * H), int(s * W)) if self.range else (H, W)
        flip = int(self._py("random") > 0.5) if self.fliplr else 0
        photo, beta, alpha_c, alpha_s, hue = 0, 0.0, 1.0, 1.0, 0
        if self.photometric:                                               # PhotoMetricDistortion.__call__, transforms.py:235-264
            def contrast():
                if self._np(2):
                    return 2, self._py("uniform", *self.contrast_range)
                return 0, 1.0
            if self._np(2):
                photo |= 1
                beta = self._py("uniform", -self.brightness_delta, self.brightness_delta)
            mode = self._np(2)
            photo |= 16 * mode
            if mode == 1:
                bit, alpha_c = contrast()
                photo |= bit
            if self._np(2):
                photo |= 4
                alpha_s = self._py("uniform", *self.saturation_range)
            if self._np(2):
                photo |= 8
                hue = self._np(-self.hue_delta, self.hue_delta)
            if mode == 0:
                bit, alpha_c = contrast()
                photo |= bit
        ch, cw = max(self.crop, rh), max(self.crop, rw)                    # canvas (transforms.py:123-124)
        pad_y, pad_x = self._np(ch - rh + 1), self._np(cw - rw + 1)
        cands = []
        for _ in range(self.n_cand):
            y = self._py("randrange", 0, ch - self.crop + 1, 1)
            cands.append((y, self._py("randrange", 0, cw - self.crop + 1, 1)))
        return s, flip, rh, rw, pad_y, pad_x, photo, beta, alpha_c, alpha_s, hue, cands

    def pack(self, draws):
        """List of draw_one() tuples -> (int32 (B, 16) records, int32 (B, n_cand, 2) candidates) in the kernels' layout.
        A candidate list shorter than n_cand is filled up by repeating its last entry (the selection cannot change: the
        repeated box is accepted or rejected like the entry it repeats, and the last candidate is the fall-back)."""
        import numpy as np
        rec = np.zeros((len(draws), 16), np.int32)
        cand = np.zeros((len(draws), self.n_cand, 2), np.int32)
        f32 = lambda v: np.float32(v).view(np.int32)                       # noqa: E731
        for b, d in enumerate(draws):
            rec[b, 0] = f32(d[0])
            rec[b, 1:7] = d[1:7]
            rec[b, 7], rec[b, 8], rec[b, 9] = f32(d[7]), f32(d[8]), f32(d[9])
            rec[b, 10] = d[10]
            c = list(d[11])
            if not 1 <= len(c) <= self.n_cand:
                raise RuntimeError(f"DeviceSegAugment: 1 to {self.n_cand} candidates per image, got {len(c)}")
            cand[b] = c + [c[-1]] * (self.n_cand - len(c))
        return torch.from_numpy(rec), torch.from_numpy(cand)

    def draw(self, B, H, W):
        """Host-side random parameters of one batch -> (records, candidates), see pack()."""
        return self.pack([self.draw_one(H, W) for _ in range(B)])

    def canvas_max(self, H, W):
        """Upper bound of the padded canvas side over every draw (sizes the kernels' per-coordinate tables)."""
        hi = self.range[1] if self.range else 1.0
        return max(self.crop, int(hi * H), int(hi * W))

    def _buffers(self, B, canvas_max, dev):
        """(image, label, img_box, sel) of one call, with the workspace grown to the batch."""
        import ctypes
        from . import _lib as L
        n = ctypes.c_long(0)
        L.lib().wc_seg_augment_workspace_ints(B, self.crop, canvas_max, self.n_cand, ctypes.byref(n))
        self._ws = _workspace(self._ws, n.value, dev)
        return (torch.empty(B, 3, self.crop, self.crop, device=dev, dtype=torch.float32),
                torch.empty(B, self.crop, self.crop, device=dev, dtype=torch.int64),
                torch.empty(B, 4, device=dev, dtype=torch.int32), torch.empty(B, 4, device=dev, dtype=torch.int32))

    def __call__(self, images_u8, labels_u8, params=None):
        """images_u8 (B,H,W,3) / labels_u8 (B,H,W) uint8 CUDA; params: a draw() / pack() result, host or device resident
        (default: a fresh draw).  -> (image (B,3,crop,crop) f32, label (B,crop,crop) int64, img_box (B,4) int32).
        With device-resident params nothing here synchronises with the host: five kernels and one memset on the current
        stream, capturable in a graph as one linear chain."""
        import ctypes
        from . import _lib as L
        L.require_gpu()
        B, H, W, C = images_u8.shape
        if C != 3 or images_u8.dtype != torch.uint8:
            raise RuntimeError("DeviceSegAugment expects uint8 (B, H, W, 3) images")
        if labels_u8.dtype != torch.uint8 or tuple(labels_u8.shape) != (B, H, W):
            raise RuntimeError("DeviceSegAugment expects uint8 (B, H, W) label maps of the images' size")
        rec, cand = self.draw(B, H, W) if params is None else params
        cm = self.canvas_max(H, W)
        if tuple(rec.shape) != (B, 16) or tuple(cand.shape) != (B, self.n_cand, 2):
            raise RuntimeError("DeviceSegAugment: params must be (B, 16) records and (B, n_cand, 2) candidates")
        if not rec.is_cuda:
            rhw = rec[:, 2:4]
            if int(rhw.min()) < 1 or H > 4 * int(rhw[:, 0].min()) or W > 4 * int(rhw[:, 1].min()) or int(rhw.max()) > cm:
                raise RuntimeError("DeviceSegAugment: rescaled size must be >= 1, within rescale_range and down-scaling at most 4x")
            lim = (rhw.clamp(min=self.crop) - self.crop)[:, None, :]
            if not cand.is_cuda and (int(cand.min()) < 0 or bool((cand > lim).any())):
                raise RuntimeError("DeviceSegAugment: candidate box outside the padded canvas")
        dev = images_u8.device
        rec = rec if rec.is_cuda else rec.pin_memory().to(dev, non_blocking=True)
        cand = cand if cand.is_cuda else cand.pin_memory().to(dev, non_blocking=True)
        out, lab, box, sel = self._buffers(B, cm, dev)
        L.lib().wc_seg_augment(L.ptr(images_u8.contiguous(), torch.uint8, "images"), L.ptr(labels_u8.contiguous(), torch.uint8, "labels"),
                               L.ptr(rec, torch.int32, "params"), L.ptr(cand, torch.int32, "candidates"), L.ptr(out),
                               L.ptr(lab, torch.int64), L.ptr(sel), L.ptr(box), L.ptr(self._ws, torch.int32), B, H, W, self.crop,
                               cm, self.n_cand, self.ignore_index, (ctypes.c_float * 3)(*self.mean),
                               (ctypes.c_float * 3)(*self.std), L.stream())
        self.sel = sel
        return out, lab, box

    @staticmethod
    def img_box(draw, crop, start):
        """`img_box` of random_crop (datasets/transforms.py:162-166) from one draw_one() tuple and the crop origin
        (H_start, W_start) the device chose for it (`sel[b, :2]`), int32 like the kernel's: a host restatement for checks."""
        import numpy as np
        _, _, rh, rw, pad_y, pad_x = draw[:6]
        cy, cx = int(start[0]), int(start[1])
        return np.asarray([max(pad_y - cy, 0), min(cy + crop, pad_y + rh), max(pad_x - cx, 0), min(cx + crop, pad_x + rw)],
                          dtype=np.int32)

    def check_ragged(self, rec, cand, sizes):
        """Host-side preconditions for host-resident records and a list of (H, W); -> canvas_max of the batch."""
        cm = self.crop
        for b, (H, W) in enumerate(sizes):
            rh, rw = int(rec[b, 2]), int(rec[b, 3])
            _check_rescale("DeviceSegAugment", b, H, W, rh, rw)
            lim = torch.tensor([max(rh, self.crop) - self.crop, max(rw, self.crop) - self.crop], dtype=cand.dtype)
            if int(cand[b].min()) < 0 or bool((cand[b] > lim).any()):
                raise RuntimeError("DeviceSegAugment: candidate box outside the padded canvas")
            cm = max(cm, rh, rw)
        return cm

    def ragged(self, src_u8, lab_u8, offsets, sizes, rec, cand, canvas_max):
        """A batch of images of different sizes (csrc/augment_seg.hip, wc_seg_augment_ragged): src_u8 flat uint8 CUDA, the
        images HWC back to back, lab_u8 their label maps in the same order (map b at byte offsets[b] / 3); offsets (B) int64,
        sizes (B,2) int32, rec (B,16) int32, cand (B,n_cand,2) int32 CUDA tensors; canvas_max: max(crop, rh, rw) over the
        batch (check_ragged).  -> (image, label, img_box) as __call__, on the current stream, without host synchronisation."""
        import ctypes
        from . import _lib as L
        L.require_gpu()
        B, dev = int(offsets.shape[0]), src_u8.device
        if src_u8.dtype != torch.uint8 or src_u8.dim() != 1 or lab_u8.dim() != 1 or 3 * lab_u8.numel() < src_u8.numel():
            raise RuntimeError("DeviceSegAugment.ragged expects flat uint8 buffers, the labels one third of the images")
        if tuple(sizes.shape) != (B, 2) or tuple(rec.shape) != (B, 16) or tuple(cand.shape) != (B, self.n_cand, 2):
            raise RuntimeError("DeviceSegAugment.ragged: (B,2) sizes, (B,16) records, (B,n_cand,2) candidates")
        out, lab, box, sel = self._buffers(B, int(canvas_max), dev)
        L.lib().wc_seg_augment_ragged(L.ptr(src_u8, torch.uint8, "images"), L.ptr(lab_u8, torch.uint8, "labels"), src_u8.numel(),
                                      L.ptr(offsets, torch.int64, "offsets"), L.ptr(sizes, torch.int32, "sizes"),
                                      L.ptr(rec, torch.int32, "params"), L.ptr(cand, torch.int32, "candidates"), L.ptr(out),
                                      L.ptr(lab, torch.int64), L.ptr(sel), L.ptr(box), L.ptr(self._ws, torch.int32), B, self.crop,
                                      int(canvas_max), self.n_cand, self.ignore_index, (ctypes.c_float * 3)(*self.mean),
                                      (ctypes.c_float * 3)(*self.std), L.stream())
        self.sel = sel
        return out, lab, box
