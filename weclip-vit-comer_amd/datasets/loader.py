"""DeviceLoader: a dataset on disk -> batches on the device, in place of `DistributedSampler` + `DataLoader` over the
reference's host transforms (scripts/dist_clip_voc.py, datasets/voc.py + datasets/transforms.py).

Host threads decode the files (Pillow releases the GIL); every batch then travels as ONE packed uint8 buffer and the whole
augmentation runs in the ragged HIP kernels (csrc/augment.hip, csrc/augment_seg.hip).  There are no worker processes: nothing
forks or re-executes a process that has opened the GPU.

Packed batch (pack_batch):

    [ image 0 HWC | image 1 | ... | image B-1 ]            offsets[b] = running sum of H*W*3, no padding between images
    [ label 0 HW | ... | label B-1 ]                       Seg datasets only; label b at images_bytes + offsets[b] / 3
    [ offsets int64 (B) | sizes int32 (B,2) {H, W} | parameter records int32 | crop candidates int32 | img_box | cls_labels ]
                                                           every table starts at a multiple of 16 bytes

BUFFER-REUSE INVARIANT.  The loader owns `prefetch + 1` (at least two) slots, each a pinned host buffer, a device buffer and
two events.  Slot s is refilled only when both hold:
  (1) the host does not write pinned[s] before `copied[s]` has passed (event.synchronize(): the previous H2D copy out of it
      has finished), and
  (2) the side stream does not start the next H2D copy into device[s] before `consumed[s]`, which is recorded on the
      consumer's stream right after the kernel that reads device[s] has been ENQUEUED there (a slot is restaged only after
      its batch was handed to the kernel; the side stream waits on the event, the host does not).
The augmentation kernel itself runs on the consumer's current stream after `wait_event(copied[s])`.
"""
import collections
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ..data import DeviceAugment, DeviceSegAugment

MAX_THREADS = 8


def index_plan(n, batch_size, shuffle=True, drop_last=False, seed=0, epoch=0, rank=0, world=1):
    """The batches (lists of dataset indices) of one rank in one epoch.  The epoch order is a permutation seeded by
    (seed, epoch), identical on every rank; rank r takes every world-th entry from position r on, so the ranks PARTITION the
    epoch (nothing is repeated to even the shares out, unlike DistributedSampler's padding: with n % world != 0 the shares
    differ by one index, and `drop_last=True` is what keeps the ranks' batch counts equal whenever that matters).
    drop_last drops a rank's trailing partial batch."""
    if not (0 <= rank < world) or batch_size < 1:
        raise ValueError("index_plan: need 0 <= rank < world and batch_size >= 1")
    order = np.random.RandomState([int(seed), int(epoch)]).permutation(n) if shuffle else np.arange(n)
    mine = [int(i) for i in order[rank::world]]
    batches = [mine[k:k + batch_size] for k in range(0, len(mine), batch_size)]
    if drop_last and batches and len(batches[-1]) < batch_size:
        batches.pop()
    return batches


def pack_batch(images, labels=None, tables=(), out=None):
    """Write a batch into one uint8 buffer in the layout of the module docstring.  images: uint8 (H,W,3) arrays; labels: None
    or uint8 (H,W) arrays; tables: arrays of any dtype appended after offsets and sizes.  out: a uint8 array to write into (it must
    be large enough) or None to allocate.  -> (buffer, offsets int64 (B), sizes int32 (B,2), layout) where layout maps
    "images" / "labels" / "offsets" / "sizes" / "table<i>" to (byte start, byte end) and "total" to the bytes used."""
    B = len(images)
    sizes = np.array([im.shape[:2] for im in images], np.int32).reshape(B, 2)
    nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    img_bytes = int(nbytes.sum())
    lab_bytes = img_bytes // 3 if labels is not None else 0
    layout = {"images": (0, img_bytes), "labels": (img_bytes, img_bytes + lab_bytes)}
    pos = img_bytes + lab_bytes
    parts = [("offsets", offsets), ("sizes", sizes)] + [(f"table{i}", np.ascontiguousarray(t)) for i, t in enumerate(tables)]
    for key, arr in parts:
        pos = -(-pos // 16) * 16
        layout[key] = (pos, pos + arr.nbytes)
        pos += arr.nbytes
    layout["total"] = pos
    buf = np.empty(pos, np.uint8) if out is None else out
    if buf.dtype != np.uint8 or buf.ndim != 1 or buf.size < pos:
        raise ValueError(f"pack_batch: need a flat uint8 buffer of at least {pos} bytes")
    for b, im in enumerate(images):
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError("pack_batch: images must be uint8 (H, W, 3)")
        buf[offsets[b]:offsets[b] + nbytes[b]] = im.reshape(-1)
        if labels is not None:
            if labels[b].dtype != np.uint8 or labels[b].shape != im.shape[:2]:
                raise ValueError("pack_batch: labels must be uint8 (H, W) of their image's size")
            o = img_bytes + offsets[b] // 3
            buf[o:o + nbytes[b] // 3] = labels[b].reshape(-1)
    buf[img_bytes + lab_bytes:pos] = 0
    for key, arr in parts:
        buf[layout[key][0]:layout[key][1]] = arr.reshape(-1).view(np.uint8)
    return buf, offsets, sizes, layout


def labels_from_onehot(cls_labels):
    """(B, C) one-hot class vectors (tensor or array) -> the list of per-image class-id lists that `TrainStep` takes as
    `labels=` (what SyntheticVOCLoader yields next to its images).  Given the device tensor of a yielded batch this reads it
    back, which waits for the stream; `loader.last_cls_labels` is the same array on the host and costs nothing."""
    rows = cls_labels.cpu().numpy() if isinstance(cls_labels, torch.Tensor) else np.asarray(cls_labels)
    return [[int(c) for c in np.nonzero(r)[0]] for r in rows]


class _Slot:
    def __init__(self):
        self.pinned = self.device = None
        self.copied, self.consumed = torch.cuda.Event(), torch.cuda.Event()
        self.used = False


class DeviceLoader:
    """Iterable over the device-resident, collated batches of `dataset` (a datasets.voc / datasets.coco class):

        Cls, aug=True     (img_names, inputs (B,3,crop,crop) f32, cls_labels (B,C), img_box (B,4) int16)
        Seg, aug=True     (img_names, inputs, labels (B,crop,crop) int64, cls_labels)
        Cls, aug=False    (img_names, inputs (1,3,H,W), cls_labels)                       batch_size = 1
        Seg, aug=False    (img_names, inputs (1,3,H,W), labels (1,H,W) int64, cls_labels)  batch_size = 1

    Every pass over the loader is one epoch and moves on to the next one (set_epoch() to choose).  The random draws come from
    DeviceAugment / DeviceSegAugment.draw_one(H_b, W_b) per image in batch order, from the private generators seeded with
    `seed + rank`, so a batch of equal-sized images gets the parameters those classes draw for it themselves."""

    def __init__(self, dataset, batch_size, shuffle=True, drop_last=False, seed=0, rank=0, world=1, threads=4, prefetch=2,
                 device="cuda"):
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        self.seed, self.rank, self.world, self.device = int(seed), int(rank), int(world), device
        self.threads = max(1, min(int(threads), MAX_THREADS))                 # never derived from os.cpu_count()
        self.prefetch = max(1, int(prefetch))
        self.epoch = 0
        self.kind, self.augment = dataset.kind, bool(dataset.aug)
        if not self.augment and self.batch_size != 1:
            raise ValueError("DeviceLoader: an aug=False dataset yields images at their own size, so batch_size must be 1")
        self.aug = None
        if self.augment and self.kind == "cls":
            self.aug = DeviceAugment(crop_size=dataset.crop_size, rescale_range=dataset.rescale_range,
                                     fliplr=dataset.img_fliplr, seed=self.seed + self.rank)
        elif self.augment:
            self.aug = DeviceSegAugment(crop_size=dataset.crop_size, rescale_range=None, fliplr=dataset.img_fliplr,
                                        ignore_index=dataset.ignore_index, seed=self.seed + self.rank)
        self.last_draws = None                                                # draw_one() tuples of the batch yielded last
        self.last_cls_labels = None                                           # its cls_labels once more, as a HOST array
        self.last_img_box = None      # Seg, aug=True: its img_box (B,4) int32 {y0,y1,x0,x1} on the DEVICE; None for the other kinds

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def plan(self, epoch=None):
        return index_plan(len(self.dataset), self.batch_size, self.shuffle, self.drop_last, self.seed,
                          self.epoch if epoch is None else epoch, self.rank, self.world)

    def __len__(self):
        mine = len(range(self.rank, len(self.dataset), self.world))
        return mine // self.batch_size if self.drop_last else -(-mine // self.batch_size)

    # ---- host side of one batch ---------------------------------------------------------------------------------------
    def _tables(self, items):
        """Draws of one decoded batch, in batch order -> (draws, tables, canvas_max).  The last table is always the stacked
        cls_labels, so they travel in the same copy."""
        cls = np.stack([np.asarray(it[3]) for it in items])
        if not self.augment:
            return None, (cls,), None
        sizes = [it[1].shape[:2] for it in items]
        draws = [self.aug.draw_one(H, W) for H, W in sizes]
        if self.kind == "cls":
            rec = self.aug.pack(draws)
            self.aug.check_ragged(rec, sizes)
            box = np.stack([DeviceAugment.img_box(d, self.aug.crop) for d in draws])    # transforms.py:162-166, on the host
            return draws, (rec.numpy(), box, cls), None
        rec, cand = self.aug.pack(draws)
        cm = self.aug.check_ragged(rec, cand, sizes)
        return draws, (rec.numpy(), cand.numpy(), cls), cm

    def _stage(self, slot, futures, side):
        """Decoded batch -> slot's pinned buffer -> one H2D copy on the side stream.  See the invariant in the module docstring."""
        items = [f.result() for f in futures]
        draws, tables, cm = self._tables(items)
        images = [it[1] for it in items]
        labels = [it[2] for it in items] if self.kind == "seg" else None
        need = sum(im.size for im in images) * (4 if labels is not None else 3) // 3 + sum(t.nbytes + 16 for t in tables) + 16 * len(items) + 48
        if slot.used:
            slot.copied.synchronize()                                         # (1): the last copy out of pinned[s] is done
        if slot.pinned is None or slot.pinned.numel() < need:
            cap = int(need * 1.25)
            slot.pinned = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            slot.device = torch.empty(cap, dtype=torch.uint8, device=self.device)
            slot.device.record_stream(side)
        _, _, _, layout = pack_batch(images, labels, tables, out=slot.pinned.numpy())
        with torch.cuda.stream(side):
            if slot.used:
                side.wait_event(slot.consumed)                                # (2): the kernel that read device[s] has run
            n = layout["total"]
            slot.device[:n].copy_(slot.pinned[:n], non_blocking=True)
            slot.copied.record(side)
        slot.used = True
        return dict(slot=slot, items=items, draws=draws, tables=tables, layout=layout, canvas_max=cm)

    def _launch(self, st):
        """The kernels of a staged batch on the consumer's current stream -> the collated tuple."""
        slot, items, lay = st["slot"], st["items"], st["layout"]
        B, dev = len(items), slot.device
        cur = torch.cuda.current_stream()
        cur.wait_event(slot.copied)

        def view(key, like, *shape):
            a, b = lay[key]
            dtype = like if isinstance(like, torch.dtype) else torch.from_numpy(np.empty(0, like.dtype)).dtype
            return dev[a:b].view(dtype).view(*(shape or like.shape))
        names = [it[0] for it in items]
        tables = st["tables"]
        box = None
        cls_labels = view(f"table{len(tables) - 1}", tables[-1]).clone()       # a copy: the slot's buffer will be reused
        src = dev[lay["images"][0]:lay["images"][1]]
        if not self.augment:
            from ..data import normalize_u8
            H, W = items[0][1].shape[:2]
            lab = dev[lay["labels"][0]:lay["labels"][1]].view(H, W) if self.kind == "seg" else None
            res = normalize_u8(src.view(H, W, 3), lab)
            out = (names, res[None], cls_labels) if lab is None else (names, res[0][None], res[1][None], cls_labels)
        elif self.kind == "cls":
            inputs = self.aug.ragged(src, view("offsets", torch.int64, B), view("sizes", torch.int32, B, 2),
                                     view("table0", torch.int32, B, 8))
            out = (names, inputs, cls_labels, view("table1", tables[1]).clone())
        else:
            lab = dev[lay["labels"][0]:lay["labels"][1]]
            inputs, labels, box = self.aug.ragged(src, lab, view("offsets", torch.int64, B), view("sizes", torch.int32, B, 2),
                                                view("table0", torch.int32, B, 16),
                                                view("table1", torch.int32, B, self.aug.n_cand, 2), st["canvas_max"])
            out = (names, inputs, labels, cls_labels)
        self.last_img_box = box
        slot.consumed.record(cur)                                             # the reading kernel is enqueued: slot reusable
        self.last_draws, self.last_cls_labels = st["draws"], tables[-1]
        return out

    def __iter__(self):
        from .. import _lib as L
        L.require_gpu()
        plan = self.plan()
        self.epoch += 1
        if not plan:
            return
        with torch.cuda.device(self.device):
            side = torch.cuda.Stream()
            slots = [_Slot() for _ in range(self.prefetch + 1)]
            pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="weclip-decode")
            try:
                decoding, staged = collections.deque(), collections.deque()
                nxt = 0                                                       # next batch of the plan to hand to the decoders
                staged_n = 0

                def submit():
                    nonlocal nxt
                    while nxt < len(plan) and len(decoding) < self.prefetch + 1:
                        decoding.append([pool.submit(self.dataset.raw, i) for i in plan[nxt]])
                        nxt += 1

                def stage_one():
                    nonlocal staged_n
                    staged.append(self._stage(slots[staged_n % len(slots)], decoding.popleft(), side))
                    staged_n += 1
                    submit()
                submit()
                while decoding and len(staged) < self.prefetch:
                    stage_one()
                while staged:
                    out = self._launch(staged.popleft())
                    if decoding:
                        stage_one()
                    yield out
            finally:
                pool.shutdown(wait=True, cancel_futures=True)
