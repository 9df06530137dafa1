"""The predict entry point: run a trained checkpoint on images that have no ground truth, and keep how sure the model is.

    python -m weclip_vit_comer_amd.predict --config configs/voc_attn_reg.yaml --model_path WeCLIP_model_iter_30000.pth \
        (--images DIR|GLOB|LIST.txt [--recursive] | --split test) [--dataset voc|coco|seg] [--out_dir predictions] \
        [--outputs prediction,prediction_cmap,confidence,overlay] [--palette] [--alpha 0.5] [--ignore_below 0] \
        [--scales 1,0.75] [--resize_long 512] [--crf] [--crf_bilateral exact|lattice]

What the reference does for a split WITH labels (test_msc_flip_voc.py `validate` :92-96 and `crf_proc` :146-161) and only half
does without (`crf_proc` has a "test" branch, `main()` never reaches it), for any folder of images or a label-free split of a
VOC / COCO tree.  Per image: `MscFlipEvaluator.logits(inputs, run_cam=False)` (the VOC model then needs no class ids), with
`--crf` the dense CRF on the multi-scale logits, and ONE launch of `wc_predict_finish` (csrc/predict.hip) over the image's own
grid: the uint8 label map (255 where the confidence is below `--ignore_below`), its colour image, the uint8 confidence map
(soft-max probability of the arg-max, or the CRF's Q of it, times 255), the colour image blended over the input, and per label
the pixel count and confidence sum.  The requested maps go to the host in one asynchronous copy into the ring of pinned buffers
of `utils.writer_ring.WriterRing`; host threads write `prediction/NAME.png` (mode L, or P with the VOC palette: what the VOC
evaluation server takes), `prediction_cmap/NAME.png`, `confidence/NAME.png`, `overlay/NAME.png`.  The per-image statistics stay
in a device table that is read once, in `finish()`, which writes `summary.json`.  Under `python -m torch.distributed.run` every
rank predicts its share of the images and writes their files; rank 0 writes the one `summary.json`.
"""
import argparse
import json
import os

import numpy as np
import torch

from . import _lib as L
from . import entry, msc_flip
from .msc_flip_eval import image_of
from .utils.writer_ring import WriterRing, _cuda_alloc, _cuda_event

F32 = torch.float32
KINDS = ("prediction", "prediction_cmap", "confidence", "overlay")
_CHANNELS = {"prediction": 1, "prediction_cmap": 3, "confidence": 1, "overlay": 3}
CRF_MAX_PIXELS = 640 * 640                                    # the dense CRF's limit (csrc/dcrf.hip)


# ---------------------------------------------------------------------------------------------- the kernel
def predict_finish(src, out_hw, image=None, pred_u8=None, cmap_rgb=None, conf_u8=None, overlay_rgb=None, stats=None, mode=0,
                   alpha256=128, ignore_below=0):
    """One launch of `wc_predict_finish` over the (H, W) = out_hw grid.  src (C,Hs,Ws) f32: logits (mode 0) or probabilities with
    (Hs, Ws) == (H, W) (mode 1); image (H,W,3) uint8 or None; pred_u8 / conf_u8 (H,W) uint8 and cmap_rgb / overlay_rgb (H,W,3)
    uint8 are written when given (overlay_rgb needs image); stats int64 (2C + 1,) is added into: [c] pixels written as c,
    [C + c] the sum of their conf_u8, [2C] pixels written as 255 because their conf_u8 < ignore_below."""
    L.require_gpu()
    if src.dim() != 3:
        raise RuntimeError(f"predict_finish: src must be (C, Hs, Ws), got {tuple(src.shape)}")
    C, Hs, Ws = src.shape
    H, W = (int(v) for v in out_hw)
    for name, t, shape in (("image", image, (H, W, 3)), ("pred_u8", pred_u8, (H, W)), ("cmap_rgb", cmap_rgb, (H, W, 3)),
                           ("conf_u8", conf_u8, (H, W)), ("overlay_rgb", overlay_rgb, (H, W, 3)), ("stats", stats, (2 * C + 1,))):
        if t is not None and tuple(t.shape) != shape:
            raise RuntimeError(f"predict_finish: {name} must be {shape}, got {tuple(t.shape)}")
    U8 = torch.uint8
    L.lib().wc_predict_finish(L.ptr(src, F32, "src"), L.ptr(image, U8, "image"), L.ptr(pred_u8, U8, "pred_u8"),
                              L.ptr(cmap_rgb, U8, "cmap_rgb"), L.ptr(conf_u8, U8, "conf_u8"), L.ptr(overlay_rgb, U8, "overlay_rgb"),
                              L.ptr(stats, torch.int64, "stats"), C, Hs, Ws, H, W, int(mode), int(alpha256), int(ignore_below),
                              L.stream())


# ---------------------------------------------------------------------------------------------- the files
def voc_palette():
    """The 256 PASCAL VOC colours as the flat [r0, g0, b0, r1, ...] list `Image.putpalette` takes: bit j of the label goes to bit
    7 - j // 3 of channel j % 3 (utils/imutils.py:136-154; `ef_colour` of csrc/voc_colour.h on the device)."""
    flat = []
    for v in range(256):
        rgb = [0, 0, 0]
        for j in range(8):
            rgb[j % 3] |= ((v >> j) & 1) << (7 - j // 3)
        flat += rgb
    return flat


def parse_outputs(text):
    """"prediction,confidence" -> the kinds in their fixed order; an unknown kind raises."""
    names = [s.strip() for s in (text.split(",") if isinstance(text, str) else text) if s.strip()]
    unknown = [n for n in names if n not in KINDS]
    if unknown:
        raise ValueError(f"outputs: unknown kind {unknown[0]!r}; choose from {', '.join(KINDS)}")
    return tuple(k for k in KINDS if k in names)


class PredictWriterPool(WriterRing):
    """The predict entry point's files behind the ring of utils/writer_ring.py: of the four kinds only those in `outputs` have a
    directory, a view in the slot and a share of the one device-to-host copy.

        slot = pool.acquire(H, W)        # slot.views[kind]: (H,W) u8 for prediction / confidence, (H,W,3) u8 for the other two
        pool.commit(slot, name)          # name may hold sub-directories ("sub/img_3"): the files mirror them

    prediction/NAME.png is mode L, or with `palette` mode P carrying the VOC palette over the same index bytes."""

    def __init__(self, out_dir, outputs=KINDS[:2], palette=False, writers=4, depth=None, alloc=_cuda_alloc, event=_cuda_event):
        self.out_dir = out_dir
        self.outputs = parse_outputs(outputs)
        self.palette = voc_palette() if palette else None
        self.dirs = {k: os.path.join(out_dir, k) for k in self.outputs}
        os.makedirs(out_dir, exist_ok=True)
        for d in self.dirs.values():
            os.makedirs(d, exist_ok=True)
        super().__init__(writers, depth, alloc, event)

    def acquire(self, H, W, block=True):
        slot = self.next_slot(block)
        used = self.carve(slot, [(k, (H, W) if _CHANNELS[k] == 1 else (H, W, 3), torch.uint8) for k in self.outputs])
        slot.layout = (H, W, self.outputs, used)
        return slot

    def _write(self, slot, name):
        from PIL import Image
        slot.copied.synchronize()
        for k in slot.layout[2]:
            path = os.path.join(self.dirs[k], name + ".png")
            if os.path.dirname(name):
                os.makedirs(os.path.dirname(path), exist_ok=True)
            im = Image.fromarray(self.host(slot, k), mode="L" if _CHANNELS[k] == 1 else "RGB")
            if k == "prediction" and self.palette is not None:
                im.putpalette(self.palette)                   # L -> P over the same bytes
            im.save(path)


# ---------------------------------------------------------------------------------------------- the images
def image_records(names, sizes, stats, num_classes):
    """The per-image part of summary.json from the stats table's rows: [{"name", "size": [H, W], "classes": {"c": {"share":
    area / (H W), "confidence": conf_sum / area / 255}} for every class with area > 0, "ignored": share}]."""
    out = []
    C = int(num_classes)
    for name, (H, W), row in zip(names, sizes, stats):
        row = [int(v) for v in row]
        classes = {str(c): {"share": row[c] / (H * W), "confidence": row[C + c] / row[c] / 255.0} for c in range(C) if row[c] > 0}
        out.append({"name": str(name), "size": [int(H), int(W)], "classes": classes, "ignored": row[2 * C] / (H * W)})
    return out


def make_summary(records, args):
    """summary.json: the run's arguments, the image count and the records sorted by name; a name that occurs twice raises."""
    records = sorted(records, key=lambda r: r["name"])
    for a, b in zip(records, records[1:]):
        if a["name"] == b["name"]:
            raise RuntimeError(f"predict: image {a['name']!r} was predicted twice")
    return entry.strict_json({"args": args, "images": len(records), "per_image": records})


def check_crf_sizes(dataset):
    """With the CRF: every image beyond the CRF's H * W <= 640^2 is reported by name before anything runs (a dataset that cannot
    tell its sizes from the headers is not checked)."""
    if not hasattr(dataset, "sizes"):
        return
    names = getattr(dataset, "name_list", None)
    bad = [(str(names[i]) if names is not None else str(i), hw) for i, hw in enumerate(dataset.sizes()) if hw[0] * hw[1] > CRF_MAX_PIXELS]
    if bad:
        listed = ", ".join(f"{n} ({h}x{w})" for n, (h, w) in bad[:10]) + (" ..." if len(bad) > 10 else "")
        raise RuntimeError(f"predict: {len(bad)} image(s) exceed the dense CRF's limit of 640*640 pixels: {listed}; "
                           "run them without --crf or resize them")


class Predictor:
    """Predict images one by one, shaped like `msc_flip_eval.SplitEvaluator`.  model: WeCLIP (VOC, COCO or the supervised variant)
    on the GPU.  crf: a utils.dcrf.DenseCRF: the maps are then the CRF's (arg-max and maximum of Q).  out_dir: where the
    directories of `outputs` and summary.json go; None writes nothing.  alpha: the colour's weight in the overlay (rounded to
    1/256).  ignore_below: pixels whose uint8 confidence is below it are written as label 255 (0: none).  rank / world: this
    process's share of the images."""

    def __init__(self, model, num_classes, scales=(1.0, 0.75), resize_long=512, crf=None, out_dir=None,
                 outputs=("prediction", "prediction_cmap"), alpha=0.5, ignore_below=0, palette=False, rank=0, world=1, writers=4):
        L.require_gpu()
        self.model, self.nc, self.rank, self.world = model, int(num_classes), int(rank), int(world)
        if not 1 <= self.nc <= 255:
            raise ValueError(f"Predictor: num_classes = {self.nc} outside [1, 255] (label 255 is the ignore label)")
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"Predictor: alpha = {alpha} outside [0, 1]")
        if not 0 <= int(ignore_below) <= 255:
            raise ValueError(f"Predictor: ignore_below = {ignore_below} outside [0, 255]")
        self.ev = msc_flip.MscFlipEvaluator(model, num_classes, scales=scales, resize_long=resize_long)
        self.crf, self.out_dir = crf, out_dir
        self.outputs = parse_outputs(outputs) if out_dir else ()
        self.alpha256, self.ignore_below, self.palette = int(round(float(alpha) * 256)), int(ignore_below), bool(palette)
        self.device = next(model.parameters()).device
        self.stats = torch.zeros(256, 2 * self.nc + 1, device=self.device, dtype=torch.int64)      # row i: image i of this rank
        self.names, self.sizes = [], []
        self.pool = PredictWriterPool(out_dir, self.outputs, palette=palette, writers=writers) if self.outputs else None
        self.args = {"num_classes": self.nc, "scales": [float(s) for s in scales], "resize_long": resize_long,
                     "crf": None if crf is None else {k: getattr(crf, k) for k in ("iter_max", "pos_w", "pos_xy_std", "bi_w",
                                                                                     "bi_xy_std", "bi_rgb_std", "bilateral")},
                     "outputs": list(self.outputs), "alpha": float(alpha), "alpha256": self.alpha256,
                     "ignore_below": self.ignore_below, "palette": self.palette, "world": self.world}

    @torch.no_grad()
    def add(self, name, inputs):
        """One image: inputs (1,3,H,W) normalised pixels, as the loader yields them.  Nothing is read back."""
        x = inputs.cuda()
        H, W = int(x.shape[2]), int(x.shape[3])
        _, msc = self.ev.logits(x, run_cam=False)
        i = len(self.names)
        if i == self.stats.shape[0]:                          # the table doubles on the device; its rows stay zero until used
            grown = torch.zeros(2 * i, self.stats.shape[1], device=self.device, dtype=torch.int64)
            grown[:i].copy_(self.stats)
            self.stats = grown
        slot = self.pool.acquire(H, W) if self.pool else None
        v = slot.views if slot else {}
        image = image_of(x) if (self.crf is not None or "overlay" in v) else None
        src, mode = msc, 0
        if self.crf is not None:
            from .utils import dcrf
            src, mode = self.crf.with_unary(image, dcrf.unary_from_logits(msc, (H, W))), 1
        predict_finish(src, (H, W), image=image if "overlay" in v else None, pred_u8=v.get("prediction"),
                       cmap_rgb=v.get("prediction_cmap"), conf_u8=v.get("confidence"), overlay_rgb=v.get("overlay"),
                       stats=self.stats[i], mode=mode, alpha256=self.alpha256, ignore_below=self.ignore_below)
        if slot:
            self.pool.commit(slot, name)
        self.names.append(str(name))
        self.sizes.append((H, W))

    def run(self, loader):
        """loader: a DeviceLoader over an aug=False dataset (batch_size 1) that yields (names, inputs, ...); sharded like
        `SplitEvaluator.run`.  -> finish()."""
        self.model.eval()
        if self.crf is not None:
            check_crf_sizes(loader.dataset)
        for batch in msc_flip.shard_batches(loader, self.rank, self.world):
            self.add(batch[0][0], batch[1])
        return self.finish()

    def finish(self):
        """Drain the writers, read the stats table once, collect every rank's records (each rank takes part, whatever its
        share); rank 0 writes summary.json.  -> the summary dict (on every rank)."""
        import torch.distributed as dist
        pool, self.pool = self.pool, None
        files_error = pool.drain() if pool is not None else None      # raised below: the other ranks wait in the gather
        n =len(self.names)
        records = image_records(self.names, self.sizes, self.stats[:n].cpu().numpy(), self.nc)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, records)
            records = [r for part in parts for r in part]
        if files_error is not None:
            raise files_error
        summary = make_summary(records, self.args)
        if self.out_dir and self.rank == 0:
            os.makedirs(self.out_dir, exist_ok=True)
            with open(os.path.join(self.out_dir, "summary.json"), "w") as f:
                json.dump(summary, f, allow_nan=False)
        return summary


# ---------------------------------------------------------------------------------------------- the command line
def build_parser():
    p = argparse.ArgumentParser(prog="python -m weclip_vit_comer_amd.predict", description=__doc__.split("\n\n")[0])
    entry.add_model_arguments(p)
    entry.add_run_arguments(p)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--images", type=str, default=None, metavar="SOURCE", help="a directory, a glob, or a text file of paths")
    src.add_argument("--split", type=str, default=None, metavar="NAME",
                     help="dataset.name_list_dir/NAME.txt of the config's VOC / COCO tree, read without label files (e.g. test)")
    p.add_argument("--recursive", action="store_true", help="with --images: sub-directories too; the outputs mirror them")
    p.add_argument("--out_dir", default="predictions", type=str)
    p.add_argument("--outputs", type=parse_outputs, default=("prediction", "prediction_cmap"),
                   help="comma-separated: " + ",".join(KINDS))
    p.add_argument("--alpha", type=float, default=0.5, help="weight of the colour in overlay/")
    p.add_argument("--ignore_below", type=int, default=0, help="0..255: write label 255 where the uint8 confidence is below it")
    p.add_argument("--palette", action="store_true", help="prediction/*.png as mode P with the VOC palette (evaluation server)")
    return p


def parse_args(argv=None):
    """The parsed arguments with the per-dataset defaults filled in."""
    p = build_parser()
    args = entry.fill_defaults(p.parse_args(argv))
    if not 0 <= args.ignore_below <= 255:
        p.error("--ignore_below must be in 0..255")
    if not 0.0 <= args.alpha <= 1.0:
        p.error("--alpha must be in 0..1")
    if args.recursive and args.images is None:
        p.error("--recursive goes with --images")
    return args


def main(argv=None):
    from .datasets import DeviceLoader
    args = parse_args(argv)
    cfg = entry.load_config(args.config)
    with entry.distributed_run() as (rank, world):
        if args.images is not None:
            from .datasets.folder import ImageFolderDataset
            dataset = ImageFolderDataset(args.images, recursive=args.recursive)
        else:
            dataset = entry.split_dataset(cfg, args, args.split, "test")
        if args.crf:
            check_crf_sizes(dataset)
        model = entry.load_model(cfg, args)
        if rank == 0:
            print(cfg)
            print(args)
        pr = Predictor(model, cfg.dataset.num_classes, scales=args.scales, resize_long=args.resize_long, crf=entry.crf_of(args),
                       out_dir=args.out_dir, outputs=args.outputs, alpha=args.alpha, ignore_below=args.ignore_below,
                       palette=args.palette, rank=rank, world=world, writers=args.writers)
        loader = DeviceLoader(dataset, batch_size=1, shuffle=False, rank=rank, world=world, threads=args.threads)
        summary = pr.run(loader)
        if rank == 0:
            print(f"{summary['images']} images -> {args.out_dir}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
