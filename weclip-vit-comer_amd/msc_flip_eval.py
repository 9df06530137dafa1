"""The evaluation entry point: multi-scale + flip evaluation of a split with the CRF leg and the prediction files, i.e. the
reference's test_msc_flip_voc.py / test_msc_flip_coco.py / test_msc_flip_seg.py around this package's `MscFlipEvaluator`.

    python -m weclip_vit_comer_amd.msc_flip_eval --config configs/voc_attn_reg.yaml --model_path WeCLIP_model_iter_30000.pth \
        [--dataset voc|coco|seg] [--work_dir results] [--eval_set val] [--scales 1,0.75] [--crf] [--save_logits]

Every image runs at its own size, exactly as `MscFlipEvaluator.add` runs it (no batching).  Per image the tail is ONE launch
of `wc_eval_finish` (csrc/evalfinish.hip): both arg-maxes on the label grid, the uint8 prediction map, the colour-mapped
image and the three histograms (scale-1, multi-scale, CAM label).  With the CRF leg `wc_label_finish` does the same for the
CRF's arg-max map.  The uint8 map and the colour image go to the host in one asynchronous copy into a ring of pinned
buffers; a pool of host threads writes `prediction/NAME.png`, `prediction_cmap/NAME.png` and `logit/NAME.npy` with Pillow /
numpy.  The histograms and the out-of-range flag are read once, in `finish()`.  Under `python -m torch.distributed.run` every
rank evaluates its share of the images and writes their files; rank 0 alone prints and writes `scores.json`.
"""
import argparse
import json
import os

import numpy as np
import torch

from . import _lib as L
from . import entry, msc_flip
from .entry import CRF_PARAMS, DEFAULTS, crf_of, distributed_run, load_model, parse_scales, split_dataset  # noqa: F401  (re-exported)
from .utils import evaluate
from .utils.writer_ring import WriterRing, _Slot, _cuda_alloc, _cuda_event  # noqa: F401  (re-exported)

F32 = torch.float32
LEGS = ("cam", "seg", "msc_seg", "crf")


# ---------------------------------------------------------------------------------------------- the two kernels
def eval_finish(seg1, msc, out_hw, num_classes, cam=None, gt=None, pred1_u8=None, predm_u8=None, cmap_rgb=None, hist=None,
                msc_hist=None, cam_hist=None, flag=None):
    """One launch of `wc_eval_finish` over the (Hl, Wl) = out_hw label grid.  seg1 / msc (C,Hs,Ws) f32 (msc may be None); cam,
    gt (Hl,Wl) int64 or None; pred1_u8 / predm_u8 (Hl,Wl) uint8 and cmap_rgb (Hl,Wl,3) uint8 are written when given; hist /
    msc_hist / cam_hist (nc,nc) int64 are added into over the pixels with 0 <= gt < nc.  flag: the device flag an out-of-range
    prediction raises (default: the one `evaluate.check_predictions_in_range` reads)."""
    L.require_gpu()
    C, Hs, Ws = seg1.shape
    Hl, Wl = (int(v) for v in out_hw)
    if msc is not None and tuple(msc.shape) != (C, Hs, Ws):
        raise RuntimeError("eval_finish: msc must have seg1's shape")
    for name, t, shape in (("cam", cam, (Hl, Wl)), ("gt", gt, (Hl, Wl)), ("pred1_u8", pred1_u8, (Hl, Wl)),
                           ("predm_u8", predm_u8, (Hl, Wl)), ("cmap_rgb", cmap_rgb, (Hl, Wl, 3))):
        if t is not None and tuple(t.shape) != shape:
            raise RuntimeError(f"eval_finish: {name} must be {shape}, got {tuple(t.shape)}")
    for name, t in (("hist", hist), ("msc_hist", msc_hist), ("cam_hist", cam_hist)):
        if t is not None and tuple(t.shape) != (num_classes, num_classes):
            raise RuntimeError(f"eval_finish: {name} must be (num_classes, num_classes)")
    if flag is None:
        flag = evaluate.range_flag(seg1.device)
    U8, I64 = torch.uint8, torch.int64
    L.lib().wc_eval_finish(L.ptr(seg1, F32, "seg1"), L.ptr(msc, F32, "msc"), L.ptr(cam, I64, "cam"), L.ptr(gt, I64, "gt"),
                           L.ptr(pred1_u8, U8, "pred1_u8"), L.ptr(predm_u8, U8, "predm_u8"), L.ptr(cmap_rgb, U8, "cmap_rgb"),
                           L.ptr(hist, I64, "hist"), L.ptr(msc_hist, I64, "msc_hist"), L.ptr(cam_hist, I64, "cam_hist"),
                           L.ptr(flag, torch.int32, "flag"), C, Hs, Ws, Hl, Wl, int(num_classes), L.stream())


def label_finish(pred, num_classes, gt=None, out_u8=None, cmap_rgb=None, hist=None, flag=None):
    """One launch of `wc_label_finish`: pred (H,W) int64 -> out_u8 (H,W) uint8, cmap_rgb (H,W,3) uint8, hist[gt, pred] += 1."""
    L.require_gpu()
    H, W = pred.shape
    for name, t, shape in (("gt", gt, (H, W)), ("out_u8", out_u8, (H, W)), ("cmap_rgb", cmap_rgb, (H, W, 3))):
        if t is not None and tuple(t.shape) != shape:
            raise RuntimeError(f"label_finish: {name} must be {shape}, got {tuple(t.shape)}")
    if hist is not None and tuple(hist.shape) != (num_classes, num_classes):
        raise RuntimeError("label_finish: hist must be (num_classes, num_classes)")
    if flag is None:
        flag = evaluate.range_flag(pred.device)
    L.lib().wc_label_finish(L.ptr(pred, torch.int64, "pred"), L.ptr(gt, torch.int64, "gt"), L.ptr(out_u8, torch.uint8, "out_u8"),
                            L.ptr(cmap_rgb, torch.uint8, "cmap_rgb"), L.ptr(hist, torch.int64, "hist"),
                            L.ptr(flag, torch.int32, "flag"), H, W, int(num_classes), L.stream())


# ---------------------------------------------------------------------------------------------- the files
def output_dirs(work_dir, eval_set):
    """The tree of test_msc_flip_voc.py:226-230: everything goes under work_dir/eval_set/."""
    out = os.path.join(work_dir, eval_set)
    return out, {k: os.path.join(out, k) for k in ("logit", "prediction", "prediction_cmap")}


class WriterPool(WriterRing):
    """The evaluation's files behind the ring of utils/writer_ring.py:

        slot = pool.acquire(H, W, logit_shape)      # waits until a pair is free: at most `depth` images are in flight
        ... kernels write slot.views["pred"] (H,W) u8, ["cmap"] (H,W,3) u8, ["segs"] / ["msc_segs"] (C,h,w) f32 ...
        pool.commit(slot, name)                      # ONE asynchronous copy dev -> host, an event, and the job is queued

    A writer waits for the slot's event and writes prediction/NAME.png (mode L), prediction_cmap/NAME.png (RGB) and, with
    save_logits, logit/NAME.npy ({"segs": (1,C,h,w), "msc_segs": (1,C,h,w)} f32, test_msc_flip_voc.py:111)."""

    def __init__(self, out_dir, writers=4, depth=None, save_logits=False, alloc=_cuda_alloc, event=_cuda_event):
        self.out_dir = out_dir
        self.save_logits = bool(save_logits)
        self.dirs = {k: os.path.join(out_dir, k) for k in ("logit", "prediction", "prediction_cmap")}
        for k, d in self.dirs.items():
            if k != "logit" or self.save_logits:
                os.makedirs(d, exist_ok=True)
        super().__init__(writers, depth, alloc, event)

    def acquire(self, H, W, logit_shape=None, block=True):
        """The next slot of the ring with views for an (H, W) image.  block=False: queue.Full when it is still in flight."""
        slot = self.next_slot(block)
        logits = tuple(logit_shape) if (self.save_logits and logit_shape is not None) else None
        sections = [("pred", (H, W), torch.uint8), ("cmap", (H, W, 3), torch.uint8)]
        if logits:
            sections += [("segs", logits, F32), ("msc_segs", logits, F32)]
        # packed [pred H*W | cmap 3*H*W], the layout the files were always cut from: it ends 4-byte aligned, where the f32 start
        slot.layout = (H, W, logits, self.carve(slot, sections, align=1))
        return slot

    def _write(self, slot, name):
        from PIL import Image
        slot.copied.synchronize()
        Image.fromarray(self.host(slot, "pred"), mode="L").save(os.path.join(self.dirs["prediction"], name + ".png"))
        Image.fromarray(self.host(slot, "cmap"), mode="RGB").save(os.path.join(self.dirs["prediction_cmap"], name + ".png"))
        if "segs" in slot.spans:
            np.save(os.path.join(self.dirs["logit"], name + ".npy"),
                    {k: self.host(slot, k)[None] for k in ("segs", "msc_segs")})


# ---------------------------------------------------------------------------------------------- the split
def image_of(inputs, mean=None, std=None):
    """inputs (1,3,H,W): the loader's normalised pixels -> the (H,W,3) uint8 image they came from (the CRF's image).  The
    normalisation is (v - mean) / std of an integer v: undoing it lands within 1e-4 of v, and rounding returns v."""
    from .data import MEAN, STD
    key = (str(inputs.device), tuple(mean or MEAN), tuple(std or STD))
    if key not in _NORM_ROWS:                                 # built once: a host list -> device tensor makes the host wait
        _NORM_ROWS[key] = tuple(torch.tensor(v, device=inputs.device, dtype=F32).view(3, 1, 1) for v in key[1:])
    m, s = _NORM_ROWS[key]
    return (inputs[0].float() * s + m).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


_NORM_ROWS = {}


class SplitEvaluator:
    """The reference's `validate` + `crf_proc` over a split, image by image.  model: WeCLIP (VOC, COCO or the supervised variant)
    on the GPU.  crf: a utils.dcrf.DenseCRF for the CRF leg; out_dir: where prediction/, prediction_cmap/ (and logit/ with
    save_logits) go -- the CRF prediction when crf is given, as in crf_proc, else the multi-scale one; None writes no file.
    rank / world: this process's share of the images (`msc_flip.shard`)."""

    def __init__(self, model, num_classes, scales=(1.0, 0.75), resize_long=512, crf=None, out_dir=None, save_logits=False, rank=0,
                 world=1, writers=4):
        L.require_gpu()
        self.model, self.nc, self.rank, self.world = model, int(num_classes), int(rank), int(world)
        self.ev = msc_flip.MscFlipEvaluator(model, num_classes, scales=scales, resize_long=resize_long)
        self.crf, self.out_dir = crf, out_dir
        self.device = next(model.parameters()).device
        # the CAM leg: known from the model (a rank whose share is empty must agree with the others)
        self.has_cam = bool(getattr(model, "val_runs_cam", False))
        zeros = lambda: torch.zeros(self.nc, self.nc, device=self.device, dtype=torch.int64)      # noqa: E731
        self.hist, self.msc_hist, self.cam_hist, self.crf_hist = zeros(), zeros(), zeros(), zeros()
        self.images = 0
        self.pool = WriterPool(out_dir, writers=writers, save_logits=save_logits) if out_dir else None

    @torch.no_grad()
    def add(self, name, inputs, labels, class_ids=None, image=None):
        """One image: inputs (1,3,H,W) normalised pixels, labels (1,Hl,Wl) integer class map (255 = ignore), class_ids the
        image's class ids (the VOC model's CAM leg), image (Hl,Wl,3) uint8 for the CRF leg."""
        gt = labels[0].to(self.device).long().contiguous()
        Hl, Wl = gt.shape
        cam = None
        if self.has_cam:
            seg1, msc, cam = self.ev.logits(inputs.cuda(), class_ids=class_ids, want_cam=True, cam_size=(Hl, Wl))
        else:
            seg1, msc = self.ev.logits(inputs.cuda())
        slot = self.pool.acquire(Hl, Wl, tuple(seg1.shape)) if self.pool else None
        views = slot.views if slot else {}
        own = slot is not None and self.crf is None                            # eval_finish writes the files' maps itself
        eval_finish(seg1, msc, (Hl, Wl), self.nc, cam=cam, gt=gt, predm_u8=views["pred"] if own else None,
                    cmap_rgb=views["cmap"] if own else None, hist=self.hist, msc_hist=self.msc_hist,
                    cam_hist=self.cam_hist if cam is not None else None)
        if self.crf is not None:
            from .utils import dcrf
            if image is None:
                raise RuntimeError("SplitEvaluator.add: the CRF leg needs image=(Hl, Wl, 3)")
            crf_pred = self.crf.with_unary(image, dcrf.unary_from_logits(msc, (Hl, Wl))).argmax(0)
            label_finish(crf_pred, self.nc, gt=gt, out_u8=views.get("pred"), cmap_rgb=views.get("cmap"), hist=self.crf_hist)
        if slot:
            if "segs" in views:
                views["segs"].copy_(seg1)
                views["msc_segs"].copy_(msc)
            self.pool.commit(slot, name)
        self.images += 1

    def run(self, loader):
        """loader: a DeviceLoader over an aug=False Seg dataset (batch_size 1); sharded like `Validator.run`.  -> finish()."""
        from .datasets import labels_from_onehot
        self.model.eval()
        for names, inputs, labels, _ in msc_flip.shard_batches(loader, self.rank, self.world):
            ids = labels_from_onehot(loader.last_cls_labels)[0] if self.has_cam else None
            self.add(names[0], inputs, labels, ids, image=image_of(inputs) if self.crf is not None else None)
        return self.finish()

    def finish(self):
        """Drain the writers, all-reduce the four histograms and the image count (every rank takes part in every reduce,
        whatever its share), check the flag.  -> {"cam" | "seg" | "msc_seg" | "crf": evaluate.scores_from_hist dict or None for
        an absent leg, "pixels": {leg: histogram sum}, "images": n}."""
        pool, self.pool = self.pool, None
        files_error = pool.drain() if pool is not None else None              # raised below: the other ranks wait in the reduces
        hists = {"cam": self.cam_hist, "seg": self.hist, "msc_seg": self.msc_hist, "crf": self.crf_hist}
        for k in LEGS:
            msc_flip.reduce_hist(hists[k])
        count = msc_flip.reduce_hist(torch.tensor([self.images], device=self.device, dtype=torch.int64))
        if files_error is not None:
            raise files_error
        if not evaluate.check_predictions_in_range(self.device):
            raise RuntimeError("SplitEvaluator: a predicted or CAM label lies outside [0, num_classes) -- the histograms skip such "
                               "pixels; check num_classes against the model and the CAM label maps")
        present = {"cam": self.has_cam, "seg": True, "msc_seg": True, "crf": self.crf is not None}
        host = torch.stack([hists[k] for k in LEGS]).cpu().numpy()
        self.hist_host = {k: host[i] for i, k in enumerate(LEGS)}
        out = {k: evaluate.scores_from_hist(self.hist_host[k]) if present[k] else None for k in LEGS}
        out["pixels"] = {k: int(self.hist_host[k].sum()) for k in LEGS}
        out["images"] = int(count.item())
        return out


def to_json(result):
    """finish()'s dict as strict JSON data: numpy scalars -> float, class-id keys -> str, non-finite -> None."""
    def plain(v):
        if isinstance(v, dict):
            return {str(k): plain(x) for k, x in v.items()}
        if isinstance(v, (np.floating, float)):
            return float(v)
        if isinstance(v, (np.integer, int)):
            return int(v)
        return v
    return entry.strict_json(plain(result))


# ---------------------------------------------------------------------------------------------- the command line
def build_parser():
    p = argparse.ArgumentParser(prog="python -m weclip_vit_comer_amd.msc_flip_eval", description=__doc__.split("\n\n")[0])
    entry.add_model_arguments(p)
    entry.add_run_arguments(p)
    p.add_argument("--work_dir", default="results", type=str, help="files go under work_dir/eval_set/")
    p.add_argument("--bkg_score", default=0.45, type=float, help="accepted and unused, as in the reference")
    p.add_argument("--eval_set", default="val", type=str)
    p.add_argument("--save_logits", action="store_true", help="logit/NAME.npy as the reference writes it")
    return p


def parse_args(argv=None):
    """The parsed arguments with the per-dataset defaults of the reference's three scripts filled in."""
    return entry.fill_defaults(build_parser().parse_args(argv))


def print_scores(result):
    """The reference's printed blocks (test_msc_flip_voc.py:206-211), plus the CRF block when that leg ran."""
    for leg, title in (("cam", "cams score:"), ("seg", "segs score:"), ("msc_seg", "msc segs score:"), ("crf", "crf score:")):
        if leg == "crf" and result[leg] is None:
            continue
        print(title)
        print(result[leg])


def main(argv=None):
    from .datasets import DeviceLoader
    args = parse_args(argv)
    cfg = entry.load_config(args.config)
    with distributed_run() as (rank, world):
        ds = cfg.dataset
        dataset = split_dataset(cfg, args, args.eval_set, "val")
        model = load_model(cfg, args)
        out_dir, _ = output_dirs(args.work_dir, args.eval_set)
        crf = crf_of(args)
        if rank == 0:
            print(cfg)
            print(args)
        ev = SplitEvaluator(model, ds.num_classes, scales=args.scales, resize_long=args.resize_long, crf=crf, out_dir=out_dir,
                            save_logits=args.save_logits, rank=rank, world=world, writers=args.writers)
        loader = DeviceLoader(dataset, batch_size=1, shuffle=False, rank=rank, world=world, threads=args.threads)
        result = ev.run(loader)
        if rank == 0:
            print_scores(result)
            # scores.json: finish()'s dict plus the four summed histograms ("hist": {leg: nc x nc counts})
            with open(os.path.join(out_dir, "scores.json"), "w") as f:
                json.dump(to_json(dict(result, hist={k: v.tolist() for k, v in ev.hist_host.items()})), f, allow_nan=False)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
