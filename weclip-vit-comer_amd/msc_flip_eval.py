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
import contextlib
import json
import os
import queue
import threading

import numpy as np
import torch

from . import _lib as L
from . import msc_flip
from .utils import evaluate

F32 = torch.float32
DEFAULTS = {"voc": ("configs/voc_attn_reg.yaml", "/your/path/WeCLIP/WeCLIP_model_iter_30000.pth"),      # test_msc_flip_voc.py:20-28
            "coco": ("configs/coco_attn_reg.yaml", "/your/path/WeCLIP/WeCLIP_model_iter_80000.pth"),    # test_msc_flip_coco.py:20-28
            "seg": ("configs/voc_attn_reg.yaml", "/your/path/WeCLIP/WeCLIP_model_iter_30000.pth")}      # test_msc_flip_seg.py:20-28
CRF_PARAMS = dict(iter_max=10, pos_xy_std=3, pos_w=3, bi_xy_std=64, bi_rgb_std=5, bi_w=4)               # test_msc_flip_voc.py:126-133
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
        from .validate import _flag
        flag = _flag(seg1.device)
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
        from .validate import _flag
        flag = _flag(pred.device)
    L.lib().wc_label_finish(L.ptr(pred, torch.int64, "pred"), L.ptr(gt, torch.int64, "gt"), L.ptr(out_u8, torch.uint8, "out_u8"),
                            L.ptr(cmap_rgb, torch.uint8, "cmap_rgb"), L.ptr(hist, torch.int64, "hist"),
                            L.ptr(flag, torch.int32, "flag"), H, W, int(num_classes), L.stream())


# ---------------------------------------------------------------------------------------------- the files
def output_dirs(work_dir, eval_set):
    """The tree of test_msc_flip_voc.py:226-230: everything goes under work_dir/eval_set/."""
    out = os.path.join(work_dir, eval_set)
    return out, {k: os.path.join(out, k) for k in ("logit", "prediction", "prediction_cmap")}


class _Slot:
    """One buffer pair of the ring: `dev` the kernels write, `host` (pinned) the writers read, one event for the copy between."""

    def __init__(self, event):
        self.dev = self.host = None
        self.copied = event
        self.free = threading.Event()
        self.free.set()
        self.views = None


def _cuda_alloc(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)


def _cuda_event():
    return torch.cuda.Event()


class WriterPool:
    """A ring of `depth` (dev, pinned host) buffer pairs and `writers` host threads behind it.

        slot = pool.acquire(H, W, logit_shape)      # waits until a pair is free: at most `depth` images are in flight
        ... kernels write slot.views["pred"] (H,W) u8, ["cmap"] (H,W,3) u8, ["segs"] / ["msc_segs"] (C,h,w) f32 ...
        pool.commit(slot, name)                      # ONE asynchronous copy dev -> host, an event, and the job is queued

    A writer waits for the slot's event, writes prediction/NAME.png (mode L), prediction_cmap/NAME.png (RGB) and, with
    save_logits, logit/NAME.npy ({"segs": (1,C,h,w), "msc_segs": (1,C,h,w)} f32, test_msc_flip_voc.py:111), then frees the
    slot.  The buffers only grow; nothing is allocated per image.  The first exception of a writer is kept and raised by
    `finish()`.  alloc / event: the device side (tests pass host stand-ins)."""

    def __init__(self, out_dir, writers=4, depth=None, save_logits=False, alloc=_cuda_alloc, event=_cuda_event):
        self.out_dir = out_dir
        self.save_logits = bool(save_logits)
        self._make_dirs()
        self.writers = max(1, int(writers))
        self.depth = int(depth) if depth else 2 * self.writers
        self._alloc = alloc
        self.slots = [_Slot(event()) for _ in range(self.depth)]
        self._next = 0
        self.jobs = queue.Queue(maxsize=self.depth)
        self.error = None
        self.written = 0
        self._lock = threading.Lock()
        self.threads = [threading.Thread(target=self._work, name=f"weclip-write-{i}", daemon=True) for i in range(self.writers)]
        for t in self.threads:
            t.start()

    def _make_dirs(self):
        """The directories this pool writes into (a subclass with other files names its own: predict.PredictWriterPool)."""
        self.dirs = {k: os.path.join(self.out_dir, k) for k in ("logit", "prediction", "prediction_cmap")}
        for k, d in self.dirs.items():
            if k != "logit" or self.save_logits:
                os.makedirs(d, exist_ok=True)

    def _next_slot(self, block):
        """The next slot of the ring once its writer has freed it.  block=False: queue.Full when it is still in flight."""
        slot = self.slots[self._next]
        if not slot.free.wait(None if block else 0):
            raise queue.Full(f"WriterPool: all {self.depth} buffers are in flight")
        self._next = (self._next + 1) % self.depth
        return slot

    def acquire(self, H, W, logit_shape=None, block=True):
        """The next slot of the ring with views for an (H, W) image.  block=False: queue.Full when it is still in flight."""
        slot = self._next_slot(block)
        n_img = 4 * H * W                                                     # [pred H*W | cmap 3*H*W]; 4-byte aligned end
        n_log = 4 * int(np.prod(logit_shape)) if (self.save_logits and logit_shape is not None) else 0
        need = n_img + 2 * n_log
        if slot.dev is None or slot.dev.numel() < need:
            slot.dev, slot.host = self._alloc(int(need * 1.25))
        d = slot.dev
        slot.views = {"pred": d[:H * W].view(H, W), "cmap": d[H * W:n_img].view(H, W, 3)}
        if n_log:
            slot.views["segs"] = d[n_img:n_img + n_log].view(F32).view(*logit_shape)
            slot.views["msc_segs"] = d[n_img + n_log:need].view(F32).view(*logit_shape)
        slot.layout = (H, W, tuple(logit_shape) if n_log else None, need)
        return slot

    def commit(self, slot, name):
        need = slot.layout[3]
        slot.free.clear()
        slot.host[:need].copy_(slot.dev[:need], non_blocking=True)
        slot.copied.record()
        self.jobs.put((slot, str(name)))

    def _write(self, slot, name):
        from PIL import Image
        H, W, logit_shape, need = slot.layout
        slot.copied.synchronize()
        host = slot.host.numpy()
        Image.fromarray(host[:H * W].reshape(H, W), mode="L").save(os.path.join(self.dirs["prediction"], name + ".png"))
        Image.fromarray(host[H * W:4 * H * W].reshape(H, W, 3), mode="RGB").save(os.path.join(self.dirs["prediction_cmap"], name + ".png"))
        if logit_shape is not None:
            n_log = (need - 4 * H * W) // 2
            a = host[4 * H * W:4 * H * W + n_log].view(np.float32).reshape((1,) + logit_shape)
            b = host[4 * H * W + n_log:need].view(np.float32).reshape((1,) + logit_shape)
            np.save(os.path.join(self.dirs["logit"], name + ".npy"), {"segs": a, "msc_segs": b})

    def _work(self):
        while True:
            job = self.jobs.get()
            try:
                if job is None:
                    return
                slot, name = job
                try:
                    self._write(slot, name)
                    with self._lock:
                        self.written += 1
                except BaseException as e:                                    # kept for finish(); the slot is freed either way
                    with self._lock:
                        if self.error is None:
                            self.error = e
                finally:
                    slot.free.set()
            finally:
                self.jobs.task_done()

    def finish(self):
        """Wait for every queued file, end the threads, raise the first writer exception.  -> number of images written."""
        self.jobs.join()
        for _ in self.threads:
            self.jobs.put(None)
        for t in self.threads:
            t.join()
        self.threads = []
        if self.error is not None:
            raise self.error
        return self.written


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
        # a loader built with this rank / world already yields the share (index_plan: order[rank::world])
        sharded = (getattr(loader, "world", 1), getattr(loader, "rank", 0)) == (self.world, self.rank)
        for i, (names, inputs, labels, _) in enumerate(loader):
            if not sharded and i % self.world != self.rank:
                continue
            ids = labels_from_onehot(loader.last_cls_labels)[0] if self.has_cam else None
            self.add(names[0], inputs, labels, ids, image=image_of(inputs) if self.crf is not None else None)
        return self.finish()

    def finish(self):
        """Drain the writers, all-reduce the four histograms and the image count (every rank takes part in every reduce,
        whatever its share), check the flag.  -> {"cam" | "seg" | "msc_seg" | "crf": evaluate.scores_from_hist dict or None for
        an absent leg, "pixels": {leg: histogram sum}, "images": n}."""
        files_error = None
        if self.pool is not None:
            try:
                self.pool.finish()
            except BaseException as e:                                        # raised below: the other ranks wait in the reduces
                files_error = e
            self.pool = None
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
    from .train import strict_json

    def plain(v):
        if isinstance(v, dict):
            return {str(k): plain(x) for k, x in v.items()}
        if isinstance(v, (np.floating, float)):
            return float(v)
        if isinstance(v, (np.integer, int)):
            return int(v)
        return v
    return strict_json(plain(result))


# ---------------------------------------------------------------------------------------------- the command line
def parse_scales(text):
    return [float(s) for s in str(text).split(",") if s.strip()]


def build_parser():
    p = argparse.ArgumentParser(prog="python -m weclip_vit_comer_amd.msc_flip_eval", description=__doc__.split("\n\n")[0])
    p.add_argument("--config", default=None, type=str, help="the reference's YAML (default: configs/voc_attn_reg.yaml, coco_attn_reg.yaml)")
    p.add_argument("--work_dir", default="results", type=str, help="files go under work_dir/eval_set/")
    p.add_argument("--bkg_score", default=0.45, type=float, help="accepted and unused, as in the reference")
    p.add_argument("--resize_long", default=512, type=int, help="resize the long side")
    p.add_argument("--eval_set", default="val", type=str)
    p.add_argument("--model_path", default=None, type=str, help="a WeCLIP_model_iter_N.pth (model.state_dict())")
    p.add_argument("--dataset", choices=("voc", "coco", "seg"), default="voc", help="seg: the supervised variant on VOC")
    p.add_argument("--scales", type=parse_scales, default=[1.0, 0.75])
    p.add_argument("--crf", action=argparse.BooleanOptionalAction, default=False, help="the crf_proc leg (commented out in the reference)")
    p.add_argument("--crf_bilateral", choices=("exact", "lattice"), default="exact",
                   help="the CRF leg's bilateral message: the exact all-pairs sum, or the permutohedral lattice (as pydensecrf)")
    p.add_argument("--save_logits", action="store_true", help="logit/NAME.npy as the reference writes it")
    p.add_argument("--threads", type=int, default=8, help="decode threads of the loader")
    p.add_argument("--writers", type=int, default=4, help="host threads that write the PNG files")
    p.add_argument("--reference_root", type=str, default=None, help="reference checkout holding clip/clip_text.py and the BPE merges")
    return p


def parse_args(argv=None):
    """The parsed arguments with the per-dataset defaults of the reference's three scripts filled in."""
    args = build_parser().parse_args(argv)
    config, model_path = DEFAULTS[args.dataset]
    args.config = args.config or config
    args.model_path = args.model_path or model_path
    return args


def print_scores(result):
    """The reference's printed blocks (test_msc_flip_voc.py:206-211), plus the CRF block when that leg ran."""
    for leg, title in (("cam", "cams score:"), ("seg", "segs score:"), ("msc_seg", "msc segs score:"), ("crf", "crf score:")):
        if leg == "crf" and result[leg] is None:
            continue
        print(title)
        print(result[leg])


@contextlib.contextmanager
def distributed_run():
    """The process group of a command-line run (shared with predict.py): -> (rank, world).  A run that ends well meets the other
    ranks in a barrier; the group is destroyed either way."""
    import torch.distributed as dist
    from . import train as T
    world = T.init_distributed()
    try:
        yield (dist.get_rank() if world > 1 else 0), world
        if world > 1:
            dist.barrier()
    finally:
        if world > 1 and dist.is_initialized():
            dist.destroy_process_group()


def split_dataset(cfg, args, split, stage):
    """The Seg dataset of `--dataset` over `split` ("val" reads the label PNGs, "test" does not)."""
    ds = cfg.dataset
    if args.dataset == "coco":
        from .datasets.coco import CocoSegDataset as SegDataset
    else:
        from .datasets.voc import VOC12SegDataset as SegDataset
    return SegDataset(root_dir=ds.root_dir, name_list_dir=ds.name_list_dir, split=split, stage=stage, aug=False,
                      ignore_index=ds.ignore_index, num_classes=ds.num_classes)


def load_model(cfg, args):
    """The model of `--dataset` with the weights of `--model_path`, in eval mode."""
    from . import train as T
    model = T.build_model(cfg, args.dataset, args.reference_root)
    model.load_state_dict(torch.load(args.model_path, map_location="cpu"), strict=False)      # test_msc_flip_voc.py:194-196
    return model.eval()


def crf_of(args):
    """The DenseCRF of `--crf` / `--crf_bilateral` with the reference's parameters, or None."""
    if not args.crf:
        return None
    from .utils.dcrf import DenseCRF
    return DenseCRF(**CRF_PARAMS, bilateral=args.crf_bilateral)


def main(argv=None):
    from . import train as T
    from .datasets import DeviceLoader
    args = parse_args(argv)
    cfg = T.load_config(args.config)
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
