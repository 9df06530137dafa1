"""Stand-alone CAM generation (reference clip/generate_cams_voc12.py / generate_cams_coco14.py) on the device: DESIGN.md §11.

    ClipPreprocess   uint8 HWC images -> CLIP's normalised tensor at the size rounded up to the patch size
                     (`_transform_resize` / `img_ms_and_flip`, voc12:76-93), csrc/preprocess.hip
    scale_cam_f16    `scale_cam_image([cam], (ori_w, ori_h))` + `.astype(np.float16)` for a set of (image, class) pairs
    resize_cam_f32   `cv2.resize(grayscale_cam, (ori_w, ori_h))`
    CamGenerator     a list of images + label id lists -> [{"keys", "attn_highres"}], the payload the dumpers save

The encoder, the batched GradCAM, the affinity weight, the Sinkhorn rounds, the box mask and the refinement are the functions
the WeCLIP model uses (clip_tool.batch_refined_cams); no adapters, decoder or PAR are constructed here.  An image whose label
list is empty is skipped and reported in `CamGenerator.skipped`; the reference returns out of its whole loop there
(voc12:123-125)."""
import ctypes
import os

import numpy as np
import torch

from .. import _lib as L
from . import clip_tool as CT
from . import vit_engine as VE

F32, I32 = torch.float32, torch.int32
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_WORKERS = 16


def target_size(H0, W0, scale=1.0, patch_size=16):
    """(h, w) of img_ms_and_flip (voc12:87): scale * original size rounded up to a multiple of the patch size."""
    return (int(np.ceil(scale * int(H0) / patch_size) * patch_size),
            int(np.ceil(scale * int(W0) / patch_size) * patch_size))


def split_dataset(dataset, n_splits):
    """Worker shares as the dumpers cut them (voc12:39-48): n_splits - 1 equal parts, the remainder to the last."""
    if n_splits == 1:
        return [dataset]
    part = len(dataset) // n_splits
    return [dataset[i * part:(i + 1) * part] for i in range(n_splits - 1)] + [dataset[(n_splits - 1) * part:]]


def bucket_images(sizes, label_ids, max_bucket=16, patch_size=16):
    """Indices of the images grouped by source size (hence token grid), in first-seen order, at most `max_bucket` per group;
    images without labels are left out and returned separately.  -> ([[index, ...], ...], [skipped index, ...])"""
    groups, skipped = {}, []
    for i, (size, ids) in enumerate(zip(sizes, label_ids)):
        if len(ids) == 0:
            skipped.append(i)
            continue
        groups.setdefault(tuple(int(s) for s in size), []).append(i)
    out = []
    for idx in groups.values():
        out += [idx[k:k + max_bucket] for k in range(0, len(idx), max_bucket)]
    return out, skipped


class ClipPreprocess:
    """`_transform_resize(h, w)` of the dumpers for a batch of equally sized images: Pillow's 8-bit BICUBIC resize, ToTensor,
    Normalize(CLIP mean / std), bit for bit (wc_clip_preprocess)."""

    def __init__(self, patch_size=16, mean=CLIP_MEAN, std=CLIP_STD):
        self.patch_size, self.mean, self.std = int(patch_size), tuple(mean), tuple(std)
        self._ws = None

    def __call__(self, images_u8, scale=1.0, flip=False, return_u8=False):
        """images_u8 (B,H0,W0,3) or (H0,W0,3) uint8 on the device -> (B,3,h,w) f32; with flip=True a pair (image, flipped
        image) as img_ms_and_flip builds per scale; with return_u8=True the resized uint8 image (B,h,w,3) is appended."""
        L.require_gpu()
        if images_u8.dim() == 3:
            images_u8 = images_u8[None]
        if images_u8.dim() != 4 or images_u8.shape[-1] != 3:
            raise RuntimeError("images: expected (B, H0, W0, 3) uint8 RGB")
        B, H0, W0, _ = images_u8.shape
        h, w = target_size(H0, W0, scale, self.patch_size)
        dev = images_u8.device
        n = ctypes.c_long(0)
        L.lib().wc_clip_preprocess_workspace_bytes(B, H0, W0, h, w, ctypes.byref(n))
        if self._ws is None or self._ws.numel() < n.value or self._ws.device != dev:
            self._ws = torch.empty(n.value, device=dev, dtype=torch.uint8)
        dst = torch.empty(B, 3, h, w, device=dev, dtype=F32)
        dflip = torch.empty_like(dst) if flip else None
        u8 = torch.empty(B, h, w, 3, device=dev, dtype=torch.uint8) if return_u8 else None
        L.lib().wc_clip_preprocess(L.ptr(images_u8.contiguous(), torch.uint8, "images"), L.ptr(dst), L.ptr(dflip), L.ptr(u8),
                                   L.ptr(self._ws), self._ws.numel(), B, H0, W0, h, w, (ctypes.c_float * 3)(*self.mean),
                                   (ctypes.c_float * 3)(*self.std), L.stream())
        out = (dst, dflip) if flip else (dst,)
        out = out + (u8,) if return_u8 else out
        return out[0] if len(out) == 1 else out


def _size_tables(sizes, dev):
    """(P,2) int32 sizes and (P,) int64 offsets on the device from ONE pinned asynchronous copy; total elements, max pixels."""
    px = [int(oh) * int(ow) for oh, ow in sizes]
    if any(p <= 0 for p in px):
        raise RuntimeError("target sizes must be positive")
    off = np.concatenate([[0], np.cumsum(px)]).astype(np.int64)
    host = torch.from_numpy(np.concatenate([off[:-1], np.asarray(sizes, np.int64).reshape(-1)]))
    host = host.pin_memory() if dev.type == "cuda" else host
    d = host.to(dev, non_blocking=True)
    P = len(sizes)
    return d[P:].to(I32).view(P, 2).contiguous(), d[:P].contiguous(), int(off[-1]), max(px)


def _resize(cams, gh, gw, sizes, normalise, flat=False):
    L.require_gpu()
    cams = cams.detach().reshape(-1, gh * gw).contiguous()
    P = cams.shape[0]
    if len(sizes) != P:
        raise RuntimeError(f"{P} CAMs but {len(sizes)} target sizes")
    sz, off, total, mx = _size_tables(sizes, cams.device)
    if normalise:
        out = torch.empty(total, device=cams.device, dtype=torch.float16)
        L.lib().wc_cam_scale_resize_f16(L.ptr(cams, F32, "cams"), L.ptr(sz, I32), L.ptr(off, torch.int64), L.ptr(out), total, P, gh, gw,
                                        mx, L.stream())
    else:
        out = torch.empty(total, device=cams.device, dtype=F32)
        L.lib().wc_cam_resize_f32(L.ptr(cams, F32, "cams"), L.ptr(sz, I32), L.ptr(off, torch.int64), L.ptr(out), total, P, gh, gw, mx,
                                  L.stream())
    if flat:
        return out
    res, o = [], 0
    for oh, ow in sizes:
        res.append(out[o:o + oh * ow].view(oh, ow))
        o += oh * ow
    return res


def scale_cam_f16(cams, gh, gw, sizes, flat=False):
    """cams (P, gh*gw) f32 on the device; sizes [(ori_h, ori_w)] per pair -> list of (ori_h, ori_w) float16 device tensors
    (views of one buffer, or with flat=True that 1-D buffer itself, pair after pair): scale_cam_image + astype(float16) of
    every pair in one launch."""
    return _resize(cams, gh, gw, sizes, True, flat)


def resize_cam_f32(cams, gh, gw, sizes):
    """The bilinear resize alone (cv2.resize of a float map), f32."""
    return _resize(cams, gh, gw, sizes, False)


class CamGenerator:
    """`perform` of the dumpers (voc12:96-217, coco14) for a list of images: per bucket of equally sized images one
    preprocess launch, one encode_image, one batched GradCAM + refinement over all (image, class) pairs, one output launch."""

    def __init__(self, clip_model, fg_text_features, bg_text_features, box_threshold, max_bucket=16, patch_size=16):
        self.model = clip_model.eval()
        self.fg, self.bg = fg_text_features, bg_text_features
        self.thr, self.max_bucket = float(box_threshold), int(max_bucket)
        self.pre = ClipPreprocess(patch_size)
        self.patch_size = int(patch_size)
        self.skipped = []
        self.last = None         # intermediates of the last bucket (tests): cams, boxes inputs, refined CAMs

    @torch.no_grad()
    def _bucket(self, images, label_ids):
        dev = images[0].device
        x = self.pre(torch.stack(images))
        B, _, H, W = x.shape
        gh, gw = H // self.patch_size, W // self.patch_size
        feats, maps = self.model.encode_image(x, H, W)
        rows, _, _ = VE.to_rows(feats)
        plan = CT.PairPlan(label_ids, self.fg.shape[0], self.bg.shape[0], dev)
        text_hat = CT.normalised_text(self.fg, self.bg, dev)
        R, cams, _, _ = CT.batch_refined_cams(self.model, rows, maps, None, plan, text_hat, gh, gw, self.thr, False, 8)
        pairs = [(i, k) for i, ids in enumerate(label_ids) for k in range(len(ids))]
        refined = R.permute(0, 2, 1)[plan.pair_img.long(), plan.pair_slot.long()].contiguous()      # (P, hw)
        H0, W0 = images[0].shape[:2]
        # every pair of the bucket has H0 * W0 elements and the pairs of an image are consecutive: one (P, H0, W0) buffer
        flat = scale_cam_f16(refined, gh, gw, [(H0, W0)] * len(pairs), flat=True).view(len(pairs), H0, W0)
        self.last = {"input": x, "grayscale_cam": cams.view(-1, gh, gw), "cam_refined": refined.view(-1, gh, gw), "pairs": pairs,
                     "grid": (gh, gw), "plan": plan}
        return flat

    def last_boxes(self):
        """Boxes of scoremap2bbox for every pair of the last bucket, [[x0, y0, x1, y1], ...] sorted; one more launch of the
        box kernel on the kept GradCAM maps (the refinement itself consumes the mask, not the list)."""
        from .. import cam_pipeline as CP
        st, (gh, gw) = self.last, self.last["grid"]
        plan = st["plan"]
        _, _, boxes, nbox = CP.box_masks(st["grayscale_cam"].reshape(-1, gh * gw).contiguous(), plan.pair_img, plan.pair_slot, plan.B,
                                         plan.K, gh, gw, self.thr, want_boxes=True)
        boxes, nbox = boxes.cpu().numpy(), nbox.cpu().numpy()
        return [sorted(map(tuple, boxes[p, :nbox[p]].tolist())) if nbox[p] else [(0, 0, 0, 0)] for p in range(len(st["pairs"]))]

    def __call__(self, images_u8, label_ids, to_numpy=True):
        """images_u8: list of (H0,W0,3) uint8 tensors (moved to the GPU if they are not there); label_ids: list of lists of
        foreground class ids.  -> list of {"keys": int64 (K,), "attn_highres": float16 (K,H0,W0)} (numpy, or device tensors
        with to_numpy=False), None for an image without labels (its index is appended to `skipped`)."""
        L.require_gpu()
        if len(images_u8) != len(label_ids):
            raise RuntimeError("one label id list per image")
        imgs = [im if im.is_cuda else im.cuda(non_blocking=True) for im in images_u8]
        buckets, skipped = bucket_images([im.shape[:2] for im in imgs], label_ids, self.max_bucket, self.patch_size)
        self.skipped += skipped
        res = [None] * len(imgs)
        for idx in buckets:
            ids = [list(map(int, label_ids[i])) for i in idx]
            flat = self._bucket([imgs[i] for i in idx], ids)
            if to_numpy:        # the only device -> host copy of the bucket
                flat = flat.cpu().numpy()
            p = 0
            for i, l in zip(idx, ids):       # (K, H0, W0) views of the bucket's buffer
                keys = torch.tensor(l, dtype=torch.int64)
                res[i] = {"keys": keys.numpy() if to_numpy else keys, "attn_highres": flat[p:p + len(l)]}
                p += len(l)
        return res


# ---- drivers ---------------------------------------------------------------------------------------------------------
def voc_label_ids(xml_text, class_names, new_class_names):
    """Image-level label ids of a VOC annotation file in first-seen order, through the reference's two name tables
    (voc12:115-121).  -> (ids, (height, width))"""
    import xml.etree.ElementTree as ET
    root = ET.fromstring(xml_text)
    size = root.find("size")
    hw = (int(size.find("height").text), int(size.find("width").text))
    ids = []
    for obj in root.iter("object"):
        i = new_class_names.index(new_class_names[class_names.index(obj.find("name").text.strip())])
        if i not in ids:
            ids.append(i)
    return ids, hw


def coco_split_line(line):
    """One line of the COCO split file: image name followed by its label ids (coco14:35-47,109-113) -> (name, ids)."""
    parts = line.split()
    return parts[0], [int(p) for p in parts[1:]]


def load_image(path):
    """Decoded on the host with Pillow, RGB uint8 (H0,W0,3)."""
    from PIL import Image
    with Image.open(path) as im:
        return torch.from_numpy(np.asarray(im.convert("RGB")).copy())


def save_payload(cam_out_dir, name, payload):
    """np.save(<name>.npy, {"keys", "attn_highres"}) as the dumpers do (voc12:211-216)."""
    np.save(os.path.join(cam_out_dir, name.replace("jpg", "npy")), payload)


def run_worker(process_id, dataset_list, img_root, cam_out_dir, generator_factory, read_item, chunk=16, seeds=None):
    """One worker: device process_id % device_count, its split_dataset share, `chunk` images per CamGenerator call.  seeds:
    seed_options()'s dict or None -- with it the maps stay on the device, go through a cam_seeds.SeedEvaluator chunk by chunk,
    and the worker leaves its counts in seed_part_<process_id>.npz next to the CAMs."""
    items = dataset_list[process_id]
    if len(items) == 0:          # more workers than images: nothing to do, the GPU is not touched
        return 0
    torch.cuda.set_device(process_id % torch.cuda.device_count())
    gen = generator_factory()
    ev = seeds["factory"]() if seeds else None
    for k in range(0, len(items), chunk):
        names, images, ids = [], [], []
        for it in items[k:k + chunk]:
            name, lab = read_item(it)
            names.append(name)
            images.append(load_image(os.path.join(img_root, name)))
            ids.append(lab)
        if ev is None:
            payloads = gen(images, ids)
        else:
            payloads = gen(images, ids, to_numpy=False)
            stems = [os.path.splitext(os.path.basename(n))[0] for n in names]
            gts = [read_gt(seeds["gt_root"], s) for s in stems] if seeds["gt_root"] else None
            ev.add(payloads, images, gts, stems)
        for name, payload in zip(names, payloads):
            if payload is None:
                print("{} not have valid object".format(name))
            elif ev is None:
                save_payload(cam_out_dir, name, payload)
            elif seeds["save_cams"]:
                save_payload(cam_out_dir, name, {"keys": payload["keys"].numpy(), "attn_highres": payload["attn_highres"].cpu().numpy()})
    if ev is not None:
        ev.finish()
        save_part(cam_out_dir, process_id, ev.arrays())
    return 0


# ---- seeds: threshold sweep, pseudo-label masks and their scores on the device (cam_seeds.py) -----------
SEED_FLAGS = ("gt_root", "eval_thresholds", "pseudo_dir", "no_save_cams")


def add_seed_arguments(p):
    p.add_argument("--gt_root", type=str, default=None, help="ground-truth label maps <name>.png (8-bit index images): scores")
    p.add_argument("--eval_thresholds", type=str, default=None,
                   help="background thresholds of the seed mIoU sweep, first:last:step (0.05:0.80:0.05) or a comma list; needs --gt_root")
    p.add_argument("--pseudo_dir", type=str, default=None, help="write the pseudo-label masks to DIR/prediction and DIR/prediction_cmap")
    p.add_argument("--low_thre", type=float, default=0.35,
                   help="at or below it a pixel is background (default 0.35: the AFA lineage's value, the reference's YAMLs carry none)")
    p.add_argument("--high_thre", type=float, default=0.55,
                   help="above it a pixel takes its class, between the two it is ignored (255) (default 0.55: the AFA lineage's value)")
    p.add_argument("--refine", choices=("none", "crf"), default="none", help="pass the two seed maps through the dense CRF before the merge")
    p.add_argument("--crf_bilateral", choices=("exact", "lattice"), default="exact")
    p.add_argument("--no_save_cams", action="store_true", help="do not write the <name>.npy maps (scores / masks only)")


def seed_options(args, num_classes):
    """None for a run with none of the new flags (such a run builds no evaluator and imports none of its code); otherwise the
    dict run_worker takes.  Flag combinations that would compute nothing are refused here, before any worker starts."""
    if not any(getattr(args, f, None) for f in SEED_FLAGS):
        if args.refine != "none":
            raise RuntimeError("--refine needs --pseudo_dir")
        return None
    if args.eval_thresholds and not args.gt_root:
        raise RuntimeError("--eval_thresholds needs --gt_root")
    if not args.eval_thresholds and not args.pseudo_dir:
        raise RuntimeError("--gt_root / --no_save_cams need --eval_thresholds or --pseudo_dir: nothing to compute")
    if args.refine != "none" and not args.pseudo_dir:
        raise RuntimeError("--refine needs --pseudo_dir")
    from . import cam_seeds as CS
    thresholds = CS.parse_thresholds(args.eval_thresholds) if args.eval_thresholds else None
    kw = dict(num_classes=num_classes, thresholds=thresholds, low_thre=args.low_thre, high_thre=args.high_thre, refine=args.refine,
              crf_bilateral=args.crf_bilateral, out_dir=args.pseudo_dir, masks=args.pseudo_dir is not None)
    CS.SeedEvaluator(**{**kw, "out_dir": None})          # argument errors now, not in every worker
    return {"factory": lambda: CS.SeedEvaluator(**kw), "gt_root": args.gt_root, "save_cams": not args.no_save_cams, "kw": kw}


def read_gt(gt_root, stem):
    from ..datasets.voc import read_label
    return read_label(os.path.join(gt_root, stem + ".png"))


def part_path(cam_out_dir, process_id):
    return os.path.join(cam_out_dir, f"seed_part_{int(process_id)}.npz")


def save_part(cam_out_dir, process_id, arrays):
    """A worker's raw counts (cam_seeds.SeedEvaluator.arrays()); a leg that did not run is stored as an empty array."""
    none = np.zeros(0, np.int64)
    np.savez(part_path(cam_out_dir, process_id), images=np.int64(arrays["images"]),
             **{k: none if arrays[k] is None else arrays[k] for k in ("bins", "hist", "cover")})


def clear_parts(cam_out_dir):
    for i in range(MAX_WORKERS):
        if os.path.exists(part_path(cam_out_dir, i)):
            os.remove(part_path(cam_out_dir, i))


def write_seed_scores(cam_out_dir, n_workers, seeds):
    """Sum the workers' parts into <cam_out_dir>/seed_scores.json (cam_seeds.summarise of the summed counts)."""
    from . import cam_seeds as CS
    total = {"bins": None, "hist": None, "cover": None, "images": 0}
    for i in range(n_workers):
        if not os.path.exists(part_path(cam_out_dir, i)):        # a worker with an empty share
            continue
        with np.load(part_path(cam_out_dir, i)) as part:
            total["images"] += int(part["images"])
            for k in ("bins", "hist", "cover"):
                if part[k].size:
                    total[k] = part[k].astype(np.int64) if total[k] is None else total[k] + part[k]
    kw = seeds["kw"]
    result = CS.summarise(kw["num_classes"], kw["thresholds"], total["bins"], total["hist"], total["cover"], total["images"],
                          kw["low_thre"], kw["high_thre"], kw["refine"], kw["crf_bilateral"])
    path = os.path.join(cam_out_dir, "seed_scores.json")
    CS.write_scores(path, result)
    return path


def worker_commands(num_workers, module, argv):
    """Command lines of the child interpreters: `python -m <module> <the parent's arguments> --num_workers n --worker_id i`.
    `module` is the driver's importable name (its `__spec__.name`: under `python -m` its `__name__` is "__main__")."""
    import sys
    n = min(int(num_workers), MAX_WORKERS)
    argv, rest, skip = list(argv), [], False
    for a in argv:               # the parent's own --num_workers is replaced by the capped one
        if skip:
            skip = False
        elif a == "--num_workers":
            skip = True
        elif not a.startswith("--num_workers="):
            rest.append(a)
    return [[sys.executable, "-m", module] + rest + ["--num_workers", str(n), "--worker_id", str(i)] for i in range(n)]


def spawn_workers(num_workers, module, argv):
    """`--num_workers N` (N > 1): N fresh child interpreters, each told its share with --worker_id; never an exec in a
    process that holds the GPU; at most MAX_WORKERS at a time."""
    import subprocess
    procs = [subprocess.Popen(cmd) for cmd in worker_commands(num_workers, module, argv)]
    rcs = [p.wait() for p in procs]
    if any(rcs):
        raise RuntimeError(f"CAM workers failed: exit codes {rcs}")
    return 0
