"""Seed scores and pseudo-label masks for CAM dumps that already exist:

    python -m weclip_vit_comer_amd.clip.eval_cams --cam_dir out --gt_root .../SegmentationClassAug --split_file voc12/train_aug.txt \\
        [--num_classes 21] [--eval_thresholds 0.05:0.80:0.05] [--pseudo_dir masks [--refine crf --img_root .../JPEGImages]]

The `<name>.npy` payloads ({"keys", "attn_highres"}, what the dumpers write) are read by host threads, a chunk of them goes to the
device in one pinned copy, and the same cam_seeds.SeedEvaluator the dumpers use does the rest; the result is the same
`seed_scores.json` (in --cam_dir unless --out names another file)."""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import generate_cams as G


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--cam_dir", type=str, required=True)
    p.add_argument("--split_file", type=str, required=True, help="one image name per line (anything after the name is ignored)")
    p.add_argument("--num_classes", type=int, default=21, help="classes including background (VOC 21, COCO 81)")
    p.add_argument("--img_root", type=str, default=None, help="the images <name>.jpg: the CRF's input with --refine crf")
    p.add_argument("--out", type=str, default=None, help="result file (default <cam_dir>/seed_scores.json)")
    p.add_argument("--chunk", type=int, default=16, help="payloads per upload")
    p.add_argument("--readers", type=int, default=4, help="host threads reading the .npy files")
    G.add_seed_arguments(p)
    return p.parse_args(argv)


def read_names(split_file):
    with open(split_file) as fid:
        names = [l.split()[0] for l in fid.read().splitlines() if l.strip()]
    return [os.path.splitext(n)[0] if n.endswith(".jpg") else n for n in names]


def load_payload(cam_dir, stem):
    """The dumpers' payload of one image, or None when the dumper skipped it (no file)."""
    path = os.path.join(cam_dir, stem + ".npy")
    if not os.path.exists(path):
        return None
    d = np.load(path, allow_pickle=True).item()
    cam = np.ascontiguousarray(d["attn_highres"])
    if cam.dtype != np.float16 or cam.ndim != 3 or cam.shape[0] != len(d["keys"]):
        raise RuntimeError(f"{path}: expected attn_highres (K, H, W) float16 with K = len(keys), got {cam.dtype} {cam.shape}")
    return {"keys": np.asarray(d["keys"], np.int64), "attn_highres": cam}


def upload(payloads, device="cuda"):
    """The chunk's maps in ONE pinned buffer and one copy; -> payloads whose attn_highres are views of the device buffer, image
    after image, so that equally sized neighbours form one (P, HW) block without a device copy."""
    sizes = [0 if p is None else p["attn_highres"].size for p in payloads]
    if not sum(sizes):
        return list(payloads)
    host = torch.empty(sum(sizes), dtype=torch.float16).pin_memory()
    o = 0
    for p, n in zip(payloads, sizes):
        if p is not None:
            host[o:o + n] = torch.from_numpy(p["attn_highres"].reshape(-1))
            o += n
    dev = host.to(device, non_blocking=True)
    out, o = [], 0
    for p, n in zip(payloads, sizes):
        out.append(None if p is None else {"keys": torch.from_numpy(p["keys"]), "attn_highres": dev[o:o + n].view(p["attn_highres"].shape)})
        o += n
    return out


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else list(argv))
    args.no_save_cams = True                             # there is nothing to save here
    seeds = G.seed_options(args, args.num_classes)
    if args.refine == "crf" and not args.img_root:
        raise RuntimeError("--refine crf needs --img_root")
    names = read_names(args.split_file)
    ev = seeds["factory"]()
    missing = 0
    with ThreadPoolExecutor(max_workers=max(1, args.readers)) as pool:
        for k in range(0, len(names), max(1, args.chunk)):
            stems = names[k:k + args.chunk]
            payloads = list(pool.map(lambda s: load_payload(args.cam_dir, s), stems))
            missing += sum(p is None for p in payloads)
            gts = [None if p is None else G.read_gt(args.gt_root, s) for p, s in zip(payloads, stems)] if args.gt_root else None
            images = ([None if p is None else G.load_image(os.path.join(args.img_root, s + ".jpg")) for p, s in zip(payloads, stems)]
                      if args.refine == "crf" else None)
            ev.add(upload(payloads), images, gts, stems)
    from . import cam_seeds as CS
    path = args.out or os.path.join(args.cam_dir, "seed_scores.json")
    CS.write_scores(path, ev.finish())
    print(f"{ev.images} images scored ({missing} without a payload): {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
