"""Drop-in for the reference's clip/generate_cams_voc12.py: refined CAMs of a VOC12 split as <name>.npy files
({"keys", "attn_highres"}), computed by generate_cams.CamGenerator.  Same command line:

    python -m weclip_vit_comer_amd.clip.generate_cams_voc12 --img_root .../JPEGImages --split_file voc12/train.txt --cam_out_dir out \\
        --model ViT-B-16.pt --num_workers 1 [--reference_root <reference checkout>]

The class-name tables (`class_names`, `new_class_names`, `BACKGROUND_CATEGORY` of clip/clip_text.py) come from the user's
reference checkout, on the clip package path after install_dropin(reference_root=...).  `clip.generate_cams_voc12` resolves to
this module only in an interpreter that has called install_dropin(); from a shell use the full module name above."""
import argparse
import importlib
import os
import sys

import numpy as np

from . import generate_cams as G

BOX_THRESHOLD = 0.4          # scoremap2bbox threshold of the VOC dumper (voc12:170)
NUM_CLASSES = 21            # background included (the seed scores of --gt_root)
FG_NAMES, BG_NAMES = "new_class_names", "BACKGROUND_CATEGORY"

MODULE = __spec__.name if __spec__ is not None else __name__      # importable name, also under `python -m`


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="")
    p.add_argument("--img_root", type=str, required=True)
    p.add_argument("--split_file", type=str, default="./voc12/train.txt")
    p.add_argument("--cam_out_dir", type=str, default="./final/ablation/voc_baseline")
    p.add_argument("--model", type=str, required=True)
    p.add_argument("--num_workers", type=int, default=1)
    p.add_argument("--reference_root", type=str, default=None, help="reference checkout holding clip/clip_text.py and the BPE merges")
    p.add_argument("--worker_id", type=int, default=None, help=argparse.SUPPRESS)
    G.add_seed_arguments(p)
    return p.parse_args(argv)


def name_tables():
    return importlib.import_module(__package__ + ".clip_text")


def make_generator(model_path, fg_names=FG_NAMES, bg_names=BG_NAMES, thr=BOX_THRESHOLD):
    from ..WeCLIP_model.model_attn_aff_voc import default_text_features
    from .clip import load
    model, _ = load(model_path, device="cuda")
    text = default_text_features(model, fg_names, bg_names)
    if text is None:
        raise RuntimeError("the class-name tables (clip.clip_text) or the BPE merges file were not found: pass "
                           "--reference_root <reference checkout>")
    bg, fg = text
    return G.CamGenerator(model, fg, bg, thr)


def read_item_factory(img_root):
    tables = []

    def read_item(name):
        if not tables:           # resolved at the first image: a worker with an empty share needs no tables
            tables.append(name_tables())
        t = tables[0]
        xml = os.path.join(img_root, name).replace("/JPEGImages", "/Annotations").replace(".jpg", ".xml")
        with open(xml) as fid:
            ids, _ = G.voc_label_ids(fid.read(), list(t.class_names), list(t.new_class_names))
        return name, ids
    return read_item


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse_args(argv)
    if args.reference_root:
        from .. import install_dropin
        install_dropin(reference_root=args.reference_root)
    os.makedirs(args.cam_out_dir, exist_ok=True)
    train_list = [str(x) + ".jpg" for x in np.atleast_1d(np.loadtxt(args.split_file, dtype=str))]
    n = min(max(args.num_workers, 1), G.MAX_WORKERS)
    seeds = G.seed_options(args, NUM_CLASSES)
    if seeds and args.worker_id is None:
        G.clear_parts(args.cam_out_dir)
    if n > 1 and args.worker_id is None:
        rc = G.spawn_workers(n, MODULE, argv)
        if seeds:
            G.write_seed_scores(args.cam_out_dir, n, seeds)
        return rc
    shares = G.split_dataset(train_list, n)
    rc = G.run_worker(args.worker_id or 0, shares, args.img_root, args.cam_out_dir, lambda: make_generator(args.model),
                      read_item_factory(args.img_root), seeds=seeds)
    if seeds and args.worker_id is None:
        G.write_seed_scores(args.cam_out_dir, 1, seeds)
    return rc


if __name__ == "__main__":
    sys.exit(main())
