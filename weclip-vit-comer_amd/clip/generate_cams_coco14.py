"""Drop-in for the reference's clip/generate_cams_coco14.py: refined CAMs of a COCO14 split as <name>.npy files, computed by
generate_cams.CamGenerator.  The split file carries the label ids: `<image name> <id> <id> ...` per line
(coco14:35-47,109-113); box threshold 0.7."""
import argparse
import os
import sys

from . import generate_cams as G
from . import generate_cams_voc12 as V

BOX_THRESHOLD = 0.7
NUM_CLASSES = 81            # background included (the seed scores of --gt_root)
FG_NAMES, BG_NAMES = "new_class_names_coco", "BACKGROUND_CATEGORY_COCO"

MODULE = __spec__.name if __spec__ is not None else __name__      # importable name, also under `python -m`


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="")
    p.add_argument("--img_root", type=str, required=True)
    p.add_argument("--split_file", type=str, default="./coco14/train.txt")
    p.add_argument("--cam_out_dir", type=str, default="./final/ablation/coco_baseline")
    p.add_argument("--model", type=str, required=True)
    p.add_argument("--num_workers", type=int, default=1)
    p.add_argument("--reference_root", type=str, default=None, help="reference checkout holding clip/clip_text.py and the BPE merges")
    p.add_argument("--worker_id", type=int, default=None, help=argparse.SUPPRESS)
    G.add_seed_arguments(p)
    return p.parse_args(argv)


def read_split(path):
    """[(file name, label ids)] of a split file."""
    with open(path) as fid:
        rows = [G.coco_split_line(l) for l in fid.read().splitlines() if l.strip()]
    return [(n if n.endswith(".jpg") else n + ".jpg", ids) for n, ids in rows]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse_args(argv)
    if args.reference_root:
        from .. import install_dropin
        install_dropin(reference_root=args.reference_root)
    os.makedirs(args.cam_out_dir, exist_ok=True)
    items = read_split(args.split_file)
    n = min(max(args.num_workers, 1), G.MAX_WORKERS)
    seeds = G.seed_options(args, NUM_CLASSES)
    if seeds and args.worker_id is None:
        G.clear_parts(args.cam_out_dir)
    if n > 1 and args.worker_id is None:
        rc = G.spawn_workers(n, MODULE, argv)
        if seeds:
            G.write_seed_scores(args.cam_out_dir, n, seeds)
        return rc
    shares = G.split_dataset(items, n)
    rc = G.run_worker(args.worker_id or 0, shares, args.img_root, args.cam_out_dir,
                      lambda: V.make_generator(args.model, FG_NAMES, BG_NAMES, BOX_THRESHOLD), lambda it: it, seeds=seeds)
    if seeds and args.worker_id is None:
        G.write_seed_scores(args.cam_out_dir, 1, seeds)
    return rc


if __name__ == "__main__":
    sys.exit(main())
