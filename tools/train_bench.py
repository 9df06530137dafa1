"""What does the training driver cost on top of the step it drives?  One process, the synthetic JPEG tree of
tools/loader_bench.py, B = 16, crop 512:

  (a) train.Trainer.step_once (log_iters = 200: no log line inside a window), graph replay;
  (b) the bare TrainStep(graph=True) + DeviceLoader loop -- row (c) of DESIGN.md section 12.3;

HIP events around windows of --steps steps after --warmup steps, --repeats windows, (a) and (b) alternating window by window on
the same box (each has its own model and loader, same seeds).  Then validation, ms per image over 32 images of 375x500:

  (v) validate.Validator.run (one wc_val_pair_hist launch per image, two reads at the end);
  (h) the reference-shaped host loop (scripts/dist_clip_voc.py:71-102: arg-max map, CAM and labels to the host as int16 per
      image, evaluate.scores at the end) around the same model.

    python tools/train_bench.py [--json profiles/train_driver_bench.json]

Needs the GPU; there is no fall-back."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(vals, key):
    return {key: round(statistics.median(vals), 2), "min": round(min(vals), 2), "max": round(max(vals), 2)}


def window(torch, fn, steps, batch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return batch * steps / (e0.elapsed_time(e1) * 1e-3)


def host_validate(torch, model, loader, nc=21):
    """validate() of scripts/dist_clip_voc.py:71-102 around this package's model and loader."""
    import torch.nn.functional as F
    from weclip_vit_comer_amd.datasets import labels_from_onehot
    from weclip_vit_comer_amd.utils import evaluate
    preds, gts, cams = [], [], []
    model.eval()
    with torch.no_grad():
        for _, inputs, labels, _ in loader:
            segs, cam, _ = model(inputs, [""], mode="val", labels=labels_from_onehot(loader.last_cls_labels))
            resized = F.interpolate(segs, size=labels.shape[1:], mode="bilinear", align_corners=False)
            preds += list(torch.argmax(resized, dim=1).cpu().numpy().astype(np.int16))
            cams += list(cam.cpu().numpy().astype(np.int16))
            gts += list(labels.cpu().numpy().astype(np.int16))
    _, seg_score = evaluate.scores(gts, preds, np.zeros((nc, nc)), num_classes=nc)
    _, cam_score = evaluate.scores(gts, cams, np.zeros((nc, nc)), num_classes=nc)
    model.train()
    return seg_score, cam_score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--val-images", type=int, default=32)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import bench
    import loader_bench
    from weclip_vit_comer_amd import train as T
    from weclip_vit_comer_amd.datasets import DeviceLoader, labels_from_onehot
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset, VOC12SegDataset
    from weclip_vit_comer_amd.train_step import TrainStep, make_optimizer
    from weclip_vit_comer_amd.validate import Validator
    assert torch.cuda.is_available(), "train_bench needs the GPU"
    with tempfile.TemporaryDirectory() as tmp:
        tree = loader_bench.write_tree(os.path.join(tmp, "tree"), args.images)
        names = open(os.path.join(tree, "train.txt")).read().split()
        from PIL import Image

        def size_of(name):
            with Image.open(os.path.join(tree, "JPEGImages", name + ".jpg")) as im:
                return im.size[::-1]
        fixed = [n for n in names if size_of(n) == (375, 500)][:args.val_images]
        assert len(fixed) == args.val_images, f"the tree holds only {len(fixed)} images of 375x500"
        with open(os.path.join(tree, "val.txt"), "w") as f:
            f.write("\n".join(fixed) + "\n")
        cfg = T._wrap({
            "dataset": {"root_dir": tree, "name_list_dir": tree, "num_classes": 21, "crop_size": args.size, "resize_range": [512, 2048],
                        "rescale_range": [0.5, 2.0], "ignore_index": 255},
            "work_dir": {"dir": os.path.join(tmp, "work"), "ckpt_dir": "checkpoints", "pred_dir": "predictions", "tb_logger_dir": "tb_logger"},
            "train": {"split": "train", "samples_per_gpu": args.batch, "max_iters": 30000, "eval_iters": 2000, "log_iters": 200},
            "val": {"split": "val"},
            "optimizer": {"learning_rate": 2e-4, "betas": [0.9, 0.999], "weight_decay": 0.01},
            "scheduler": {"warmup_iter": 50, "warmup_ratio": 1e-6, "power": 1.0},
            "clip_init": {}})
        targs = T.build_parser().parse_args(["--config", "-", "--crop_size", str(args.size), "--threads", "8", "--prefetch", "2"])
        trainer = T.Trainer(cfg, targs, model=bench.make_model("cuda"))
        # (b): what the trainer wraps, written out (the loop of tools/loader_bench.py row (c))
        ds = VOC12ClsDataset(root_dir=tree, name_list_dir=tree, split="train", stage="train", crop_size=args.size, aug=True)
        loader = DeviceLoader(ds, args.batch, shuffle=True, drop_last=True, seed=1, threads=8, prefetch=2)
        bare_model = bench.make_model("cuda")
        step = TrainStep(bare_model, make_optimizer(bare_model, lr=2e-4, weight_decay=0.01, betas=(0.9, 0.999), warmup_iter=50,
                                                    max_iter=30000, warmup_ratio=1e-6, power=1.0), radius=8, graph=True)     # = cfg above

        def batches():
            while True:
                for b in loader:
                    yield b[1], labels_from_onehot(loader.last_cls_labels)
        it = batches()

        def bare():
            img, labels = next(it)
            step(img, labels=labels)
        for fn in (trainer.step_once, bare):
            for _ in range(args.warmup + 2):
                fn()
        ra, rb = [], []
        for _ in range(args.repeats):
            ra.append(window(torch, trainer.step_once, args.steps, args.batch))
            rb.append(window(torch, bare, args.steps, args.batch))
        it.close()
        rec = trainer.log()                                            # the window's log line still works after the timing
        # validation: the driver's Validator against the reference-shaped host loop, same model, alternating
        val_ds = VOC12SegDataset(root_dir=tree, name_list_dir=tree, split="val", stage="train", aug=False)
        n_val = len(val_ds)
        v = Validator(trainer.model, 21)
        mv, mh = [], []
        scores = None
        for r in range(args.repeats + 1):
            for which, out in (("v", mv), ("h", mh)):
                ld = DeviceLoader(val_ds, 1, shuffle=False, threads=8, prefetch=2)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s = v.run(ld) if which == "v" else host_validate(torch, trainer.model, ld)
                torch.cuda.synchronize()
                if r:                                                  # the first round warms both up
                    out.append((time.perf_counter() - t0) * 1e3 / n_val)
                scores = scores or {}
                scores[which] = float(s[0]["miou"])
        trainer.close()
    a, b = stats(ra, "images_per_s"), stats(rb, "images_per_s")
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "size": args.size, "images": args.images, "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats, "a_trainer_step_once": a, "b_bare_trainstep_device_loader": b,
           "ratio_a_over_b": round(a["images_per_s"] / b["images_per_s"], 4),
           "b_window_spread": round((b["max"] - b["min"]) / b["images_per_s"], 4),
           "last_log_record": T.strict_json(rec), "val_images": n_val, "val_size": [375, 500],
           "v_validator_ms_per_image": stats(mv, "ms_per_image"), "h_host_loop_ms_per_image": stats(mh, "ms_per_image"),
           "val_seg_miou": scores,
           "how": "python tools/train_bench.py (HIP events, windows of `steps` steps after `warmup`, `repeats` windows, median; (a) and "
                  "(b) alternate in one process; validation: wall clock around whole passes ending in a device synchronise)"}
    print(json.dumps(res, indent=1, allow_nan=False))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1, allow_nan=False)
            f.write("\n")


if __name__ == "__main__":
    main()
