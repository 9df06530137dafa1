"""What does the supervised variant's training driver (`train.py --dataset seg`) cost?  Three legs, each one JSON object:

  --kernel  us of wc_step_pair_hist at B x nc x size/16 x size/16 logits against size x size labels, nc = 21 and 81, for a random
            label map and for a map dominated by one class that the logits also predict (the hot cell), with and without the
            per-wave pre-aggregation (WECLIP_STEP_HIST_AGG=1 / 0), beside one read of the label tensor (torch.sum);
  --step    ms of LoggedSupervisedTrainStep(graph=True) against the parent's SupervisedTrainStep(graph=True) (tools/seg_bench.py's
            model and batch), three alternating runs of each;
  --driver  images/s of Trainer.step_once (--dataset seg, log_iters = 200) against the bare SupervisedTrainStep(graph=True) loop fed
            by the same DeviceLoader, on the synthetic tree of tools/loader_bench.py, alternating window by window.

Medians of HIP-event timings after warm-up.  Not part of bench.py.  Needs the GPU; there is no fall-back.

    python tools/seg_train_bench.py --kernel --step --driver [--repeats 15] [--json <file>]

profiles/seg_train_driver_bench.json collects the legs of several such runs.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def median_us(torch, fn, reps=30, inner=10, warmup=3):
    """Median over `reps` event pairs of (time of `inner` back-to-back calls) / inner, in us."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return round(statistics.median(ts), 2)


def kernel_leg(torch, B, S):
    from weclip_vit_comer_amd.validate import step_pair_hist
    out = {"batch": B, "logits": [S // 16, S // 16], "labels": [S, S], "label_bytes": B * S * S * 8}
    before = os.environ.get("WECLIP_STEP_HIST_AGG")
    for nc in (21, 81):
        g = torch.Generator().manual_seed(7)
        seg = torch.randn(B, nc, S // 16, S // 16, generator=g)
        maps = {"random": (seg, torch.randint(0, nc, (B, S, S), generator=g))}
        hot = seg.clone()
        hot[:, 0] += 8.0                                               # class 0 wins nearly everywhere: (0, 0) is the hot cell
        lab = torch.zeros(B, S, S, dtype=torch.int64)
        lab[:, S // 3:S // 2, S // 4:S // 2] = 5                       # one object and a 255 outline, as a real mask has
        lab[:, S // 3, S // 4:S // 2] = 255
        maps["one_class"] = (hot, lab)
        row = {}
        for name, (s, l) in maps.items():
            s, l = s.cuda(), l.cuda()
            flag = torch.zeros(1, device="cuda", dtype=torch.int32)
            hists = {}
            for agg in ("0", "1"):
                os.environ["WECLIP_STEP_HIST_AGG"] = agg
                hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
                step_pair_hist(s, l, nc, hist, flag)
                hists[agg] = hist.clone()
                row[f"{name}_us_agg{agg}"] = median_us(torch, lambda: step_pair_hist(s, l, nc, hist, flag))
            assert torch.equal(hists["0"], hists["1"]), "the two counting forms disagree"
            row[f"{name}_label_read_us"] = median_us(torch, lambda: l.sum())
            row[f"{name}_diag_share"] = round(float(hists["1"].diagonal().max() / hists["1"].sum()), 4)
        out[f"nc{nc}"] = row
    if before is None:
        os.environ.pop("WECLIP_STEP_HIST_AGG", None)
    else:
        os.environ["WECLIP_STEP_HIST_AGG"] = before
    return out


def step_leg(torch, B, S, steps, warmup):
    from oracle import synth
    from weclip_vit_comer_amd.train import LoggedSupervisedTrainStep
    from weclip_vit_comer_amd.train_step import SupervisedTrainStep
    from weclip_vit_comer_amd.WeCLIP_model import model_attn_aff_voc_seg as SEG
    nc = 21
    sd = synth.make_clip_state_dict(seed=0, with_text=False)
    fuse, dec = synth.make_head_state_dicts(width=768)
    img = synth.make_images(B, S, S, seed=100).cuda()
    g = torch.Generator().manual_seed(7)
    lab = torch.randint(0, nc, (B, S // 16, S // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)
    lab[:, :8] = 255
    lab = lab.cuda()

    def run(cls):
        m = SEG.WeCLIP(num_classes=nc, clip_model=sd, embedding_dim=256, in_channels=[768] * 4, device="cuda")
        m.decoder_fts_fuse.load_state_dict(fuse)
        m.decoder.load_state_dict(dec)
        step = cls(m.train(), graph=True)
        return round(median_us(torch, lambda: step(img, lab), reps=steps, inner=1, warmup=warmup) * 1e-3, 3)
    parent, logged = [], []
    for _ in range(3):
        parent.append(run(SupervisedTrainStep))
        logged.append(run(LoggedSupervisedTrainStep))
    pm, lm = statistics.median(parent), statistics.median(logged)
    return {"batch": B, "size": S, "nc": nc, "parent_step_ms": parent, "logged_step_ms": logged, "parent_median_ms": pm,
            "logged_median_ms": lm, "difference_ms": round(lm - pm, 3), "parent_spread_ms": round(max(parent) - min(parent), 3)}


def driver_leg(torch, B, S, images, steps, warmup, repeats):
    import loader_bench
    from oracle import synth
    from train_bench import stats, window
    from weclip_vit_comer_amd import train as T
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12SegDataset
    from weclip_vit_comer_amd.train_step import SupervisedTrainStep, make_optimizer
    from weclip_vit_comer_amd.WeCLIP_model import model_attn_aff_voc_seg as SEG
    sd = synth.make_clip_state_dict(seed=0, with_text=False)
    fuse, dec = synth.make_head_state_dicts(width=768)

    def model():
        m = SEG.WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[768] * 4, device="cuda")
        m.decoder_fts_fuse.load_state_dict(fuse)
        m.decoder.load_state_dict(dec)
        return m.train()
    with tempfile.TemporaryDirectory() as tmp:
        tree = loader_bench.write_tree(os.path.join(tmp, "tree"), images)
        names = open(os.path.join(tree, "train.txt")).read().split()
        with open(os.path.join(tree, "val.txt"), "w") as f:
            f.write("\n".join(names[:4]) + "\n")
        cfg = T._wrap({
            "dataset": {"root_dir": tree, "name_list_dir": tree, "num_classes": 21, "crop_size": S, "resize_range": [512, 2048],
                        "rescale_range": [0.5, 2.0], "ignore_index": 255},
            "work_dir": {"dir": os.path.join(tmp, "work"), "ckpt_dir": "checkpoints", "pred_dir": "predictions", "tb_logger_dir": "tb_logger"},
            "train": {"split": "train", "samples_per_gpu": B, "max_iters": 30000, "eval_iters": 2000, "log_iters": 200},
            "val": {"split": "val"},
            "optimizer": {"learning_rate": 2e-4, "betas": [0.9, 0.999], "weight_decay": 0.01},
            "scheduler": {"warmup_iter": 50, "warmup_ratio": 1e-6, "power": 1.0},
            "clip_init": {}})
        targs = T.build_parser().parse_args(["--config", "-", "--dataset", "seg", "--crop_size", str(S), "--threads", "8", "--prefetch", "2"])
        trainer = T.Trainer(cfg, targs, model=model())
        ds = VOC12SegDataset(root_dir=tree, name_list_dir=tree, split="train", stage="train", crop_size=S, aug=True)
        loader = DeviceLoader(ds, B, shuffle=True, drop_last=True, seed=1, threads=8, prefetch=2)
        bare_model = model()
        step = SupervisedTrainStep(bare_model, make_optimizer(bare_model, lr=2e-4, weight_decay=0.01, betas=(0.9, 0.999), warmup_iter=50,
                                                              max_iter=30000, warmup_ratio=1e-6, power=1.0), graph=True)

        def batches():
            while True:
                for b in loader:
                    yield b[1], b[2]
        it = batches()

        def bare():
            step(*next(it))
        for fn in (trainer.step_once, bare):
            for _ in range(warmup + 2):
                fn()
        ra, rb = [], []
        for _ in range(repeats):
            ra.append(window(torch, trainer.step_once, steps, B))
            rb.append(window(torch, bare, steps, B))
        it.close()
        rec = trainer.log()
        trainer.close()
    a, b = stats(ra, "images_per_s"), stats(rb, "images_per_s")
    return {"batch": B, "size": S, "images": images, "steps": steps, "warmup": warmup, "repeats": repeats, "a_trainer_step_once": a,
            "b_bare_step_device_loader": b, "ratio_a_over_b": round(a["images_per_s"] / b["images_per_s"], 4),
            "b_window_spread": round((b["max"] - b["min"]) / b["images_per_s"], 4), "last_log_record": T.strict_json(rec)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--driver", action="store_true")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "seg_train_bench needs the GPU"
    res = {"device": torch.cuda.get_device_name(0),
           "how": "python tools/seg_train_bench.py --kernel --step --driver (HIP events after warm-up, medians; compared forms alternate "
                  "in one process)"}
    if args.kernel:
        res["kernel"] = kernel_leg(torch, args.batch, args.size)
    if args.step:
        res["step"] = step_leg(torch, args.batch, args.size, args.steps, args.warmup)
    if args.driver:
        res["driver"] = driver_leg(torch, args.batch, args.size, args.images, args.steps, args.warmup, args.repeats)
    print(json.dumps(res, indent=1, allow_nan=False))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1, allow_nan=False)
            f.write("\n")


if __name__ == "__main__":
    main()
