"""What do the training image panels (`train.py --panel_iters`, utils/panels.py, csrc/panels.hip) cost?  Four legs, one JSON object:

  --kernel  us of wc_panel_snapshot at B x 21 x size/16 x size/16 logits, B x size x size int64 labels and (B, hw, hw) attn_pred,
            beside a device-to-device copy (Tensor.copy_ of a contiguous uint8 buffer: hipMemcpyAsync) of the bytes it reads,
            alternating;
  --render  ms of one full panel set (images, pseudo_label, prediction, seg_conf, four attn_pred grids) into a PanelWriter slot,
            the asynchronous copy to the host included, the PNG encoding (writer threads) not;
  --step    ms of the graph-replayed LoggedTrainStep with panels= set against the same step without (bench.py's model and
            synthetic batch), three alternating runs of each;
  --driver  images/s of Trainer.fit windows of 200 iterations with --panel_iters 200 against off, on the synthetic tree of
            tools/loader_bench.py, alternating window by window.

Medians of HIP-event timings after warm-up.  Not part of bench.py.  Needs the GPU; there is no fall-back.

    python tools/panel_bench.py --kernel --render --step --driver [--json profiles/panel_bench.json]
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


def timed(torch, fn, reps=30, inner=10, warmup=3, scale=1e3):
    """Median over `reps` event pairs of (time of `inner` back-to-back calls) / inner; scale 1e3: us, 1: ms."""
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
        ts.append(a.elapsed_time(b) * scale / inner)
    return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)


def kernel_leg(torch, B, S):
    from weclip_vit_comer_amd.utils.panels import StepSnapshot
    hw = (S // 16) ** 2
    g = torch.Generator().manual_seed(7)
    seg = torch.randn(B, 21, S // 16, S // 16, generator=g).cuda()
    lab = torch.randint(0, 21, (B, S, S), generator=g).cuda()
    attn = torch.rand(B, hw, hw, generator=g).cuda()
    snap = StepSnapshot()
    read = seg.numel() * 4 + lab.numel() * 8 + B * 4 * hw * 4
    src, dst = torch.empty(read, dtype=torch.uint8, device="cuda"), torch.empty(read, dtype=torch.uint8, device="cuda")
    rows = {"snapshot_us": [], "copy_us": []}
    for _ in range(3):
        rows["snapshot_us"].append(timed(torch, lambda: snap.take(seg, lab, attn))[0])
        rows["copy_us"].append(timed(torch, lambda: dst.copy_(src))[0])
    return {"batch": B, "size": S, "bytes_read": read, "bytes_written": seg.numel() * 4 + lab.numel() + B * 4 * hw * 4, **rows,
            "snapshot_median_us": statistics.median(rows["snapshot_us"]), "copy_median_us": statistics.median(rows["copy_us"])}


def render_leg(torch, B, S, tmp):
    from weclip_vit_comer_amd import train as T
    from weclip_vit_comer_amd.utils.panels import StepSnapshot
    hw = (S // 16) ** 2
    g = torch.Generator().manual_seed(8)

    class Host:                                           # what Trainer.render_panels reads of a trainer
        kind, n_iter = "voc", 0
        render_panels = T.Trainer.render_panels
    host = Host()
    host.snapshot = StepSnapshot().take(torch.randn(B, 21, S // 16, S // 16, generator=g).cuda(),
                                        torch.randint(0, 21, (B, S, S), generator=g).cuda(), torch.rand(B, hw, hw, generator=g).cuda())
    host._last_inputs = torch.randn(B, 3, S, S, generator=g).cuda()
    host.panel_writer = T.PanelWriter(os.path.join(tmp, "panels"), depth=2)
    real, host.panel_writer._write = host.panel_writer._write, lambda slot, n: slot.copied.synchronize()      # no PNG encoding
    med, lo, hi = timed(torch, host.render_panels, reps=10, inner=1, warmup=2, scale=1)
    host.panel_writer._write = real
    host.render_panels()                                  # one real set: the files' sizes
    host.panel_writer.finish()
    sizes = {f: os.path.getsize(os.path.join(tmp, "panels", f)) for f in sorted(os.listdir(os.path.join(tmp, "panels")))}
    return {"batch": B, "size": S, "render_ms": med, "min": lo, "max": hi, "png_bytes": sizes}


def step_leg(torch, B, S, steps, warmup):
    import bench
    from weclip_vit_comer_amd.data import SyntheticVOCLoader
    from weclip_vit_comer_amd.train import LoggedTrainStep
    from weclip_vit_comer_amd.utils.panels import StepSnapshot
    img, labels = SyntheticVOCLoader(B, S, 2, rank=0, world=1, device="cuda", source="uint8").next()

    def run(panels):
        step = LoggedTrainStep(bench.make_model("cuda"), graph=True, panels=StepSnapshot() if panels else None)
        return timed(torch, lambda: step(img, labels=labels), reps=steps, inner=1, warmup=warmup, scale=1)[0]
    off, on = [], []
    for _ in range(3):
        off.append(run(False))
        on.append(run(True))
    return {"batch": B, "size": S, "panels_off_step_ms": off, "panels_on_step_ms": on, "off_median_ms": statistics.median(off),
            "on_median_ms": statistics.median(on), "difference_ms": round(statistics.median(on) - statistics.median(off), 3),
            "off_spread_ms": round(max(off) - min(off), 3)}


def driver_leg(torch, B, S, images, repeats, tmp):
    import bench
    import loader_bench
    from train_bench import stats, window
    from weclip_vit_comer_amd import train as T
    tree = loader_bench.write_tree(os.path.join(tmp, "tree"), images)
    names = open(os.path.join(tree, "train.txt")).read().split()
    with open(os.path.join(tree, "val.txt"), "w") as f:
        f.write("\n".join(names[:4]) + "\n")

    def trainer(panel_iters):
        cfg = T._wrap({
            "dataset": {"root_dir": tree, "name_list_dir": tree, "num_classes": 21, "crop_size": S, "resize_range": [512, 2048],
                        "rescale_range": [0.5, 2.0], "ignore_index": 255},
            "work_dir": {"dir": os.path.join(tmp, f"work{panel_iters}"), "ckpt_dir": "checkpoints", "pred_dir": "predictions",
                         "tb_logger_dir": "tb_logger"},
            "train": {"split": "train", "samples_per_gpu": B, "max_iters": 30000, "eval_iters": 100000, "log_iters": 200},
            "val": {"split": "val"},
            "optimizer": {"learning_rate": 2e-4, "betas": [0.9, 0.999], "weight_decay": 0.01},
            "scheduler": {"warmup_iter": 50, "warmup_ratio": 1e-6, "power": 1.0},
            "clip_init": {}})
        targs = T.build_parser().parse_args(["--config", "-", "--crop_size", str(S), "--threads", "8", "--prefetch", "2",
                                             "--panel_iters", str(panel_iters)])
        return T.Trainer(cfg, targs, model=bench.make_model("cuda"))
    on, off = trainer(200), trainer(0)
    for tr in (on, off):
        tr.fit(until=8)                                   # eager, capture, first replays
    ra, rb = [], []
    for _ in range(repeats):                              # every `on` window holds exactly one render (iteration 200 k)
        ra.append(window(torch, lambda: on.fit(until=on.n_iter + 1), 200, B))
        rb.append(window(torch, lambda: off.fit(until=off.n_iter + 1), 200, B))
    on.close()
    off.close()
    a, b = stats(ra, "images_per_s"), stats(rb, "images_per_s")
    return {"batch": B, "size": S, "window_steps": 200, "repeats": repeats, "a_panel_iters_200": a, "b_panels_off": b,
            "ratio_a_over_b": round(a["images_per_s"] / b["images_per_s"], 4),
            "b_window_spread": round((b["max"] - b["min"]) / b["images_per_s"], 4),
            "panel_files": len(os.listdir(os.path.join(tmp, "work200", "panels")))}


def main():
    ap = argparse.ArgumentParser()
    for leg in ("kernel", "render", "step", "driver"):
        ap.add_argument("--" + leg, action="store_true")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "panel_bench needs the GPU"
    res = {"device": torch.cuda.get_device_name(0),
           "how": "python tools/panel_bench.py --kernel --render --step --driver (HIP events after warm-up, medians; compared forms "
                  "alternate in one process)"}
    with tempfile.TemporaryDirectory() as tmp:
        if args.kernel:
            res["kernel"] = kernel_leg(torch, args.batch, args.size)
        if args.render:
            res["render"] = render_leg(torch, args.batch, args.size, tmp)
        if args.step:
            res["step"] = step_leg(torch, args.batch, args.size, args.steps, args.warmup)
        if args.driver:
            res["driver"] = driver_leg(torch, args.batch, args.size, args.images, args.repeats, tmp)
    print(json.dumps(res, indent=1, allow_nan=False))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1, allow_nan=False)
            f.write("\n")


if __name__ == "__main__":
    main()
