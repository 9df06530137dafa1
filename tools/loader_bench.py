"""Does decoding on 4-8 host threads keep up with the training step?  Three rates, images/s:

  (a) datasets.DeviceLoader alone over a synthetic VOC-shaped tree (JPEGs of mixed sizes up to 500x500 + PNG labels written
      with Pillow into a temporary directory), per decode-thread count;
  (b) TrainStep(graph=True) at B=16, 512x512 fed from SyntheticVOCLoader(source="uint8") (device-resident pool: no decoding);
  (c) the same step fed from DeviceLoader (threads=8).

    python tools/loader_bench.py [--json profiles/loader_bench.json] [--parent-root DIR]

HIP events around windows of --steps steps after --warmup steps, --repeats windows, median reported with min / max; (b) and
(c) alternate window by window in one process.  --parent-root: a built checkout of the parent commit; its (b) is measured by
this file in a fresh child process on the same machine, before this process touches the GPU.  Needs the GPU; there is no fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_tree(root, n, seed=0):
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "SegmentationClassAug"))
    names, onehot = [], {}
    for i in range(n):
        H, W = (int(rs.randint(280, 501)), int(rs.randint(333, 501))) if i % 4 else (375, 500)
        if i % 7 == 3:
            H, W = W, H
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.stack([127 + 90 * np.sin(xx / (9.0 + 3 * c) + i) * np.cos(yy / (11.0 + c)) for c in range(3)], -1)
        img = np.clip(img + rs.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)
        name = f"{2007 + i % 6}_{i:06d}"
        Image.fromarray(img).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=90)
        ids = sorted(rs.choice(20, size=2, replace=False).tolist())       # two classes per image, as bench.py's batches
        lab = np.zeros((H, W), np.uint8)
        lab[H // 5:H // 2, W // 6:W // 2] = ids[0] + 1
        lab[H // 2:, W // 2:] = ids[1] + 1
        Image.fromarray(lab).save(os.path.join(root, "SegmentationClassAug", name + ".png"))
        v = np.zeros(20, np.float32)
        v[ids] = 1
        names.append(name)
        onehot[name] = v
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    np.save(os.path.join(root, "cls_labels_onehot.npy"), onehot)
    return root


def stats(rates):
    return {"images_per_s": round(statistics.median(rates), 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}


def window(torch, step, feed, steps, batch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        img, labels = feed()
        step(img, labels=labels)
    e1.record()
    torch.cuda.synchronize()
    return batch * steps / (e0.elapsed_time(e1) * 1e-3)


def synthetic_feed(args):
    from weclip_vit_comer_amd.data import SyntheticVOCLoader
    return SyntheticVOCLoader(args.batch, args.size, 2, device="cuda", source="uint8").next


def make_step():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    from weclip_vit_comer_amd.train_step import TrainStep
    return TrainStep(bench.make_model("cuda"), graph=True)


def only_b(args):
    import torch
    step, feed = make_step(), synthetic_feed(args)
    for _ in range(args.warmup + 2):
        img, labels = feed()
        step(img, labels=labels)
    rates = [window(torch, step, feed, args.steps, args.batch) for _ in range(args.repeats)]
    print("LOADER_BENCH_B " + json.dumps(stats(rates)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--commit", default=None, help="recorded in the JSON (a checkout without .git cannot tell)")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--only-b", action="store_true", help="measure (b) alone and print it (the child of --parent-root)")
    ap.add_argument("--root", default=None, help="with --only-b: the checkout whose package and bench.py are imported")
    args = ap.parse_args()
    if args.only_b:
        global ROOT
        ROOT = args.root or ROOT
        return only_b(args)
    parent_b = None
    if args.parent_root:                 # a fresh child, run to its end before this process opens the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--only-b", "--root", os.path.abspath(args.parent_root)]
        cmd += ["--batch", str(args.batch), "--size", str(args.size), "--steps", str(args.steps), "--warmup", str(args.warmup),
                "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=args.parent_root, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith("LOADER_BENCH_B ")]
        if r.returncode != 0 or not line:
            raise RuntimeError("parent (b) failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        parent_b = json.loads(line[-1][len("LOADER_BENCH_B "):])
    sys.path.insert(0, ROOT)
    import torch
    from weclip_vit_comer_amd.datasets import DeviceLoader, labels_from_onehot
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset
    assert torch.cuda.is_available(), "loader_bench needs the GPU"
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        write_tree(tmp, args.images)
        t_tree = time.perf_counter() - t0
        ds = VOC12ClsDataset(root_dir=tmp, name_list_dir=tmp, split="train", stage="train", crop_size=args.size, aug=True)
        # (a) the loader alone: one warm epoch (page cache, pinned buffers), then --repeats epochs per thread count
        alone = {}
        for threads in (1, 2, 4, 8):
            ld = DeviceLoader(ds, args.batch, shuffle=True, drop_last=True, seed=1, threads=threads, prefetch=2)
            for _ in ld:
                pass
            rates = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 0
                for batch in ld:
                    n += len(batch[0])
                torch.cuda.synchronize()
                rates.append(n / (time.perf_counter() - t0))
            alone[str(threads)] = stats(rates)
            print(f"(a) loader alone, {threads} threads: {alone[str(threads)]}", flush=True)
        # (b) / (c): one step object, the two feeds alternating window by window
        step, feed_b = make_step(), synthetic_feed(args)
        ld = DeviceLoader(ds, args.batch, shuffle=True, drop_last=True, seed=1, threads=8, prefetch=2)

        def batches():
            while True:
                for b in ld:
                    yield b[1], labels_from_onehot(ld.last_cls_labels)
        it = batches()
        feed_c = lambda: next(it)          # noqa: E731
        for feed in (feed_b, feed_c):
            for _ in range(args.warmup + 2):
                img, labels = feed()
                step(img, labels=labels)
        rb, rc = [], []
        for _ in range(args.repeats):
            rb.append(window(torch, step, feed_b, args.steps, args.batch))
            rc.append(window(torch, step, feed_c, args.steps, args.batch))
        it.close()
    b, c = stats(rb), stats(rc)
    keep_up = [int(t) for t in alone if alone[t]["images_per_s"] >= b["images_per_s"]]
    res = {"commit": args.commit, "parent_commit": args.parent_commit, "device": torch.cuda.get_device_name(0), "batch": args.batch,
           "size": args.size, "images": args.images, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "tree_write_s": round(t_tree, 1), "a_loader_alone_by_threads": alone, "b_step_synthetic": b, "c_step_device_loader": c,
           "b_parent_commit_same_box": parent_b, "ratio_c_over_b": round(c["images_per_s"] / b["images_per_s"], 4),
           "threads_where_a_reaches_b": min(keep_up) if keep_up else None,
           "how": "python tools/loader_bench.py (HIP events, windows of `steps` steps after `warmup`, `repeats` windows, median; "
                  "(b) and (c) alternate in one process; (a) wall clock around whole epochs ending in a device synchronise)"}
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
