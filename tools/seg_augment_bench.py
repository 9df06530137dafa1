"""Time of the label-aware device input pipeline (data.DeviceSegAugment) next to the image-only DeviceAugment.

    python tools/seg_augment_bench.py [--batch 16] [--reps 100] [--json out.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/seg_augment_bench.py --reps 50      (per-kernel times)

ms per batch (B = 16, 375 x 500 uint8 sources -> 512 x 512), parameters device-resident, HIP events around `reps` calls
after a warm-up, median of 5 such rounds:
  image_only        DeviceAugment, rescale_range=None (same geometry as the seg calls)
  image_only_scaled DeviceAugment with its default rescale_range (0.5, 2.0)
  seg_geometry      DeviceSegAugment(photometric=False)
  seg_full          DeviceSegAugment()
  select_alone      wc_seg_crop_select: index tables + candidate histograms + select (no gather)
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=10, rounds=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--crop", type=int, default=512)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import weclip_vit_comer_amd  # noqa: F401
    from weclip_vit_comer_amd import _lib as L
    from weclip_vit_comer_amd import synth
    from weclip_vit_comer_amd.data import DeviceAugment, DeviceSegAugment
    B, H, W, crop = a.batch, 375, 500, a.crop
    f = synth.make_images(B, H, W, seed=100)
    imgs = (f * 58.0 + 118.0).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
    labs = synth.make_label_maps(B, H, W, regions=8, seed=7).cuda()
    res = {}

    def add(name, fn):
        med, lo, hi = timed(fn, a.reps)
        res[name] = dict(ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4))
        print(f"{name:18s} {med:8.4f} ms per batch  (rounds {lo:.4f} ... {hi:.4f})", file=sys.stderr)

    for name, rng in (("image_only", None), ("image_only_scaled", (0.5, 2.0))):
        aug = DeviceAugment(crop_size=crop, rescale_range=rng, seed=1)
        p = aug.draw(B, H, W).cuda()
        add(name, lambda aug=aug, p=p: aug(imgs, p))
    for name, photo in (("seg_geometry", False), ("seg_full", True)):
        aug = DeviceSegAugment(crop_size=crop, photometric=photo, seed=1)
        rec, cand = (t.cuda() for t in aug.draw(B, H, W))
        add(name, lambda aug=aug, rec=rec, cand=cand: aug(imgs, labs, (rec, cand)))
    sel = torch.empty(B, 4, dtype=torch.int32, device="cuda")
    box = torch.empty_like(sel)
    cm = aug.canvas_max(H, W)
    add("select_alone", lambda: L.lib().wc_seg_crop_select(L.ptr(labs, torch.uint8), L.ptr(rec, torch.int32), L.ptr(cand, torch.int32),
                                                           L.ptr(sel), L.ptr(box), L.ptr(aug._ws, torch.int32), B, H, W, crop, cm,
                                                           aug.n_cand, 255, L.stream()))
    out = dict(batch=B, src_hw=[H, W], crop=crop, reps=a.reps, device=torch.cuda.get_device_name(0), results=res)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
