"""What the CAM-seed path costs on one GPU.

    python tools/camseed_bench.py [--images 64] [--crf-images 8] [--reps 5] [--out profiles/camseed_bench.json]

kernels   wc_cam_seed_sweep at 32 pairs of 375 x 500 (16 images x 2 classes), T = 16, nc = 21 and nc = 81, and at 16 times as many
          pairs: microseconds per launch (device events around `--calls` back-to-back launches, tables already on the device;
          median of --reps windows after warm-up), against
            floor      one read of its inputs at the HBM peak (8 TB/s): K x HW x 2 B + HW B per image.  The 32-pair input is
                       15 MB and stays in the 256 MiB Infinity Cache between launches: the floor is an HBM figure, the
                       measurement at that size is not
            stock      the same confusion matrices by stock tensor ops on the same GPU: T times (threshold plane + maps,
                       arg-max, table look-up, bincount)
            numpy      the per-image, per-threshold loop of tests/camseed_ref.py on the host (one pass, host clock)
          and wc_cam_seed_labels + wc_cam_seed_merge on the same 32 pairs.
dumper    CamGenerator over the 64 synthetic VOC-shaped images of tools/camgen_bench.py in chunks of 16, as run_worker drives
          it, images/s (host clock around a whole pass that ends in a device synchronise; one warm-up pass; median of --reps):
          as today / with the sweep / with masks, scores and PNGs (refine none) / with the CRF in each bilateral mode (the CRF
          rows over the first --crf-images images only).  No .npy file is written in any row; the maps are copied to the host
          in every row, as the dumpers do unless --no_save_cams is given.
"""
import argparse
import ctypes
import json
import os
import socket
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import weclip_vit_comer_amd  # noqa: E402,F401
from oracle import synth  # noqa: E402
from weclip_vit_comer_amd import _lib as L  # noqa: E402
from weclip_vit_comer_amd import clip  # noqa: E402
from weclip_vit_comer_amd.clip import cam_seeds as CS  # noqa: E402
from weclip_vit_comer_amd.clip import generate_cams as G  # noqa: E402

HBM_PEAK = 8.0e12
THRESHOLDS = [round(0.05 + 0.05 * i, 10) for i in range(16)]
H0, W0 = 375, 500


def windows(fn, calls, reps, warmup=3):
    """Microseconds per call: median, min, max over `reps` windows of `calls` back-to-back calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return dict(us=round(statistics.median(out), 2), us_min=round(min(out), 2), us_max=round(max(out), 2))


def synthetic_bucket(B, K, nc, seed):
    """B images of H0 x W0 with K maps each: smooth maps in [0, 1] (a 25-pixel grid, bilinearly up-sampled, plus noise) and a
    block ground truth with an ignore border, built on the device from a seeded generator."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    coarse = torch.rand(B * K, 1, H0 // 25 + 2, W0 // 25 + 2, device="cuda", generator=g)
    cams = torch.nn.functional.interpolate(coarse, size=(H0, W0), mode="bilinear", align_corners=False)[:, 0]
    cams = (0.9 * cams + 0.1 * torch.rand(B * K, H0, W0, device="cuda", generator=g)).to(torch.float16).contiguous()
    rng = np.random.default_rng(seed)
    keys = [sorted(int(v) for v in rng.choice(nc - 1, K, replace=False)) for _ in range(B)]
    gt = torch.zeros(B, H0, W0, dtype=torch.uint8, device="cuda")
    for b in range(B):
        for k in keys[b]:
            y, x = int(rng.integers(0, H0 - 120)), int(rng.integers(0, W0 - 160))
            gt[b, y:y + 120, x:x + 160] = k + 1
        gt[b, :3] = 255
    return cams.view(B * K, H0 * W0), keys, gt.view(B, H0 * W0)


def stock_sweep(cams, tables, gt, thresholds, nc):
    """The same (T, nc, nc) matrices from stock tensor ops (keys ascending per image, so the first maximum is the smallest id)."""
    B, K = tables.B, tables.Kmax
    maps = cams.view(B, K, -1).float()
    g = gt.long()
    valid = g < nc
    conf = []
    for t in thresholds:
        plane = torch.full_like(maps[:, :1], t)
        slot = torch.cat([plane, maps], 1).argmax(1)                       # the threshold plane first: it wins a tie
        label = tables.slot_class.long().gather(1, slot)
        conf.append(torch.bincount(nc * g[valid] + label[valid], minlength=nc * nc).view(nc, nc))
    return torch.stack(conf)


def sweep_rows(reps, calls):
    import camseed_ref as R
    rows = {}
    for nc in (21, 81):
        for B in (16, 256):
            K = 2
            cams, keys, gt = synthetic_bucket(B, K, nc, 10 + nc)
            t = CS.PairTables(keys, nc, cams.device)
            T = len(THRESHOLDS)
            bins = torch.zeros(nc, nc, T + 1, device="cuda", dtype=torch.int64)
            thr = (ctypes.c_float * T)(*THRESHOLDS)
            flag = torch.zeros(1, device="cuda", dtype=torch.int32)
            ptrs = [L.ptr(x) for x in (cams, t.first, t.keys, gt)] + [thr, L.ptr(bins), L.ptr(flag)]
            entry = L.lib().wc_cam_seed_sweep                     # the C entry itself: the wrapper's host checks are not the kernel

            def fn(force=0):
                entry(*ptrs, B, B * K, H0 * W0, nc, T, K, force, L.stream())
            nbytes = B * (K * H0 * W0 * 2 + H0 * W0)
            floor_us = nbytes / HBM_PEAK * 1e6
            row = dict(pairs=B * K, images=B, size=[H0, W0], T=T, nc=nc, path=CS.sweep_path(nc, K, T), input_bytes=nbytes,
                       floor_us=round(floor_us, 2), kernel=windows(fn, calls, reps))
            row["times_floor"] = round(row["kernel"]["us"] / floor_us, 2)
            row["input_bytes_per_s"] = round(nbytes / (row["kernel"]["us"] * 1e-6) / 1e12, 3)
            row["kernel_global_atomics"] = windows(lambda: fn(1), max(1, calls // 4), reps)
            assert int(flag.item()) == 0
            if B == 16:
                bins.zero_()
                fn()
                got = CS.confusion_from_bins(bins)
                stock = stock_sweep(cams, t, gt, THRESHOLDS, nc)
                assert torch.equal(got, stock), "the stock-op form and the kernel disagree"
                row["stock_tensor_ops"] = windows(lambda: stock_sweep(cams, t, gt, THRESHOLDS, nc), max(1, calls // 10), reps)
                row["stock_over_kernel"] = round(row["stock_tensor_ops"]["us"] / row["kernel"]["us"], 1)
                hc = cams.view(B, K, H0, W0).cpu().numpy()
                hg = gt.view(B, H0, W0).cpu().numpy()
                t0 = time.perf_counter()
                ref = R.sweep_confusion(list(hc), keys, list(hg), THRESHOLDS, nc)
                dt = time.perf_counter() - t0
                assert np.array_equal(ref, got.cpu().numpy()), "the numpy loop and the kernel disagree"
                row["numpy_loop"] = dict(us=round(dt * 1e6, 0), images_per_s=round(B / dt, 2), threads=torch.get_num_threads())
                row["numpy_over_kernel"] = round(dt * 1e6 / row["kernel"]["us"], 0)
            rows[f"sweep_nc{nc}_pairs{B * K}"] = row
    # the two label kernels on the 32-pair bucket
    cams, keys, gt = synthetic_bucket(16, 2, 21, 5)
    t = CS.PairTables(keys, 21, cams.device)
    low, high = CS.seed_labels(cams, None, 0.35, 0.55, tables=t)
    label = torch.empty(16, H0 * W0, device="cuda", dtype=torch.uint8)
    cmap = torch.empty(16, H0 * W0, 3, device="cuda", dtype=torch.uint8)
    hist, cover = torch.zeros(21, 21, device="cuda", dtype=torch.int64), torch.zeros(2, device="cuda", dtype=torch.int64)
    px = 16 * H0 * W0
    r = windows(lambda: CS.seed_labels(cams, None, 0.35, 0.55, tables=t), calls, reps)
    b = 32 * H0 * W0 * 2 + 2 * px * 8
    rows["labels_pairs32"] = dict(kernel=r, bytes=b, floor_us=round(b / HBM_PEAK * 1e6, 2), note="incl. the allocation of the two int64 maps")
    r = windows(lambda: CS.merge_labels(low, high, None, 21, gt=gt, label=label, cmap=cmap, hist=hist, cover=cover, tables=t), calls, reps)
    b = px * (16 + 1 + 1 + 3)
    rows["merge_pairs32"] = dict(kernel=r, bytes=b, floor_us=round(b / HBM_PEAK * 1e6, 2))
    return rows


def dumper_rows(n_images, n_crf, reps):
    from camgen_bench import THR, make_data
    model, _ = clip.load(synth.make_clip_state_dict(with_text=False), device="cuda")
    bg, fg = (t.cuda() for t in synth.make_text_features(20, 25, 512))
    imgs, labels = make_data(n_images)
    rng = np.random.default_rng(1)
    gts = []
    for im, ids in zip(imgs, labels):
        g = np.zeros(im.shape[:2], np.uint8)
        for k in ids:
            y, x = int(rng.integers(0, g.shape[0] - 100)), int(rng.integers(0, g.shape[1] - 100))
            g[y:y + 100, x:x + 100] = k + 1
        g[:2] = 255
        gts.append(g)
    dev_imgs = [im.cuda() for im in imgs]
    gen = G.CamGenerator(model, fg, bg, THR, max_bucket=16)

    def one_pass(n, make_ev):
        ev = make_ev() if make_ev else None
        for k in range(0, n, 16):
            sl = slice(k, min(k + 16, n))
            if ev is None:
                gen(dev_imgs[sl], labels[sl])
                continue
            payloads = gen(dev_imgs[sl], labels[sl], to_numpy=False)
            ev.add(payloads, dev_imgs[sl], gts[sl], [f"im{i}" for i in range(sl.start, sl.stop)])
            for p in payloads:                                   # the dumpers still save the maps
                p["attn_highres"].cpu().numpy()
        if ev is not None:
            ev.finish()
        torch.cuda.synchronize()

    def rate(n, make_ev):
        one_pass(n, make_ev)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            one_pass(n, make_ev)
            ts.append(time.perf_counter() - t0)
        return dict(images=n, images_per_s=round(n / statistics.median(ts), 2), s_all_reps=[round(t, 3) for t in ts])

    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        rows["as_today"] = rate(n_images, None)
        rows["eval_thresholds"] = rate(n_images, lambda: CS.SeedEvaluator(21, THRESHOLDS, masks=False))
        rows["pseudo_dir_refine_none"] = rate(n_images, lambda: CS.SeedEvaluator(21, THRESHOLDS, out_dir=os.path.join(tmp, "none")))
        for mode in ("exact", "lattice"):
            rows[f"pseudo_dir_refine_crf_{mode}"] = rate(
                n_crf, lambda: CS.SeedEvaluator(21, THRESHOLDS, refine="crf", crf_bilateral=mode, out_dir=os.path.join(tmp, mode)))
        rows["as_today_first_crf_images"] = rate(n_crf, None)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--crf-images", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--skip-dumper", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camseed_bench.json"))
    args = ap.parse_args()
    L.require_gpu()
    res = dict(box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, reps=args.reps, calls=args.calls,
               protocol="kernels: device events around `calls` back-to-back launches, 3 warm-up calls, median / min / max of `reps` windows; "
                        "dumper: host clock around a whole pass ending in a device synchronise, one warm-up pass, median of `reps`")
    res["kernels"] = sweep_rows(args.reps, args.calls)
    if not args.skip_dumper:
        res["dumper"] = dumper_rows(args.images, args.crf_images, max(2, args.reps - 2))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
