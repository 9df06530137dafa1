"""Throughput of the stand-alone CAM generation on one GPU, HIP-event timed.

    python tools/camgen_bench.py [--images 64] [--reps 3] [--out profiles/camgen_bench.json]

64 synthetic VOC-shaped uint8 images (sizes drawn from 500x375, 375x500, 500x333, 333x500), 2 labels each, ViT-B/16 with
synthetic weights.  Rows, images/s each (median of --reps passes over all images after one warm-up pass):
  yardstick        the reference-shaped loop written with the public API that existed before CamGenerator: one image and one
                   class at a time -- preprocessing on the host by Pillow, `encode_image`, `GradCAM.__call__` (map returned
                   to the host), head-mean of the last 8 maps, `compute_trans_mat`, box mask on the host (oracle.box_mask),
                   mask / matmul, min-max + bilinear resize + float16 on the host.  Needs Pillow; recorded as null without it.
  camgen_bucket_N  CamGenerator with at most N images per bucket (N = 1, 4, 16), images already on the device, payload copied
                   to the host as the drivers do.
  wc_clip_preprocess / wc_cam_scale_resize_f16 alone: microseconds per launch, bytes moved, fraction of the HBM peak (8 TB/s).
"""
import argparse
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import weclip_vit_comer_amd  # noqa: E402,F401
from oracle import synth  # noqa: E402
from oracle import weclip_oracle as O  # noqa: E402
from weclip_vit_comer_amd import clip  # noqa: E402
from weclip_vit_comer_amd.clip import generate_cams as G  # noqa: E402
from weclip_vit_comer_amd.clip.clip_tool import ClipOutputTarget, compute_trans_mat  # noqa: E402
from weclip_vit_comer_amd.pytorch_grad_cam import GradCAM  # noqa: E402

SIZES = [(375, 500), (500, 375), (333, 500), (500, 333)]
HBM_PEAK = 8.0e12
THR = 0.4


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def make_data(n):
    rng = np.random.default_rng(0)
    imgs, labels = [], []
    for i in range(n):
        h, w = SIZES[int(rng.integers(0, 4))]
        base = rng.integers(0, 256, (h // 25 + 1, w // 25 + 1, 3)).repeat(25, 0).repeat(25, 1)[:h, :w]
        imgs.append(torch.from_numpy(np.clip(base + rng.integers(-15, 16, (h, w, 3)), 0, 255).astype(np.uint8)))
        labels.append([int(v) for v in rng.choice(20, 2, replace=False)])
    return imgs, labels


def yardstick_pass(model, cam, bg, fg, imgs, labels):
    from PIL import Image
    mean, std = torch.tensor(G.CLIP_MEAN)[:, None, None], torch.tensor(G.CLIP_STD)[:, None, None]
    for im, ids in zip(imgs, labels):
        H0, W0 = im.shape[:2]
        h, w = G.target_size(H0, W0)
        pil = Image.fromarray(im.numpy()).resize((w, h), Image.BICUBIC)
        x = torch.from_numpy(np.asarray(pil).copy()).permute(2, 0, 1).float().div(255).sub_(mean).div_(std)[None].cuda()
        feats, maps = model.encode_image(x, h, w)
        text = torch.cat([fg[ids], bg], 0)
        out = []
        for k in range(len(ids)):
            g, _, last = cam(input_tensor=[feats, text, h, w], targets=[ClipOutputTarget(k)], target_size=None)
            if k == 0:
                aff = torch.stack([m[:, 1:, 1:] for m in list(maps) + [last]], 0)[-8:].mean(0)[0]
                trans = compute_trans_mat(aff)
            mask = torch.from_numpy(np.asarray(O.box_mask(g[0], THR), np.float32)).reshape(1, -1).cuda()
            refined = ((trans * mask) @ torch.from_numpy(g[0]).reshape(-1, 1).cuda()).reshape(h // 16, w // 16).cpu()
            refined = refined - refined.min()
            refined = refined / (1e-7 + refined.max())
            out.append(F.interpolate(refined[None, None], size=(H0, W0), mode="bilinear", align_corners=False)[0, 0].numpy()
                       .astype(np.float16))
        np.stack(out)


def kernel_rows(reps):
    rows = {}
    B, H0, W0 = 16, 375, 500
    src = torch.randint(0, 256, (B, H0, W0, 3), dtype=torch.uint8, device="cuda")
    pre = G.ClipPreprocess()
    h, w = G.target_size(H0, W0)
    t = statistics.median(timed(lambda: pre(src), reps, 3))
    nbytes = B * (H0 * W0 * 3 + 2 * H0 * w * 3 + h * w * 3 * 4)
    rows["wc_clip_preprocess"] = dict(batch=B, src=[H0, W0], dst=[h, w], us=round(t * 1e3, 1), bytes=nbytes,
                                      hbm_fraction=round(nbytes / (t * 1e-3) / HBM_PEAK, 4),
                                      note="three launches (tables, horizontal, vertical pass) incl. the output allocation")
    P, gh, gw = 32, h // 16, w // 16
    cams = torch.rand(P, gh * gw, device="cuda")
    t = statistics.median(timed(lambda: G.scale_cam_f16(cams, gh, gw, [(H0, W0)] * P, flat=True), reps, 3))
    nbytes = P * (gh * gw * 4 + H0 * W0 * 2)
    rows["wc_cam_scale_resize_f16"] = dict(pairs=P, grid=[gh, gw], dst=[H0, W0], us=round(t * 1e3, 1), bytes=nbytes,
                                           hbm_fraction=round(nbytes / (t * 1e-3) / HBM_PEAK, 4),
                                           note="one launch incl. the size / offset table upload and the output allocation")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camgen_bench.json"))
    args = ap.parse_args()
    model, _ = clip.load(synth.make_clip_state_dict(with_text=False), device="cuda")
    bg, fg = (t.cuda() for t in synth.make_text_features(20, 25, 512))
    imgs, labels = make_data(args.images)
    res = dict(box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), images=args.images, labels_per_image=2, reps=args.reps,
               protocol="HIP events around a whole pass over all images, one warm-up pass, median of reps", rows={})
    try:
        import PIL  # noqa: F401
        cam = GradCAM(model=model, target_layers=[model.visual.transformer.resblocks[-1].ln_1])
        ts = timed(lambda: yardstick_pass(model, cam, bg, fg, imgs, labels), args.reps)
        res["rows"]["yardstick"] = dict(images_per_s=round(args.images / (statistics.median(ts) * 1e-3), 2), ms_all_reps=[round(t, 1) for t in ts])
    except ImportError:
        res["rows"]["yardstick"] = dict(images_per_s=None, note="Pillow is not installed on this box")
    dev_imgs = [im.cuda() for im in imgs]
    for nb in (1, 4, 16):
        gen = G.CamGenerator(model, fg, bg, THR, max_bucket=nb)
        ts = timed(lambda: gen(dev_imgs, labels), args.reps)
        res["rows"][f"camgen_bucket_{nb}"] = dict(images_per_s=round(args.images / (statistics.median(ts) * 1e-3), 2),
                                                  ms_all_reps=[round(t, 1) for t in ts])
    res["kernels"] = kernel_rows(20)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
