"""Fully supervised WeCLIP variant: one JSON line with
  * images/s of SupervisedTrainStep at B x 512 x 512, nc = 21 (ViT-B/16 synthetic weights), eager and graph replay;
  * ms of the variant's val forward against the VOC model's val forward (labels given, CAM/PAR chain) on the same weights;
  * us of wc_ce_loss_fwd_bwd (utils.losses.get_ce_loss_fused, forward + backward) against the torch composition
    F.cross_entropy(F.interpolate(seg, (H, W), bilinear), label, ignore_index=255) + backward.
Medians of CUDA-event timings after warm-up.  Not part of bench.py.

    python tools/seg_bench.py [--batch 16] [--size 512] [--steps 10] [--warmup 3]

--loss-only skips the model legs: one JSON line with us of forward + backward of get_seg_loss_fused and get_ce_loss_fused
at nc = 21 (VOC) and nc = 81 (COCO), B x nc x size/16 x size/16 logits against size x size labels.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def loss_only(B, S, steps, warmup):
    from weclip_vit_comer_amd.utils.losses import get_ce_loss_fused, get_seg_loss_fused
    out = {"batch": B, "size": S}
    for nc in (21, 81):
        g = torch.Generator().manual_seed(7)
        lab = torch.randint(0, nc, (B, S // 16, S // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)
        lab[:, :8] = 255
        lab = lab.cuda()
        seg = torch.randn(B, nc, S // 16, S // 16, generator=g).cuda().requires_grad_(True)
        for name, fn in (("seg", get_seg_loss_fused), ("ce", get_ce_loss_fused)):
            out[f"{name}_us_nc{nc}"] = round(_median_ms(lambda: fn(seg, lab, 255).backward(), 4 * steps, warmup) * 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loss-only", action="store_true")
    a = ap.parse_args()
    if a.loss_only:
        print(json.dumps(loss_only(a.batch, a.size, a.steps, a.warmup)), flush=True)
        return
    from oracle import synth
    from weclip_vit_comer_amd.train_step import SupervisedTrainStep
    from weclip_vit_comer_amd.utils.losses import get_ce_loss_fused
    from weclip_vit_comer_amd.WeCLIP_model import model_attn_aff_voc as VOC
    from weclip_vit_comer_amd.WeCLIP_model import model_attn_aff_voc_seg as SEG
    B, S, nc = a.batch, a.size, 21
    sd = synth.make_clip_state_dict(seed=0, with_text=False)
    fuse, dec = synth.make_head_state_dicts(width=768)
    bg, fg = synth.make_text_features(20, 25, 512)

    def build(cls, **kw):
        m = cls.WeCLIP(num_classes=nc, clip_model=sd, embedding_dim=256, in_channels=[768] * 4, device="cuda", **kw)
        m.decoder_fts_fuse.load_state_dict(fuse)
        m.decoder.load_state_dict(dec)
        return m

    img = synth.make_images(B, S, S, seed=100).cuda()
    g = torch.Generator().manual_seed(7)
    lab = torch.randint(0, nc, (B, S // 16, S // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)
    lab[:, :8] = 255
    lab = lab.cuda()
    out = {"batch": B, "size": S, "nc": nc}
    for graph in (False, True):
        m = build(SEG).train()
        step = SupervisedTrainStep(m, graph=graph)
        ms = _median_ms(lambda: step(img, lab), a.steps, a.warmup)
        out["step_ms_graph" if graph else "step_ms_eager"] = round(ms, 3)
        out["images_per_s_graph" if graph else "images_per_s_eager"] = round(B / ms * 1e3, 1)
        del m, step
    seg_m = build(SEG).eval()
    voc_m = build(VOC, text_features=(bg.cuda(), fg.cuda())).eval()
    labels = synth.make_label_lists(B, 2, seed=7)
    with torch.no_grad():
        out["val_forward_ms_seg"] = round(_median_ms(lambda: seg_m(img, mode="val"), a.steps, a.warmup), 3)
        out["val_forward_ms_voc"] = round(_median_ms(lambda: voc_m(img, [""] * B, mode="val", labels=labels), a.steps, a.warmup), 3)
    del seg_m, voc_m
    seg = torch.randn(B, nc, S // 16, S // 16, device="cuda", requires_grad=True)

    def fused():
        get_ce_loss_fused(seg, lab, 255).backward()

    def composed():
        F.cross_entropy(F.interpolate(seg, size=(S, S), mode="bilinear", align_corners=False), lab, ignore_index=255).backward()

    out["ce_us_fused"] = round(_median_ms(fused, 4 * a.steps, a.warmup) * 1e3, 1)
    out["ce_us_torch"] = round(_median_ms(composed, 4 * a.steps, a.warmup) * 1e3, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
