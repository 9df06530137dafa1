"""What does the evaluation entry point cost per image, next to the way the parent commit offers?  One process, a synthetic
tree of 500x375 JPEGs written with Pillow, the ViT-B/16 supervised VOC variant (21 classes: `MscFlipEvaluator.add` runs it
without label files, and the CRF is the 21-class one), scales 1 and 0.75, long side 512:

  (n0) msc_flip_eval.SplitEvaluator, no files            (p0) MscFlipEvaluator.add
  (n1) SplitEvaluator writing prediction/ + _cmap/       (p1) add, .cpu() of both maps, serial Pillow save of the msc map and table[map]
  (n2) SplitEvaluator with the CRF leg and files         (p2) add_with_crf, .cpu() of the maps, serial Pillow save of the CRF map
  (n3) n2 with DenseCRF(..., bilateral="lattice"): the CRF leg's bilateral message on the permutohedral lattice
  (v)  SplitEvaluator on the VOC model with its CAM leg and files (the parent cannot evaluate a VOC model built without
       dataset_root_path: no counterpart)

Images per second = images / wall clock around a whole pass over the loader, ending in `finish()` (which drains the writers) or a
device synchronise; the first pass of every row warms it up and is dropped; rows alternate pass by pass in one process.  Then
the launch itself, HIP events around --calls calls: `wc_eval_finish` (both maps, colour image, three histograms) against the
launches it replaces (2 x wc_resize_argmax + 3 x wc_confusion_hist, int64 maps), at (21, 24, 32) -> (375, 500) and at 81 classes.

    python tools/eval_bench.py [--json profiles/eval_bench.json]

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
    return {key: round(statistics.median(vals), 3), "min": round(min(vals), 3), "max": round(max(vals), 3)}


def write_tree(root, n):
    from PIL import Image
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "SegmentationClassAug"))
    rs = np.random.RandomState(0)
    names, onehot = [], {}
    yy, xx = np.mgrid[0:375, 0:500]
    for i in range(n):
        img = np.stack([127 + 90 * np.sin(xx / (9.0 + 3 * c) + i) * np.cos(yy / (11.0 + c)) for c in range(3)], -1)
        img = np.clip(img + rs.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)
        name = f"2007_{i:06d}"
        Image.fromarray(img).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=90)
        ids = sorted(rs.choice(20, size=2, replace=False).tolist())
        lab = np.zeros((375, 500), np.uint8)
        lab[75:187, 83:250] = ids[0] + 1
        lab[187:, 250:] = ids[1] + 1
        lab[:, :3] = 255
        Image.fromarray(lab).save(os.path.join(root, "SegmentationClassAug", name + ".png"))
        v = np.zeros(20, np.float32)
        v[ids] = 1
        names.append(name)
        onehot[name] = v
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    np.save(os.path.join(root, "cls_labels_onehot.npy"), onehot)
    return root


def make_models(torch):
    from weclip_vit_comer_amd import synth
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP as Voc
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc_seg import WeCLIP as Seg
    sd = synth.make_clip_state_dict(seed=0, with_text=False)
    bg, fg = synth.make_text_features(20, 25, 512)
    fuse, dec = synth.make_head_state_dicts()
    out = []
    for cls, extra in ((Seg, {}), (Voc, {"dataset_root_path": None})):
        m = cls(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[768] * 4, device="cuda",
                text_features=(bg.cuda(), fg.cuda()), **extra)
        m.decoder_fts_fuse.load_state_dict(fuse)
        m.decoder.load_state_dict(dec)
        out.append(m.eval())
    return out


def parent_pass(torch, model, loader, out_dir, crf, table):
    """The parent commit's way: add / add_with_crf, the maps to the host, one Pillow save after the other."""
    from PIL import Image
    from weclip_vit_comer_amd import msc_flip_eval as E
    from weclip_vit_comer_amd.msc_flip import MscFlipEvaluator
    ev = MscFlipEvaluator(model, 21, scales=(1.0, 0.75), resize_long=512, crf=crf)
    if out_dir:
        for k in ("prediction", "prediction_cmap"):
            os.makedirs(os.path.join(out_dir, k), exist_ok=True)
    for names, inputs, labels, _ in loader:
        if crf is not None:
            maps = ev.add_with_crf(inputs, labels, E.image_of(inputs))
        else:
            maps = ev.add(inputs, labels)
        if out_dir:
            host = [m.cpu().numpy() for m in maps]
            pred = host[-1].astype(np.uint8)
            Image.fromarray(pred, mode="L").save(os.path.join(out_dir, "prediction", names[0] + ".png"))
            Image.fromarray(table[pred], mode="RGB").save(os.path.join(out_dir, "prediction_cmap", names[0] + ".png"))
    torch.cuda.synchronize()
    return ev.msc_hist


def new_pass(torch, model, loader, out_dir, crf, writers):
    from weclip_vit_comer_amd import msc_flip_eval as E
    ev = E.SplitEvaluator(model, 21, scales=(1.0, 0.75), resize_long=512, crf=crf, out_dir=out_dir, writers=writers)
    ev.run(loader)
    return ev.msc_hist


def launch_times(torch, C, nc, calls, repeats):
    """ms per image of the tail: one wc_eval_finish against 2 x wc_resize_argmax + 3 x wc_confusion_hist."""
    from weclip_vit_comer_amd import msc_flip_eval as E
    from weclip_vit_comer_amd.msc_flip import resize_argmax
    from weclip_vit_comer_amd.utils import evaluate
    g = torch.Generator().manual_seed(0)
    seg1, msc = torch.randn(C, 24, 32, generator=g).cuda(), torch.randn(C, 24, 32, generator=g).cuda()
    gt, cam = torch.randint(0, nc, (375, 500), generator=g).cuda(), torch.randint(0, nc, (375, 500), generator=g).cuda()
    u8, rgb = torch.empty(375, 500, dtype=torch.uint8, device="cuda"), torch.empty(375, 500, 3, dtype=torch.uint8, device="cuda")
    h = [torch.zeros(nc, nc, dtype=torch.int64, device="cuda") for _ in range(6)]

    def fused():
        E.eval_finish(seg1, msc, (375, 500), nc, cam=cam, gt=gt, predm_u8=u8, cmap_rgb=rgb, hist=h[0], msc_hist=h[1], cam_hist=h[2])

    def parent():
        a, b = resize_argmax(seg1, (375, 500)), resize_argmax(msc, (375, 500))
        evaluate.confusion_hist(gt, a, nc, out=h[3])
        evaluate.confusion_hist(gt, b, nc, out=h[4])
        evaluate.confusion_hist(gt, cam, nc, out=h[5])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls
    for fn in (fused, parent):
        for _ in range(20):
            fn()
    tf, tp = [], []
    for _ in range(repeats):
        tf.append(timed(fused))
        tp.append(timed(parent))
    assert all(torch.equal(h[i], h[i + 3]) for i in range(3)), "fused and separate launches disagree"
    return {"C": C, "nc": nc, "grid": [24, 32], "label": [375, 500], "eval_finish_ms": stats(tf, "ms"),
            "replaced_launches_ms": stats(tp, "ms"), "ratio_fused_over_replaced": round(statistics.median(tf) / statistics.median(tp), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--crf-images", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12SegDataset
    from weclip_vit_comer_amd.utils.dcrf import DenseCRF
    from weclip_vit_comer_amd import msc_flip_eval as E
    assert torch.cuda.is_available(), "eval_bench needs the GPU"
    table = np.load(os.path.join(ROOT, "tests", "golden", "voc_cmap.npz"))["cmap"]
    seg_model, voc_model = make_models(torch)
    crf = DenseCRF(**E.CRF_PARAMS)
    crf_lattice = DenseCRF(**E.CRF_PARAMS, bilateral="lattice")
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        tree = write_tree(os.path.join(tmp, "tree"), args.images)
        ds = VOC12SegDataset(root_dir=tree, name_list_dir=tree, split="val", stage="val", aug=False)

        with open(os.path.join(tree, "val_few.txt"), "w") as f:    # the first images of the split: the CRF rows
            f.write("\n".join(open(os.path.join(tree, "val.txt")).read().split()[:args.crf_images]) + "\n")
        few = VOC12SegDataset(root_dir=tree, name_list_dir=tree, split="val_few", stage="val", aug=False)
        plan = [("n0", lambda d: new_pass(torch, seg_model, d, None, None, args.writers), ds),
                ("p0", lambda d: parent_pass(torch, seg_model, d, None, None, table), ds),
                ("n1", lambda d: new_pass(torch, seg_model, d, os.path.join(tmp, "n1"), None, args.writers), ds),
                ("p1", lambda d: parent_pass(torch, seg_model, d, os.path.join(tmp, "p1"), None, table), ds),
                ("n2", lambda d: new_pass(torch, seg_model, d, os.path.join(tmp, "n2"), crf, args.writers), few),
                ("p2", lambda d: parent_pass(torch, seg_model, d, os.path.join(tmp, "p2"), crf, table), few),
                ("n3", lambda d: new_pass(torch, seg_model, d, os.path.join(tmp, "n3"), crf_lattice, args.writers), few),
                ("v", lambda d: new_pass(torch, voc_model, d, os.path.join(tmp, "v"), None, args.writers), ds)]
        rates = {k: [] for k, _, _ in plan}
        hists = {}
        for r in range(args.repeats + 1):
            for key, fn, data in plan:
                loader = DeviceLoader(data, 1, shuffle=False, threads=8, prefetch=2)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hists[key] = fn(loader)
                dt = time.perf_counter() - t0
                if r:                                                # the first round warms every row up
                    rates[key].append(len(data) / dt)
        same = bool(torch.equal(hists["n1"], hists["p1"]) and torch.equal(hists["n0"], hists["p0"]) and torch.equal(hists["n2"], hists["p2"]))
        files_equal = all(open(os.path.join(tmp, a, k, f), "rb").read() == open(os.path.join(tmp, b, k, f), "rb").read()
                          for a, b in (("n1", "p1"), ("n2", "p2")) for k in ("prediction", "prediction_cmap")
                          for f in sorted(os.listdir(os.path.join(tmp, b, k))))
        rows = {k: stats(v, "images_per_s") for k, v in rates.items()}
    launches = [launch_times(torch, 21, 21, args.calls, args.repeats + 2), launch_times(torch, 81, 81, args.calls, args.repeats + 2)]
    res = {"device": torch.cuda.get_device_name(0), "image_size": [375, 500], "images": args.images, "crf_images": args.crf_images,
           "repeats": args.repeats, "writers": args.writers, "scales": [1.0, 0.75], "resize_long": 512, "model": "ViT-B/16, 21 classes",
           "n0_split_evaluator_no_files": rows["n0"], "p0_parent_add": rows["p0"],
           "n1_split_evaluator_files": rows["n1"], "p1_parent_add_cpu_serial_save": rows["p1"],
           "n2_split_evaluator_crf_files": rows["n2"], "p2_parent_add_with_crf_cpu_serial_save": rows["p2"],
           "n3_split_evaluator_crf_lattice_files": rows["n3"],
           "ratio_n3_over_n2": round(rows["n3"]["images_per_s"] / rows["n2"]["images_per_s"], 3),
           "v_split_evaluator_voc_cam_leg_files": rows["v"],
           "ratio_n0_over_p0": round(rows["n0"]["images_per_s"] / rows["p0"]["images_per_s"], 3),
           "ratio_n1_over_p1": round(rows["n1"]["images_per_s"] / rows["p1"]["images_per_s"], 3),
           "ratio_n2_over_p2": round(rows["n2"]["images_per_s"] / rows["p2"]["images_per_s"], 3),
           "p0_pass_spread": round((rows["p0"]["max"] - rows["p0"]["min"]) / rows["p0"]["images_per_s"], 3),
           "histograms_equal_new_vs_parent": same, "png_files_byte_equal_new_vs_parent": files_equal,
           "tail_launch": launches,
           "how": "python tools/eval_bench.py (wall clock around whole passes over a DeviceLoader, each ending in finish() / a device "
                  "synchronise; first pass of every row dropped; rows alternate pass by pass in one process; median of `repeats` passes; "
                  "tail_launch: HIP events around `calls` calls, fused and replaced alternating)"}
    print(json.dumps(res, indent=1, allow_nan=False))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1, allow_nan=False)
            f.write("\n")


if __name__ == "__main__":
    main()
