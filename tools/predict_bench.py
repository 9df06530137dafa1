"""What does the predict entry point cost per image?  One process, 32 synthetic 500x375 JPEGs written with Pillow, the ViT-B/16
supervised VOC variant (21 classes), scales 1 and 0.75, long side 512, 8 decode threads, 4 writers:

  (p0) predict.Predictor, no files                          (e1) msc_flip_eval.SplitEvaluator writing prediction/ + prediction_cmap/
  (p1) Predictor writing prediction/ + prediction_cmap/           on the same images with label maps: the parent commit's nearest row
  (p2) Predictor writing all four kinds
  (p3) p1 with DenseCRF(..., bilateral="lattice") on the first --crf-images images

Images per second = images / wall clock around a whole pass over a DeviceLoader, ending in `finish()` (which drains the writers);
the first pass of every row warms it up and is dropped; rows alternate pass by pass.  Then the launch itself, HIP events around
--calls calls, alternating: `wc_predict_finish` with all four maps and the statistics against the parent commit's nearest job,
`wc_eval_finish` with gt = NULL, predm_u8 and cmap_rgb, at (21, 24, 32) -> (375, 500) and (81, 30, 40) -> (480, 640), and
against the time the new kernel's own bytes (logits and image in, four maps out) take at the HBM peak of 8 TB/s.

    python tools/predict_bench.py [--json profiles/predict_bench.json]

Needs the GPU; there is no fall-back."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12                                             # bytes / s, the MI355X's specified peak


def stats(vals, key, digits=3):
    return {key: round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def launch_times(torch, C, src_hw, out_hw, calls, repeats):
    """ms per image of the tail: wc_predict_finish (everything) against wc_eval_finish (uint8 map + colour image, two arg-maxes)."""
    from weclip_vit_comer_amd import msc_flip_eval as E
    from weclip_vit_comer_amd import predict as P
    g = torch.Generator().manual_seed(0)
    H, W = out_hw
    seg1, msc = torch.randn(C, *src_hw, generator=g).cuda(), torch.randn(C, *src_hw, generator=g).cuda()
    image = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")      # noqa: E731
    new = dict(pred_u8=u8(H, W), cmap_rgb=u8(H, W, 3), conf_u8=u8(H, W), overlay_rgb=u8(H, W, 3),
               stats=torch.zeros(2 * C + 1, dtype=torch.int64, device="cuda"))
    old_u8, old_rgb = u8(H, W), u8(H, W, 3)

    def predict():
        P.predict_finish(msc, out_hw, image=image, mode=0, alpha256=128, ignore_below=0, **new)

    def evaluate():
        E.eval_finish(seg1, msc, out_hw, C, predm_u8=old_u8, cmap_rgb=old_rgb)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls
    for fn in (predict, evaluate):
        for _ in range(20):
            fn()
    tn, to = [], []
    for _ in range(repeats):
        tn.append(timed(predict))
        to.append(timed(evaluate))
    assert torch.equal(new["pred_u8"], old_u8) and torch.equal(new["cmap_rgb"], old_rgb), "the two kernels' maps disagree"
    nbytes = 4 * C * src_hw[0] * src_hw[1] + 3 * H * W + 8 * H * W           # logits + image in; 1 + 3 + 1 + 3 bytes per pixel out
    floor_ms = nbytes / HBM_PEAK * 1e3
    return {"C": C, "grid": list(src_hw), "out": list(out_hw), "predict_finish_ms": stats(tn, "ms", 4),
            "eval_finish_gt_null_ms": stats(to, "ms", 4), "ratio_predict_over_eval": round(statistics.median(tn) / statistics.median(to), 3),
            "bytes": nbytes, "hbm_floor_ms_at_8TBs": round(floor_ms, 5),
            "share_of_hbm_peak": round(floor_ms / statistics.median(tn), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--crf-images", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from eval_bench import make_models, write_tree
    from weclip_vit_comer_amd import msc_flip_eval as E
    from weclip_vit_comer_amd import predict as P
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.folder import ImageFolderDataset
    from weclip_vit_comer_amd.datasets.voc import VOC12SegDataset
    from weclip_vit_comer_amd.utils.dcrf import DenseCRF
    assert torch.cuda.is_available(), "predict_bench needs the GPU"
    model, _ = make_models(torch)
    lattice = DenseCRF(**E.CRF_PARAMS, bilateral="lattice")
    with tempfile.TemporaryDirectory() as tmp:
        tree = write_tree(os.path.join(tmp, "tree"), args.images)
        folder = ImageFolderDataset(os.path.join(tree, "JPEGImages"))
        few_list = os.path.join(tmp, "few.txt")
        with open(few_list, "w") as f:
            f.write("\n".join(folder.paths[:args.crf_images]) + "\n")
        few = ImageFolderDataset(few_list)
        labelled = VOC12SegDataset(root_dir=tree, name_list_dir=tree, split="val", stage="val", aug=False)

        def predictor(out, outputs, crf=None):
            return lambda data: P.Predictor(model, 21, scales=(1.0, 0.75), resize_long=512, crf=crf, out_dir=out and os.path.join(tmp, out),
                                            outputs=outputs, writers=args.writers).run(data)

        def evaluator(data):
            return E.SplitEvaluator(model, 21, scales=(1.0, 0.75), resize_long=512, out_dir=os.path.join(tmp, "e1"),
                                    writers=args.writers).run(data)
        plan = [("p0", predictor(None, ()), folder), ("p1", predictor("p1", P.KINDS[:2]), folder), ("e1", evaluator, labelled),
                ("p2", predictor("p2", P.KINDS), folder), ("p3", predictor("p3", P.KINDS[:2], lattice), few)]
        rates = {k: [] for k, _, _ in plan}
        for r in range(args.repeats + 1):
            for key, fn, data in plan:
                loader = DeviceLoader(data, 1, shuffle=False, threads=8, prefetch=2)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(loader)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(f"pass {r} {key}: {len(data) / dt:.1f} images/s", file=sys.stderr, flush=True)
                if r:                                                # the first round warms every row up
                    rates[key].append(len(data) / dt)
        files_equal = all(open(os.path.join(tmp, "p1", k, f), "rb").read() == open(os.path.join(tmp, "e1", k, f), "rb").read()
                          for k in ("prediction", "prediction_cmap") for f in sorted(os.listdir(os.path.join(tmp, "e1", k))))
        rows = {k: stats(v, "images_per_s") for k, v in rates.items()}
    launches = [launch_times(torch, 21, (24, 32), (375, 500), args.calls, args.repeats + 2),
                launch_times(torch, 81, (30, 40), (480, 640), args.calls, args.repeats + 2)]
    spread = lambda k: round((rows[k]["max"] - rows[k]["min"]) / rows[k]["images_per_s"], 3)      # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "image_size": [375, 500], "images": args.images, "crf_images": args.crf_images,
           "repeats": args.repeats, "writers": args.writers, "scales": [1.0, 0.75], "resize_long": 512, "model": "ViT-B/16, 21 classes",
           "p0_predictor_no_files": rows["p0"], "p1_predictor_prediction_cmap": rows["p1"], "p2_predictor_all_four": rows["p2"],
           "e1_split_evaluator_prediction_cmap": rows["e1"], "p3_predictor_crf_lattice_prediction_cmap": rows["p3"],
           "ratio_p1_over_e1": round(rows["p1"]["images_per_s"] / rows["e1"]["images_per_s"], 3),
           "p1_pass_spread": spread("p1"), "e1_pass_spread": spread("e1"),
           "png_files_byte_equal_p1_vs_e1": files_equal, "tail_launch": launches,
           "how": "python tools/predict_bench.py (wall clock around whole passes over a DeviceLoader, each ending in finish() and a "
                  "device synchronise; first pass of every row dropped; rows alternate pass by pass in one process; median of "
                  "`repeats` passes; tail_launch: HIP events around `calls` calls, the two kernels alternating)"}
    print(json.dumps(res, indent=1, allow_nan=False))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1, allow_nan=False)
            f.write("\n")


if __name__ == "__main__":
    main()
