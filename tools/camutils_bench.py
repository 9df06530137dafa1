"""HIP-event time of the AFA pseudo-label chain (utils.camutils; the lineage's dist_train_voc lines :310-339) and of its random
walk alone, against the same chain written with stock torch ops on the same card.

    python tools/camutils_bench.py [--windows 5] [--out profiles/camutils_bench.json] [--small-only]

Sizes: B = 4, 320 x 320, C = 20 with n = 400 and n = 900 tokens (the reference's default and its 1.5x inference grid), and B = 16,
512 x 512, n = 1024 with C = 20 and C = 80; every image has 1-5 classes present.
Method: one process; a warm-up call of both sides, then --windows windows of each, alternating (ours,
stock, ours, ...); a window is `iters` calls between two events; reported: median (min .. max) of the windows' ms per call.
The stock side is tests/camutils_ref.py run in f32 on the device with this package's PAR as `ref_mod`: the reference's
structure (per-image loops, `nonzero` per image, 4 B refinement calls, four (B, n, n) temporaries in the walk); the parent
commit has no implementation to compare with.  `walk_kernel_ms`: the library's own event pair around aff_walk_kernel, and
`walk_TBps` the bytes of `aff` over it, against the 6.29 TB/s this card's copy kernel measures."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import camutils_cases as K  # noqa: E402
import camutils_ref as R  # noqa: E402
import weclip_vit_comer_amd  # noqa: E402,F401
from weclip_vit_comer_amd.ops import KernelTimer  # noqa: E402
from weclip_vit_comer_amd.resize import bilinear_resize  # noqa: E402
from weclip_vit_comer_amd.utils import camutils as M  # noqa: E402
from weclip_vit_comer_amd.WeCLIP_model.PAR import PAR  # noqa: E402

COPY_TBPS = 6.29
CASES = [dict(B=4, S=320, C=20, grid=(20, 20), iters=(20, 3)), dict(B=4, S=320, C=20, grid=(30, 30), iters=(20, 3)),
         dict(B=16, S=512, C=20, grid=(32, 32), iters=(5, 1)), dict(B=16, S=512, C=80, grid=(32, 32), iters=(5, 1))]


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def run_case(B, S, C, grid, iters, windows):
    import numpy as np
    n = grid[0] * grid[1]
    img = torch.from_numpy(30.0 + 170.0 * K.smooth((B, 3), S, S, 1, cell=32) + 25.0 * K.noise((B, 3, S, S), 2)).float().cuda()
    cams = torch.from_numpy(K.smooth((B, C), S, S, 3, cell=40)).float().cuda()
    cls = torch.zeros(B, C)
    for b in range(B):
        cls[b, [(7 * b + 3 * j) % C for j in range(1 + b % 5)]] = 1
    cls = cls.cuda()
    aff = torch.sigmoid(torch.from_numpy(8.0 * K.noise((B, n, n), 4) - 4.0).float()).cuda()
    box = [[0, S, 0, S] for _ in range(B)]
    box[1] = [S // 16, S - S // 8, S // 10, S - S // 16]
    c = dict(images=img, cams=cams, cls=cls, aff=aff, box=box, cfg=K.make_cfg())
    par = PAR(K.DILATIONS, K.NUM_ITER).cuda()
    mask = M.get_mask_by_radius(*grid, radius=8).cuda()
    amask = M.get_mask_by_radius(S // 16, S // 16, radius=8).cuda()
    resized = bilinear_resize(cams * cls[:, :, None, None], grid)
    stock_resize = lambda x, size: F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)
    sides = {
        "walk": (lambda: M.propagte_aff_cam_with_bkg(resized, aff=aff, mask=mask, cls_labels=cls, bkg_score=K.THRE[0]),
                 lambda: R.propagte_aff_cam_with_bkg(resized, aff=aff, mask=mask, cls_labels=cls, bkg_score=K.THRE[0])),
        "chain": (lambda: K.run_chain(M, par, c, mask, amask, bilinear_resize, M.cams_to_affinity_label, grid=grid),
                  lambda: K.run_chain(R, par, c, mask, amask, stock_resize, M.cams_to_affinity_label, grid=grid)),
    }
    res = dict(B=B, H=S, W=S, C=C, n=n, classes_present=[int(v) for v in cls.sum(1).tolist()], windows=windows,
               iters_per_window=list(iters))
    for name, (ours, stock) in sides.items():
        a, b = ours(), stock()
        torch.cuda.synchronize()
        if name == "walk":
            res["walk_ours_vs_stock_rel_of_max"] = ((a - b).abs().max() / b.abs().max()).item()
        else:
            res["chain_labels_differ"] = {k: float((a[k] != b[k]).float().mean().item()) for k in a}
        to, ts = [], []
        for _ in range(windows):
            to.append(window(ours, iters[0] * (10 if name == "walk" else 1)))
            ts.append(window(stock, iters[1] * (10 if name == "walk" else 1)))
        res[name] = dict(ours=stats(to), stock_torch=stats(ts), ours_all_ms=[round(t, 4) for t in to],
                         stock_all_ms=[round(t, 4) for t in ts], speedup=round(statistics.median(ts) / statistics.median(to), 2))
    KernelTimer.enable(1)
    for _ in range(5):
        sides["walk"][0]()
    rec = KernelTimer.summary().get("aff_walk_kernel", {})
    KernelTimer.enable(0)
    ms = rec["ms"] / max(rec["launches"], 1) if rec else float("nan")
    res["walk_kernel"] = dict(raw=rec, aff_bytes=4 * B * n * n, grid=[-(-n // 32), B], workgroup=256)
    res["walk_kernel_ms"] = round(ms, 4)
    res["walk_TBps"] = round(4 * B * n * n / (ms * 1e-3) / 1e12, 3) if ms == ms and ms > 0 else None
    res["walk_vs_one_read"] = round(COPY_TBPS / res["walk_TBps"], 2) if res["walk_TBps"] else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("camutils_bench: needs the GPU; there is nothing to time without one")
    res = [run_case(**c, windows=a.windows) for c in (CASES[:2] if a.small_only else CASES)]
    res = dict(device=torch.cuda.get_device_name(0), copy_ceiling_TBps=COPY_TBPS, cases=res)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
