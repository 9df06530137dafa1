"""HIP-event time of one dense CRF call (utils.dcrf.DenseCRF), split into the bilateral passes and the rest.

    python tools/dcrf_bench.py [--reps 5] [--out profiles/dcrf_bench.json]

Cases: 500x375, C = 21 with crf_proc's parameters (iter_max 10, pos 3 / w 3, bilateral 64 / 5 / w 4), and 640x480, C = 81.
A call runs 11 bilateral passes (S, then one per iteration).  `total_ms`: events around the whole call (median of --reps,
after a warm-up call); `bilateral_ms`: the library's per-launch event pairs on dcrf_bil_kernel (a separate timed call, the
pairs fence each launch); `rest_ms` = total - bilateral.  Random uint8 image of smooth regions plus noise, random
probabilities."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import weclip_vit_comer_amd  # noqa: E402,F401
from weclip_vit_comer_amd.ops import KernelTimer  # noqa: E402
from weclip_vit_comer_amd.utils import dcrf  # noqa: E402

CASES = [dict(H=375, W=500, C=21), dict(H=480, W=640, C=81)]
PARAMS = dict(iter_max=10, pos_w=3, pos_xy_std=3, bi_w=4, bi_xy_std=64, bi_rgb_std=5)


def run_case(H, W, C, reps):
    g = torch.Generator().manual_seed(0)
    base = torch.rand(3, 6, 8, generator=g) * 255
    img = (F.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
           + 8 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8).cuda()
    P = torch.softmax(2 * torch.randn(C, H, W, generator=g), 0).cuda()
    crf = dcrf.DenseCRF(**PARAMS)
    crf(img, P)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        crf(img, P)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    KernelTimer.enable(1)
    crf(img, P)
    rec = KernelTimer.summary().get("dcrf_bil_kernel", {})
    KernelTimer.enable(0)
    total = statistics.median(times)
    bil = rec.get("ms", float("nan"))
    n = H * W
    cp = 32 * ((C + 31) // 32)
    return dict(H=H, W=W, C=C, CP=cp, total_ms=round(total, 3), bilateral_ms=round(bil, 3), rest_ms=round(total - bil, 3),
                bilateral_passes=rec.get("launches", 0), ms_per_bilateral_pass=round(bil / max(1, rec.get("launches", 1)), 3),
                pairs_per_pass=n * n, total_ms_all_reps=[round(t, 3) for t in times], params=PARAMS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = [run_case(**c, reps=a.reps) for c in CASES]
    res = dict(device=torch.cuda.get_device_name(0), cases=res)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
