"""HIP-event time of one dense CRF call (utils.dcrf.DenseCRF), split into the bilateral passes and the rest.

    python tools/dcrf_bench.py [--reps 5] [--out profiles/dcrf_lattice_bench.json]

Cases: 500x375, C = 21 with crf_proc's parameters (iter_max 10, pos 3 / w 3, bilateral 64 / 5 / w 4), and 640x480, C = 81.
A call runs 11 bilateral passes (S, then one per iteration).  `total_ms`: events around the whole call (median of --reps,
after a warm-up call); `bilateral_ms`: the library's per-launch event pairs on dcrf_bil_kernel (a separate timed call, the
pairs fence each launch); `rest_ms` = total - bilateral.  Random uint8 image of smooth regions plus noise, random
probabilities.

Beside every exact row, from the same process and alternating with it call by call, the lattice row
(DenseCRF(..., bilateral="lattice")): `total_ms` of the whole call; `build_ms`: the lattice build with its one host read and
the allocations; `passes_ms`: the library call at iter_max = 10 minus the same call at iter_max = 0 (ten filters, Gaussian
messages and updates); `rest_ms` = total - build - passes (normalisers, Q0, unary).  `agreement`: arg-max agreement and
max |Q_lattice - Q_exact| on the benchmark image.  One flat-image row (every pixel one colour: six vertices own all the
entries, the splat's chunked path) is timed for the lattice alone."""
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


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def _lattice_split(img, P, H, W, C):
    """(build_ms, passes_ms) of one lattice call: the build, and the library call at iter_max = 10 minus at 0."""
    from weclip_vit_comer_amd import _lib as L
    p = PARAMS
    U = dcrf.unary_from_prob(P)
    Q = torch.empty_like(U)
    build, lt = _timed(lambda: dcrf._Lattice(img, C, H, W, p["bi_xy_std"], p["bi_rgb_std"]))

    def call(iters):
        return _timed(lambda: L.lib().wc_dcrf_lattice_inference(
            L.ptr(lt.lat), L.ptr(U), L.ptr(Q), L.ptr(lt.vals), L.ptr(lt.ws), C, H, W, lt.M, iters, float(p["pos_w"]),
            float(p["pos_xy_std"]), float(p["bi_w"]), L.stream()))[0]
    call(10)
    return build, call(10) - call(0), lt.M


def run_lattice(img, P, H, W, C, reps, times=None):
    lat = dcrf.DenseCRF(**PARAMS, bilateral="lattice")
    lat(img, P)
    torch.cuda.synchronize()
    times = [_timed(lambda: lat(img, P))[0] for _ in range(reps)] if times is None else times
    splits = [_lattice_split(img, P, H, W, C) for _ in range(reps)]
    total = statistics.median(times)
    build, passes = statistics.median(s[0] for s in splits), statistics.median(s[1] for s in splits)
    return dict(total_ms=round(total, 3), build_ms=round(build, 3), passes_ms=round(passes, 3),
                rest_ms=round(total - build - passes, 3), vertices=splits[0][2], vertices_per_pixel=round(splits[0][2] / (H * W), 4),
                total_ms_all_reps=[round(t, 3) for t in times])


def run_case(H, W, C, reps):
    g = torch.Generator().manual_seed(0)
    base = torch.rand(3, 6, 8, generator=g) * 255
    img = (F.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
           + 8 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8).cuda()
    P = torch.softmax(2 * torch.randn(C, H, W, generator=g), 0).cuda()
    crf = dcrf.DenseCRF(**PARAMS)
    lat = dcrf.DenseCRF(**PARAMS, bilateral="lattice")
    Qe, Ql = crf(img, P), lat(img, P)
    torch.cuda.synchronize()
    agreement = dict(argmax_agreement=round((Qe.argmax(0) == Ql.argmax(0)).float().mean().item(), 5),
                     max_abs_dQ=round((Qe - Ql).abs().max().item(), 4),
                     argmax_changed_by_exact=round((Qe.argmax(0) != P.argmax(0)).float().mean().item(), 5),
                     argmax_changed_by_lattice=round((Ql.argmax(0) != P.argmax(0)).float().mean().item(), 5))
    times, ltimes = [], []
    for _ in range(reps):                                   # exact and lattice calls alternate
        times.append(_timed(lambda: crf(img, P))[0])
        ltimes.append(_timed(lambda: lat(img, P))[0])
    lattice = run_lattice(img, P, H, W, C, reps, ltimes)
    lattice["agreement"] = agreement
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
                pairs_per_pass=n * n, total_ms_all_reps=[round(t, 3) for t in times], params=PARAMS, lattice=lattice,
                lattice_speedup=round(total / lattice["total_ms"], 1))


def run_flat(H, W, C, reps):
    img = torch.full((H, W, 3), 117, dtype=torch.uint8).cuda()
    P = torch.softmax(2 * torch.randn(C, H, W, generator=torch.Generator().manual_seed(1)), 0).cuda()
    return dict(H=H, W=W, C=C, image="flat", lattice=run_lattice(img, P, H, W, C, reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = [run_case(**c, reps=a.reps) for c in CASES]
    res = dict(device=torch.cuda.get_device_name(0), cases=res, flat=run_flat(**CASES[0], reps=a.reps))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
