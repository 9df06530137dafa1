"""HIP-event time of one forward + backward of the dense energy loss (utils.losses.DenseEnergyLossFunction) against the same loss
written with stock torch ops on the same card.

    python tools/energy_bench.py [--windows 5] [--out profiles/energy_bench.json] [--key NAME] [--small-only]

Sizes: N = 4, K = 21, 160 x 160 (the reference's default: crop 320, batch 4, scale 0.5) and N = 16, K = 21, 256 x 256.
Method: a warm-up call of both, then --windows windows of each, alternating (ours, stock, ours, ...); a window is `iters`
forward + backward calls between two events; reported: median (min .. max) of the windows' ms per call.  The stock form computes
the pairwise exponent in row chunks (a matmul of the centred features, exp) and contracts it with a matmul; it is the comparison, the parent commit has no
implementation.  `filter_ms`: the library's own event pair around energy_filter_kernel in a separate call.  `estimate_ms`: the
dense CRF's measured 29.101 ms per 3.515625e10 pairs at CP = 32 (profiles/dcrf_bench.json) scaled to this size's pairs.
The `lattice` row is the same call with bilateral="lattice" (csrc/energy_lattice.hip), timed in the same
process in windows that alternate with the exact ones; `lattice_split_ms`: the library's event pairs around the per-image build
(key kernel, sort, scans, neighbours) and filter (splat, blur, slice), summed over the images of one call, and the rest of a
forward + backward; `lattice_M_per_pixel`: lattice vertices per pixel of every image.  The lattice AS is about half the exact
AS, so `lattice_vs_exact` is recorded as a description of the two filters, not as an error.  --key NAME stores the result under
that key of the JSON file --out, keeping the file's other keys."""
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
from weclip_vit_comer_amd.utils import losses  # noqa: E402

CASES = [dict(N=4, K=21, H=160, W=160, iters=(100, 5)), dict(N=16, K=21, H=256, W=256, iters=(5, 1))]
SIGMA_RGB, SIGMA_XY = 15.0, 50.0
CHUNK = 2048


def stock_fwd_bwd(img, P, roi, unl, g):
    """(loss, grad_P) of the same definition with stock ops: Gate, S, chunked exp(-d^2 / 2) @ S, the two products.  The
    exponent's matmul form cancels (about 1e-4 of k at these sizes): it is the comparison's speed that is reported."""
    N, K, H, W = P.shape
    HW = H * W
    gate = roi - P.max(1).values
    gate = torch.where(unl, torch.ones_like(gate), gate).clamp_min(0)
    S = P * roi[:, None]
    ys, xs = torch.meshgrid(torch.arange(H, device=P.device, dtype=P.dtype), torch.arange(W, device=P.device, dtype=P.dtype),
                            indexing="ij")
    AS = torch.empty(N, HW, K, device=P.device, dtype=P.dtype)
    for n in range(N):
        f = torch.cat([torch.stack([xs, ys]).reshape(2, HW) / SIGMA_XY, img[n].reshape(3, HW) / SIGMA_RGB]).T.contiguous()
        f = f - f.mean(0)
        hn = -0.5 * (f * f).sum(1)
        Sn = S[n].reshape(K, HW).T.contiguous()
        for s in range(0, HW, CHUNK):
            # -|f_i - f_j|^2 / 2 = f_i . f_j - |f_i|^2 / 2 - |f_j|^2 / 2 on centred features: one matmul per chunk
            e = torch.addmm(hn[None, :], f[s:s + CHUNK], f.T).add_(hn[s:s + CHUNK, None])
            AS[n, s:s + CHUNK] = torch.exp_(e.clamp_(max=0)) @ Sn
    A = gate[:, None] * AS.transpose(1, 2).reshape(N, K, H, W)
    loss = -(S * A).sum().reshape(1) / N
    return loss, (-2.0 / N) * g * A * roi[:, None]


def ours_fwd_bwd(img, P, roi, unl, g):
    p = P.detach().requires_grad_(True)
    loss = losses.DenseEnergyLossFunction.apply(img, p, SIGMA_RGB, SIGMA_XY, roi, unl)
    loss.backward(g)
    return loss.detach(), p.grad


LATTICE_WS = {}


def lattice_fwd_bwd(img, P, roi, unl, g):
    p = P.detach().requires_grad_(True)
    loss, A, _ = losses.dense_energy_forward(img, p, SIGMA_RGB, SIGMA_XY, roi, unl, "lattice",
                                             losses._lattice_workspace(*P.shape, P.device, LATTICE_WS))
    return loss, losses.dense_energy_backward(g, A, roi)


def window(fn, args, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn(*args)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def run_case(N, K, H, W, iters, windows):
    g = torch.Generator().manual_seed(0)
    base = torch.rand(N, 3, 6, 8, generator=g) * 255
    img = (F.interpolate(base, size=(H, W), mode="bilinear", align_corners=False) + 8 * torch.randn(N, 3, H, W, generator=g)).clamp(0, 255).cuda()
    P = torch.softmax(2 * torch.randn(N, K, H, W, generator=g), 1).cuda()
    roi = torch.zeros(N, H, W)
    roi[:, H // 16:H - H // 16, W // 16:W - W // 16] = 1
    roi = roi.cuda()
    unl = (torch.rand(N, H, W, generator=g) > 0.9).cuda()
    gout = torch.ones(1, device="cuda")
    args = (img, P, roi, unl, gout)
    l1, g1 = ours_fwd_bwd(*args)
    l2, g2 = stock_fwd_bwd(*args)
    torch.cuda.synchronize()
    agree = dict(loss_rel=abs(l1.item() - l2.item()) / abs(l2.item()), grad_rel_of_max=((g1 - g2).abs().max() / g2.abs().max()).item())
    l3, g3 = lattice_fwd_bwd(*args)
    torch.cuda.synchronize()
    flag, M = losses.lattice_vertex_counts(losses._lattice_workspace(N, K, H, W, P.device, LATTICE_WS)[0], N)
    lat_vs_exact = dict(loss_ratio=l3.item() / l1.item(), grad_max_ratio=(g3.abs().max() / g1.abs().max()).item(), clamp_flag=flag.item())
    ours, stock, lat = [], [], []
    for _ in range(windows):
        ours.append(window(ours_fwd_bwd, args, iters[0]))
        lat.append(window(lattice_fwd_bwd, args, iters[0]))
        stock.append(window(stock_fwd_bwd, args, iters[1]))
    KernelTimer.enable(1)
    lattice_fwd_bwd(*args)
    rec = KernelTimer.summary()
    KernelTimer.enable(0)
    build_ms, filt_ms = (rec.get(k, {}).get("ms", float("nan")) for k in ("energy_lattice_build", "energy_lattice_filter"))
    lat_med = statistics.median(lat)
    split = dict(build=round(build_ms, 3), filter=round(filt_ms, 3), rest=round(lat_med - build_ms - filt_ms, 3))
    KernelTimer.enable(1)
    ours_fwd_bwd(*args)
    rec = KernelTimer.summary().get("energy_filter_kernel", {})
    KernelTimer.enable(0)
    pairs = N * (H * W) ** 2
    return dict(N=N, K=K, H=H, W=W, CP=32 * ((K + 31) // 32), pairs=pairs, iters_per_window=list(iters), windows=windows,
                ours=stats(ours), lattice=stats(lat), lattice_split_ms=split, lattice_M_per_pixel=[round(m / (H * W), 3) for m in M.tolist()],
                exact_over_lattice=round(statistics.median(ours) / lat_med, 2), lattice_all_ms=[round(t, 3) for t in lat],
                lattice_vs_exact=lat_vs_exact, stock_torch=stats(stock), filter_ms=round(rec.get("ms", float("nan")), 3),
                estimate_ms=round(29.101 * pairs / 3.515625e10, 3), ours_all_ms=[round(t, 3) for t in ours],
                stock_all_ms=[round(t, 3) for t in stock], ours_vs_stock=agree, sigma_rgb=SIGMA_RGB, sigma_xy=SIGMA_XY)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--key", default=None, help="store the result under this key of the JSON file --out, keeping its other keys")
    ap.add_argument("--small-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("energy_bench: needs the GPU; there is nothing to time without one")
    res = [run_case(**c, windows=a.windows) for c in (CASES[:1] if a.small_only else CASES)]
    res = dict(device=torch.cuda.get_device_name(0), cases=res)
    print(json.dumps(res, indent=1))
    if a.out and a.key:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res = dict(old, **{a.key: res})
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
