"""HIP-event time of utils.mmdloss.mmd_rbf (csrc/mmd.hip), forward alone and forward + gradient, against stock torch forms of the
same loss on the same card.

    python tools/mmd_bench.py [--windows 5] [--out profiles/mmd_bench.json]

Sizes (B rows per side, width d): (256, 768), (2048, 768), (8192, 256); kernel_mul 2, kernel_num 5, bandwidth from the data.
Method: a warm-up call of each form, then --windows windows of each, alternating; a window is `iters` calls between two events;
reported: median (min .. max) of the windows' ms per call.
  ours        : the whole call (prep kernels, main kernel, finish; with the gradient also autograd's scaling of it).
  main_kernel : the library's own event pair around mmd_main_kernel in a separate call, its issued MFMA FLOPs (the S product
                over every tile visited -- the upper triangle for the forward alone, every tile once per 128-column chunk with
                the gradient -- plus the second product) and that as a fraction of the 157 TF f32-input-MFMA peak.
  expanded    : the reference's formulation, the (N, N, d) difference tensor, with autograd; only where it fits (B = 256).
  cdist       : torch.cdist(X, X)^2, the exponentials and the block means with autograd; `peak_MiB` is
                torch.cuda.max_memory_allocated over the inputs during one forward + backward.
`ours_vs_stock`: relative difference of the two losses and of the gradients (of the gradient's largest magnitude)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import weclip_vit_comer_amd  # noqa: E402,F401
from weclip_vit_comer_amd.ops import KernelTimer  # noqa: E402
from weclip_vit_comer_amd.utils import mmdloss  # noqa: E402

CASES = [dict(B=256, d=768, iters=(200, 5), expanded=True), dict(B=2048, d=768, iters=(20, 3), expanded=False),
         dict(B=8192, d=256, iters=(5, 1), expanded=False)]
MUL, NUM = 2.0, 5
PEAK_TF = 157.0
TILE, CHUNK = 64, 128


def _loss_from_l2(L2, B):
    N = 2 * B
    bw = L2.detach().sum() / (N * N - N) / MUL ** (NUM // 2)
    K = sum(torch.exp(-L2 / (bw * MUL ** b)) for b in range(NUM))
    return (K[:B, :B] + K[B:, B:] - K[:B, B:] - K[B:, :B]).mean()


def expanded_loss(s, t):
    X = torch.cat([s, t])
    return _loss_from_l2((X[None, :, :] - X[:, None, :]).square().sum(2), s.shape[0])


def cdist_loss(s, t):
    X = torch.cat([s, t])
    return _loss_from_l2(torch.cdist(X, X).square(), s.shape[0])


def fwd(loss_fn):
    def run(s, t):
        with torch.no_grad():
            return loss_fn(s, t)
    return run


def fwd_bwd(loss_fn):
    def run(s, t):
        s, t = s.detach().requires_grad_(True), t.detach().requires_grad_(True)
        loss = loss_fn(s, t)
        return (loss.detach(),) + torch.autograd.grad(loss, (s, t))
    return run


def window(fn, args, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn(*args)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def main_kernel(fn, args, name, flops):
    KernelTimer.enable(1)
    fn(*args)
    rec = KernelTimer.summary().get(name, {})
    KernelTimer.enable(0)
    ms = rec.get("ms", float("nan"))
    return dict(ms=round(ms, 4), issued_gflop=round(flops / 1e9, 2), fraction_of_peak=round(flops / (ms * 1e-3) / (PEAK_TF * 1e12), 4))


def peak_mib(fn, args):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(*args)
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def run_case(B, d, iters, expanded, windows):
    g = torch.Generator().manual_seed(0)
    s = torch.randn(B, d, generator=g).cuda()
    t = (1.3 * torch.randn(B, d, generator=g) + 0.5).cuda()
    args = (s, t)
    forms = {"ours_fwd": (fwd(mmdloss.mmd_rbf), iters[0]), "ours_fwd_bwd": (fwd_bwd(mmdloss.mmd_rbf), iters[0]),
             "cdist_fwd": (fwd(cdist_loss), iters[1]), "cdist_fwd_bwd": (fwd_bwd(cdist_loss), iters[1])}
    if expanded:
        forms.update(expanded_fwd=(fwd(expanded_loss), iters[1]), expanded_fwd_bwd=(fwd_bwd(expanded_loss), iters[1]))
    outs = {k: f(*args) for k, (f, _) in forms.items()}                       # warm-up
    torch.cuda.synchronize()
    ours, stock = outs["ours_fwd_bwd"], outs["cdist_fwd_bwd"]
    agree = dict(loss_rel=abs(ours[0].item() - stock[0].item()) / abs(stock[0].item()),
                 grad_rel_of_max=max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(ours[1:], stock[1:])))
    ts = {k: [] for k in forms}
    for _ in range(windows):
        for k, (f, n) in forms.items():
            ts[k].append(window(f, args, n))
    N, dp = 2 * B, 32 * ((d + 31) // 32)
    nt, nchunk = (N + TILE - 1) // TILE, (dp + CHUNK - 1) // CHUNK
    tile_s = 2.0 * TILE * TILE * dp
    res = dict(B=B, d=d, N=N, windows=windows, iters_per_window=list(iters), ours_vs_cdist=agree)
    res.update({k: stats(v) for k, v in ts.items()})
    res["main_kernel_fwd"] = main_kernel(forms["ours_fwd"][0], args, "mmd_main_kernel<loss>", nt * (nt + 1) / 2 * tile_s)
    res["main_kernel_fwd_bwd"] = main_kernel(forms["ours_fwd_bwd"][0], args, "mmd_main_kernel<grad>",
                                             nchunk * nt * nt * (tile_s + 2.0 * TILE * TILE * CHUNK))
    res["minimal_gflop_fwd_bwd"] = round(2.0 * N * N * (2 * d) / 1e9, 2)    # S once, the second product once
    res["peak_MiB"] = {k: peak_mib(forms[k][0], args) for k in forms if k.endswith("fwd_bwd")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mmd_bench: needs the GPU; there is nothing to time without one")
    res = dict(device=torch.cuda.get_device_name(0), kernel_mul=MUL, kernel_num=NUM, peak_tf=PEAK_TF,
               cases=[run_case(**c, windows=a.windows) for c in CASES])
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
