"""What the dense energy loss costs as a term of the training step (utils.losses.get_energy_loss_fused, TrainStep(reg=...)).

    python tools/energy_step_bench.py [--windows 5] [--out profiles/energy_step_bench.json] [--key NAME] [--small-only]

Shapes: N = 4, 20 x 20 -> 320 x 320 and N = 16, 32 x 32 -> 512 x 512, K = 21, scale_factor 0.5.
  (a) term:  forward + backward of the fused term against the stock composition get_energy_loss(img, F.interpolate(seg, (H, W)),
             label, img_box, layer) on the same card: a warm-up call of both, then --windows windows of each, alternating; a window
             is `iters` calls between two HIP events; median (min .. max) of the windows' ms per call.  Also
             torch.cuda.max_memory_allocated over one call of each, above what the inputs hold.
  (b) prep:  wc_energy_prep_fwd and wc_energy_prep_bwd alone: 20 calls captured in a graph, replayed between two events (no host
             time in the figure).
  (c) step:  a graph-replayed TrainStep on the synthetic flagship model with and without the term at B = 4 / 320 and
             B = 16 / 512, alternating windows of whole steps (optimizer included), the same batch every step.
Beside every exact figure stands the lattice one (bilateral="lattice", csrc/energy_lattice.hip): `fused_lattice`
in (a), `step_with_lattice_term` in (c), timed in the same process in windows that alternate with the exact ones.  The synthetic
images are noise, which puts nearly every pixel on vertices of its own (`lattice_M_per_pixel`): the lattice's slow end.
--key NAME stores the result under that key of the JSON file --out, keeping the file's other keys."""
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
from weclip_vit_comer_amd import synth  # noqa: E402
from weclip_vit_comer_amd.utils import losses  # noqa: E402

K = 21
CASES = [dict(N=4, h=20, H=320, iters=(50, 50), step_iters=10), dict(N=16, h=32, H=512, iters=(5, 5), step_iters=5)]
LAYER = dict(weight=1e-7, sigma_rgb=15, sigma_xy=100, scale_factor=0.5)
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                all_ms=[round(t, 4) for t in ts])


def alternating(f1, f2, iters, windows, f3=None):
    """Windows of f1, f2 (and f3, at f1's iterations) in turn -> their stats."""
    t1, t2, t3 = [], [], []
    for _ in range(windows):
        t1.append(window(f1, iters[0]))
        if f3 is not None:
            t3.append(window(f3, iters[0]))
        t2.append(window(f2, iters[1]))
    return (stats(t1), stats(t2)) + ((stats(t3),) if f3 is not None else ())


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def graphed_ms(fn, windows, reps=20):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    return stats([window(g.replay, 1) / reps for _ in range(windows)])


def inputs(N, h, H):
    g = torch.Generator().manual_seed(0)
    img = synth.make_images(N, H, H, seed=7).cuda()
    seg = (2 * torch.randn(N, K, h, h, generator=g)).cuda()
    label = torch.randint(0, K, (N, H, H), generator=g)
    label[torch.rand(N, H, H, generator=g) > 0.9] = 255
    box = [[H // 16 + n, H - H // 16, n, H - H // 16] for n in range(N)]
    return img, seg, label.cuda(), box


def run_term(N, h, H, iters, windows):
    img, seg, label, box = inputs(N, h, H)
    layer = losses.DenseEnergyLoss(**LAYER)
    lat_layer = losses.DenseEnergyLoss(**LAYER, bilateral="lattice")
    lat_layer.workspace_cache = {}                        # as TrainStep keeps it: allocated once
    dbox = torch.tensor(box, dtype=torch.int32).cuda()

    def fused(layer=layer):
        p = seg.detach().requires_grad_(True)
        loss = losses.get_energy_loss_fused(img, p, label, dbox, layer)
        loss.backward()
        return loss.detach(), p.grad

    fused_lattice = lambda: fused(lat_layer)             # noqa: E731

    def stock():
        p = seg.detach().requires_grad_(True)
        logits = F.interpolate(p, size=(H, H), mode="bilinear", align_corners=False)
        loss = losses.get_energy_loss(img, logits, label, box, layer)
        loss.backward()
        return loss.detach(), p.grad

    (l1, g1), (l2, g2) = fused(), stock()
    agree = dict(loss_rel=abs(l1.item() - l2.item()) / abs(l2.item()), grad_rel_of_max=((g1 - g2).abs().max() / g2.abs().max()).item())
    mem = dict(fused_peak_mib=peak_mib(fused), stock_peak_mib=peak_mib(stock))
    l3, g3 = fused_lattice()
    flag, M = losses.lattice_vertex_counts(next(iter(lat_layer.workspace_cache.values()))[0], N)
    lat = dict(loss_ratio_to_exact=l3.item() / l1.item(), grad_max_ratio_to_exact=(g3.abs().max() / g1.abs().max()).item(),
               clamp_flag=flag.item(), lattice_M_per_pixel=[round(m / ((H // 2) ** 2), 3) for m in M.tolist()],
               lattice_peak_mib=peak_mib(fused_lattice))
    t_fused, t_stock, t_lat = alternating(fused, stock, iters, windows, fused_lattice)
    # the prep pair alone, on the filter's output of this input
    e = 1
    i32, s32, lab = img.float().contiguous(), seg.float().contiguous(), label.long().contiguous()
    images_s, P_s, rois_s, unl = losses.energy_prep_forward(i32, s32, lab, dbox, e, MEAN, STD)
    _, A, _ = losses.dense_energy_forward(images_s, P_s, LAYER["sigma_rgb"], LAYER["sigma_xy"] * 0.5, rois_s, unl)
    prep_fwd = graphed_ms(lambda: losses.energy_prep_forward(i32, s32, lab, dbox, e, MEAN, STD), windows)
    prep_bwd = graphed_ms(lambda: losses.energy_prep_backward(A, rois_s, s32, -2e-7 / N, (H, H), e), windows)
    return dict(N=N, K=K, h=h, w=h, H=H, W=H, scale_factor=0.5, iters_per_window=list(iters), windows=windows, fused=t_fused,
                stock=t_stock, fused_lattice=t_lat, exact_over_lattice=round(t_fused["median_ms"] / t_lat["median_ms"], 2), **lat,
                fused_vs_stock=agree, **mem, prep_fwd=prep_fwd, prep_bwd=prep_bwd)


def make_step(reg):
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP
    from weclip_vit_comer_amd.train_step import TrainStep
    sd = synth.make_clip_state_dict(seed=0, with_text=False)
    bg, fg = synth.make_text_features(20, 25, 512)
    fuse, dec = synth.make_head_state_dicts()
    torch.manual_seed(0)
    model = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[768] * 4, dataset_root_path=None, device="cuda",
                   text_features=(bg.cuda(), fg.cuda()))
    model.decoder_fts_fuse.load_state_dict(fuse)
    model.decoder.load_state_dict(dec)
    model.train()
    return TrainStep(model, graph=True, reg=reg)


def run_step(B, size, iters, windows):
    img = synth.make_images(B, size, size, seed=100).cuda()
    labels = synth.make_label_lists(B, 2)
    box = torch.tensor([[size // 16 + n, size - size // 16, n, size - size // 16] for n in range(B)], dtype=torch.int16).cuda()
    plain, reg, lat = make_step(None), make_step({}), make_step({"bilateral": "lattice"})
    f_plain = lambda: plain(img, labels=labels)                       # noqa: E731
    f_reg = lambda: reg(img, labels=labels, img_box=box)              # noqa: E731
    f_lat = lambda: lat(img, labels=labels, img_box=box)              # noqa: E731
    for _ in range(3):               # eager, capture, one replay
        f_plain()
        out = f_reg()
        out_lat = f_lat()
    torch.cuda.synchronize()
    t_plain, t_reg, t_lat = alternating(f_plain, f_reg, (iters, iters), windows, f_lat)
    term = round(t_reg["median_ms"] - t_plain["median_ms"], 4)
    term_lat = round(t_lat["median_ms"] - t_plain["median_ms"], 4)
    return dict(B=B, size=size, iters_per_window=iters, windows=windows, plain_step=t_plain, step_with_term=t_reg,
                step_with_lattice_term=t_lat, term_ms=term, lattice_term_ms=term_lat,
                graphs=[len(plain._graphs), len(reg._graphs), len(lat._graphs)], energy_last=out[3].item(),
                lattice_energy_last=out_lat[3].item(), lattice_workspaces=len(lat.reg.layer.workspace_cache))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--key", default=None, help="store the result under this key of the JSON file --out, keeping its other keys")
    ap.add_argument("--small-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("energy_step_bench: needs the GPU; there is nothing to time without one")
    cases = CASES[:1] if a.small_only else CASES
    res = dict(device=torch.cuda.get_device_name(0),
               term=[run_term(c["N"], c["h"], c["H"], c["iters"], a.windows) for c in cases],
               step=[run_step(c["N"], c["H"], c["step_iters"], a.windows) for c in cases])
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
