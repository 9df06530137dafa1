#!/usr/bin/env python3
"""Benchmark of the WeCLIP hot path on MI355X.

A step = one full training step of `WeCLIP` (VOC head, 21 classes) on one synthetic VOC-shaped
batch: frozen CLIP ViT-B/16 encoder forward, adapters + decoder forward, block-12 forward +
GradCAM for K=2 classes per image, affinity refinement, PAR (20 iterations), losses, backward of
adapters/decoder, (DP: one RCCL all-reduce of the 5.99 M gradients), AdamW step.
BASELINE.json metric: images/sec (train fwd+bwd) ViT-B/16 512x512; per-GPU batch 16 (configs[2]).

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --full      (everything the benchmark measures and checks)
    python bench.py --gpus 4 ...          (starts 4 rank processes itself when WORLD_SIZE is unset)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line on rank 0.
  * `value`: the timed region replays the HIP graph of the step (train_step.TrainStep(graph=True)); every step gets
    another batch from the per-rank seeded loader.
A plain run does only what `value` needs: set-up, `--warmup` steps, ONE timed region of `--steps` steps, the outputs of
`--dump-outputs`, the JSON line.  Everything else needs `--full`:
  * `repeat_ms_per_step` etc. (`--repeats` timed regions, `value` stays the first), `host_work_ms_per_step_idle_queue`, and
    at N > 1 `dp_check` / `dp_diag`.
  * `roofline`: dominant kernel family timed with HIP events on the launch stream, recorded by the C library at its
    launch sites during `--roof-steps` EAGER steps of the same workload right after the timed region (a captured
    graph has no per-launch call sites to put the event pairs at).
  * `cpu_baseline`: the CPU oracle (oracle/weclip_oracle.py, a port of the reference's CPU path) on a bounded sample.
  * extra legs at N=1 (`--no-extras` skips them): `seg_trans_branch` (the iter > 15000 affinity branch),
    `exact_precision` (fp16 hi+lo operands, fp32 PAR), `fast_gemm_fp32_par` (the headline's GEMM precision with the
    reference's fp32 PAR affinities: what the 16-bit PAR layout alone buys), `with_comer` (BASELINE configs[2] as written: + ViT-CoMer
    inserts; parity unpinned, no reference code), `encoder_only_b32` (BASELINE configs[1]).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16, help="images per GPU")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes-per-image", type=int, default=2)
    ap.add_argument("--precision", default=None, choices=[None, "fast", "exact"])
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: repeats, host / DP diagnostics, roofline, extra legs, CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the seg-trans / exact / CoMer / encoder-only legs")
    ap.add_argument("--no-graph", action="store_true", help="time eager steps (every launch through Python)")
    ap.add_argument("--comer", action="store_true",
                    help="main leg with the ViT-CoMer inserts (no reference code exists for them; off = the reference model)")
    ap.add_argument("--seg-trans", action="store_true", help="main leg in the seg-trans affinity branch (iter > 15000)")
    ap.add_argument("--timer-stride", type=int, default=7,
                    help="HIP-event pair around 1 of every n instrumented kernel launches (0: none, roofline = null)")
    ap.add_argument("--roof-steps", type=int, default=8, help="eager instrumented steps for the roofline leg")
    ap.add_argument("--single-stream", action="store_true",
                    help="head forward on the step's own stream instead of beside the CAM chain (profiling passes: a kernel trace "
                         "then times every kernel alone)")
    ap.add_argument("--repeats", type=int, default=5,
                    help="--full: the timed region of --steps steps is run this many times; `value` is the first, all are "
                         "reported")
    ap.add_argument("--cpu-images", type=int, default=1, help="images per point of the CPU-oracle thread sweep")
    ap.add_argument("--cpu-threads", default="1,8,32,all", help="thread counts of the CPU-oracle sweep")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step of the --repeats regions computed (losses, "
                         "gradients, updated parameters) as DIR/<name>.npy (float32, <= 64 MB in all)")
    return ap.parse_args()


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes (one per GPU) BEFORE this process
    makes any GPU call, wait for them, pass rank 0's JSON line through.  Never re-execs a GPU-initialised process."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for p in procs:
        rc = max(rc, abs(p.wait()))
    sys.exit(rc)


def cpu_baseline(args):
    """Oracle (port of the reference CPU path) on `cpu_images` images of the same workload:
    forward + losses + backward of the trainable heads."""
    import torch
    from oracle import synth
    from oracle import weclip_oracle as O
    sd = synth.make_clip_state_dict(seed=0, with_text=False)
    bg, fg = synth.make_text_features(20, 25, 512)

    def run(n):
        fuse, dec = synth.make_head_state_dicts()
        fuse = {k: v.requires_grad_(True) for k, v in fuse.items()}
        dec = {k: v.requires_grad_(True) for k, v in dec.items()}
        img = synth.make_images(n, args.size, args.size, seed=100)
        labels = synth.make_label_lists(n, args.classes_per_image)
        t0 = time.time()
        seg, cam, ap = O.weclip_forward(img, labels, sd, fuse, dec, bg, fg, heads=12)
        loss, _, _ = O.train_losses(seg, cam, ap)
        loss.backward()
        return time.time() - t0

    what = (f"{args.cpu_images} image(s) {args.size}x{args.size}, K={args.classes_per_image}: oracle forward (encoder, GradCAM, "
            f"affinity, PAR) + losses + head backward")
    allc = torch.get_num_threads()
    counts = []
    for tok in str(args.cpu_threads).split(","):
        n = allc if tok.strip() == "all" else int(tok)
        if 1 <= n <= allc and n not in counts:
            counts.append(n)
    sweep = {}
    try:
        for n in counts:          # SURVEY section 8d asks n in {1, all}; the port's many small torch ops peak in between
            torch.set_num_threads(n)
            dt = run(args.cpu_images)
            sweep[n] = (args.cpu_images / dt, dt)
    finally:
        torch.set_num_threads(allc)
    best = max(sweep, key=lambda n: sweep[n][0])
    return {"value": sweep[best][0], "unit": "images/sec", "cores": best, "best_threads": best, "kind": "port",
            "host_cores": allc,
            "sample": f"{what}; best of a thread sweep, {sweep[best][1]:.1f} s at {best} threads",
            "thread_sweep": {str(n): {"images_per_sec": round(v[0], 4), "seconds": round(v[1], 1)} for n, v in sweep.items()}}


def make_model(dev, comer=False, seg_trans=False):
    import torch
    from weclip_vit_comer_amd import synth
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP
    sd = synth.make_clip_state_dict(seed=0, with_text=False)
    bg, fg = synth.make_text_features(20, 25, 512)
    fuse, dec = synth.make_head_state_dicts()
    torch.manual_seed(0)
    model = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[768] * 4,
                   dataset_root_path=None, device=dev, text_features=(bg.to(dev), fg.to(dev)), comer=comer)
    model.decoder_fts_fuse.load_state_dict(fuse)
    model.decoder.load_state_dict(dec)
    model.train()
    if seg_trans:
        model.iter_num = 20000
    return model


def timed_steps(step, loader, n, world, dev, last=None):
    """EXACTLY n steps between barrier + synchronize on both sides; returns (seconds [max over ranks], host seconds).
    `last` (a list): receives the outputs of the last step."""
    import torch
    import torch.distributed as dist
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    c0 = time.process_time()
    out = None
    for _ in range(n):
        img, labels = loader.next()
        out = step(img, labels=labels)
    if last is not None:
        last[:] = [out]
    t_enq = time.perf_counter() - t0          # host wall time until the last step is enqueued (includes waiting on a full queue)
    t_cpu = time.process_time() - c0          # CPU time this process burnt doing it (all threads)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    per_rank = [dt]
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        per_rank = [float(x.item()) for x in allt]
        dt = max(per_rank)                      # the job is as slow as its slowest rank
    return dt, t_enq, t_cpu, per_rank


DUMP_MAX_ELEMS = 7_000_000       # per array: the two parameter-sized arrays stay under 64 MB of float32 together


def dump_outputs(out_dir, step, out):
    """What the caller of the timed step holds after its last step: the three losses it returned, the (all-reduced)
    gradients of the trainable parameters and those parameters after the optimizer step.  float32 .npy files; an array
    longer than DUMP_MAX_ELEMS is replaced by a fixed, seeded sample of its elements (same indices in every run)."""
    import numpy as np
    import torch
    loss, seg_loss, attn_loss = out
    params = step.model.get_param_groups()[3]
    if step.bucket is not None:
        grads = step.bucket.flat
    else:
        grads = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().flatten() for p in params])
    arrays = {"loss": loss, "seg_loss": seg_loss, "attn_loss": attn_loss, "grads": grads,
              "params": torch.cat([p.detach().flatten() for p in params])}
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.size > DUMP_MAX_ELEMS:
            idx = np.sort(np.random.default_rng(0).choice(a.size, DUMP_MAX_ELEMS, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float32))


def run_leg(args, dev, rank, world, *, comer=False, seg_trans=False, steps=None, warmup=None, graph=True, repeats=1,
            diagnostics=True, dump_dir=None):
    """Build a model + TrainStep, warm up, time `repeats` regions of `steps` steps.  -> (dict, step, loader)
    diagnostics: then also the repeat spread, the host work per step on an idle queue and at N > 1 the DP checks (--full).
    dump_dir: rank 0 writes there the outputs of the last step of `--repeats` regions (dump_outputs)."""
    from weclip_vit_comer_amd.data import SyntheticVOCLoader
    from weclip_vit_comer_amd.train_step import TrainStep
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    model = make_model(dev, comer=comer, seg_trans=seg_trans)
    if args.single_stream:
        model.fork_head = False
    use_graph = graph
    step = TrainStep(model, graph=use_graph)
    loader = SyntheticVOCLoader(args.batch, args.size, args.classes_per_image, rank=rank, world=world, device=dev,
                                source="uint8")      # device-side rescale / flip / crop / normalise inside every step
    for _ in range(2 if use_graph else 0):   # set-up of the graph mode: one eager step, then the capturing step
        img, labels = loader.next()
        step(img, labels=labels)
    for _ in range(warmup):
        img, labels = loader.next()
        step(img, labels=labels)
    last = []
    dt, t_enq, t_cpu, per_rank = timed_steps(step, loader, steps, world, dev, last)
    # the same region again (a 0.26 s region cannot resolve 2 %): `value` stays the FIRST region of exactly
    # `steps` steps; the repeats show the run-to-run spread inside one process on one box
    rep_ms = [dt / steps * 1e3]
    for _ in range(max(0, repeats - 1)):
        rep_ms.append(timed_steps(step, loader, steps, world, dev, last)[0] / steps * 1e3)
    if dump_dir is not None:
        # what is written is the state after `--repeats` regions however many of them were timed: a plain run (one timed
        # region) runs the steps of the others here, untimed, on every rank
        for _ in range((max(1, args.repeats) - max(1, repeats)) * steps):
            img, labels = loader.next()
            last[:] = [step(img, labels=labels)]
        if rank == 0:
            dump_outputs(dump_dir, step, last[0])
    res = {"value": round(world * args.batch * steps / dt, 3), "ms_per_step": round(dt / steps * 1e3, 3),
           "host_enqueue_ms_per_step": round(t_enq / steps * 1e3, 3),
           "host_cpu_ms_per_step": round(t_cpu / steps * 1e3, 3), "steps": steps,
           "launch_mode": "hipGraph replay" if use_graph else "eager"}
    if diagnostics:
        res.update(leg_diagnostics(step, loader, world, dev, steps, rep_ms, per_rank))
    return res, step, loader


def leg_diagnostics(step, loader, world, dev, steps, rep_ms, per_rank):
    """--full: spread of the repeated regions, host work per step on an idle queue, at N > 1 the gradient exchange alone
    and whether the ranks hold the same parameters."""
    # host work per step, free of back-pressure: each step enqueued onto an IDLE queue (in the timed region above the host
    # runs ahead of the GPU-bound device and then blocks in the loader's pinned-buffer event, which is waiting, not work)
    import torch
    t_idle = 0.0
    for _ in range(5):
        img, labels = loader.next()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(img, labels=labels)
        t_idle += time.perf_counter() - t0
    torch.cuda.synchronize()
    dp_check = None
    dp_diag = None
    if world > 1:      # every rank must hold the same parameters after the same number of all-reduced steps
        import torch.distributed as dist
        # diagnostics for the first multi-GPU hardware run: the gradient exchange alone (the bucket's all-reduce + 1/world scale,
        # 20 back-to-back calls on an otherwise idle GPU, HIP events on this rank's stream) and the spread of the ranks' clocks
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        keep = step.bucket.flat.clone()
        step.bucket.all_reduce_mean()
        torch.cuda.synchronize()
        dist.barrier()
        e0.record()
        for _ in range(20):
            step.bucket.all_reduce_mean()
        e1.record()
        torch.cuda.synchronize()
        step.bucket.flat.copy_(keep)
        dp_diag = {"allreduce_ms_per_step": round(e0.elapsed_time(e1) / 20, 4),
                   "allreduce_bytes": int(step.bucket.flat.numel() * 4),
                   "rank_ms_per_step_min": round(min(per_rank) / steps * 1e3, 3),
                   "rank_ms_per_step_max": round(max(per_rank) / steps * 1e3, 3)}
        ps = [p.detach().double() for p in step.model.get_param_groups()[3]]
        ck = torch.stack([sum(p.sum() for p in ps), sum((p * p).sum() for p in ps)]).to(dev)
        allck = [torch.zeros_like(ck) for _ in range(world)]
        dist.all_gather(allck, ck)
        dp_check = {"params_identical_across_ranks": bool(all(torch.equal(allck[0], c) for c in allck)),
                    "param_checksum": [float(v) for v in allck[0].tolist()]}
    srt = sorted(rep_ms)
    return {"dp_check": dp_check, "dp_diag": dp_diag, "repeat_ms_per_step": [round(r, 3) for r in rep_ms],
            "repeat_median_ms": round(srt[len(srt) // 2], 3), "repeat_min_ms": round(srt[0], 3), "repeat_max_ms": round(srt[-1], 3),
            "host_work_ms_per_step_idle_queue": round(t_idle / 5 * 1e3, 3)}


def roofline_leg(args, step, loader, dev, use_traffic=True, traffic_files="r*_traffic.json"):
    """Eager instrumented steps of the same TrainStep: HIP-event pairs at the C library's launch sites."""
    import torch
    from weclip_vit_comer_amd import ops
    B, S, K = args.batch, args.size, args.classes_per_image
    step.graph = False
    # one stream for these steps: an event pair around a launch must time THAT kernel, not its share of the GPU beside the
    # head forward that the timed (graph) steps run on a second stream
    fork_was = getattr(step.model, "fork_head", False)
    step.model.fork_head = False
    for _ in range(2):
        img, labels = loader.next()
        step(img, labels=labels)
    torch.cuda.synchronize()
    ops.KernelTimer.enable(args.timer_stride)
    n = args.roof_steps
    t0 = time.perf_counter()
    for _ in range(n):
        img, labels = loader.next()
        step(img, labels=labels)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    summ = ops.KernelTimer.summary()
    ops.KernelTimer.enable(0)
    step.model.fork_head = fork_was
    stride = max(args.timer_stride, 1)

    # peaks from guides/MI355X_MICROARCH.md: dense fp16 MFMA 2.5 PFLOP/s, HBM3E 8 TB/s
    HBM = ("par_", "matvec", "aff_", "tsym", "sinkhorn")

    def peak_of(name):
        return ("hbm", 8000.0, "GB/s") if name.startswith(HBM) else ("mfma", 2500.0, "TFLOP/s")
    # HBM traffic per launch from committed rocprofv3 PMC passes of this same command (tools/refresh_profiles.sh +
    # tools/pmc_traffic.py -> profiles/rNN_traffic.json; 2*FETCH_SIZE + WRITE_SIZE, KiB, per the MI355X guide), keyed by the
    # same kernel names -- accepted ONLY when the kernel sources the passes were taken from are the sources of this build
    # (content hash recorded in the file); otherwise null, with the reason in `traffic_source`.
    import glob
    import __graft_entry__
    cur = __graft_entry__._load_build_module().source_hash()
    traffic, tsrc = {}, "none: no profiles/r*_traffic.json carries the source hash of this build (%s)" % cur
    tpaths = [t for t in glob.glob(os.path.join(ROOT, "profiles", traffic_files))
              if ("_comer_" in os.path.basename(t)) == ("_comer_" in traffic_files)]
    for tpath in sorted(tpaths, reverse=True):
        if not (B == 16 and S == 512 and K == 2) or not use_traffic:
            tsrc = "none: PMC passes exist for B=16, 512x512, K=2 only"
            break
        data = json.load(open(tpath))
        if data.get("__meta__", {}).get("source_hash") == cur:
            traffic = {k: round(v["hbm_bytes_per_launch"]) for k, v in data.items() if k != "__meta__"}
            # the library times the deformable-attention kernels per direction (<1> / <3> levels) and the weight-gradient GEMM
            # under one name; rocprofv3 reports template arguments: map the ones that correspond one to one (the gather / bucket
            # kernels are one instantiation for both directions: no per-direction counter value, left null)
            for lib, prof in (("msda_fwd4f_kernel<1>", "msda_fwd4f_kernel<__half, 1, 4>"), ("msda_fwd4f_kernel<3>", "msda_fwd4f_kernel<__half, 3, 4>"),
                              ("msda_bwd4f_kernel<1>", "msda_bwd4f_kernel<__half, __half, 1, 4>"),
                              ("msda_bwd4f_kernel<3>", "msda_bwd4f_kernel<__half, __half, 3, 4>")):
                if prof in traffic:
                    traffic[lib] = traffic[prof]
            tsrc = ("profiles/" + os.path.basename(tpath) + " (committed rocprofv3 --pmc passes of this command on the same "
                    "kernel sources, hash %s; a separate run, as the guide prescribes)" % cur)
            break
    # north-star group "ViT attention": in-projection + attention forward + head-mean maps + out-projection of the 12 ViT
    # blocks (tagged at their call sites, clip/vit_engine.py) -- flops over time of the group as a whole
    grp = [(n, r) for n, r in summ.items() if n.endswith("@vit_attn")]
    group = None
    if grp and sum(r["ms"] for _, r in grp) > 0:
        gw, gms = sum(r["work"] for _, r in grp), sum(r["ms"] for _, r in grp)
        group = {"kernels": sorted(n[:-len("@vit_attn")] for n, _ in grp), "achieved": round(gw / (gms * 1e-3) / 1e12, 1),
                 "peak": 2500.0, "unit": "TFLOP/s", "frac": round(gw / (gms * 1e-3) / 2.5e15, 4),
                 "frac_of_practical_mfma_ceiling_1733": round(gw / (gms * 1e-3) / 1.733e15, 4),
                 "ms_per_step": round(gms * stride / n, 3)}
    merged = {}
    for name, r in summ.items():          # fold the tagged records back into their kernels for the per-kernel rows
        base = name.split("@")[0]
        m = merged.setdefault(base, {"ms": 0.0, "launches": 0, "work": 0.0, "est_ms": 0.0, "bytes": 0.0})
        for k in m:
            m[k] += r[k]
    summ = merged
    roofs = []
    for name, r in summ.items():
        bound, peak, unit = peak_of(name)
        sec = r["ms"] * 1e-3
        if sec <= 0:
            continue
        extra = {}
        if r["bytes"] > 0:      # kernels that report their algorithmic HBM bytes (row-streaming GEMM, deformable attention): HBM-bound
            bound, peak, unit = "hbm", 8000.0, "GB/s"
            ach = r["bytes"] / sec / 1e9
            if r["work"] > 0:
                extra = {"mfma_tflops": round(r["work"] / sec / 1e12, 1), "mfma_frac": round(r["work"] / sec / 2.5e15, 4)}
        else:
            ach = r["work"] / sec / (1e12 if bound == "mfma" else 1e9)
        roofs.append({"kernel": name, "bound": bound, "achieved": round(ach, 2), "peak": peak, "unit": unit, **extra,
                      "frac": round(ach / peak, 4), "traffic": traffic.get(name), "launches_timed": r["launches"],
                      "sampling": f"1 of {stride} instrumented launches on average (fixed pseudo-random pick), {n} eager steps",
                      "avg_launch_us": round(r["ms"] * 1e3 / max(r["launches"], 1), 2),
                      "share_of_eager_step": round(r["est_ms"] * 1e-3 / dt, 4)})
    roofs.sort(key=lambda x: -x["share_of_eager_step"])
    # the north-star group "ViT attention" = in-projection + QK^T/softmax/PV + head-mean maps + out-projection is
    # reported by the library under its own tag when the launch sites carry it (csrc/core.hip wc_prof groups)
    return roofs, {"eager_instrumented_ms_per_step": round(dt / n * 1e3, 3), "traffic_source": tsrc, "vit_attention_group": group,
                   "practical_mfma_ceiling": "1733 TFLOP/s at 1.71 GHz in-kernel clock (tools/probes/mfma_clock.hip, profiles/r02_probes.txt)"}


def encoder_leg(args, dev):
    """BASELINE configs[1]: frozen encoder forward (11 blocks + all head-mean maps), batch 32 at 512x512."""
    import torch
    from weclip_vit_comer_amd import synth
    model = make_model(dev)
    model.eval()
    img = synth.make_images(32, args.size, args.size, seed=300).to(dev)
    with torch.no_grad():
        for _ in range(2):
            model.encode(img, False)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            xs, maps, _, _ = model.encode(img, False)
        g.replay()
        torch.cuda.synchronize()
        n = 10
        t0 = time.perf_counter()
        for _ in range(n):
            g.replay()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    gf = 196.3e9 * (args.size / 512) ** 2      # 196.3 GF per image at 512^2 (approximate away from it)
    return {"value": round(32 * n / dt, 2), "unit": "images/sec", "ms_per_step": round(dt / n * 1e3, 3),
            "workload": f"ViT-B/16 encoder forward, batch 32 at {args.size}x{args.size}, maps of the last 8 of 12 layers",
            "mfma_tflops": round(32 * n * gf / dt / 1e12, 1), "frac_of_2500": round(32 * n * gf / dt / 2.5e15, 4)}


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args)
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    # WECLIP_DIST_BACKEND=gloo is a rehearsal switch: N ranks sharing the GPUs that exist (LOCAL_RANK modulo the device
    # count), gradients exchanged through the host -- exercises the launcher, rendezvous, barriers, graph capture with a
    # process group alive and the rank-0 JSON on a one-GPU box.  The measured path is RCCL ("nccl"), one rank per GPU.
    backend = os.environ.get("WECLIP_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)
        if dist.get_world_size() != world:
            sys.exit("bench.py: RCCL reports a different world size than the launcher")
    import __graft_entry__
    if rank == 0:
        __graft_entry__.build()
    if world > 1:
        dist.barrier()
    from weclip_vit_comer_amd import config
    if args.precision:
        config.precision = args.precision

    res, step, loader = run_leg(args, dev, rank, world, comer=args.comer, seg_trans=args.seg_trans, graph=not args.no_graph,
                                repeats=args.repeats if args.full else 1, diagnostics=args.full, dump_dir=args.dump_outputs)
    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    B, S, K = args.batch, args.size, args.classes_per_image
    roofs, roof_meta = ([], {})
    if args.full and args.timer_stride > 0 and args.roof_steps > 0 and world == 1:
        roofs, roof_meta = roofline_leg(args, step, loader, dev, traffic_files="r*_comer_traffic.json" if args.comer else "r*_traffic.json")
    del step, loader
    torch.cuda.empty_cache()
    out = {
        "metric": "images/sec (train fwd+bwd) ViT-B/16 512x512 VOC",
        "value": res["value"],
        "unit": "images/sec",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": res["ms_per_step"],
        "host_enqueue_ms_per_step": res["host_enqueue_ms_per_step"],
        "host_cpu_ms_per_step": res["host_cpu_ms_per_step"],
        "launch_mode": res["launch_mode"],
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": ("f16 MFMA operands / f32 accumulate, f32 residual+softmax+LN, PAR f32 arithmetic on 16-bit fixed-point "
                  "affinities (precision=fast)") if config.precision == "fast" else
                 "f16 hi+lo MFMA operands / f32 accumulate, f32 residual+softmax+LN+PAR (precision=%s)" % config.precision,
        "data": "synthetic (per-rank seeded loader: uint8 375x500 images resident on the device, random rescale / flip / "
                "crop / normalise by the HIP input-pipeline kernel inside every step; a different batch every step)",
        "config": {"workload": f"WeCLIP VOC full train step (the reference's model: frozen CLIP ViT-B/16 + adapters + decoder + "
                               f"GradCAM/affinity/PAR pseudo-labels), batch {B}/GPU at {S}x{S}, K={K} classes/image "
                               f"(BASELINE configs[2]{'/[3] DP' if world > 1 else ''}"
                               + (" with" if args.comer else " without") + " the ViT-CoMer inserts, for which the reference has no code"
                               + ("; seg-trans affinity branch" if args.seg_trans else "") + ")",
                   "global_batch": world * B, "parallelism": f"dp{world}"},
    }
    if args.full:
        out.update({k: res[k] for k in ("host_work_ms_per_step_idle_queue", "dp_check", "dp_diag", "repeat_ms_per_step",
                                        "repeat_median_ms", "repeat_min_ms", "repeat_max_ms")})
        out.update({"roofline": roofs[0] if roofs else None, "roofline_other": roofs[1:]}, **roof_meta)
    if args.full and world == 1 and not args.no_extras:
        few = max(4, min(10, args.steps))
        if not args.seg_trans:
            r, _, _ = run_leg(args, dev, rank, world, seg_trans=True, steps=few, warmup=2)
            out["seg_trans_branch"] = r
            torch.cuda.empty_cache()
        if config.precision == "fast":
            config.precision = "exact"
            try:
                r, _, _ = run_leg(args, dev, rank, world, steps=few, warmup=2)
                r["dtype"] = "f16 hi+lo MFMA operands / f32 accumulate, f32 PAR (precision=exact)"
                out["exact_precision"] = r
            finally:
                config.precision = "fast"
            torch.cuda.empty_cache()
        if config.precision == "fast" and config.par_q16:
            # the PAR compression alone: fp16 single-pass GEMMs as in the headline, but PAR on fp32 affinities like the reference
            config.par_q16 = False
            try:
                r, _, _ = run_leg(args, dev, rank, world, steps=few, warmup=2)
                r["dtype"] = "f16 MFMA operands / f32 accumulate (precision=fast), PAR on fp32 affinities (WECLIP_PAR_F16=0)"
                out["fast_gemm_fp32_par"] = r
            finally:
                config.par_q16 = True
            torch.cuda.empty_cache()
        if not args.comer:
            r, cstep, cloader = run_leg(args, dev, rank, world, comer=True, steps=few, warmup=2)
            r["note"] = "BASELINE configs[2] as written (+ ViT-CoMer inserts); parity unpinned: the reference ships no CoMer code"
            if args.timer_stride > 0 and args.roof_steps > 0:
                # the inserts' own kernels against their rooflines: the deformable-attention gathers and the
                # row-streaming GEMM of the 86 016 x 256 x 256 Linear layers report ALGORITHMIC bytes (nL * nP * 4 corner rows of dh
                # values per (query, head); A + side input + outputs once) -> achieved GB/s of the 8 TB/s HBM peak; the GEMM also
                # its TFLOP/s.  Same HIP-event pairs at the library's launch sites as the main roofline.
                croofs, cmeta = roofline_leg(args, cstep, cloader, dev, traffic_files="r*_comer_traffic.json")
                r["traffic_source"] = cmeta["traffic_source"]
                keep = ("msda_", "gemm_row_kernel", "mrfp_", "ln_bwd", "gemm_km")
                r["roofline"] = [x for x in croofs if x["kernel"].startswith(keep)]
                r["eager_instrumented_ms_per_step"] = cmeta["eager_instrumented_ms_per_step"]
            del cstep, cloader
            out["with_comer"] = r
            torch.cuda.empty_cache()
        out["encoder_only_b32"] = encoder_leg(args, dev)
        torch.cuda.empty_cache()
    if args.full and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args)
    print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
