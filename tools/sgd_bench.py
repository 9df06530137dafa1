"""What does the optimizer step cost?  The trainable parameters of the VOC model (get_param_groups()[3], 5,985,045 fp32) with
their gradients in `GradBucket` layout, one process, three contenders alternated window by window:

  (s) utils.optimizer.PolyWarmupSGD on its HIP path (csrc/sgd_ops.hip, one launch);
  (a) utils.optimizer.PolyWarmupAdamW on its HIP path (csrc/train_ops.hip, one launch): the in-tree yardstick;
  (t) torch.optim.SGD(momentum=0.9, foreach=True) with the same lr written into its group before every step.

HIP events around windows of --steps steps after --warmup steps, median of --repeats windows: microseconds per optimizer step as
the training loop sees it (host enqueue and kernels, whichever is longer).  For the new kernel alone, back-to-back launches of
`wc_sgd_multi` on the same table give its device time, and 20 bytes x elements over that time its traffic rate, next to the
HBM rates of the MI355X (8.0 TB/s specified, 6.29 TB/s measured with a float4 copy).

    python tools/sgd_bench.py [--json profiles/sgd_bench.json]

Needs the GPU; there is no fall-back."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29
SCHED = dict(warmup_iter=50, max_iter=30000, power=1.0)


def window_us(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def stats(vals):
    return {"us": round(statistics.median(vals), 2), "min": round(min(vals), 2), "max": round(max(vals), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sgd_bench.json"))
    args = ap.parse_args()
    import torch
    import bench
    from weclip_vit_comer_amd import _lib as L
    from weclip_vit_comer_amd.train_step import GradBucket
    from weclip_vit_comer_amd.utils.optimizer import PolyWarmupAdamW, PolyWarmupSGD
    assert torch.cuda.is_available(), "sgd_bench needs the GPU"
    model = bench.make_model("cuda")
    shapes = [tuple(p.shape) for p in model.get_param_groups()[3] if p.requires_grad]
    del model
    torch.cuda.empty_cache()

    def param_set(seed):
        gen = torch.Generator().manual_seed(seed)
        ps = [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.02).cuda()) for s in shapes]
        bucket = GradBucket(ps)
        bucket.flat.copy_(torch.randn(bucket.flat.numel(), generator=gen) * 1e-3)
        return ps, bucket
    kw = dict(lr=2e-3, weight_decay=0.01, betas=[0.9, 0.999], warmup_ratio=1e-6, **SCHED)
    ps_s, keep_s = param_set(1)
    ps_a, keep_a = param_set(2)
    ps_t, keep_t = param_set(3)
    sgd, adamw = PolyWarmupSGD(ps_s, **kw), PolyWarmupAdamW(ps_a, **kw)
    plain = torch.optim.SGD(ps_t, lr=2e-3, momentum=0.9, weight_decay=0.01, foreach=True)
    tstep = [0]

    def plain_step():
        s = tstep[0]
        if s < SCHED["warmup_iter"]:
            plain.param_groups[0]["lr"] = 2e-3 * (1 - s / SCHED["warmup_iter"]) ** SCHED["power"] * 10
        elif s < SCHED["max_iter"]:
            plain.param_groups[0]["lr"] = 2e-3 * (1 - (s - SCHED["warmup_iter"]) / (SCHED["max_iter"] - SCHED["warmup_iter"])) ** SCHED["power"]
        plain.step()
        tstep[0] += 1
    contenders = {"PolyWarmupSGD (HIP)": sgd.step, "PolyWarmupAdamW (HIP)": adamw.step, "torch.optim.SGD(foreach=True)": plain_step}
    assert sgd._hip_ok() and adamw._hip_ok()
    for fn in contenders.values():
        for _ in range(args.warmup):
            fn()
    assert len(sgd._hip) == 1 and len(adamw._hip) == 1            # both took their one-launch path
    times = {k: [] for k in contenders}
    for _ in range(args.repeats):
        for k, fn in contenders.items():
            times[k].append(window_us(torch, fn, args.steps))

    # the kernel alone: back-to-back launches on the class's own table (lr 0 would leave the parameters alone but also change
    # nothing else about the traffic; the real lr is used, on parameters nobody reads afterwards)
    st = sgd._hip[0]
    table, count, stream = L.ptr(st["table"], torch.int64, "table"), st["count"], L.stream()
    launch = lambda: L.lib().wc_sgd_multi(table, count, 2e-3, 0.9, 0.01, 64, stream)      # noqa: E731
    for _ in range(args.warmup):
        launch()
    kernel = [window_us(torch, launch, args.steps) for _ in range(args.repeats)]
    elements = sum(p.numel() for p in ps_s)
    k_us = statistics.median(kernel)
    tbs = 20.0 * elements / (k_us * 1e-6) / 1e12
    out = {"device": torch.cuda.get_device_name(0), "tensors": len(shapes), "elements": elements, "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats, "us_per_optimizer_step": {k: stats(v) for k, v in times.items()},
           "sgd_multi_kernel": dict(stats(kernel), bytes_per_element=20, tb_per_s=round(tbs, 3),
                                    of_hbm_spec=round(tbs / HBM_SPEC_TBS, 3), of_hbm_copy=round(tbs / HBM_COPY_TBS, 3),
                                    note="device time of back-to-back launches: an upper bound of the kernel's own time")}
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    del keep_s, keep_a, keep_t


if __name__ == "__main__":
    main()
