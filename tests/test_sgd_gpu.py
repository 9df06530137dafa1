"""GPU tests of the SGD path: `wc_sgd_multi` (csrc/sgd_ops.hip) on both kernel paths against the fp64 restatement of
tests/sgd_ref.py within its derived bounds (4 u A_buf, 7 u A_p; the code under test is never the yardstick), `PolyWarmupSGD`
over five scheduled steps on gradients laid out like `GradBucket`, state interchange with torch.optim.SGD in both directions,
`TrainStep` with make_optimizer(type="SGD") eager against graph replay, and the training driver with `optimizer.type: SGD`
(log line, checkpoint pair, resume, and the refusal of a state of the other optimizer)."""
import glob
import os

import pytest
import torch

import dataset_trees as DT
from oracle import synth
from tests import sgd_ref as S

pytestmark = pytest.mark.gpu

F64, F32, I64, U8 = torch.float64, torch.float32, torch.int64, torch.uint8
GUARD = 64              # guard words either side of every written allocation
H, W = synth.TINY_HW
WORST = {}              # path -> worst err / bound seen


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """Prints the worst err / bound per kernel path after the module (visible with -s)."""
    yield
    print()
    for k in sorted(WORST):
        print(f"WORST {k}: {WORST[k]:.3g}")


def _L():
    from weclip_vit_comer_amd import _lib as L
    return L


def _bits(t):
    return t.contiguous().view(-1).view(U8)


def _check(path, what, got, ref, bound):
    got = got.double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{path} {what}: elements not finite"
    err = (got - ref).abs()
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print(f"{path} {what}: err / bound {ratio:.3g}")
    if (err > bound).any():
        i = int(torch.argmax(err - bound))
        raise AssertionError(f"{path} {what}: {int((err > bound).sum())} of {err.numel()} elements outside the bound, worst err / bound "
                             f"{ratio:.3g}; at {i}: got {got[i]:.9g} ref {ref[i]:.9g}")
    WORST[path] = max(WORST.get(path, 0.0), ratio)


def _check_step(tag, k, got_p, got_buf, before, grp):
    """One step of tensor k from `before` = (p, g, buf) fp32 on the host, against the fp64 step from those same values."""
    po, bo, A_p, A_buf = S.sgd(*before, **grp)
    bp, bb = S.sgd_bounds(A_p, A_buf)
    _check(S.sgd_path(k) + " p", f"{tag} n={po.numel()}", got_p, po, bp)
    _check(S.sgd_path(k) + " buf", f"{tag} n={po.numel()}", got_buf, bo, bb)


def _guarded(values):
    """values (n,) fp32 on the host -> (allocation of GUARD + n + GUARD words, 0xFF bytes around the values; the view of them)."""
    n = values.numel()
    t = torch.empty(n + 2 * GUARD, dtype=F32, device="cuda")
    t.view(U8).fill_(255)
    t[GUARD:GUARD + n] = values.cuda()
    return t, t[GUARD:GUARD + n]


def _guards_intact(name, t, n):
    assert int((_bits(t[:GUARD]) != 255).sum()) == 0, f"{name}: written in front of element 0"
    assert int((_bits(t[GUARD + n:]) != 255).sum()) == 0, f"{name}: written behind element {n - 1}"


# ---------------------------------------------------------------------------------------------------------------------
# the C entry, one step

@pytest.mark.parametrize("fresh", [True, False], ids=["zero_buffer", "nonzero_buffer"])
@pytest.mark.parametrize("gi", [0, 1])
def test_sgd_multi_one_step(gi, fresh):
    """All five sizes in one table (three on the 16-byte path, two on the scalar one: a size that is no multiple of 4 and a
    gradient at a 4-byte offset), a zero buffer (torch's first step) and a non-zero one."""
    grp = S.SGD_GROUPS[gi]
    host = [S.sgd_inputs(n, seed=gi, fresh=fresh) for n in S.SGD_SIZES]
    rows, held = [], []
    for k, (p, g, buf) in enumerate(host):
        n = p.numel()
        off = 1 if k == 4 else 0                              # the last tensor's grad: a view at a 4-byte offset
        gb = torch.zeros(n + 4, device="cuda")
        gb[off:off + n] = g.cuda()
        gd = gb[off:off + n]
        pa, pv = _guarded(p)
        ba, bv = _guarded(buf)
        assert GUARD % 4 == 0 and pv.data_ptr() % 16 == 0 and bv.data_ptr() % 16 == 0 and gd.data_ptr() % 16 == 4 * off
        vector = n % 4 == 0 and off == 0
        assert vector == S.SGD_VECTOR[k]
        rows.append([pv.data_ptr(), gd.data_ptr(), bv.data_ptr(), n, 0, 0, 0, 0])
        held.append((pa, pv, ba, bv, gd))
    table = torch.tensor(rows, dtype=I64).cuda()
    _L().lib().wc_sgd_multi(_L().ptr(table), len(rows), grp["lr"], S.MOMENTUM, grp["weight_decay"], 64, _L().stream())
    torch.cuda.synchronize()
    for k, ((p, g, buf), (pa, pv, ba, bv, gd)) in enumerate(zip(host, held)):
        n = p.numel()
        _guards_intact(f"p of tensor {k}", pa, n)
        _guards_intact(f"momentum_buffer of tensor {k}", ba, n)
        assert torch.equal(_bits(gd.cpu()), _bits(g)), f"grad of tensor {k} changed"
        _check_step(f"group {gi} {'zero' if fresh else 'non-zero'} buffer", k, pv.cpu(), bv.cpu(), (p, g, buf), grp)
        if fresh:                 # mu * 0 + g' is g' exactly: the first step needs no flag
            assert torch.equal(bv.cpu(), S.sgd(p, g, buf, dt=F32, **grp)[1])


# ---------------------------------------------------------------------------------------------------------------------
# the class, five scheduled steps

def _bucket_layout(sizes, misaligned):
    """Offsets of a flat gradient buffer laid out like GradBucket (every tensor on a 16-byte start), except tensor
    `misaligned`, which starts one element further."""
    offs, off = [], 0
    for k, n in enumerate(sizes):
        if k == misaligned:
            off += 1
        offs.append(off)
        off = (off + n + 3) & ~3
    return offs, off


def test_poly_warmup_sgd_five_steps():
    """Five steps (three of warm-up, then the decay) in two groups.  Every step is checked on its own: the fp64 reference steps
    from the state the device held before it (read back bit for bit) with the lr of the restated schedule, so that the one-step
    bounds apply to every step and no drift model is needed.  The pointer table is rebuilt exactly when a .grad is replaced."""
    from weclip_vit_comer_amd.utils.optimizer import PolyWarmupSGD
    host = [S.sgd_inputs(n, seed=5) for n in S.SGD_SIZES]
    ps = [torch.nn.Parameter(p.cuda()) for p, _, _ in host]
    split = (0, 1, 0, 1, 1)
    groups = [dict(params=[p for p, s in zip(ps, split) if s == gi], **S.SGD_GROUPS[gi]) for gi in (0, 1)]
    sched = dict(warmup_iter=3, max_iter=100, power=0.9)
    opt = PolyWarmupSGD(groups, lr=1e-3, weight_decay=0.01, betas=[0.9, 0.999], warmup_ratio=1e-6, **sched)
    offs, total = _bucket_layout(S.SGD_SIZES, misaligned=4)
    flat = torch.zeros(total + 4, device="cuda")
    assert flat.data_ptr() % 16 == 0
    for k, p in enumerate(ps):
        p.grad = flat[offs[k]:offs[k] + p.numel()]
        assert p.grad.data_ptr() % 16 == (4 if k == 4 else 0)
    tables, versions = None, [p._version for p in ps]
    for it in range(5):
        gen = torch.Generator().manual_seed(100 + it)
        grads = []
        for k, p in enumerate(ps):
            g = torch.randn(p.numel(), generator=gen) * (0.1 + it)
            g[it::7] = 0.0
            grads.append(g)
            if it == 3 and k == 2:        # a replaced .grad (same values elsewhere): the table of ITS group must be rebuilt
                p.grad = g.cuda()
            else:
                p.grad.copy_(g)           # new values in the same memory: no rebuild
        before = []
        for k, p in enumerate(ps):
            mb = opt.state[p].get("momentum_buffer") if len(opt.state[p]) else None
            before.append((p.detach().cpu(), grads[k], torch.zeros(p.numel()) if mb is None else mb.cpu()))
        assert opt._hip_ok()
        opt.step()
        torch.cuda.synchronize()
        now = [opt._hip[gi]["table"] for gi in (0, 1)]
        if tables is not None:
            assert (now[0] is tables[0]) == (it != 3), f"step {it + 1}: group 0's table"
            assert now[1] is tables[1], f"step {it + 1}: group 1's table was rebuilt"
        tables = now
        assert opt.global_step == it + 1
        for k, p in enumerate(ps):
            gi = split[k]
            lr = S.sgd_lr(S.SGD_GROUPS[gi]["lr"], it, **sched)
            assert opt.param_groups[gi]["lr"] == lr
            assert set(opt.state[p]) == {"momentum_buffer"}
            assert torch.equal(_bits(p.grad.cpu()), _bits(grads[k])), f"step {it + 1}: grad of tensor {k} changed"
            assert p._version > versions[k], f"step {it + 1}: version counter of tensor {k} not bumped"
            versions[k] = p._version
            _check_step(f"PolyWarmupSGD step {it + 1}", k, p.detach().cpu(), opt.state[p]["momentum_buffer"].cpu(), before[k],
                        dict(S.SGD_GROUPS[gi], lr=lr))
    assert opt.param_groups[0]["lr"] < S.SGD_GROUPS[0]["lr"] < S.sgd_lr(S.SGD_GROUPS[0]["lr"], 0, **sched)     # warm-up ran at 10x


# ---------------------------------------------------------------------------------------------------------------------
# state_dict in both directions

def _pair(device):
    from weclip_vit_comer_amd.utils.optimizer import PolyWarmupSGD
    sizes = (2 * 16384 + 5, 4096)
    ps = [torch.nn.Parameter(S.sgd_inputs(n, seed=9)[0].to(device)) for n in sizes]
    groups = [dict(params=[p], **grp) for p, grp in zip(ps, S.SGD_GROUPS)]
    return ps, PolyWarmupSGD(groups, lr=1e-3, weight_decay=0.01, betas=[0.9, 0.999], warmup_iter=1, max_iter=50, warmup_ratio=1e-6,
                             power=0.9)


def _grads(ps, it):
    gen = torch.Generator().manual_seed(300 + it)
    return [torch.randn(p.numel(), generator=gen) for p in ps]


@pytest.mark.parametrize("first", ["hip", "torch"])
def test_state_interop_with_torch_sgd(first):
    """Two steps on one side (the HIP path, or stock torch on CPU fp32), its state_dict() loaded into the other side (a plain
    torch.optim.SGD on CPU; PolyWarmupSGD on the GPU), then one more step on each side from the same gradients: both are fp32
    evaluations of one step from the same state: each lies within the one-step bound of the fp64 step, and the two sides agree
    within that bound as well."""
    from weclip_vit_comer_amd.utils.optimizer import PolyWarmupSGD
    ps, opt = _pair("cuda" if first == "hip" else "cpu")
    for it in range(2):
        for p, g in zip(ps, _grads(ps, it)):
            p.grad = g.to(p.device)
        assert opt._hip_ok() == (first == "hip")
        opt.step()
    sd = opt.state_dict()
    assert all(set(s) == {"momentum_buffer"} for s in sd["state"].values()) and len(sd["state"]) == 2
    if first == "hip":
        qs = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
        other = torch.optim.SGD([dict(params=[q]) for q in qs], lr=1e-3, momentum=0.9)
        other.load_state_dict(sd)                                   # groups (lr as scheduled at step 2, wd, momentum) and buffers
    else:
        qs, other = _pair("cuda")
        for q, p in zip(qs, ps):
            q.data.copy_(p.detach())
        other.load_state_dict(sd)
        other.global_step = opt.global_step
        assert isinstance(other, PolyWarmupSGD)
    for q, p in zip(qs, ps):
        assert torch.equal(other.state[q]["momentum_buffer"].cpu(), opt.state[p]["momentum_buffer"].cpu())
    before = [(p.detach().cpu().clone(), g, opt.state[p]["momentum_buffer"].cpu().clone()) for p, g in zip(ps, _grads(ps, 2))]
    for side, params in ((opt, ps), (other, qs)):
        for p, (_, g, _) in zip(params, before):
            p.grad = g.to(p.device)
        if not isinstance(side, PolyWarmupSGD):                       # the plain SGD has no schedule: it is handed the step's lr
            for go, gs in zip(side.param_groups, opt.param_groups):
                go["lr"] = gs["lr"]
        side.step()
    torch.cuda.synchronize()
    hip_side = opt if first == "hip" else other
    assert len(hip_side._hip) == 2
    for k, (p, q) in enumerate(zip(ps, qs)):
        lr = opt.param_groups[k]["lr"]
        assert other.param_groups[k]["lr"] == lr and lr == S.sgd_lr(S.SGD_GROUPS[k]["lr"], 2, 1, 50, 0.9)
        po, bo, A_p, A_buf = S.sgd(*before[k], lr=lr, weight_decay=S.SGD_GROUPS[k]["weight_decay"])
        bp, bb = S.sgd_bounds(A_p, A_buf)
        path = "sgd_multi_kernel (" + ("vector" if p.numel() % 4 == 0 else "scalar") + ")"
        for side, t in ((opt, p), (other, q)):
            what = f"state interop ({first} first) " + ("hip" if side is hip_side else "torch") + " side"
            _check(path + " p", what, t.detach().cpu(), po, bp)
            _check(path + " buf", what, side.state[t]["momentum_buffer"].cpu(), bo, bb)
        # the two sides against each other, within the one-step bound
        _check("hip vs torch, " + path + " p", f"state interop ({first} first)", p.detach().cpu(), q.detach().cpu().double(), bp)
        _check("hip vs torch, " + path + " buf", f"state interop ({first} first)", opt.state[p]["momentum_buffer"].cpu(),
               other.state[q]["momentum_buffer"].cpu().double(), bb)


# ---------------------------------------------------------------------------------------------------------------------
# the training step, eager against graph replay

BATCHES = [(11, [[3, 7], [0, 14]]), (12, [[1, 2], [5, 19]]), (13, [[4, 6], [8, 9]]), (14, [[3, 7], [10, 11]]),
           (15, [[0, 1], [2, 3]])]


def _tiny_model():
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP
    sd = synth.make_clip_state_dict(**synth.TINY)
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
    m = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4, dataset_root_path=None,
               device="cuda", text_features=(bg.cuda(), fg.cuda()))
    m.decoder_fts_fuse.load_state_dict(fuse)
    m.decoder.load_state_dict(dec)
    return m.eval()          # eval: no Dropout2d, so eager and replayed steps see the same arithmetic


def _run_steps(kind, graph):
    from weclip_vit_comer_amd.train_step import TrainStep, make_optimizer
    torch.manual_seed(0)
    m = _tiny_model()
    opt = make_optimizer(m, type=kind)
    step = TrainStep(m, optimizer=opt, graph=graph)
    losses, grads = [], []
    for seed, labels in BATCHES:
        out = step(synth.make_images(2, H, W, seed=seed).cuda(), labels=labels)
        losses.append(torch.stack(out).cpu())
        grads.append(step.bucket.flat.clone())
    return losses, grads, torch.cat([p.detach().flatten() for p in m.get_param_groups()[3]]), step


def test_train_step_with_sgd_graph_replay_equals_eager():
    from weclip_vit_comer_amd.utils.optimizer import PolyWarmupSGD
    le, ge, pe, se = _run_steps("SGD", False)
    lg, gg, pg, sg = _run_steps("SGD", True)
    assert isinstance(se.opt, PolyWarmupSGD) and se.opt.global_step == sg.opt.global_step == len(BATCHES)
    assert len(sg._graphs) == 1 and next(iter(sg._graphs.values()))["graph"] is not None
    assert all(torch.isfinite(l).all() for l in le) and torch.isfinite(pe).all()
    for a, b in zip(le, lg):
        assert torch.equal(a, b), (le, lg)
    for a, b in zip(ge, gg):
        assert torch.equal(a, b)
    assert torch.equal(pe, pg)
    # the bucket's views ARE the table's grad pointers, and their 16-byte starts put every tensor whose size is a multiple of
    # four on the vector path (an odd-sized one, the 21-class bias, takes the scalar path: its size decides, not its start)
    for step in (se, sg):
        params = [p for p in step.opt.param_groups[3]["params"] if p.grad is not None]
        assert [id(p) for p in params] == [id(p) for p in step.bucket.params]
        table = step.opt._hip[3]["table"].cpu()
        assert sorted(step.opt._hip) == [3] and table.shape == (len(params), 8)
        lo = step.bucket.flat.data_ptr()
        for row, p, off in zip(table.tolist(), params, step.bucket.offsets):
            buf = step.opt.state[p]["momentum_buffer"]
            assert row == [p.data_ptr(), lo + 4 * off, buf.data_ptr(), p.numel(), 0, 0, 0, 0]
            assert row[1] == p.grad.data_ptr() and row[0] % 16 == row[1] % 16 == row[2] % 16 == 0
            assert set(step.opt.state[p]) == {"momentum_buffer"}
        assert any(p.numel() % 4 for p in params) and sum(p.numel() % 4 == 0 for p in params) > len(params) // 2
    # and it is another optimizer than the default one
    la, _, pa, sa = _run_steps("AdamW", False)
    assert torch.equal(la[0], le[0]) and not torch.equal(pa, pe)
    assert "exp_avg" in sa.opt.state[sa.bucket.params[0]]


# ---------------------------------------------------------------------------------------------------------------------
# the driver

YAML = """\
dataset:
  root_dir: {root}
  name_list_dir: {lists}
  num_classes: 21
  crop_size: 320
  resize_range: [512, 2048]
  rescale_range: [0.5, 2.0]
  ignore_index: 255
work_dir:
  dir: {work}
  ckpt_dir: checkpoints
  pred_dir: predictions
  segs_dir: segs
  tb_logger_dir: tb_logger
train:
  split: train
  samples_per_gpu: 2
  max_iters: 4
  cam_iters: 2000
  eval_iters: 2
  log_iters: 2
val:
  split: val
optimizer:
  type: SGD
  learning_rate: 2e-4
{betas}  weight_decay: 0.01
scheduler:
  warmup_iter: 3
  warmup_ratio: 1e-6
  power: 0.9
clip_init:
  clip_pretrain_path: {clip}
  embedding_dim: 256
  in_channels: [64, 64, 64, 64]
  text_features: {text}
"""


def _trainable(model):
    return torch.cat([p.detach().flatten() for p in model.get_param_groups()[3]]).cpu()


def test_driver_trains_checkpoints_and_resumes_with_sgd(tmp_path, golden):
    """`python -m weclip_vit_comer_amd.train` (its main(), in this process) on the synthetic VOC tree with `optimizer.type: SGD`
    and no `betas`: four iterations at crop 64 and batch 2, log and checkpoint pairs at 2 and 4.  A trainer resumed from the
    pair of iteration 2 holds the uninterrupted run's parameters and momentum buffers of that iteration bit for bit and goes on
    under the same schedule (the dropout and augmentation streams restart on a resume, as train.Trainer.resume says, so the
    later iterations are not compared).  The same files under --optimizer AdamW are refused."""
    from weclip_vit_comer_amd import train as T
    tmp = str(tmp_path)
    root, lists, _ = DT.write_voc_tree(os.path.join(tmp, "voc"), golden("dataset_ragged_ref.npz"))
    clip, text = os.path.join(tmp, "tiny_clip.pt"), os.path.join(tmp, "text_rows.pt")
    torch.save(synth.make_clip_state_dict(**synth.TINY), clip)
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    torch.save({"bg": bg, "fg": fg}, text)

    def config(work, betas=""):
        path = os.path.join(tmp, f"cfg_{work}.yaml")
        with open(path, "w") as f:
            f.write(YAML.format(root=root, lists=lists, work=os.path.join(tmp, work), clip=clip, text=text, betas=betas))
        return path
    argv = ["--crop_size", "64", "--threads", "2", "--save_after", "0"]
    handlers = list(T.LOG.handlers)
    try:
        assert T.main(["--config", config("run"), *argv]) == 0
    finally:
        for h in [h for h in T.LOG.handlers if h not in handlers]:
            T.LOG.removeHandler(h)
            h.close()
    work = os.path.join(tmp, "run")
    logs = glob.glob(os.path.join(work, "*.log"))
    assert len(logs) == 1
    with open(logs[0]) as f:
        text_log = f.read()
    first = text_log.split("args:")[0]
    assert "optimizer: SGD" in first and "Iter:" not in first and text_log.count("pseudo_seg_loss: ") == 2
    assert [m["iter"] for m in T.read_metrics(os.path.join(work, "metrics.jsonl"))] == [2, 4]
    ckpt, = glob.glob(os.path.join(work, "checkpoints", "*"))
    assert sorted(os.listdir(ckpt)) == ["WeCLIP_model_iter_2.pth", "WeCLIP_model_iter_4.pth", "train_state_iter_2.pth",
                                        "train_state_iter_4.pth"]
    model2, state2 = T.checkpoint_paths(ckpt, 2)
    st2 = torch.load(state2, map_location="cpu", weights_only=False)
    st4 = torch.load(T.checkpoint_paths(ckpt, 4)[1], map_location="cpu", weights_only=False)
    assert st2["optimizer_type"] == st4["optimizer_type"] == "SGD" and (st2["global_step"], st4["global_step"]) == (2, 4)
    states = list(st2["optimizer"]["state"].values())
    assert states and all(set(s) == {"momentum_buffer"} for s in states)           # no exp_avg: the YAML's type was honoured
    assert all(torch.isfinite(s["momentum_buffer"]).all() and s["momentum_buffer"].abs().max() > 0 for s in states)
    assert all(g["momentum"] == 0.9 for g in st2["optimizer"]["param_groups"])
    # resume from the middle, in another work_dir
    cfg_path = config("resumed")
    cfg = T.load_config(cfg_path, crop_size=64)
    args = T.build_parser().parse_args(["--config", cfg_path, *argv, "--resume", model2])
    b = T.Trainer(cfg, args, timestamp="t")
    assert b.optimizer_type == "SGD" and (b.n_iter, b.opt.global_step) == (2, 2)
    saved = torch.load(model2, map_location="cpu")
    assert all(torch.equal(v.cpu(), saved[k]) for k, v in b.model.state_dict().items())
    params = b.step.bucket.params
    assert len(params) == len(states)
    for p, s in zip(params, states):
        assert set(b.opt.state[p]) == {"momentum_buffer"}
        assert torch.equal(_bits(b.opt.state[p]["momentum_buffer"].cpu()), _bits(s["momentum_buffer"]))
    b.step_once()
    assert b.n_iter == 3 and b.opt.param_groups[3]["lr"] == S.sgd_lr(2e-4 * 10, 2, 3, 4, 0.9)
    assert sorted(b.opt._hip) == [3] and torch.isfinite(_trainable(b.model)).all()
    b.close()
    # the same files under the other optimizer (which needs its betas)
    cfg2_path = config("refused", betas="  betas: [0.9, 0.999]\n")
    args2 = T.build_parser().parse_args(["--config", cfg2_path, *argv, "--resume", model2, "--optimizer", "AdamW"])
    with pytest.raises(RuntimeError, match="optimizer SGD.*configured for AdamW"):
        T.Trainer(T.load_config(cfg2_path, crop_size=64), args2, timestamp="t")
