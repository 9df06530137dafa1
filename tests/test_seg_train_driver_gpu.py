"""GPU tests of the supervised variant's training driver (`train.py --dataset seg`) on the tiny synthetic CLIP and a VOC tree
written with Pillow: LoggedSupervisedTrainStep against the parent step, the driver against a hand-written loop over
DeviceLoader + SupervisedTrainStep, its log output and host synchronisations, Validator.run on the seg-only model, checkpoint /
resume, --reg_loss with the loader's img_box, and the command line with one process and with two ranks."""
import glob
import math
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import dataset_trees as DT
from oracle import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = 21
TRAIN_SIZES = [(70, 90), (131, 64), (64, 64), (97, 150), (75, 111), (66, 81), (90, 70), (64, 100), (120, 77), (83, 83), (71, 139),
               (101, 68)]
VAL_SIZES = [(70, 90), (75, 111), (70, 90), (97, 150), (131, 69)]          # three and more distinct sizes, none a multiple of 16

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
  max_iters: {max_iters}
  cam_iters: 2000
  eval_iters: {eval_iters}
  log_iters: {log_iters}
val:
  split: val
optimizer:
  type: AdamW
  learning_rate: 2e-4
  betas: [0.9, 0.999]
  weight_decay: 0.01
scheduler:
  warmup_iter: 50
  warmup_ratio: 1e-6
  power: 1.0
clip_init:
  clip_pretrain_path: {clip}
  embedding_dim: 256
  in_channels: [64, 64, 64, 64]
"""


def _write_voc(root):
    """Ground-truth masks with two object classes per image, a 255 border column and a 255 outline row."""
    from PIL import Image
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "SegmentationClassAug"))
    lists = os.path.join(root, "lists")
    os.makedirs(lists)
    onehot = {}
    for split, sizes in (("train", TRAIN_SIZES), ("val", VAL_SIZES)):
        names = []
        for i, (H, W) in enumerate(sizes):
            name = f"{split}_{i:04d}"
            Image.fromarray(DT.smooth_image(H, W, 60 + i)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=92)
            lab = np.zeros((H, W), np.uint8)
            lab[H // 5:H // 2, W // 6:] = 1 + (3 * i) % 20
            lab[H // 2:, :W // 2] = 1 + (7 * i + 5) % 20
            lab[:, :2] = 255
            lab[H // 2, :] = 255
            Image.fromarray(lab).save(os.path.join(root, "SegmentationClassAug", name + ".png"))
            onehot[name] = DT.onehot20(lab)
            names.append(name)
        with open(os.path.join(lists, split + ".txt"), "w") as f:
            f.write("\n".join(names) + "\n")
    np.save(os.path.join(lists, "cls_labels_onehot.npy"), onehot)
    return root, lists


def _cfg(tmp, root, lists, max_iters=6, eval_iters=1000, log_iters=3, clip="none", work="work"):
    from weclip_vit_comer_amd import train as T
    path = os.path.join(tmp, f"cfg_{work}.yaml")
    with open(path, "w") as f:
        f.write(YAML.format(root=root, lists=lists, work=os.path.join(tmp, work), max_iters=max_iters, eval_iters=eval_iters,
                            log_iters=log_iters, clip=clip))
    return path, T.load_config(path, crop_size=64)


def _args(path, *more):
    from weclip_vit_comer_amd import train as T
    return T.build_parser().parse_args(["--config", path, "--dataset", "seg", "--crop_size", "64", "--threads", "2", *more])


def _model(train=True):
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc_seg import WeCLIP
    sd = synth.make_clip_state_dict(**synth.TINY)
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
    m = WeCLIP(num_classes=NC, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4, device="cuda")
    m.decoder_fts_fuse.load_state_dict(fuse)
    m.decoder.load_state_dict(dec)
    return m.train() if train else m.eval()


def _params(model):
    return torch.cat([p.detach().flatten() for p in model.get_param_groups()[3]]).clone()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("seg_driver"))
    root, lists = _write_voc(os.path.join(tmp, "voc"))
    return tmp, root, lists


class _Once:
    """Results computed once per module and shared by its tests; dropped (models, trainers, captured graphs) with the module."""

    def __init__(self):
        self._done = {}

    def __call__(self, fn, *args):
        key = (fn.__name__,) + args
        if key not in self._done:
            self._done[key] = fn(*args)
        return self._done[key]

    def clear(self):
        self._done.clear()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def once():
    o = _Once()
    yield o
    o.clear()


class _Syncs:
    """Counts the synchronisation warnings torch raises inside the block (torch.cuda.set_sync_debug_mode("warn"))."""

    def __enter__(self):
        self.n = 0
        self._cm = warnings.catch_warnings(record=True)
        self._log = self._cm.__enter__()
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        return self

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        self.n = sum("synchroniz" in str(w.message).lower() for w in self._log)
        self._cm.__exit__(*exc)


# ---------------------------------------------------------------------------------------------- the logged step
STEP_SEEDS = [11, 12, 13, 14]


def _step_labels(seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, NC, (2, 64, 64), generator=g)
    lab[:, :3] = 255
    lab[1, :, -5:] = 255
    return lab


def _run_steps(kind, graph):
    """tests/test_seg_variant_gpu.py's seeding (_run_steps there): torch.manual_seed(0), the model in eval mode."""
    from weclip_vit_comer_amd import train as T
    from weclip_vit_comer_amd.train_step import SupervisedTrainStep
    from weclip_vit_comer_amd.validate import step_pair_hist

    class Probe(T.LoggedSupervisedTrainStep):              # keeps the step's logits (graph mode: the replayed graph's own tensor)
        def loss(self, seg, label):
            self.seg = seg.detach()
            return super().loss(seg, label)
    torch.manual_seed(0)
    m = _model(train=False)
    step = (SupervisedTrainStep if kind == "parent" else Probe)(m, graph=graph)
    losses, hists = [], []
    for s in STEP_SEEDS:
        img = synth.make_images(2, 64, 64, seed=s).cuda()
        lab = _step_labels(s).cuda()
        losses.append(step(img, lab).item())
        if kind != "parent":
            eager = step_pair_hist(step.seg.float().contiguous(), lab, NC, torch.zeros(NC, NC, device="cuda", dtype=torch.int64))
            hists.append((step.hist.clone(), eager, int(((lab >= 0) & (lab < NC)).sum()), step.ce.item()))
            step.hist.zero_()
    return losses, _params(m), step, hists


@pytest.mark.parametrize("graph", [False, True])
def test_logged_step_equals_parent_and_counts_every_step(once, graph):
    ref_losses, ref_params, _, _ = once(_run_steps, "parent", graph)
    losses, params, step, hists = once(_run_steps, "logged", graph)
    print(f"graph {graph}: losses {losses}; per-step counted pixels {[int(h.sum()) for h, _, _, _ in hists]}")
    if graph:
        assert len(step._graphs) == 1 and next(iter(step._graphs.values()))["graph"] is not None
    assert losses == ref_losses and len(set(losses)) == 4 and all(np.isfinite(losses))
    assert torch.equal(params, ref_params)
    for (hist, eager, valid, ce), loss in zip(hists, losses):
        assert int(hist.sum()) == valid and 0 < valid < 2 * 64 * 64      # ignored pixels are in no cell; graph mode: captured
        assert torch.equal(hist, eager)
        assert ce == loss
    # eager and graph replay are bit-identical, as the parent's are
    other = once(_run_steps, "logged", not graph)
    assert losses == other[0] and torch.equal(params, other[1])
    assert all(torch.equal(a[0], b[0]) for a, b in zip(hists, other[3]))


# ---------------------------------------------------------------------------------------------- the driver
def _driver_run(tmp, root, lists, graph):
    from weclip_vit_comer_amd import train as T
    path, cfg = _cfg(tmp, root, lists, work=f"drv{int(graph)}")
    tr = T.Trainer(cfg, _args(path, "--graph" if graph else "--no-graph"), model=_model(), timestamp="t")
    recs = []
    for _ in range(3):
        tr.step_once()
    with _Syncs() as log_syncs:
        recs.append(tr.log())
    with _Syncs() as syncs:
        tr.step_once()
        tr.step_once()
    tr.step_once()
    recs.append(tr.log())
    tr.close()
    with open(tr.metrics_path) as f:
        assert "NaN" not in f.read()
    return recs, _params(tr.model), syncs.n, log_syncs.n, tr


def _hand_run(tmp, root, lists, graph):
    """DeviceLoader + the parent's SupervisedTrainStep, written out; a probe keeps each step's logits for the histograms."""
    from weclip_vit_comer_amd import train as T
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12SegDataset
    from weclip_vit_comer_amd.train_step import SupervisedTrainStep, make_optimizer
    from weclip_vit_comer_amd.utils.evaluate import scores_from_hist
    from weclip_vit_comer_amd.validate import step_pair_hist

    class Probe(SupervisedTrainStep):
        def loss(self, seg, label):
            self.seg = seg.detach()
            return super().loss(seg, label)
    model = _model()
    T.setup_seed(1)
    ds = VOC12SegDataset(root_dir=root, name_list_dir=lists, split="train", stage="train", aug=True, crop_size=64, img_fliplr=True,
                         ignore_index=255)
    loader = DeviceLoader(ds, batch_size=2, shuffle=True, drop_last=True, seed=1, threads=2, prefetch=2)
    opt = make_optimizer(model, lr=2e-4, weight_decay=0.01, betas=(0.9, 0.999), warmup_iter=50, max_iter=6, warmup_ratio=1e-6, power=1.0)
    step = Probe(model, opt, ignore_index=255, graph=graph)

    def batches():
        while True:
            for b in loader:
                yield b[1], b[2]
    it = batches()
    windows, losses, syncs = [], [], None
    hist = torch.zeros(NC, NC, device="cuda", dtype=torch.int64)
    for n in range(1, 7):
        if n == 4:
            syncs = _Syncs().__enter__()
        inputs, labels = next(it)
        loss = step(inputs, labels)
        if n == 5:
            syncs.__exit__(None, None, None)
        assert labels.dtype == torch.int64 and labels.is_cuda and int((labels == 255).sum()) > 0
        losses.append(loss.double().item())
        step_pair_hist(step.seg.float().contiguous(), labels, NC, hist)
        if n % 3 == 0:
            h = hist.cpu().numpy()
            score = scores_from_hist(h)
            windows.append({"iter": n, "lr": opt.param_groups[0]["lr"], "losses": losses, "hist_sum": int(h.sum()),
                            "pAcc": float(score["pAcc"]), "mAcc": float(score["mAcc"]), "miou": float(score["miou"])})
            hist.zero_()
            losses = []
    it.close()
    return windows, _params(model), syncs.n


@pytest.mark.parametrize("graph", [False, True])
def test_driver_equals_hand_written_loop(tree, once, graph):
    """Same seeds, same graph setting: the LR and the parameters after step 6 are bit-equal (the driver adds no arithmetic to
    the step).  The logged seg_loss is the window mean: the driver sums the three fp32 losses on the device in fp32, so it
    lies within 3 fp32 roundings of the fp64 mean of the loop's own losses.  pAcc / mAcc / miou are integer counts through
    the same host function: equal to `scores_from_hist` of the loop's per-step histograms summed over the window."""
    from weclip_vit_comer_amd import train as T
    recs, params, _, _, tr = once(_driver_run, *tree, graph)
    windows, ref_params, _ = once(_hand_run, *tree, graph)
    if graph:
        assert any(e["graph"] is not None for e in tr.step._graphs.values())
    for r, w in zip(recs, windows):
        print(f"graph {graph} iter {r['iter']}: driver {r}  loop {w}")
    assert [r["iter"] for r in recs] == [3, 6]
    for r, w in zip(recs, windows):
        assert sorted(r) == ["iter", "lr", "mAcc", "miou", "pAcc", "seg_loss"]
        mean = sum(w["losses"]) / 3
        assert np.isfinite(r["seg_loss"]) and abs(r["seg_loss"] - mean) <= 3 * 2.0 ** -23 * abs(mean)
        assert (r["iter"], r["lr"]) == (w["iter"], w["lr"])
        assert (r["pAcc"], r["mAcc"], r["miou"]) == (w["pAcc"], w["mAcc"], w["miou"])
        assert 0.0 <= r["pAcc"] <= 1.0 and 0 < w["hist_sum"] < 3 * 2 * 64 * 64
    assert torch.equal(params, ref_params)
    assert T.read_metrics(tr.metrics_path) == recs
    assert int(tr.step.hist.sum()) == 0                                  # zeroed behind the read


def test_log_line_carries_the_window_scores(tree, once):
    recs, _, _, _, tr = once(_driver_run, *tree, True)
    # (the logger has no file handler here: format the line from the record as Trainer._seg_log does)
    from weclip_vit_comer_amd import train as T
    r = recs[-1]
    line = T.format_seg_log_line(r["iter"], "0:00:01", "0:00:00", r["lr"], r["seg_loss"], r["pAcc"], r["mAcc"], r["miou"])
    assert line.startswith("Iter: 6; Elasped: 0:00:01; ETA: 0:00:00; LR: ")
    assert line.endswith("seg_loss: %.4f, seg_pAcc: %.4f, seg_mAcc: %.4f, seg_mIoU: %.4f" % (r["seg_loss"], r["pAcc"], r["mAcc"], r["miou"]))


def test_driver_host_synchronisations(tree, once):
    """Steps 4..5 (replays: no log line, no capture) under torch.cuda.set_sync_debug_mode("warn"): the driver raises no
    synchronisation warning at all (the hand-written loop raises its own: it reads every loss and checks its labels on the
    host), and a log line is ONE host read."""
    _, _, driver_syncs, log_syncs, _ = once(_driver_run, *tree, True)
    _, _, loop_syncs = once(_hand_run, *tree, True)
    print(f"sync warnings over steps 4..5: driver {driver_syncs}, hand-written loop {loop_syncs}; in one log line {log_syncs}")
    assert driver_syncs == 0 and driver_syncs <= loop_syncs
    assert log_syncs == 1
    with _Syncs() as probe:                     # the instrument itself: a host read is counted
        torch.zeros(1, device="cuda").item()
    assert probe.n >= 1


# ---------------------------------------------------------------------------------------------- validation
def _validation(tmp, root, lists):
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12SegDataset
    from weclip_vit_comer_amd.msc_flip import resize_argmax
    from weclip_vit_comer_amd.utils import evaluate
    from weclip_vit_comer_amd.validate import Validator
    model = _model()
    ds = VOC12SegDataset(root_dir=root, name_list_dir=lists, split="val", stage="train", aug=False, ignore_index=255)
    ref = torch.zeros(NC, NC, device="cuda", dtype=torch.int64)
    sizes = []
    model.eval()
    with torch.no_grad():
        for _, inputs, labels, _ in DeviceLoader(ds, 1, shuffle=False, threads=2):
            seg = model(inputs, mode="val")
            gt = labels[0].contiguous()
            evaluate.confusion_hist(gt, resize_argmax(seg[0].float().contiguous(), tuple(gt.shape)), NC, out=ref)
            sizes.append(tuple(gt.shape))
    model.train()
    v = Validator(model, NC)
    scores = v.run(DeviceLoader(ds, 1, shuffle=False, threads=2))
    return v, scores, ref, sizes, model.training


def test_validator_on_the_seg_only_model(tree, once):
    from weclip_vit_comer_amd.utils import evaluate
    v, (seg_score, cam_score), ref, sizes, training = once(_validation, *tree)
    print(f"seg-only val: {v.images} images of sizes {sizes}, hist sum {int(v.seg_hist.sum())}, miou {seg_score['miou']:.4f}")
    assert v.images == 5 and len(set(sizes)) >= 3 and all(h % 16 and w % 16 for h, w in sizes)
    assert cam_score is None and v.has_cam is False and v.cam_hist_host is None and int(v.cam_hist.sum()) == 0
    assert training is True
    assert torch.equal(v.seg_hist, ref) and int(ref.sum()) > 0
    np.testing.assert_equal(seg_score, evaluate.scores_from_hist(ref.cpu().numpy()))


# ---------------------------------------------------------------------------------------------- checkpoints
def _tiny_clip(tmp):
    clip = os.path.join(tmp, "tiny_clip.pt")
    if not os.path.exists(clip):
        torch.save(synth.make_clip_state_dict(**synth.TINY), clip)
    return clip


def test_checkpoint_pair_loads_strict_and_evaluates_and_resume(tree):
    from weclip_vit_comer_amd import train as T
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.msc_flip import MscFlipEvaluator
    tmp, root, lists = tree
    path, cfg = _cfg(tmp, root, lists, max_iters=4, eval_iters=2, log_iters=2, clip=_tiny_clip(tmp), work="ckpt")
    a = T.Trainer(cfg, _args(path, "--save_after", "0", "--no-graph"), model=_model(), timestamp="t")
    a.fit(until=2)
    model2, state2 = T.checkpoint_paths(cfg.work_dir.ckpt_dir, 2)
    assert os.path.isfile(model2) and os.path.isfile(state2) and a.n_iter == 2
    at2 = dict(iter_num=a.model.iter_num, epoch=a.train_loader.epoch, global_step=a.opt.global_step,
               opt=[{k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.opt.state[p].items()} for p in a.step.bucket.params])
    assert at2["iter_num"] == 2 + len(a.val_dataset)
    a.step_once()
    lr3 = a.opt.param_groups[0]["lr"]
    a.fit()
    assert a.n_iter == 4
    assert sorted(os.listdir(cfg.work_dir.ckpt_dir)) == ["WeCLIP_model_iter_2.pth", "WeCLIP_model_iter_4.pth", "train_state_iter_2.pth",
                                                         "train_state_iter_4.pth"]
    vals = T.read_metrics(a.val_metrics_path)
    assert [v["iter"] for v in vals] == [2, 4] and vals[0]["cam"] is None and vals[0]["cam_hist_sum"] is None
    assert vals[0]["seg_hist_sum"] > 0 and 0.0 <= vals[0]["seg"]["pAcc"] <= 1.0
    # the model file is what `msc_flip_eval --dataset seg` loads: strict, into build_model(cfg, "seg")
    fresh = T.build_model(cfg, "seg")
    fresh.load_state_dict(torch.load(T.checkpoint_paths(cfg.work_dir.ckpt_dir, 4)[0], map_location="cpu"), strict=True)
    assert torch.equal(_params(fresh), _params(a.model))
    fresh.eval()
    ev = MscFlipEvaluator(fresh, NC, scales=(1.0, 0.75), resize_long=96)
    _, inputs, labels, _ = next(iter(DeviceLoader(a.val_dataset, 1, shuffle=False, threads=2)))
    pred, msc_pred = ev.add(inputs, labels)
    assert tuple(pred.shape) == tuple(labels.shape[1:]) == tuple(msc_pred.shape) and 0 <= int(pred.min()) and int(pred.max()) < NC
    assert int(ev.hist.sum()) == int(((labels >= 0) & (labels < NC)).sum()) > 0
    # resume from iteration 2 in another work_dir
    path_b, cfg_b = _cfg(tmp, root, lists, max_iters=4, eval_iters=2, log_iters=2, work="ckpt_resumed")
    b = T.Trainer(cfg_b, _args(path_b, "--save_after", "0", "--no-graph", "--resume", model2), model=_model(), timestamp="t")
    assert (b.n_iter, b.model.iter_num, b.train_loader.epoch, b.opt.global_step) == (2, at2["iter_num"], at2["epoch"], at2["global_step"])
    saved = torch.load(model2, map_location="cuda")
    assert all(torch.equal(v, saved[k]) for k, v in b.model.state_dict().items())
    for p, ref in zip(b.step.bucket.params, at2["opt"]):
        st = b.opt.state[p]
        assert set(st) == set(ref) == {"step", "exp_avg", "exp_avg_sq"}
        for k in ref:
            assert torch.equal(st[k].cpu(), ref[k].cpu()), k
    b.step_once()
    assert b.n_iter == 3 and b.opt.param_groups[0]["lr"] == lr3
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- --reg_loss
@pytest.mark.parametrize("graph", [False, True])
def test_reg_loss_runs_on_the_loaders_img_box(tree, graph):
    from weclip_vit_comer_amd import train as T
    from weclip_vit_comer_amd.data import DeviceSegAugment
    tmp, root, lists = tree
    path, cfg = _cfg(tmp, root, lists, max_iters=3, log_iters=3, work=f"reg{int(graph)}")
    tr = T.Trainer(cfg, _args(path, "--reg_loss", "--reg_start", "0", "--reg_scale", "0.5", "--graph" if graph else "--no-graph"),
                   model=_model(), timestamp="t")
    assert tr.reg == {"coef": 0.01, "scale_factor": 0.5, "start_iter": 0} and tr.acc.numel() == 3
    seen = {}

    class Spy(type(tr.step)):                                            # what the step is called with
        def __call__(self, img, target, img_box=None, names=None):
            seen["box"] = img_box
            return super().__call__(img, target, img_box, names)
    tr.step.__class__ = Spy
    for _ in range(3):
        out = tr.step_once()
        loader = tr.train_loader
        box = loader.last_img_box
        assert seen["box"] is box and box.is_cuda and box.dtype == torch.int32 and tuple(box.shape) == (2, 4)
        sel = loader.aug.sel.cpu().numpy()
        ref = np.stack([DeviceSegAugment.img_box(d, 64, sel[b, :2]) for b, d in enumerate(loader.last_draws)])
        assert np.array_equal(box.cpu().numpy(), ref)
        assert (ref[:, 0] < ref[:, 1]).all() and (ref[:, 2] < ref[:, 3]).all()
        assert len(out) == 2
    rec = tr.log()
    tr.close()
    print(f"graph {graph}: {rec}")
    assert sorted(rec) == ["iter", "lr", "mAcc", "miou", "pAcc", "reg_loss", "seg_loss"]
    assert math.isfinite(rec["reg_loss"]) and rec["reg_loss"] != 0.0 and math.isfinite(rec["seg_loss"])
    assert T.read_metrics(tr.metrics_path) == [rec]


def test_other_loader_kinds_have_no_img_box(tree):
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset, VOC12SegDataset
    _, root, lists = tree
    val = DeviceLoader(VOC12SegDataset(root_dir=root, name_list_dir=lists, split="val", stage="train", aug=False), 1, shuffle=False,
                       threads=2)
    assert val.last_img_box is None
    batch = next(iter(val))
    assert len(batch) == 4 and val.last_img_box is None
    cls = DeviceLoader(VOC12ClsDataset(root_dir=root, name_list_dir=lists, split="train", stage="train", aug=True, crop_size=64,
                                       resize_range=[512, 2048], rescale_range=[0.5, 2.0], num_classes=21), 2, threads=2)
    batch = next(iter(cls))
    assert len(batch) == 4 and cls.last_img_box is None


# ---------------------------------------------------------------------------------------------- the command line
def _cli_env(**more):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **more)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def test_cli_one_process(tree):
    from weclip_vit_comer_amd import train as T
    tmp, root, lists = tree
    path, cfg = _cfg(tmp, root, lists, max_iters=4, eval_iters=4, log_iters=2, clip=_tiny_clip(tmp), work="cli")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "weclip_vit_comer_amd.train", "--config", path, "--dataset", "seg",
           "--crop_size", "64", "--threads", "2", "--max_iters", "4", "--save_after", "0"]
    r = subprocess.run(cmd, env=_cli_env(), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    work = cfg.work_dir.dir
    logs = glob.glob(os.path.join(work, "*.log"))
    assert len(logs) == 1
    with open(logs[0]) as f:
        text = f.read()
    assert text.count("seg_loss: ") == 2 and "seg_mIoU: " in text and "segs score:" in text
    assert "cams score:" not in text and "pseudo_seg" not in text
    recs = T.read_metrics(os.path.join(work, "metrics.jsonl"))
    assert [m["iter"] for m in recs] == [2, 4] and all(math.isfinite(m["seg_loss"]) and 0.0 <= m["pAcc"] <= 1.0 for m in recs)
    vals = T.read_metrics(os.path.join(work, "val_metrics.jsonl"))
    assert len(vals) == 1 and vals[0]["iter"] == 4 and vals[0]["cam"] is None and vals[0]["seg_hist_sum"] > 0
    assert len(glob.glob(os.path.join(work, "checkpoints", "*", "WeCLIP_model_iter_4.pth"))) == 1


def test_cli_two_ranks_share_the_gpu(tree):
    """`python -m torch.distributed.run --nproc-per-node 2 -m weclip_vit_comer_amd.train --dataset seg` with the gloo rehearsal
    backend (pattern and environment of tests/test_train_driver_gpu.py): 2 steps and one validation."""
    from weclip_vit_comer_amd import train as T
    tmp, root, lists = tree
    path, cfg = _cfg(tmp, root, lists, max_iters=2, eval_iters=2, log_iters=1, clip=_tiny_clip(tmp), work="dp")
    dump = os.path.join(tmp, "rank_dumps")
    os.makedirs(dump)
    env = _cli_env(WECLIP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", WECLIP_TRAIN_RANK_DUMP=dump)
    with socket.socket() as sock:                # a port that is free now
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), "-m", "weclip_vit_comer_amd.train", "--config", path, "--dataset", "seg",
           "--crop_size", "64", "--threads", "2", "--max_iters", "2", "--save_after", "0"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d0, d1 = (torch.load(os.path.join(dump, f"rank{k}.pth"), map_location="cpu") for k in (0, 1))
    assert (d0["rank"], d1["rank"], d0["iter"], d1["iter"]) == (0, 1, 2, 2) and d0["model_iter_num"] == d1["model_iter_num"] == 2 + 5
    assert torch.isfinite(d0["params"]).all() and torch.equal(d0["params"], d1["params"])
    # the all-reduced validation histogram: the same on both ranks, every valid val pixel counted once
    assert torch.equal(d0["seg_hist"], d1["seg_hist"]) and int(d0["cam_hist"].sum()) == 0
    valid = sum(H * W - 2 * H - (W - 2) for H, W in VAL_SIZES)          # the 255 column pair and the 255 row of _write_voc
    assert int(d0["seg_hist"].sum()) == valid
    work = cfg.work_dir.dir
    assert len(glob.glob(os.path.join(work, "*.log"))) == 1 and len(os.listdir(os.path.join(work, "checkpoints"))) == 1
    assert [m["iter"] for m in T.read_metrics(os.path.join(work, "metrics.jsonl"))] == [1, 2]
    assert len(T.read_metrics(os.path.join(work, "val_metrics.jsonl"))) == 1
    assert sorted(os.listdir(dump)) == ["rank0.pth", "rank1.pth"]
