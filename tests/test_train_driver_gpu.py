"""GPU tests of the training driver (weclip_vit_comer_amd.train / .validate) on the tiny synthetic CLIP and trees written
with Pillow: the driver against a hand-written loop over DeviceLoader + the parent's TrainStep, its host synchronisations,
Validator.run against resize_argmax + confusion_hist, checkpoint / resume, and two ranks sharing the GPU through the CLI."""
import glob
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dataset_trees as DT
from oracle import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_SIZES = [(70, 90), (131, 64), (64, 64), (97, 150), (75, 111), (66, 81), (90, 70), (64, 100), (120, 77), (83, 83), (71, 139),
               (101, 68)]
VAL_SIZES = [(70, 90), (75, 111), (70, 90), (97, 150), (131, 69)]          # three and more distinct sizes, none a multiple of 16

YAML = """\
dataset:
  root_dir: {root}
  name_list_dir: {lists}
  num_classes: {nc}
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
{extra}"""


def _write_voc(root):
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
            Image.fromarray(DT.smooth_image(H, W, 30 + i)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=92)
            lab = np.zeros((H, W), np.uint8)
            lab[H // 5:H // 2, W // 6:] = 1 + (3 * i) % 20
            lab[H // 2:, :W // 2] = 1 + (7 * i + 5) % 20
            lab[:, :2] = 255
            Image.fromarray(lab).save(os.path.join(root, "SegmentationClassAug", name + ".png"))
            onehot[name] = DT.onehot20(lab)
            names.append(name)
        with open(os.path.join(lists, split + ".txt"), "w") as f:
            f.write("\n".join(names) + "\n")
    np.save(os.path.join(lists, "cls_labels_onehot.npy"), onehot)
    return root, lists


def _cfg(tmp, root, lists, nc=21, max_iters=6, eval_iters=1000, log_iters=3, clip="none", extra="", work="work"):
    from weclip_vit_comer_amd import train as T
    path = os.path.join(tmp, f"cfg_{work}.yaml")
    with open(path, "w") as f:
        f.write(YAML.format(root=root, lists=lists, nc=nc, work=os.path.join(tmp, work), max_iters=max_iters, eval_iters=eval_iters,
                            log_iters=log_iters, clip=clip, extra=extra))
    return path, T.load_config(path, crop_size=64)


def _args(path, *more):
    from weclip_vit_comer_amd import train as T
    return T.build_parser().parse_args(["--config", path, "--crop_size", "64", "--threads", "2", *more])


def _model(kind="voc"):
    if kind == "voc":
        from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP
        nc, n_fg, seed = 21, 20, {}
    else:
        from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_coco import WeCLIP
        nc, n_fg, seed = 81, 80, {"seed": 3}
    sd = synth.make_clip_state_dict(**synth.TINY)
    bg, fg = synth.make_text_features(n_fg, 25, synth.TINY["embed_dim"])
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"], num_classes=nc, **seed)
    m = WeCLIP(num_classes=nc, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4, dataset_root_path=None,
               device="cuda", text_features=(bg.cuda(), fg.cuda()))
    m.decoder_fts_fuse.load_state_dict(fuse)
    m.decoder.load_state_dict(dec)
    return m


def _params(model):
    return torch.cat([p.detach().flatten() for p in model.get_param_groups()[3]]).clone()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("driver"))
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


def _torch_macc(seg, cam):
    """The reference's expression (scripts/dist_clip_voc.py:250, 274-277) and the fraction of near-tie pixels."""
    up = F.interpolate(seg.float(), size=cam.shape[1:], mode="bilinear", align_corners=False)
    top = up.topk(2, dim=1).values
    return ((up.argmax(1) == cam).sum() / cam.numel()).item(), ((top[:, 0] - top[:, 1]) < 1e-4).float().mean().item()


def _driver_run(tmp, root, lists, graph):
    from weclip_vit_comer_amd import train as T
    path, cfg = _cfg(tmp, root, lists, work=f"drv{int(graph)}")
    tr = T.Trainer(cfg, _args(path, "--graph" if graph else "--no-graph"), model=_model(), timestamp="t")
    recs = []
    for _ in range(3):
        tr.step_once()
    recs.append(tr.log())
    with _Syncs() as syncs:
        tr.step_once()
        tr.step_once()
    tr.step_once()
    recs.append(tr.log())
    tr.close()
    return recs, _params(tr.model), syncs.n, tr


def _hand_run(tmp, root, lists, graph):
    """DeviceLoader + the parent's TrainStep, written out: what INTEGRATION.md section A tells a user to write."""
    from weclip_vit_comer_amd import train as T
    from weclip_vit_comer_amd.datasets import DeviceLoader, labels_from_onehot
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset
    from weclip_vit_comer_amd.train_step import TrainStep, make_optimizer

    class Probe(TrainStep):                     # keeps the step's seg / cam (in graph mode: the replayed graph's own tensors)
        def losses(self, seg, cam, attn_pred):
            self.seg, self.cam = seg.detach(), cam
            return super().losses(seg, cam, attn_pred)
    model = _model().train()
    T.setup_seed(1)
    ds = VOC12ClsDataset(root_dir=root, name_list_dir=lists, split="train", stage="train", aug=True, resize_range=[512, 2048],
                         rescale_range=[0.5, 2.0], crop_size=64, img_fliplr=True, ignore_index=255, num_classes=21)
    loader = DeviceLoader(ds, batch_size=2, shuffle=True, drop_last=True, seed=1, threads=2, prefetch=2)
    opt = make_optimizer(model, lr=2e-4, weight_decay=0.01, betas=(0.9, 0.999), warmup_iter=50, max_iter=6, warmup_ratio=1e-6, power=1.0)
    step = Probe(model, opt, radius=8, ignore_index=255, graph=graph)

    def batches():
        while True:
            for b in loader:
                yield b[1], labels_from_onehot(loader.last_cls_labels)
    it = batches()
    windows, acc, syncs = [], torch.zeros(3, device="cuda"), None
    for n in range(1, 7):
        if n == 4:
            syncs = _Syncs().__enter__()
        inputs, labels = next(it)
        acc.add_(torch.stack(step(inputs, labels=labels)))
        if n == 5:
            syncs.__exit__(None, None, None)
        if n % 3 == 0:
            s = acc.double().cpu().tolist()
            macc, ties = _torch_macc(step.seg, step.cam)
            windows.append({"iter": n, "lr": opt.param_groups[0]["lr"], "seg_loss": s[1] / 3, "attn_loss": s[2] / 3,
                            "pseudo_seg_mAcc": macc, "ties": ties})
            acc.zero_()
    it.close()
    return windows, _params(model), syncs.n


@pytest.mark.parametrize("graph", [False, True])
def test_driver_equals_hand_written_loop(tree, once, graph):
    """Same seeds, same graph setting: window means of the losses, the LR and the parameters after step 6 are bit-equal
    (tests/test_graph_step_gpu.py:52-55 asserts bit equality between step forms: the driver adds no arithmetic to the step, so
    the same rule holds).  pseudo_seg_mAcc is compared with the torch expression on the loop's own seg / cam: the kernel and
    ATen may order a pixel's two largest logits differently only where they lie within fp32 rounding of each other, so the two
    fractions differ by at most the fraction of pixels whose top-2 gap is below 1e-4 (measured in the same run)."""
    recs, params, _, tr = once(_driver_run, *tree, graph)
    windows, ref_params, _ = once(_hand_run, *tree, graph)
    if graph:
        assert any(e["graph"] is not None for e in tr.step._graphs.values())
    for r, w in zip(recs, windows):
        print(f"graph {graph} iter {r['iter']}: driver {r}  loop {w}")
    assert [r["iter"] for r in recs] == [3, 6]
    for r, w in zip(recs, windows):
        assert np.isfinite(r["seg_loss"]) and np.isfinite(r["attn_loss"])
        assert (r["iter"], r["lr"], r["seg_loss"], r["attn_loss"]) == (w["iter"], w["lr"], w["seg_loss"], w["attn_loss"])
        assert abs(r["pseudo_seg_mAcc"] - w["pseudo_seg_mAcc"]) <= w["ties"] + 1e-12
        assert w["ties"] <= 0.01 and 0.0 <= r["pseudo_seg_mAcc"] <= 1.0
    assert torch.equal(params, ref_params)
    from weclip_vit_comer_amd import train as T
    assert T.read_metrics(tr.metrics_path) == recs


def test_driver_adds_no_host_synchronisation(tree, once):
    """Steps 4..5 (replays: no log line, no capture) under torch.cuda.set_sync_debug_mode("warn"): the driver raises no more
    synchronisation warnings than the hand-written loop over the parent's TrainStep, measured in the same process."""
    _, _, driver_syncs, _ = once(_driver_run, *tree, True)
    _, _, loop_syncs = once(_hand_run, *tree, True)
    print(f"sync warnings over steps 4..5: driver {driver_syncs}, hand-written loop {loop_syncs}")
    assert driver_syncs <= loop_syncs
    with _Syncs() as probe:                     # the instrument itself: a host read is counted
        torch.zeros(1, device="cuda").item()
    assert probe.n >= 1


def _val_reference(model, ds, nc):
    """The loop the parent commit offers: model in 'val', resize_argmax + confusion_hist per leg, maps kept for the host."""
    from weclip_vit_comer_amd.datasets import DeviceLoader, labels_from_onehot
    from weclip_vit_comer_amd.msc_flip import resize_argmax
    from weclip_vit_comer_amd.utils import evaluate
    seg_hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
    cam_hist = torch.zeros(nc, nc, device="cuda", dtype=torch.int64)
    gts, preds, cams = [], [], []
    model.eval()
    loader = DeviceLoader(ds, 1, shuffle=False, threads=2)
    with torch.no_grad():
        for _, inputs, labels, _ in loader:
            seg, cam, _ = model(inputs, [""], mode="val", labels=labels_from_onehot(loader.last_cls_labels))
            gt = labels[0].contiguous()
            pred = resize_argmax(seg[0].float().contiguous(), tuple(gt.shape))
            evaluate.confusion_hist(gt, pred, nc, out=seg_hist)
            gts.append(gt.cpu().numpy())
            preds.append(pred.cpu().numpy())
            if cam is not None:
                cam = (cam[0] if isinstance(cam, (list, tuple)) else cam.reshape(gt.shape)).contiguous()
                evaluate.confusion_hist(gt, cam, nc, out=cam_hist)
                cams.append(cam.cpu().numpy())
    _, seg_score = evaluate.scores(gts, preds, np.zeros((nc, nc)), num_classes=nc)
    cam_score = evaluate.scores(gts, cams, np.zeros((nc, nc)), num_classes=nc)[1] if cams else None
    return seg_hist, cam_hist, seg_score, cam_score


def _voc_validation(tmp, root, lists):
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12SegDataset
    from weclip_vit_comer_amd.validate import Validator
    model = _model()
    ds = VOC12SegDataset(root_dir=root, name_list_dir=lists, split="val", stage="train", aug=False, ignore_index=255, num_classes=21)
    assert len(ds) == 5
    ref = _val_reference(model, ds, 21)
    model.eval()
    v = Validator(model, 21)
    scores = v.run(DeviceLoader(ds, 1, shuffle=False, threads=2))
    return v, scores, ref, model.training


def test_validator_equals_resize_argmax_plus_confusion_hist_voc(tree, once):
    v, (seg_score, cam_score), (ref_seg, ref_cam, ref_seg_score, ref_cam_score), training = once(_voc_validation, *tree)
    print(f"VOC val: {v.images} images, seg hist sum {int(v.seg_hist.sum())}, cam hist sum {int(v.cam_hist.sum())}, "
          f"seg miou {seg_score['miou']:.4f} cam miou {cam_score['miou']:.4f}")
    assert v.images == 5 and training is True
    assert torch.equal(v.seg_hist, ref_seg) and torch.equal(v.cam_hist, ref_cam)
    assert int(ref_seg.sum()) == int(ref_cam.sum()) > 0
    np.testing.assert_equal(seg_score, ref_seg_score)
    np.testing.assert_equal(cam_score, ref_cam_score)


def test_validator_coco_has_no_cam_score(tmp_path):
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.coco import CocoSegDataset
    from weclip_vit_comer_amd.validate import Validator
    root, lists, _ = DT.write_coco_tree(str(tmp_path / "coco"))
    ds = CocoSegDataset(root_dir=root, name_list_dir=lists, split="val", stage="val", aug=False, ignore_index=255, num_classes=81)
    model = _model("coco")
    ref_seg, _, ref_seg_score, ref_cam_score = _val_reference(model, ds, 81)
    v = Validator(model, 81)
    seg_score, cam_score = v.run(DeviceLoader(ds, 1, shuffle=False, threads=2))
    assert cam_score is None and ref_cam_score is None and model.training
    assert torch.equal(v.seg_hist, ref_seg) and int(v.cam_hist.sum()) == 0 and int(ref_seg.sum()) > 0
    np.testing.assert_equal(seg_score, ref_seg_score)


def test_checkpoint_and_resume(tree):
    from weclip_vit_comer_amd import train as T
    tmp, root, lists = tree
    path, cfg = _cfg(tmp, root, lists, max_iters=4, eval_iters=2, log_iters=2, work="ckpt")
    a = T.Trainer(cfg, _args(path, "--save_after", "0", "--no-graph"), model=_model(), timestamp="t")
    a.fit(until=2)
    model2, state2 = T.checkpoint_paths(cfg.work_dir.ckpt_dir, 2)
    assert os.path.isfile(model2) and os.path.isfile(state2) and a.n_iter == 2
    at2 = dict(iter_num=a.model.iter_num, epoch=a.train_loader.epoch, global_step=a.opt.global_step,
               opt=[{k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.opt.state[p].items()} for p in a.step.bucket.params])
    assert at2["iter_num"] == 2 + len(a.val_dataset)                  # the validation's forwards are counted, as in the reference
    a.step_once()
    lr3 = a.opt.param_groups[0]["lr"]
    a.fit()
    assert a.n_iter == 4
    assert sorted(os.listdir(cfg.work_dir.ckpt_dir)) == ["WeCLIP_model_iter_2.pth", "WeCLIP_model_iter_4.pth", "train_state_iter_2.pth",
                                                         "train_state_iter_4.pth"]
    for n in (2, 4):
        fresh = _model()
        fresh.load_state_dict(torch.load(T.checkpoint_paths(cfg.work_dir.ckpt_dir, n)[0], map_location="cpu"), strict=True)
    assert torch.equal(_params(fresh), _params(a.model))               # iteration 4's file holds the final parameters
    vals = T.read_metrics(a.val_metrics_path)
    assert [v["iter"] for v in vals] == [2, 4] and vals[0]["cam"] is not None and vals[0]["seg_hist_sum"] == vals[0]["cam_hist_sum"]
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
    b.close()


def test_two_ranks_share_the_gpu_through_the_cli(tree, once):
    """`python -m torch.distributed.run --nproc-per-node 2 -m weclip_vit_comer_amd.train` with the gloo rehearsal backend
    (pattern and environment of tests/test_bench_dp_gpu.py): 2 steps and one validation."""
    from weclip_vit_comer_amd import train as T
    tmp, root, lists = tree
    clip = os.path.join(tmp, "tiny_clip.pt")
    torch.save(synth.make_clip_state_dict(**synth.TINY), clip)
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    text = os.path.join(tmp, "text_rows.pt")
    torch.save({"bg": bg, "fg": fg}, text)
    path, cfg = _cfg(tmp, root, lists, max_iters=2, eval_iters=2, log_iters=1, clip=clip, extra=f"  text_features: {text}\n", work="dp")
    dump = os.path.join(tmp, "rank_dumps")
    os.makedirs(dump)
    env = dict(os.environ, WECLIP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", WECLIP_TRAIN_RANK_DUMP=dump,
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    with socket.socket() as sock:                # a port that is free now, as bench.py picks its own
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(port), "-m", "weclip_vit_comer_amd.train", "--config", path, "--crop_size", "64", "--threads", "2", "--save_after", "0"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d0, d1 = (torch.load(os.path.join(dump, f"rank{k}.pth"), map_location="cpu") for k in (0, 1))
    assert (d0["rank"], d1["rank"], d0["iter"], d1["iter"]) == (0, 1, 2, 2) and d0["model_iter_num"] == d1["model_iter_num"] == 2 + 5
    assert torch.isfinite(d0["params"]).all() and torch.equal(d0["params"], d1["params"])
    # what rank 0 saved is what rank 1 holds
    work = cfg.work_dir.dir
    ckpts = glob.glob(os.path.join(work, "checkpoints", "*", "WeCLIP_model_iter_2.pth"))
    assert len(ckpts) == 1
    fresh = _model()
    fresh.load_state_dict(torch.load(ckpts[0], map_location="cpu"), strict=True)
    assert torch.equal(_params(fresh).cpu(), d1["params"])
    # the all-reduced validation histograms: the same on both ranks, and as many pixels as one process counts
    assert torch.equal(d0["seg_hist"], d1["seg_hist"]) and torch.equal(d0["cam_hist"], d1["cam_hist"])
    single = once(_voc_validation, *tree)[0]
    assert int(d0["seg_hist"].sum()) == int(single.seg_hist.sum()) and int(d0["cam_hist"].sum()) == int(single.cam_hist.sum())
    # one log, one checkpoint directory, one line per logged step: rank 0 alone wrote
    assert len(glob.glob(os.path.join(work, "*.log"))) == 1 and len(os.listdir(os.path.join(work, "checkpoints"))) == 1
    assert [m["iter"] for m in T.read_metrics(os.path.join(work, "metrics.jsonl"))] == [1, 2]
    assert len(T.read_metrics(os.path.join(work, "val_metrics.jsonl"))) == 1
    assert sorted(os.listdir(dump)) == ["rank0.pth", "rank1.pth"]
