"""GPU tests of the evaluation entry point (weclip_vit_comer_amd.msc_flip_eval) on the tiny synthetic CLIP and trees written
with Pillow: `MscFlipEvaluator.logits` with and without its new arguments, `SplitEvaluator` against the parent's
`MscFlipEvaluator.add` / `add_with_crf` loop, the files it writes, its host synchronisations, and the command line in one
process and on two ranks sharing the GPU."""
import json
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import dataset_trees as DT
from oracle import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAL_SIZES = [(70, 90), (75, 111), (70, 90), (97, 150), (131, 69)]          # three and more distinct sizes, none a multiple of 16
RESIZE_LONG, SCALES = 128, (1.0, 0.75)
CRF = dict(iter_max=2, pos_xy_std=3, pos_w=3, bi_xy_std=64, bi_rgb_std=5, bi_w=4)      # the reference's, with fewer iterations

YAML = """\
dataset:
  root_dir: {root}
  name_list_dir: {lists}
  num_classes: 21
  ignore_index: 255
clip_init:
  clip_pretrain_path: {clip}
  embedding_dim: 256
  in_channels: [64, 64, 64, 64]
  text_features: {text}
"""


def _write_voc(root):
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "SegmentationClassAug"))
    lists = os.path.join(root, "lists")
    os.makedirs(lists)
    names, onehot = [], {}
    for i, (H, W) in enumerate(VAL_SIZES):
        name = f"val_{i:04d}"
        Image.fromarray(DT.smooth_image(H, W, 30 + i)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=92)
        lab = np.zeros((H, W), np.uint8)
        lab[H // 5:H // 2, W // 6:] = 1 + (3 * i) % 20
        lab[H // 2:, :W // 2] = 1 + (7 * i + 5) % 20
        lab[:, :2] = 255
        Image.fromarray(lab).save(os.path.join(root, "SegmentationClassAug", name + ".png"))
        onehot[name] = DT.onehot20(lab)
        names.append(name)
    # what a model built with dataset_root_path reads for the image name "" that MscFlipEvaluator.logits passes
    Image.fromarray(lab).save(os.path.join(root, "SegmentationClassAug", ".png"), format="PNG")
    with open(os.path.join(lists, "val.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    np.save(os.path.join(lists, "cls_labels_onehot.npy"), onehot)
    return root, lists, names


def _model(kind="voc", root=None):
    if kind == "voc":
        from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP
        nc, n_fg, seed = 21, 20, {}
    else:
        from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_coco import WeCLIP
        nc, n_fg, seed = 81, 80, {"seed": 3}
    sd = synth.make_clip_state_dict(**synth.TINY)
    bg, fg = synth.make_text_features(n_fg, 25, synth.TINY["embed_dim"])
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"], num_classes=nc, **seed)
    m = WeCLIP(num_classes=nc, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4, dataset_root_path=root,
               device="cuda", text_features=(bg.cuda(), fg.cuda()))
    m.decoder_fts_fuse.load_state_dict(fuse)
    m.decoder.load_state_dict(dec)
    return m.eval()


def _loader(root, lists, kind="voc"):
    from weclip_vit_comer_amd.datasets import DeviceLoader
    if kind == "voc":
        from weclip_vit_comer_amd.datasets.voc import VOC12SegDataset
        ds = VOC12SegDataset(root_dir=root, name_list_dir=lists, split="val", stage="val", aug=False, ignore_index=255, num_classes=21)
    else:
        from weclip_vit_comer_amd.datasets.coco import CocoSegDataset
        ds = CocoSegDataset(root_dir=root, name_list_dir=lists, split="val", stage="val", aug=False, ignore_index=255, num_classes=81)
    return DeviceLoader(ds, 1, shuffle=False, threads=2)


class _Once:
    """Results computed once per module and shared by its tests; dropped with the module."""

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


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("msc_eval"))
    root, lists, names = _write_voc(os.path.join(tmp, "voc"))
    return tmp, root, lists


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


def _first_image(root, lists, kind="voc"):
    from weclip_vit_comer_amd.datasets import labels_from_onehot
    loader = _loader(root, lists, kind)
    it = iter(loader)
    names, inputs, labels, _ = next(it)
    ids = labels_from_onehot(loader.last_cls_labels)[0]
    it.close()
    return names[0], inputs.clone(), labels.clone(), ids


# ---------------------------------------------------------------------------------------------- logits()
def test_logits_default_is_the_parents_arithmetic(tree):
    """A literal restatement of the parent's `logits` from scale_flip_pair / flip_avg: bit-equal."""
    from weclip_vit_comer_amd import msc_flip as MF
    _, root, lists = tree
    _, inputs, _, _ = _first_image(root, lists)
    m = _model("coco")
    ev = MF.MscFlipEvaluator(m, 81, scales=SCALES, resize_long=RESIZE_LONG)
    seg1, msc = ev.logits(inputs)
    with torch.no_grad():
        x = inputs[0].float().contiguous()
        _, H, W = x.shape
        ratio = RESIZE_LONG / max(H, W)
        h1, w1 = int(H * ratio), int(W * ratio)
        pair = MF.scale_flip_pair(x, (h1, w1), H / h1, W / w1)
        segs = m(pair, ["", ""], mode="val")[0].float().contiguous()
        ref_msc = torch.empty_like(segs[0])
        MF.flip_avg(segs, ref_msc, 0.5, accumulate=False)
        pair_s = MF.scale_flip_pair(pair[0], (int(h1 * 0.75), int(w1 * 0.75)), 1 / 0.75, 1 / 0.75)
        MF.flip_avg(m(pair_s, ["", ""], mode="val")[0].float().contiguous(), ref_msc, 0.5, accumulate=True)
    assert torch.equal(seg1, segs[0]) and torch.equal(msc, ref_msc) and torch.isfinite(msc).all()
    assert len(ev.logits(inputs, want_cam=True)) == 3 and ev.logits(inputs, want_cam=True)[2] is None      # COCO: no CAM leg in 'val'


def test_logits_with_class_ids_and_cam(tree):
    """On a VOC model built with dataset_root_path (it can run both ways): seg1 and msc of the class_ids path -- which skips the
    CAM / PAR chain at the 0.75 scale -- are bit-equal to the default path's; the CAM map is the model's own 'val' output for the
    pair's first image; the instance-level switch is gone afterwards.  A model without the root runs with class_ids alone."""
    from weclip_vit_comer_amd import msc_flip as MF
    _, root, lists = tree
    _, inputs, labels, ids = _first_image(root, lists)
    Hl, Wl = labels.shape[1:]
    m = _model("voc", root)
    ev = MF.MscFlipEvaluator(m, 21, scales=SCALES, resize_long=RESIZE_LONG)
    seg1, msc = ev.logits(inputs)
    s2, m2, cam = ev.logits(inputs, class_ids=ids, want_cam=True)
    assert torch.equal(s2, seg1) and torch.equal(m2, msc)
    assert "val_runs_cam" not in vars(m) and m.val_runs_cam is True
    with torch.no_grad():
        x = inputs[0].float().contiguous()
        _, H, W = x.shape
        ratio = RESIZE_LONG / max(H, W)
        h1, w1 = int(H * ratio), int(W * ratio)
        pair = MF.scale_flip_pair(x, (h1, w1), H / h1, W / w1)
        own = m(pair, ["", ""], mode="val", labels=[ids, ids])[1]
        own_sized = m(pair, ["", ""], mode="val", labels=[ids, ids], sizes=[(Hl, Wl)] * 2)[1]
    assert tuple(cam.shape) == (h1, w1) and cam.dtype == torch.int64 and torch.equal(cam, own[0].long())
    s3, m3, cam_l = ev.logits(inputs, class_ids=ids, want_cam=True, cam_size=(Hl, Wl))
    assert tuple(cam_l.shape) == (Hl, Wl) and torch.equal(cam_l, own_sized[0].long()) and torch.equal(s3, seg1) and torch.equal(m3, msc)
    assert int(cam_l.min()) >= 0 and int(cam_l.max()) < 21
    ev_b = MF.MscFlipEvaluator(_model("voc"), 21, scales=SCALES, resize_long=RESIZE_LONG)
    s4, m4 = ev_b.logits(inputs, class_ids=ids)
    assert torch.equal(s4, seg1) and torch.equal(m4, msc)


def test_skipping_cam_on_a_forward_leaves_seg_bit_equal(tree):
    """The model's own forward with and without the CAM / PAR chain (instance-level val_runs_cam = False) on a 0.75-scale pair."""
    from weclip_vit_comer_amd import msc_flip as MF
    _, root, lists = tree
    _, inputs, _, ids = _first_image(root, lists)
    m = _model("voc")
    x = inputs[0].float().contiguous()
    pair = MF.scale_flip_pair(x, (int(x.shape[1] * 0.75), int(x.shape[2] * 0.75)), 1 / 0.75, 1 / 0.75)
    with torch.no_grad():
        seg_a, cam_a, ap_a = m(pair, ["", ""], mode="val", labels=[ids, ids])
        m.val_runs_cam = False
        try:
            seg_b, cam_b, ap_b = m(pair, ["", ""], mode="val", labels=[ids, ids])
        finally:
            del m.val_runs_cam
    assert cam_a is not None and cam_b is None
    assert torch.equal(seg_a, seg_b) and torch.equal(ap_a, ap_b)


# ---------------------------------------------------------------------------------------------- SplitEvaluator
def _parent_voc(tmp, root, lists):
    """The parent commit's way over the split: MscFlipEvaluator.add_with_crf per image (it updates hist / msc_hist exactly as
    `add` does), the maps kept; plus the scale-1 CAM maps of `logits` for the CAM leg."""
    from weclip_vit_comer_amd import msc_flip as MF
    from weclip_vit_comer_amd import msc_flip_eval as E
    from weclip_vit_comer_amd.datasets import labels_from_onehot
    from weclip_vit_comer_amd.utils import evaluate
    from weclip_vit_comer_amd.utils.dcrf import DenseCRF
    m = _model("voc", root)
    ev = MF.MscFlipEvaluator(m, 21, scales=SCALES, resize_long=RESIZE_LONG, crf=DenseCRF(**CRF))
    cam_hist = torch.zeros(21, 21, device="cuda", dtype=torch.int64)
    rec = {}
    loader = _loader(root, lists)
    for names, inputs, labels, _ in loader:
        ids = labels_from_onehot(loader.last_cls_labels)[0]
        image = E.image_of(inputs)
        jpg = np.asarray(Image.open(os.path.join(root, "JPEGImages", names[0] + ".jpg")).convert("RGB"))
        assert np.array_equal(image.cpu().numpy(), jpg)                       # the CRF's image is the decoded file
        seg_pred, msc_pred, crf_pred = ev.add_with_crf(inputs, labels, image)
        seg1, msc, cam = ev.logits(inputs, class_ids=ids, want_cam=True, cam_size=tuple(labels.shape[1:]))
        evaluate.confusion_hist(labels[0].long(), cam, 21, out=cam_hist)
        rec[names[0]] = dict(gt=labels[0].cpu().numpy(), seg=seg_pred.cpu().numpy(), msc=msc_pred.cpu().numpy(),
                             crf=crf_pred.cpu().numpy(), cam=cam.cpu().numpy(), seg1=seg1.cpu().numpy(), msc_logits=msc.cpu().numpy())
    return ev, cam_hist, rec


def _split_voc(tmp, root, lists, crf):
    from weclip_vit_comer_amd import msc_flip_eval as E
    from weclip_vit_comer_amd.utils.dcrf import DenseCRF
    out = os.path.join(tmp, "split_crf" if crf else "split")
    ev = E.SplitEvaluator(_model("voc"), 21, scales=SCALES, resize_long=RESIZE_LONG, crf=DenseCRF(**CRF) if crf else None,
                          out_dir=out, save_logits=not crf, writers=2)
    return ev, ev.run(_loader(root, lists)), out


def _host_scores(rec, key):
    from weclip_vit_comer_amd.utils import evaluate
    names = sorted(rec)
    return evaluate.scores([rec[n]["gt"] for n in names], [rec[n][key] for n in names], np.zeros((21, 21)), num_classes=21)[1]


@pytest.mark.parametrize("crf", [False, True])
def test_split_evaluator_equals_the_parents_loop_voc(tree, once, crf):
    parent, cam_hist, rec = once(_parent_voc, *tree)
    ev, result, _ = once(_split_voc, *tree, crf)
    print(f"VOC split (crf={crf}): {result['images']} images, pixels {result['pixels']}, msc miou {result['msc_seg']['miou']:.4f}")
    assert result["images"] == ev.images == 5
    assert torch.equal(ev.hist, parent.hist) and torch.equal(ev.msc_hist, parent.msc_hist) and torch.equal(ev.cam_hist, cam_hist)
    np.testing.assert_equal(result["seg"], _host_scores(rec, "seg"))
    np.testing.assert_equal(result["msc_seg"], _host_scores(rec, "msc"))
    np.testing.assert_equal(result["cam"], _host_scores(rec, "cam"))
    valid = sum(int((r["gt"] < 21).sum()) for r in rec.values())
    legs = ("cam", "seg", "msc_seg") + (("crf",) if crf else ())
    assert all(result["pixels"][k] == valid for k in legs) and valid > 0
    if crf:
        assert torch.equal(ev.crf_hist, parent.crf_hist)
        np.testing.assert_equal(result["crf"], _host_scores(rec, "crf"))
    else:
        assert result["crf"] is None and result["pixels"]["crf"] == 0


@pytest.mark.parametrize("crf", [False, True])
def test_split_evaluator_files(tree, once, golden, crf):
    """One file per image and directory; the PNG decodes to the device prediction (the CRF one with crf, else the multi-scale one)
    at the label's size; the colour PNG is table[prediction]; the .npy holds the reference's dict."""
    _, _, rec = once(_parent_voc, *tree)
    _, _, out = once(_split_voc, *tree, crf)
    table = golden("voc_cmap.npz")["cmap"]
    want = ["prediction", "prediction_cmap"] + ([] if crf else ["logit"])
    assert sorted(os.listdir(out)) == sorted(want)
    for k in want:
        assert sorted(os.listdir(os.path.join(out, k))) == sorted(n + (".npy" if k == "logit" else ".png") for n in rec)
    for name, r in rec.items():
        pred = r["crf" if crf else "msc"]
        p = Image.open(os.path.join(out, "prediction", name + ".png"))
        c = Image.open(os.path.join(out, "prediction_cmap", name + ".png"))
        assert (p.mode, c.mode) == ("L", "RGB") and (p.size[1], p.size[0]) == r["gt"].shape == pred.shape
        assert np.array_equal(np.asarray(p), pred.astype(np.uint8)) and np.array_equal(np.asarray(c), table[pred])
        if not crf:
            d = np.load(os.path.join(out, "logit", name + ".npy"), allow_pickle=True).item()
            assert sorted(d) == ["msc_segs", "segs"] and d["segs"].dtype == d["msc_segs"].dtype == np.float32
            assert d["segs"].shape == d["msc_segs"].shape == (1,) + r["seg1"].shape and d["segs"].shape[1] == 21
            assert np.array_equal(d["segs"][0], r["seg1"]) and np.array_equal(d["msc_segs"][0], r["msc_logits"])


def _coco(tmp):
    from weclip_vit_comer_amd import msc_flip as MF
    from weclip_vit_comer_amd import msc_flip_eval as E
    root, lists, _ = DT.write_coco_tree(os.path.join(tmp, "coco"))
    m = _model("coco")
    parent = MF.MscFlipEvaluator(m, 81, scales=SCALES, resize_long=RESIZE_LONG)
    for _, inputs, labels, _ in _loader(root, lists, "coco"):
        parent.add(inputs, labels)
    out = os.path.join(tmp, "coco_out")
    ev = E.SplitEvaluator(m, 81, scales=SCALES, resize_long=RESIZE_LONG, out_dir=out, writers=2)
    return m, parent, ev, ev.run(_loader(root, lists, "coco")), out, root, lists


def test_split_evaluator_coco_has_no_cam_leg(tree, once):
    _, parent, ev, result, out, _, _ = once(_coco, tree[0])
    assert result["cam"] is None and result["pixels"]["cam"] == 0 and int(ev.cam_hist.sum()) == 0 and result["images"] == 2
    assert torch.equal(ev.hist, parent.hist) and torch.equal(ev.msc_hist, parent.msc_hist) and int(ev.hist.sum()) > 0
    s1, s2 = parent.scores()
    np.testing.assert_equal(result["seg"], s1)
    np.testing.assert_equal(result["msc_seg"], s2)
    assert len(os.listdir(os.path.join(out, "prediction"))) == len(os.listdir(os.path.join(out, "prediction_cmap"))) == 2


def test_add_raises_no_more_host_synchronisations_than_the_parent(tree, once):
    """Per image, files included: SplitEvaluator.add against MscFlipEvaluator.add plus .cpu() of its two maps, in this process."""
    from weclip_vit_comer_amd import msc_flip as MF
    from weclip_vit_comer_amd import msc_flip_eval as E
    m, _, _, _, _, root, lists = once(_coco, tree[0])
    _, inputs, labels, _ = _first_image(root, lists, "coco")
    parent = MF.MscFlipEvaluator(m, 81, scales=SCALES, resize_long=RESIZE_LONG)
    ev = E.SplitEvaluator(m, 81, scales=SCALES, resize_long=RESIZE_LONG, out_dir=os.path.join(tree[0], "sync_out"), writers=2)
    parent.add(inputs, labels)
    ev.add("warm", inputs, labels)
    torch.cuda.synchronize()
    with _Syncs() as old:
        a, b = parent.add(inputs, labels)
        a.cpu(), b.cpu()
    with _Syncs() as new:
        ev.add("x", inputs, labels)
    ev.finish()
    print(f"sync warnings per image: SplitEvaluator.add {new.n}, MscFlipEvaluator.add + 2 x .cpu() {old.n}")
    assert new.n <= old.n and old.n >= 2
    with _Syncs() as probe:                     # the instrument itself: a host read is counted
        torch.zeros(1, device="cuda").item()
    assert probe.n >= 1


# ---------------------------------------------------------------------------------------------- the command line
def _cli_files(tmp, root, lists):
    clip = os.path.join(tmp, "tiny_clip.pt")
    torch.save(synth.make_clip_state_dict(**synth.TINY), clip)
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    text = os.path.join(tmp, "text_rows.pt")
    torch.save({"bg": bg, "fg": fg}, text)
    cfg = os.path.join(tmp, "eval.yaml")
    with open(cfg, "w") as f:
        f.write(YAML.format(root=root, lists=lists, clip=clip, text=text))
    ckpt = os.path.join(tmp, "WeCLIP_model_iter_7.pth")
    torch.save(_model("voc").state_dict(), ckpt)
    return cfg, ckpt


def _cli_args(cfg, ckpt, work):
    return ["--config", cfg, "--model_path", ckpt, "--work_dir", work, "--resize_long", str(RESIZE_LONG), "--scales", "1,0.75",
            "--threads", "2", "--writers", "2"]


def test_cli_one_process(tree, once, capsys):
    from weclip_vit_comer_amd import msc_flip_eval as E
    tmp, root, lists = tree
    cfg, ckpt = once(_cli_files, *tree)
    work = os.path.join(tmp, "results")
    assert E.main(_cli_args(cfg, ckpt, work)) == 0
    printed = capsys.readouterr().out
    at = [printed.index(h) for h in ("cams score:", "segs score:", "msc segs score:")]
    assert at == sorted(at) and "crf score:" not in printed
    out = os.path.join(work, "val")
    with open(os.path.join(out, "scores.json")) as f:
        got = json.load(f)
    ev, result, _ = once(_split_voc, *tree, False)
    assert got == json.loads(json.dumps(E.to_json(dict(result, hist={k: v.tolist() for k, v in ev.hist_host.items()}))))
    assert got["images"] == 5 and got["pixels"]["seg"] > 0
    assert sorted(os.listdir(os.path.join(out, "prediction"))) == sorted(f"val_{i:04d}.png" for i in range(5))


def test_cli_two_ranks_share_the_gpu(tree, once):
    """`python -m torch.distributed.run --nproc-per-node 2 -m weclip_vit_comer_amd.msc_flip_eval` with the gloo rehearsal
    backend (pattern and environment of the training driver's test)."""
    tmp, root, lists = tree
    cfg, ckpt = once(_cli_files, *tree)
    work = os.path.join(tmp, "results_dp")
    env = dict(os.environ, WECLIP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    with socket.socket() as sock:                # a port that is free now
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(port), "-m", "weclip_vit_comer_amd.msc_flip_eval"] + _cli_args(cfg, ckpt, work)
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = os.path.join(work, "val")
    with open(os.path.join(out, "scores.json")) as f:
        got = json.load(f)
    ev, result, _ = once(_split_voc, *tree, False)
    for k in ("cam", "seg", "msc_seg", "crf"):      # the all-reduced histograms are the single process's
        assert got["hist"][k] == ev.hist_host[k].tolist(), k
    assert got["images"] == 5 and got["pixels"] == result["pixels"]
    for k in ("prediction", "prediction_cmap"):      # every image once, whichever rank wrote it
        assert sorted(os.listdir(os.path.join(out, k))) == sorted(f"val_{i:04d}.png" for i in range(5))
    assert sorted(os.listdir(out)) == ["prediction", "prediction_cmap", "scores.json"]
    assert r.stdout.count("msc segs score:") == 1      # rank 0 alone prints
