"""GPU tests of the predict entry point (weclip_vit_comer_amd.predict): `wc_predict_finish` against the restatement of
tests/predict_ref.py, its argument checks, `Predictor` on folders of JPEG / PNG images with the tiny synthetic CLIP (all three
models, against `SplitEvaluator`'s files, summary.json against the written PNGs, host synchronisations), and the command line
in one process, on two ranks sharing the GPU, and over a split of a tree without label files."""
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
import predict_ref as R
from oracle import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(70, 90), (75, 111), (70, 90), (97, 150), (131, 69)]              # none a multiple of 16
RESIZE_LONG, SCALES = 128, (1.0, 0.75)
CRF = dict(iter_max=2, pos_xy_std=3, pos_w=3, bi_xy_std=64, bi_rgb_std=5, bi_w=4)      # the reference's, with fewer iterations
KINDS = ("prediction", "prediction_cmap", "confidence", "overlay")

# (C, Hs, Ws) -> (H, W), mode, seed.  The seeds are chosen so that the restatement alone puts at most 2 % of a case's pixels
# into the rounding band (asserted below, on the CPU).
CASES = {
    "odd_width": ((21, 8, 7), (75, 111), 0, 0),
    "coco": ((81, 24, 32), (97, 150), 0, 1),
    "one_class": ((1, 3, 3), (5, 5), 0, 2),
    "most_classes": ((255, 2, 2), (9, 6), 0, 3),
    "same_size": ((3, 4, 5), (4, 5), 0, 4),
    "crf_q": ((21, 37, 53), (37, 53), 1, 5),
}


def _inputs(case):
    (C, Hs, Ws), (H, W), mode, seed = CASES[case]
    rs = np.random.RandomState(seed)
    src = (3.0 * rs.randn(C, Hs, Ws)).astype(np.float32)
    if mode == 1:                                             # rows that are a soft-max, as the CRF's Q
        e = np.exp(src.astype(np.float64) - src.max(0))
        src = (e / e.sum(0)).astype(np.float32)
    image = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    return src, image, (H, W), mode


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


def _reference(case):
    """The restatement's arg-max and 255 * conf of a case, computed once and not modified."""
    src, image, hw, mode = _inputs(case)
    best, x = R.confidence(src, hw, mode)
    best.setflags(write=False)
    x.setflags(write=False)
    return src, image, hw, mode, best, x


def _gpu(src, hw, image, mode, alpha256=128, ignore_below=0, skip=(), stats=None):
    from weclip_vit_comer_amd import predict as P
    H, W = hw
    C = src.shape[0]
    u8 = lambda *s: torch.full(s, 7, device="cuda", dtype=torch.uint8)      # noqa: E731
    out = dict(pred=u8(H, W), cmap=u8(H, W, 3), conf=u8(H, W), overlay=u8(H, W, 3),
               stats=torch.zeros(2 * C + 1, device="cuda", dtype=torch.int64) if stats is None else stats)
    for k in skip:
        out[k] = None
    img = None if image is None else torch.from_numpy(image).cuda()
    P.predict_finish(torch.from_numpy(src).cuda(), hw, image=img, pred_u8=out["pred"], cmap_rgb=out["cmap"], conf_u8=out["conf"],
                     overlay_rgb=out["overlay"], stats=out["stats"], mode=mode, alpha256=alpha256, ignore_below=ignore_below)
    return out


def _host(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _check_conf(conf, x, C, what):
    """The confidence rule: equal to floor(x + 0.5) outside the band, within one step inside it.  -> pixels in the band."""
    want = np.floor(x + 0.5).astype(np.int64)
    inside = R.band(x, C)
    diff = conf.astype(np.int64) - want
    assert (diff[~inside] == 0).all(), f"{what}: conf_u8 differs outside the rounding band at {int((diff[~inside] != 0).sum())} pixels"
    assert (np.abs(diff[inside]) <= 1).all(), f"{what}: conf_u8 is more than one step off inside the band"
    return int(inside.sum()), int((diff != 0).sum())


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("case", list(CASES))
def test_band_holds_at_most_two_percent_of_a_case(case, once):
    """A condition on the inputs, from the restatement alone."""
    src, _, hw, _, _, x = once(_reference, case)
    assert R.band(x, src.shape[0]).mean() <= 0.02


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_equals_the_restatement(case, once, golden):
    from weclip_vit_comer_amd import msc_flip as MF
    from weclip_vit_comer_amd import msc_flip_eval as E
    table = golden("voc_cmap.npz")["cmap"]
    src, image, hw, mode, best, x = once(_reference, case)
    C = src.shape[0]
    for ignore_below in (0, 128, 255):
        for alpha256 in (0, 77, 256):
            got = _host(_gpu(src, hw, image, mode, alpha256, ignore_below))
            n_band, n_diff = _check_conf(got["conf"], x, C, f"{case} ignore_below={ignore_below} alpha256={alpha256}")
            # what follows from the confidence is compared with the GPU's own conf_u8 (checked above) in the ignore rule
            want = R.finish(best, got["conf"], table, C, image=image, alpha256=alpha256, ignore_below=ignore_below)
            for k in ("pred", "cmap", "overlay", "stats"):
                assert np.array_equal(got[k], want[k]), (case, ignore_below, alpha256, k)
            assert got["stats"][:C].sum() + got["stats"][2 * C] == hw[0] * hw[1]
    print(f"{case}: {n_band} of {hw[0] * hw[1]} pixels in the rounding band, {n_diff} rounded the other way")
    if ignore_below == 255 and C > 1:
        assert got["stats"][2 * C] > 0                                     # the ignore rule was exercised
    # the arg-max is wc_resize_argmax's and wc_eval_finish's, bit for bit
    dev = torch.from_numpy(src).cuda()
    plain = _gpu(src, hw, image, mode)["pred"]
    assert torch.equal(plain, MF.resize_argmax(dev, hw).to(torch.uint8))
    via_eval = torch.empty(hw, device="cuda", dtype=torch.uint8)
    E.eval_finish(dev, dev, hw, C, predm_u8=via_eval)
    assert torch.equal(plain, via_eval)
    assert np.array_equal(plain.cpu().numpy(), best.astype(np.uint8))


@pytest.mark.parametrize("case", ["odd_width", "crf_q"])
def test_every_output_is_optional_and_calls_repeat(case, once):
    src, image, hw, mode, _, _ = once(_reference, case)
    full = _gpu(src, hw, image, mode, 77, 128)
    again = _gpu(src, hw, image, mode, 77, 128)
    assert all(torch.equal(full[k], again[k]) for k in full)               # two calls, the same bits
    twice = _gpu(src, hw, image, mode, 77, 128, stats=again["stats"])["stats"]
    assert torch.equal(twice, 2 * full["stats"]) and twice is again["stats"]      # stats is added into
    for absent in ("pred", "cmap", "conf", "overlay", "stats"):
        part = _gpu(src, hw, image, mode, 77, 128, skip=(absent,))
        assert part[absent] is None and all(torch.equal(part[k], full[k]) for k in full if k != absent), absent
    bare = _gpu(src, hw, None, mode, 77, 128, skip=("overlay",))          # no image, no overlay
    assert all(torch.equal(bare[k], full[k]) for k in full if k != "overlay")
    none = _gpu(src, hw, None, mode, 77, 128, skip=("pred", "cmap", "conf", "overlay"))
    assert torch.equal(none["stats"], full["stats"])


def test_torch_op(once):
    import weclip_vit_comer_amd
    weclip_vit_comer_amd.register_torch_ops()
    src, image, hw, mode, _, _ = once(_reference, "odd_width")
    full = _gpu(src, hw, image, mode, 77, 128)
    got = torch.ops.weclip.predict_finish(torch.from_numpy(src).cuda(), torch.from_numpy(image).cuda(), hw[0], hw[1], mode, 77, 128)
    assert all(torch.equal(a, full[k]) for a, k in zip(got, ("pred", "cmap", "conf", "overlay", "stats")))
    bare = torch.ops.weclip.predict_finish(torch.from_numpy(src).cuda(), None, hw[0], hw[1], mode, 77, 128)
    assert torch.equal(bare[0], full["pred"]) and int(bare[3].sum()) == 0


def test_argument_errors_launch_nothing():
    from weclip_vit_comer_amd import _lib as L
    from weclip_vit_comer_amd import predict as P
    src = torch.randn(3, 4, 5, device="cuda")
    image = torch.zeros(6, 7, 3, device="cuda", dtype=torch.uint8)
    pred = torch.full((6, 7), 7, device="cuda", dtype=torch.uint8)
    over = torch.full((6, 7, 3), 7, device="cuda", dtype=torch.uint8)
    stats = torch.zeros(7, device="cuda", dtype=torch.int64)

    def call(match, src=src, hw=(6, 7), image=image, overlay=over, **kw):
        with pytest.raises(RuntimeError, match=match):
            P.predict_finish(src, hw, image=image, pred_u8=pred if tuple(hw) == (6, 7) else None,
                             overlay_rgb=overlay if tuple(hw) == (6, 7) else None,
                             stats=stats if src.shape[0] == 3 else None, **kw)
    call("mode", mode=2)
    call("mode", mode=-1)
    call("mode 1 needs", mode=1)                                           # (4, 5) is not (6, 7)
    call("alpha256", alpha256=257)
    call("alpha256", alpha256=-1)
    call("ignore_below", ignore_below=256)
    call("ignore_below", ignore_below=-1)
    call("overlay_rgb needs image", image=None)
    call("C = 256", src=torch.zeros(256, 2, 2, device="cuda"), image=None, overlay=None)
    call("H x W", hw=(0, 7), image=None, overlay=None)
    call("H x W", hw=(6, -7), image=None, overlay=None)
    # the cases an empty or missing tensor cannot express go to the library directly: (C, Hs, Ws, H, W) around a valid src
    for match, src_ptr, dims in (("src is NULL", None, (3, 4, 5, 6, 7)), ("C = 0", L.ptr(src), (0, 4, 5, 6, 7)),
                                 ("Hs x Ws", L.ptr(src), (3, 0, 5, 6, 7)), ("Hs x Ws", L.ptr(src), (3, 4, -5, 6, 7))):
        with pytest.raises(RuntimeError, match=match):
            L.lib().wc_predict_finish(src_ptr, None, L.ptr(pred), None, None, None, L.ptr(stats), *dims, 0, 128, 0, L.stream())
    with pytest.raises(RuntimeError, match="pred_u8 must be"):              # the binding's shape checks
        P.predict_finish(src, (6, 7), pred_u8=pred[:5])
    with pytest.raises(RuntimeError, match="stats must be"):
        P.predict_finish(src, (6, 7), stats=stats[:6])
    torch.cuda.synchronize()
    assert int(stats.sum()) == 0 and bool((pred == 7).all()) and bool((over == 7).all())


# ---------------------------------------------------------------------------------------------- Predictor
def _model(kind="voc", root=None):
    if kind == "seg":
        from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc_seg import WeCLIP
        sd = synth.make_clip_state_dict(**synth.TINY)
        fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
        m = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4, device="cuda")
    else:
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


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """A VOC tree whose label maps have the images' sizes (five JPEGs), and a folder of two more images, a PNG and a JPEG, with
    a third one in a sub-directory."""
    tmp = str(tmp_path_factory.mktemp("predict"))
    root = os.path.join(tmp, "voc")
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "SegmentationClassAug"))
    lists = os.path.join(root, "lists")
    os.makedirs(lists)
    names, onehot = [], {}
    for i, (H, W) in enumerate(SIZES):
        name = f"img_{i:04d}"
        Image.fromarray(DT.smooth_image(H, W, 30 + i)).save(os.path.join(root, "JPEGImages", name + ".jpg"), quality=92)
        lab = np.zeros((H, W), np.uint8)
        lab[H // 5:H // 2, W // 6:] = 1 + (3 * i) % 20
        lab[:, :2] = 255
        Image.fromarray(lab).save(os.path.join(root, "SegmentationClassAug", name + ".png"))
        onehot[name] = DT.onehot20(lab)
        names.append(name)
    with open(os.path.join(lists, "val.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    np.save(os.path.join(lists, "cls_labels_onehot.npy"), onehot)
    photos = os.path.join(tmp, "photos")
    os.makedirs(os.path.join(photos, "trip"))
    Image.fromarray(DT.smooth_image(75, 111, 1)).save(os.path.join(photos, "a.png"))
    Image.fromarray(DT.smooth_image(97, 150, 2)).save(os.path.join(photos, "b.jpg"), quality=90)
    Image.fromarray(DT.smooth_image(131, 69, 3)).save(os.path.join(photos, "trip", "c.jpeg"), quality=90)
    return tmp, root, lists, photos


def _folder_loader(source, recursive=False):
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.folder import ImageFolderDataset
    return DeviceLoader(ImageFolderDataset(source, recursive=recursive), 1, shuffle=False, threads=2)


def _first_inputs(source):
    it = iter(_folder_loader(source))
    _, inputs, _ = next(it)
    inputs = inputs.clone()
    it.close()
    return inputs


def _voc_loader(root, lists):
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12SegDataset
    ds = VOC12SegDataset(root_dir=root, name_list_dir=lists, split="val", stage="val", aug=False, ignore_index=255, num_classes=21)
    return DeviceLoader(ds, 1, shuffle=False, threads=2)


def _check_summary(summary, out, nc, names, ignore_below=0):
    """summary.json against NumPy on the written PNGs: area[c] = count(pred == c), conf_sum[c] = sum(conf[pred == c]), exactly."""
    with open(os.path.join(out, "summary.json")) as f:
        on_disk = json.load(f)
    assert on_disk == json.loads(json.dumps(summary, allow_nan=False))
    assert summary["images"] == len(names) and [r["name"] for r in summary["per_image"]] == sorted(names)
    for r in summary["per_image"]:
        pred = np.asarray(Image.open(os.path.join(out, "prediction", r["name"] + ".png")))
        conf = np.asarray(Image.open(os.path.join(out, "confidence", r["name"] + ".png")))
        H, W = pred.shape
        assert r["size"] == [H, W] and conf.shape == (H, W)
        want = {}
        for c in range(nc):
            area = int((pred == c).sum())
            if area:
                want[str(c)] = {"share": area / (H * W), "confidence": int(conf[pred == c].astype(np.int64).sum()) / area / 255.0}
        assert r["classes"] == want and r["ignored"] == int((pred == 255).sum()) / (H * W)
        assert set(np.unique(pred)) <= set(range(nc)) | {255}
        if ignore_below:
            assert (conf[pred == 255] < ignore_below).all() and (conf[pred != 255] >= ignore_below).all()
        else:
            assert not (pred == 255).any()


def test_logits_without_the_cam_chain(tree):
    """run_cam=False on a VOC model built without dataset_root_path and given no labels: seg1 / msc bit-equal to the class_ids
    path's, no CAM map, and the instance-level switch is gone afterwards."""
    from weclip_vit_comer_amd import msc_flip as MF
    _, _, _, photos = tree
    inputs = _first_inputs(photos)
    m = _model("voc")
    ev = MF.MscFlipEvaluator(m, 21, scales=SCALES, resize_long=RESIZE_LONG)
    seg1, msc = ev.logits(inputs, run_cam=False)
    assert "val_runs_cam" not in vars(m) and m.val_runs_cam is True
    s2, m2 = ev.logits(inputs, class_ids=[3, 7])
    assert torch.equal(seg1, s2) and torch.equal(msc, m2) and torch.isfinite(msc).all()
    s3, m3, cam = ev.logits(inputs, run_cam=False, want_cam=True)
    assert cam is None and torch.equal(s3, seg1) and torch.equal(m3, msc) and "val_runs_cam" not in vars(m)


def _predict_folder(tmp, photos, kind):
    from weclip_vit_comer_amd import predict as P
    out = os.path.join(tmp, f"folder_{kind}")
    nc = 81 if kind == "coco" else 21
    pr = P.Predictor(_model(kind), nc, scales=SCALES, resize_long=RESIZE_LONG, out_dir=out, outputs=KINDS, alpha=0.3,
                     ignore_below=40 if kind == "coco" else 0, palette=kind == "seg", writers=2)
    return pr.run(_folder_loader(photos, recursive=True)), out


@pytest.mark.parametrize("kind", ["voc", "coco", "seg"])
def test_predictor_runs_every_model_on_a_folder(tree, once, golden, kind):
    tmp, _, _, photos = tree
    summary, out = once(_predict_folder, tmp, photos, kind)
    names = ["a", "b", "trip/c"]
    assert sorted(os.listdir(out)) == sorted(KINDS + ("summary.json",))
    _check_summary(summary, out, 81 if kind == "coco" else 21, names, ignore_below=40 if kind == "coco" else 0)
    table = golden("voc_cmap.npz")["cmap"]
    for name, hw in zip(names, [(75, 111), (97, 150), (131, 69)]):
        ims = {k: Image.open(os.path.join(out, k, name + ".png")) for k in KINDS}
        assert {k: im.mode for k, im in ims.items()} == {"prediction": "P" if kind == "seg" else "L", "prediction_cmap": "RGB",
                                                         "confidence": "L", "overlay": "RGB"}
        assert all((im.size[1], im.size[0]) == hw for im in ims.values())
        pred, cmap = np.asarray(ims["prediction"]), np.asarray(ims["prediction_cmap"])
        assert np.array_equal(cmap, table[pred])
        src = np.asarray(Image.open(os.path.join(photos, name + (".png" if name == "a" else ".jpg" if name == "b" else ".jpeg"))).convert("RGB"))
        a = int(round(0.3 * 256))
        assert np.array_equal(np.asarray(ims["overlay"]), ((a * cmap.astype(np.int64) + (256 - a) * src.astype(np.int64) + 128) >> 8).astype(np.uint8))
    assert summary["args"]["alpha256"] == 77 and summary["args"]["outputs"] == list(KINDS)


def _split_files(tmp, root, lists, crf):
    from weclip_vit_comer_amd import msc_flip_eval as E
    from weclip_vit_comer_amd.utils.dcrf import DenseCRF
    out = os.path.join(tmp, "split_crf" if crf else "split")
    ev = E.SplitEvaluator(_model("voc"), 21, scales=SCALES, resize_long=RESIZE_LONG, crf=DenseCRF(**CRF) if crf else None,
                          out_dir=out, writers=2)
    ev.run(_voc_loader(root, lists))
    return out


def _predict_files(tmp, root, crf):
    from weclip_vit_comer_amd import predict as P
    from weclip_vit_comer_amd.utils.dcrf import DenseCRF
    out = os.path.join(tmp, "predict_crf" if crf else "predict")
    pr = P.Predictor(_model("voc"), 21, scales=SCALES, resize_long=RESIZE_LONG, crf=DenseCRF(**CRF) if crf else None, out_dir=out,
                     outputs=("prediction", "prediction_cmap", "confidence"), writers=2)
    return pr.run(_folder_loader(os.path.join(root, "JPEGImages"))), out


@pytest.mark.parametrize("crf", [False, True])
def test_predictor_writes_the_evaluators_files(tree, once, crf):
    """On a VOC tree whose labels have the images' sizes: prediction/ and prediction_cmap/ byte-equal to SplitEvaluator's."""
    tmp, root, lists, _ = tree
    theirs = once(_split_files, tmp, root, lists, crf)
    summary, ours = once(_predict_files, tmp, root, crf)
    names = [f"img_{i:04d}" for i in range(5)]
    assert sorted(os.listdir(ours)) == ["confidence", "prediction", "prediction_cmap", "summary.json"]
    for k in ("prediction", "prediction_cmap"):
        assert sorted(os.listdir(os.path.join(ours, k))) == sorted(os.listdir(os.path.join(theirs, k))) == [n + ".png" for n in names]
        for n in names:
            with open(os.path.join(ours, k, n + ".png"), "rb") as a, open(os.path.join(theirs, k, n + ".png"), "rb") as b:
                assert a.read() == b.read(), (k, n)
    _check_summary(summary, ours, 21, names)
    assert summary["args"]["crf"] == (dict(CRF, bilateral="exact") if crf else None)


def test_confidence_under_the_crf_is_the_rounded_maximum_of_q(tree, once):
    from weclip_vit_comer_amd import msc_flip as MF
    from weclip_vit_comer_amd import msc_flip_eval as E
    from weclip_vit_comer_amd.utils import dcrf
    tmp, root, lists, _ = tree
    _, ours = once(_predict_files, tmp, root, True)
    ev = MF.MscFlipEvaluator(_model("voc"), 21, scales=SCALES, resize_long=RESIZE_LONG)
    crf = dcrf.DenseCRF(**CRF)
    for names, inputs, _ in _folder_loader(os.path.join(root, "JPEGImages")):
        H, W = inputs.shape[2:]
        _, msc = ev.logits(inputs, run_cam=False)
        Q = crf.with_unary(E.image_of(inputs), dcrf.unary_from_logits(msc, (H, W)))
        q = Q.cpu().numpy()
        x = 255.0 * np.clip(q.max(0).astype(np.float64), 0.0, 1.0)
        conf = np.asarray(Image.open(os.path.join(ours, "confidence", names[0] + ".png")))
        pred = np.asarray(Image.open(os.path.join(ours, "prediction", names[0] + ".png")))
        _check_conf(conf, x, 21, names[0])
        assert np.array_equal(pred, q.argmax(0).astype(np.uint8))


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
        # (the first switch to "warn" in a process announces itself as "a prototype feature [that] does not yet detect all
        #  synchronizing operations": that notice is not a synchronisation)
        self.where = [f"{w.filename}:{w.lineno}: {w.message}" for w in self._log
                      if "synchroniz" in str(w.message).lower() and "prototype feature" not in str(w.message)]
        self.n = len(self.where)
        self._cm.__exit__(*exc)


def test_add_does_not_synchronise(tree):
    from weclip_vit_comer_amd import predict as P
    tmp, _, _, photos = tree
    inputs = _first_inputs(photos)
    pr = P.Predictor(_model("voc"), 21, scales=SCALES, resize_long=RESIZE_LONG, out_dir=os.path.join(tmp, "sync_out"), outputs=KINDS,
                     writers=2)
    pr.add("warm", inputs)
    torch.cuda.synchronize()
    with _Syncs() as s:
        pr.add("x", inputs)
    summary = pr.finish()
    assert s.n == 0, s.where
    assert summary["images"] == 2
    with _Syncs() as probe:                     # the instrument itself: a host read is counted
        torch.zeros(1, device="cuda").item()
    assert probe.n >= 1


# ---------------------------------------------------------------------------------------------- the command line
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


def _cli_files(tmp, root, lists):
    clip = os.path.join(tmp, "tiny_clip.pt")
    torch.save(synth.make_clip_state_dict(**synth.TINY), clip)
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    text = os.path.join(tmp, "text_rows.pt")
    torch.save({"bg": bg, "fg": fg}, text)
    cfg = os.path.join(tmp, "predict.yaml")
    with open(cfg, "w") as f:
        f.write(YAML.format(root=root, lists=lists, clip=clip, text=text))
    ckpt = os.path.join(tmp, "WeCLIP_model_iter_7.pth")
    torch.save(_model("voc").state_dict(), ckpt)
    return cfg, ckpt


def _cli_args(cfg, ckpt, out):
    return ["--config", cfg, "--model_path", ckpt, "--out_dir", out, "--resize_long", str(RESIZE_LONG), "--scales", "1,0.75",
            "--threads", "2", "--writers", "2"]


def test_cli_one_process(tree, once, capsys):
    from weclip_vit_comer_amd import predict as P
    tmp, root, lists, photos = tree
    cfg, ckpt = once(_cli_files, tmp, root, lists)
    out = os.path.join(tmp, "cli_out")
    assert P.main(_cli_args(cfg, ckpt, out) + ["--images", photos, "--recursive", "--outputs", ",".join(KINDS), "--palette"]) == 0
    assert "3 images" in capsys.readouterr().out
    assert sorted(os.listdir(out)) == sorted(KINDS + ("summary.json",))
    for k in KINDS:
        assert sorted(os.listdir(os.path.join(out, k))) == ["a.png", "b.png", "trip"]
        assert os.listdir(os.path.join(out, k, "trip")) == ["c.png"]
    with open(os.path.join(out, "summary.json")) as f:
        got = json.load(f)
    _check_summary(got, out, 21, ["a", "b", "trip/c"])
    assert Image.open(os.path.join(out, "prediction", "a.png")).mode == "P"
    # the same model on the same folder through Predictor: the same maps
    _, ref = once(_predict_folder, tmp, photos, "voc")
    for n in ("a", "b", "trip/c"):
        for k in ("prediction", "confidence"):
            assert np.array_equal(np.asarray(Image.open(os.path.join(out, k, n + ".png"))), np.asarray(Image.open(os.path.join(ref, k, n + ".png"))))
    # not recursive, the default outputs
    out2 = os.path.join(tmp, "cli_out_default")
    assert P.main(_cli_args(cfg, ckpt, out2) + ["--images", photos]) == 0
    assert sorted(os.listdir(out2)) == ["prediction", "prediction_cmap", "summary.json"]
    assert sorted(os.listdir(os.path.join(out2, "prediction"))) == ["a.png", "b.png"]


def test_cli_two_ranks_share_the_gpu(tree, once):
    """`python -m torch.distributed.run --nproc-per-node 2 -m weclip_vit_comer_amd.predict` with the gloo rehearsal backend
    (pattern and environment of the evaluation entry point's test): every image's files once, one summary.json with all."""
    tmp, root, lists, _ = tree
    cfg, ckpt = once(_cli_files, tmp, root, lists)
    out = os.path.join(tmp, "cli_out_dp")
    env = dict(os.environ, WECLIP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    with socket.socket() as sock:                # a port that is free now
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(port), "-m", "weclip_vit_comer_amd.predict"] + _cli_args(cfg, ckpt, out) + [
               "--images", os.path.join(root, "JPEGImages"), "--outputs", "prediction,confidence"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    names = [f"img_{i:04d}" for i in range(5)]
    assert sorted(os.listdir(out)) == ["confidence", "prediction", "summary.json"]
    for k in ("prediction", "confidence"):
        assert sorted(os.listdir(os.path.join(out, k))) == [n + ".png" for n in names]
    with open(os.path.join(out, "summary.json")) as f:
        got = json.load(f)
    _check_summary(got, out, 21, names)
    assert got["args"]["world"] == 2 and r.stdout.count("5 images") == 1      # rank 0 alone prints
    _, single = once(_predict_files, tmp, root, False)                         # the single process's maps
    for n in names:
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "prediction", n + ".png"))),
                              np.asarray(Image.open(os.path.join(single, "prediction", n + ".png"))))


def test_cli_split_of_a_tree_without_label_files(tree, once):
    """--split NAME: the names of name_list_dir/NAME.txt on a tree that has JPEGImages/ and the list, nothing else."""
    from weclip_vit_comer_amd import predict as P
    tmp, root, lists, _ = tree
    bare = os.path.join(tmp, "voc_test")
    os.makedirs(os.path.join(bare, "JPEGImages"))
    os.makedirs(os.path.join(bare, "lists"))
    names = ["2008_000001", "2008_000002"]
    for i, n in enumerate(names):
        Image.fromarray(DT.smooth_image(*SIZES[i + 1], 50 + i)).save(os.path.join(bare, "JPEGImages", n + ".jpg"), quality=92)
    with open(os.path.join(bare, "lists", "test.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    cfg, ckpt = once(_cli_files, tmp, root, lists)
    cfg_bare = os.path.join(tmp, "predict_bare.yaml")
    with open(cfg) as f, open(cfg_bare, "w") as g:
        g.write(f.read().replace(f"root_dir: {root}", f"root_dir: {bare}").replace(f"name_list_dir: {lists}",
                                                                                    f"name_list_dir: {os.path.join(bare, 'lists')}"))
    out = os.path.join(tmp, "cli_out_split")
    assert P.main(_cli_args(cfg_bare, ckpt, out) + ["--split", "test", "--outputs", "prediction,confidence", "--palette"]) == 0
    assert sorted(os.listdir(os.path.join(bare))) == ["JPEGImages", "lists"]
    assert sorted(os.listdir(os.path.join(out, "prediction"))) == [n + ".png" for n in names]
    with open(os.path.join(out, "summary.json")) as f:
        _check_summary(json.load(f), out, 21, names)
    p = Image.open(os.path.join(out, "prediction", names[0] + ".png"))
    assert p.mode == "P" and (p.size[1], p.size[0]) == SIZES[1]
