"""GPU tests of the CAM-seed path (csrc/camseed.hip, clip/cam_seeds.py).  Every comparison is `==` on integers:
against the unmodified reference's recorded outputs (tests/golden/camseed_ref.npz) where it has them, against the numpy
restatement tests/camseed_ref.py (itself pinned to that fixture in tests/test_camseed_cpu.py) elsewhere, and for the CRF leg
against this package's own crf_inference_label, which is bit-identical from run to run."""
import gzip
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camseed_cases as K  # noqa: E402
import camseed_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own limit."""
    def boom(*_):
        raise TimeoutError("test exceeded its 120 s limit")
    old = signal.signal(signal.SIGALRM, boom)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def CS():
    from weclip_vit_comer_amd.clip import cam_seeds
    return cam_seeds


def dev(case):
    cams, gt = K.flat(case)
    return torch.from_numpy(cams).cuda(), torch.from_numpy(gt).cuda()


def sweep(CS, case, **kw):
    cams, gt = dev(case)
    return CS.sweep_confusion(cams, case["keys"], gt, case["thresholds"], case["nc"], **kw)


def test_case1_sweep_lds_path_equals_the_reference_and_accumulates(CS, golden):
    g, c = golden("camseed_ref.npz"), K.case1()
    assert int(g["case1_check"][0]) == K.check(c)
    assert CS.sweep_path(c["nc"], 3, len(c["thresholds"])) == "lds"
    cams, gt = dev(c)
    bins = CS.sweep_bins(cams, c["keys"], gt, c["thresholds"], c["nc"])
    conf = CS.confusion_from_bins(bins)
    assert conf.dtype == torch.int64 and tuple(conf.shape) == (16, 21, 21)
    assert np.array_equal(conf.cpu().numpy(), g["case1_conf"])
    assert np.array_equal(bins.cpu().numpy(), R.sweep_bins(c["cams"], c["keys"], c["gt"], c["thresholds"], c["nc"]))
    again = CS.sweep_confusion(cams, c["keys"], gt, c["thresholds"], c["nc"], bins=bins)          # a second call doubles every count
    assert np.array_equal(again.cpu().numpy(), 2 * g["case1_conf"])
    # both paths give the same counts
    forced = sweep(CS, c, force_global=True)
    assert np.array_equal(forced.cpu().numpy(), g["case1_conf"])
    assert CS.check_tables_in_range(cams.device)


def test_case1_sweep_through_the_registered_op(CS, golden):
    import weclip_vit_comer_amd
    weclip_vit_comer_amd.register_torch_ops()
    g, c = golden("camseed_ref.npz"), K.case1()
    cams, gt = dev(c)
    t = CS.PairTables(c["keys"], c["nc"], cams.device)
    bins = torch.ops.weclip.cam_seed_sweep(cams, t.first, t.keys, gt, c["thresholds"], c["nc"], t.Kmax)
    assert np.array_equal(CS.confusion_from_bins(bins).cpu().numpy(), g["case1_conf"])


def test_case2_sweep_smallest(CS, golden):
    g, c = golden("camseed_ref.npz"), K.case2()
    assert np.array_equal(sweep(CS, c).cpu().numpy(), g["case2_conf"])


def test_case3_sweep_global_path(CS, golden):
    g, c = golden("camseed_ref.npz"), K.case3()
    assert CS.sweep_path(c["nc"], 12, len(c["thresholds"])) == "global"
    got = sweep(CS, c).cpu().numpy()
    assert np.array_equal(got, R.sweep_confusion(c["cams"], c["keys"], c["gt"], c["thresholds"], c["nc"]))
    assert np.array_equal(got, g["case3_conf"])


def test_sweep_of_one_wide_image_takes_every_load_form(CS):
    """HW = 97 * 101 = 9797 (odd, 5 mod 8) with K = 5: the ten pairs start at every residue of 8 elements, so the 16-byte load, the
    word loads and the shifted word loads all run; 1225 groups of 8 pixels are two workgroups per image, and the last 13 pixels
    are read element by element."""
    H, W, nc = 97, 101, 21
    keys = [[9, 4, 17, 0, 12], [3, 19, 8, 1, 6]]
    c = dict(cams=[K._maps(5, H, W, 700 + b) for b in range(2)], keys=keys, gt=np.stack([K._gt(H, W, [10, 5, 18, 1], 710 + b) for b in range(2)]),
             nc=nc, thresholds=K.SWEEP_16)
    want = R.sweep_confusion(c["cams"], c["keys"], c["gt"], c["thresholds"], nc)
    assert np.array_equal(sweep(CS, c).cpu().numpy(), want)
    assert np.array_equal(sweep(CS, c, force_global=True).cpu().numpy(), want)


def test_sweep_with_unevenly_spaced_thresholds(CS):
    """The kernel finds a pixel's threshold count from a straight-line guess and steps to the exact count: clustered, negative and
    far-out thresholds make the guess as wrong as it gets.  Case 1's maps (with their values equal to 0.25, 0.5 and 0.75)."""
    c = dict(K.case1())
    for thr in ([-0.5, 0.0, 0.001, 0.0011, 0.0012, 0.25, 0.5, 0.75, 0.7501, 0.98, 3.0], [0.5, 1e6], [-1e6, 0.25], [0.2, 0.2000001, 0.9]):
        c["thresholds"] = thr
        want = R.sweep_confusion(c["cams"], c["keys"], c["gt"], thr, c["nc"])
        assert np.array_equal(sweep(CS, c).cpu().numpy(), want), thr
        assert np.array_equal(sweep(CS, c, force_global=True).cpu().numpy(), want), thr


def test_case4_labels_and_merge(CS, golden):
    g, c = golden("camseed_ref.npz"), K.case1()
    cams, gt = dev(c)
    B, (H, W) = 3, c["gt"].shape[1:]
    low, high = CS.seed_labels(cams.view(-1, H, W), c["keys"], K.LOW_THRE, K.HIGH_THRE, c["nc"])
    assert low.dtype == torch.int64 and tuple(low.shape) == (B, H, W)
    for b in range(B):
        rl, rh = R.slot_maps(c["cams"][b], c["keys"][b], K.LOW_THRE, K.HIGH_THRE)
        assert np.array_equal(low[b].cpu().numpy(), rl) and np.array_equal(high[b].cpu().numpy(), rh)
    label, cmap, hist, cover = CS.merge_labels(low, high, c["keys"], c["nc"], gt=gt, want_cmap=True)
    label = label.cpu().numpy()
    assert label.dtype == np.uint8 and np.array_equal(label, g["case1_ignore_mid"])
    assert np.array_equal(hist.cpu().numpy(), g["case1_mask_hist"])
    assert cover.cpu().tolist() == [int(g["case1_mask_hist"].sum()), int(g["case1_conf"][0].sum())]
    assert np.array_equal(cmap.cpu().numpy(), golden("voc_cmap.npz")["cmap"][label])
    # accumulation, and the same through the registered op
    CS.merge_labels(low, high, c["keys"], c["nc"], gt=gt, hist=hist, cover=cover)
    assert np.array_equal(hist.cpu().numpy(), 2 * g["case1_mask_hist"])
    import weclip_vit_comer_amd
    weclip_vit_comer_amd.register_torch_ops()
    t = CS.PairTables(c["keys"], c["nc"], cams.device)
    ol, oh = torch.ops.weclip.cam_seed_labels(cams, t.first, t.keys, K.LOW_THRE, K.HIGH_THRE)
    assert torch.equal(ol.view(B, H, W), low) and torch.equal(oh.view(B, H, W), high)
    lab2, cmap2, hist2, cover2 = torch.ops.weclip.cam_seed_merge(ol, oh, t.slot_class, gt, c["nc"])
    assert np.array_equal(lab2.view(B, H, W).cpu().numpy(), label) and np.array_equal(hist2.cpu().numpy(), g["case1_mask_hist"])
    assert torch.equal(cmap2.view(B, H, W, 3), cmap)


@pytest.mark.parametrize("bilateral", ["exact", "lattice"])
def test_case5_crf_leg(CS, bilateral):
    from weclip_vit_comer_amd.utils import dcrf
    c = K.case1()
    cam, keys, gt = c["cams"][0], c["keys"][0], c["gt"][0]
    img = torch.from_numpy(K.case5_image()).cuda()
    ev = CS.SeedEvaluator(c["nc"], None, K.LOW_THRE, K.HIGH_THRE, refine="crf", crf_bilateral=bilateral, keep_labels=True)
    ev.add([{"keys": torch.tensor(keys), "attn_highres": torch.from_numpy(cam).cuda()}], [img], [gt], ["a"])
    got = ev.last_labels[0].cpu().numpy()
    res = ev.finish()
    low, high = R.slot_maps(cam, keys, K.LOW_THRE, K.HIGH_THRE)
    low_crf = dcrf.crf_inference_label(img, torch.from_numpy(low).cuda(), n_labels=len(keys) + 1, bilateral=bilateral).cpu().numpy()
    high_crf = dcrf.crf_inference_label(img, torch.from_numpy(high).cuda(), n_labels=len(keys) + 1, bilateral=bilateral).cpu().numpy()
    want = R.merge(low_crf, high_crf, keys)
    assert np.array_equal(got, want)
    assert (want != R.merge(low, high, keys)).any(), "the CRF changed nothing: the case does not test the leg"
    assert np.array_equal(res["masks"]["hist"], R.mask_hist([gt], [want], c["nc"]))
    assert [res["masks"]["labelled"], res["masks"]["valid"]] == R.coverage([gt], [want], c["nc"]).tolist()


def tiny_inputs(golden):
    g = golden("camgen_tiny.npz")
    n = int(g["n_images"])
    imgs = [torch.from_numpy(g[f"img{i}_src"]) for i in range(n)]
    labels = [g[f"img{i}_labels"].tolist() for i in range(n)]
    gts = [K._gt(im.shape[0], im.shape[1], [1 + labels[i][0], 1 + labels[i][-1], 9, 255], 800 + i) for i, im in enumerate(imgs)]
    return imgs, labels, gts


def test_case6_evaluator_on_device_payloads_equals_the_restatement(CS, golden, tmp_path):
    from PIL import Image
    from weclip_vit_comer_amd import clip
    from weclip_vit_comer_amd.clip.generate_cams import CamGenerator
    model, _ = clip.load(synth.make_clip_state_dict(**synth.TINY), device="cuda")
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    gen = CamGenerator(model, fg.cuda(), bg.cuda(), 0.4)
    imgs, labels, gts = tiny_inputs(golden)
    payloads = gen(imgs, labels, to_numpy=False)
    assert len({tuple(im.shape) for im in imgs}) < len(imgs), "no two images share a bucket: the multi-image block is untested"
    thr = K.SWEEP_16
    ev = CS.SeedEvaluator(21, thr, K.LOW_THRE, K.HIGH_THRE, out_dir=str(tmp_path), keep_labels=True)
    names = [f"im{i}" for i in range(len(imgs))]
    ev.add(payloads, imgs, gts, names)
    got_labels = [t.cpu().numpy() for t in ev.last_labels]
    res = ev.finish()
    cams = [p["attn_highres"].cpu().numpy() for p in payloads]
    keys = [p["keys"].tolist() for p in payloads]
    assert keys == labels
    want_labels = [R.ignore_mid_label(c, k, K.LOW_THRE, K.HIGH_THRE) for c, k in zip(cams, keys)]
    assert np.array_equal(res["bins"], R.sweep_bins(cams, keys, gts, thr, 21))
    assert np.array_equal(res["masks"]["hist"], R.mask_hist(gts, want_labels, 21))
    assert [res["masks"]["labelled"], res["masks"]["valid"]] == R.coverage(gts, want_labels, 21).tolist()
    assert res["images"] == len(imgs) and len(res["sweep"]) == 16
    table = golden("voc_cmap.npz")["cmap"]
    for n, got, want in zip(names, got_labels, want_labels):
        assert np.array_equal(got, want)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "prediction" / (n + ".png"))), want)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "prediction_cmap" / (n + ".png"))), table[want])


VOC_XML = "<annotation><size><width>{w}</width><height>{h}</height><depth>3</depth></size>{objs}</annotation>"


def test_case6_dumper_with_two_workers_in_a_child_process(golden, tmp_path):
    """python -m ...generate_cams_voc12 --num_workers 2 --gt_root ... --pseudo_dir ... on a four-image tree, in a fresh child
    (which starts the two workers itself): seed_scores.json is the sum of the workers' parts, the parts are the restatement's
    counts of the maps the workers saved, and the PNGs decode to those maps' labels."""
    from PIL import Image
    from weclip_vit_comer_amd.clip import cam_seeds as CS
    from weclip_vit_comer_amd.clip import generate_cams as G
    from weclip_vit_comer_amd.clip import tokenizer as TK
    imgs, labels, gts = tiny_inputs(golden)
    fg = [f"thing {chr(97 + i)}" for i in range(20)]
    root = tmp_path / "voc"
    for d in ("JPEGImages", "Annotations", "gt", "ref/clip"):
        (root / d).mkdir(parents=True)
    names = [f"2007_{i:06d}" for i in range(len(imgs))]
    for n, im, ids, gt in zip(names, imgs, labels, gts):
        Image.fromarray(im.numpy()).save(root / "JPEGImages" / (n + ".jpg"), format="PNG")          # lossless under the .jpg name
        objs = "".join(f"<object><name>{fg[i]}</name></object>" for i in ids)
        (root / "Annotations" / (n + ".xml")).write_text(VOC_XML.format(w=im.shape[1], h=im.shape[0], objs=objs))
        Image.fromarray(gt).save(root / "gt" / (n + ".png"))
    (root / "train.txt").write_text("\n".join(names) + "\n")
    bg = ["ground", "sky", "wall", "lower tree", "new water"]
    (root / "ref" / "clip" / "clip_text.py").write_text(f"class_names = {fg!r}\nnew_class_names = {fg!r}\nBACKGROUND_CATEGORY = {bg!r}\n")
    with gzip.open(root / "ref" / "clip" / TK.BPE_NAME, "wt", encoding="utf-8") as fh:
        fh.write("#version: test\nl o\nlo w</w>\ne r</w>\nn e\nne w\n")
    torch.save(synth.make_clip_state_dict(**synth.TINY), root / "tiny.pt")
    out, masks = root / "cams", root / "masks"
    cmd = [sys.executable, "-m", "weclip_vit_comer_amd.clip.generate_cams_voc12", "--img_root", str(root / "JPEGImages"), "--split_file",
           str(root / "train.txt"), "--cam_out_dir", str(out), "--model", str(root / "tiny.pt"), "--reference_root", str(root / "ref"),
           "--num_workers", "2", "--gt_root", str(root / "gt"), "--eval_thresholds", "0.05:0.80:0.05", "--pseudo_dir", str(masks)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    parts = [np.load(G.part_path(str(out), i)) for i in range(2)]
    assert [int(p["images"]) for p in parts] == [2, 2]
    got = json.load(open(out / "seed_scores.json"))
    total = {k: parts[0][k] + parts[1][k] for k in ("bins", "hist", "cover")}
    want = CS.to_json(CS.summarise(21, K.SWEEP_16, total["bins"], total["hist"], total["cover"], 4, 0.35, 0.55, "none", "exact"))
    assert got == json.loads(json.dumps(want))
    cams, keys = [], []
    for n in names:
        d = np.load(out / (n + ".npy"), allow_pickle=True).item()
        assert d["attn_highres"].dtype == np.float16 and d["keys"].dtype == np.int64
        cams.append(d["attn_highres"])
        keys.append(d["keys"].tolist())
    assert keys == labels
    want_labels = [R.ignore_mid_label(c, k, 0.35, 0.55) for c, k in zip(cams, keys)]
    assert np.array_equal(total["bins"], R.sweep_bins(cams, keys, gts, K.SWEEP_16, 21))
    assert np.array_equal(total["hist"], R.mask_hist(gts, want_labels, 21))
    assert total["cover"].tolist() == R.coverage(gts, want_labels, 21).tolist()
    table = golden("voc_cmap.npz")["cmap"]
    for n, lab in zip(names, want_labels):
        assert np.array_equal(np.asarray(Image.open(masks / "prediction" / (n + ".png"))), lab)
        assert np.array_equal(np.asarray(Image.open(masks / "prediction_cmap" / (n + ".png"))), table[lab])


def test_eval_cams_scores_existing_dumps(CS, golden, tmp_path):
    """python -m ...clip.eval_cams (called in process): case 1 written as the dumpers write it, one payload missing."""
    from PIL import Image
    from weclip_vit_comer_amd.clip import eval_cams as E
    from weclip_vit_comer_amd.clip import generate_cams as G
    g, c = golden("camseed_ref.npz"), K.case1()
    cams, gts = tmp_path / "cams", tmp_path / "gt"
    cams.mkdir()
    gts.mkdir()
    names = ["a", "b", "c"]
    for n, cam, keys, gt in zip(names, c["cams"], c["keys"], c["gt"]):
        G.save_payload(str(cams), n + ".jpg", {"keys": np.asarray(keys, np.int64), "attn_highres": cam})
        Image.fromarray(gt).save(gts / (n + ".png"))
    (tmp_path / "split.txt").write_text("a\nskipped\nb\nc\n")
    out = tmp_path / "scores.json"
    assert E.main(["--cam_dir", str(cams), "--gt_root", str(gts), "--split_file", str(tmp_path / "split.txt"), "--eval_thresholds",
                   "0.05:0.80:0.05", "--pseudo_dir", str(tmp_path / "masks"), "--chunk", "2", "--out", str(out)]) == 0
    got = json.load(open(out))
    assert got["images"] == 3
    assert np.array_equal(CS.confusion_from_bins(np.asarray(got["bins"], np.int64)), g["case1_conf"])
    assert np.array_equal(got["masks"]["hist"], g["case1_mask_hist"])
    for n, lab in zip(names, g["case1_ignore_mid"]):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "masks" / "prediction" / (n + ".png"))), lab)


def test_case7_argument_errors_raise_before_any_launch(CS):
    c = K.case2()
    cams, gt = dev(c)
    bins = torch.zeros(21, 21, 2, device="cuda", dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ascending"):
        CS.sweep_bins(cams, c["keys"], gt, [0.5, 0.4], 21)
    with pytest.raises(RuntimeError, match="65"):
        CS.sweep_bins(cams, c["keys"], gt, [i / 100 for i in range(65)], 21)
    with pytest.raises(RuntimeError, match="257"):
        CS.sweep_bins(cams, c["keys"], gt, [0.4], 257)
    with pytest.raises(RuntimeError, match="class id"):
        CS.sweep_bins(cams, [[20]], gt, [0.4], 21, bins=bins)
    with pytest.raises(RuntimeError, match="class id"):
        CS.seed_labels(cams, [[20]], 0.35, 0.55, 21)
    with pytest.raises(RuntimeError):
        CS.seed_labels(cams, c["keys"], 0.6, 0.5, 21)
    # the C entry has the same limits of its own (the custom op reaches it with device tables)
    import ctypes
    from weclip_vit_comer_amd import _lib as L
    t = CS.PairTables(c["keys"], 21, cams.device)
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    for thr, nc, T in (([0.5, 0.4], 21, 2), ([0.4] * 65, 21, 65), ([0.4], 257, 1), ([float("inf")], 21, 1)):
        with pytest.raises(RuntimeError, match="wc_cam_seed_sweep"):
            L.lib().wc_cam_seed_sweep(L.ptr(cams), L.ptr(t.first), L.ptr(t.keys), L.ptr(gt), (ctypes.c_float * len(thr))(*thr), L.ptr(bins),
                                      L.ptr(flag), 1, 1, cams.shape[1], nc, T, 1, 0, L.stream())
    torch.cuda.synchronize()
    assert int(bins.sum()) == 0 and int(flag.item()) == 0                # nothing ran


def test_a_class_id_out_of_range_in_device_tables_is_flagged_not_counted(CS):
    """The registered op's tables are device tensors: no host check.  The kernel skips such a pixel and raises the flag."""
    c = K.case2()
    cams, gt = dev(c)
    flag = CS._flag(cams.device)
    before = int(flag.item())
    first = torch.tensor([0, 1], device="cuda", dtype=torch.int32)
    keys = torch.tensor([20], device="cuda", dtype=torch.int32)
    t = CS.PairTables.from_device(21, first, keys, Kmax=1)
    for force in (False, True):
        flag.zero_()
        bins = CS.sweep_bins(cams, None, gt, [0.4], 21, tables=t, force_global=force)
        assert int(bins.sum()) == 0 and int(flag.item()) == 1
    flag.fill_(before)
