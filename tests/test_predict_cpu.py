"""CPU tests of the predict entry point (weclip_vit_comer_amd.predict): the command line, `ImageFolderDataset`, the writer pool
behind the host stand-ins of tests/test_msc_flip_eval_cpu.py, summary.json, and the fp64 restatement's hand-computed cases."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import dataset_trees as DT
import predict_ref as R
import weclip_vit_comer_amd  # noqa: F401  (import alias for the hyphenated package dir)
from weclip_vit_comer_amd import _lib
from weclip_vit_comer_amd import predict as P
from weclip_vit_comer_amd.datasets.folder import ImageFolderDataset


# ---------------------------------------------------------------------------------------------- the command line
def test_parser_defaults():
    a = P.parse_args(["--images", "photos"])
    assert (a.config, a.model_path, a.dataset) == ("configs/voc_attn_reg.yaml", "/your/path/WeCLIP/WeCLIP_model_iter_30000.pth", "voc")
    assert (a.scales, a.resize_long, a.crf, a.crf_bilateral, a.threads, a.writers) == ([1.0, 0.75], 512, False, "exact", 8, 4)
    assert (a.images, a.split, a.recursive, a.out_dir) == ("photos", None, False, "predictions")
    assert (a.outputs, a.alpha, a.ignore_below, a.palette) == (("prediction", "prediction_cmap"), 0.5, 0, False)
    c = P.parse_args(["--dataset", "coco", "--split", "test"])
    assert (c.config, c.model_path, c.split, c.images) == (
        "configs/coco_attn_reg.yaml", "/your/path/WeCLIP/WeCLIP_model_iter_80000.pth", "test", None)


def test_parser_switches_and_refusals():
    a = P.parse_args(["--images", "d", "--recursive", "--outputs", "overlay, confidence,prediction", "--palette", "--alpha", "0.25",
                      "--ignore_below", "200", "--crf", "--crf_bilateral", "lattice", "--scales", "1"])
    assert a.outputs == ("prediction", "confidence", "overlay")          # the fixed order, whatever the user's
    assert (a.recursive, a.palette, a.alpha, a.ignore_below, a.crf, a.crf_bilateral, a.scales) == (True, True, 0.25, 200, True, "lattice", [1.0])
    assert P.parse_args(["--images", "d", "--outputs", ""]).outputs == ()
    for bad in (["--images", "d", "--split", "test"], [], ["--images", "d", "--ignore_below", "256"], ["--images", "d", "--alpha", "1.5"],
                ["--images", "d", "--outputs", "logit"], ["--split", "test", "--recursive"]):
        with pytest.raises(SystemExit):
            P.parse_args(bad)


def test_new_symbol_is_declared():
    protos = {name: args for name, _, args in _lib.parse_header()}
    assert [n for _, n in protos["wc_predict_finish"]] == ["src", "image", "pred_u8", "cmap_rgb", "conf_u8", "overlay_rgb", "stats", "C",
                                                          "Hs", "Ws", "H", "W", "mode", "alpha256", "ignore_below", "stream"]
    from weclip_vit_comer_amd import torch_ops
    assert "predict_finish" in torch_ops.OPS


def test_palette_is_the_golden_table(golden):
    assert np.array_equal(np.array(P.voc_palette(), np.uint8).reshape(256, 3), golden("voc_cmap.npz")["cmap"])


# ---------------------------------------------------------------------------------------------- ImageFolderDataset
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """a.jpg (RGB), b.PNG (grey, upper-case extension), c.bmp, d.webp, notes.txt, sub/e.jpeg, sub/deep/f.png."""
    root = str(tmp_path_factory.mktemp("photos"))
    os.makedirs(os.path.join(root, "sub", "deep"))
    sizes = {"a.jpg": (31, 45), "b.PNG": (20, 17), "c.bmp": (9, 12), "d.webp": (16, 16), "sub/e.jpeg": (25, 33), "sub/deep/f.png": (7, 5)}
    for i, (rel, (H, W)) in enumerate(sizes.items()):
        img = DT.smooth_image(H, W, i)
        im = Image.fromarray(img[..., 0]) if rel == "b.PNG" else Image.fromarray(img)
        im.save(os.path.join(root, rel), **({"format": "PNG"} if rel == "b.PNG" else {}))
    with open(os.path.join(root, "notes.txt"), "w") as f:
        f.write("not an image\n")
    return root, sizes


def test_folder_dataset_on_a_directory(folder):
    root, sizes = folder
    ds = ImageFolderDataset(root)
    assert (ds.kind, ds.aug, len(ds)) == ("cls", False, 4)
    assert ds.name_list == ["a", "b", "c", "d"]                           # sorted; the sub-directory and notes.txt are not taken
    assert ds.sizes() == [sizes[k] for k in ("a.jpg", "b.PNG", "c.bmp", "d.webp")]
    for i in range(len(ds)):
        name, image, label, cls = ds.raw(i)
        assert label is None and cls.dtype == np.uint8 and cls.shape == (1,) and not cls.any()
        assert image.dtype == np.uint8 and image.shape == ds.sizes()[i] + (3,)
    grey = ds.raw(1)[1]                                                   # the grey PNG comes out as RGB with equal channels
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 0], DT.smooth_image(20, 17, 1)[..., 0])
    assert np.array_equal(ds.raw(2)[1], DT.smooth_image(9, 12, 2))        # BMP is lossless
    name, chw, cls = ds[2]
    assert name == "c" and chw.shape == (3, 9, 12) and chw.dtype == np.float32


def test_folder_dataset_recursive_mirrors_sub_directories(folder):
    root, sizes = folder
    ds = ImageFolderDataset(root, recursive=True)
    assert ds.name_list == ["a", "b", "c", "d", "sub/deep/f", "sub/e"]
    assert ds.sizes()[4:] == [sizes["sub/deep/f.png"], sizes["sub/e.jpeg"]]


def test_folder_dataset_on_a_glob_and_a_list_file(folder, tmp_path):
    root, sizes = folder
    g = ImageFolderDataset(os.path.join(root, "*.[jP]*"))                  # a.jpg and b.PNG
    assert g.name_list == ["a", "b"] and os.path.samefile(g.base, root)
    deep = ImageFolderDataset(os.path.join(root, "**", "*.png"), recursive=True)      # f.png alone (b.PNG is upper case)
    assert deep.name_list == ["f"]
    both = ImageFolderDataset(os.path.join(root, "**", "*.jp*g"), recursive=True)
    assert both.name_list == ["a", "sub/e"]
    lst = tmp_path / "list.txt"
    lst.write_text(f"# my images\n{os.path.join(root, 'sub', 'e.jpeg')}\n\n{os.path.join(root, 'c.bmp')}\n")
    ds = ImageFolderDataset(str(lst))
    assert ds.name_list == ["c", "sub/e"] and ds.sizes() == [sizes["c.bmp"], sizes["sub/e.jpeg"]]
    (tmp_path / "rel.txt").write_text("x.png\n")
    Image.fromarray(DT.smooth_image(4, 6, 0)).save(str(tmp_path / "x.png"))
    assert ImageFolderDataset(str(tmp_path / "rel.txt")).name_list == ["x"]           # relative to the list file
    (tmp_path / "missing.txt").write_text("nowhere.png\n")
    with pytest.raises(FileNotFoundError, match="nowhere.png"):
        ImageFolderDataset(str(tmp_path / "missing.txt"))
    with pytest.raises(FileNotFoundError):
        ImageFolderDataset(str(tmp_path / "no_such_*.jpg"))


def test_folder_dataset_refuses_two_inputs_with_one_name(tmp_path):
    for ext in ("jpg", "png"):
        Image.fromarray(DT.smooth_image(6, 8, 0)).save(str(tmp_path / f"same.{ext}"))
    with pytest.raises(ValueError, match="same"):
        ImageFolderDataset(str(tmp_path))


def test_crf_size_check_names_the_images(tmp_path):
    Image.new("RGB", (800, 600)).save(str(tmp_path / "big.png"))           # 480,000 pixels > 640^2 = 409,600
    Image.new("RGB", (640, 640)).save(str(tmp_path / "fits.png"))
    with pytest.raises(RuntimeError, match=r"big \(600x800\)"):
        P.check_crf_sizes(ImageFolderDataset(str(tmp_path)))
    os.remove(str(tmp_path / "big.png"))
    P.check_crf_sizes(ImageFolderDataset(str(tmp_path)))


# ---------------------------------------------------------------------------------------------- the writer
class _Event:
    """Stands in for torch.cuda.Event: the host 'copy' is complete when copy_ returns."""

    def record(self):
        pass

    def synchronize(self):
        pass


def _host_alloc(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8), torch.empty(nbytes, dtype=torch.uint8)


def _fill(slot, seed, H, W):
    rs = np.random.RandomState(seed)
    data = {}
    for k, view in slot.views.items():
        data[k] = rs.randint(0, 256, tuple(view.shape)).astype(np.uint8)
        view.copy_(torch.from_numpy(data[k]))
    return data


SIZES = [(7, 9), (33, 17), (5, 5), (64, 3), (9, 40), (33, 17), (12, 13)]          # more images than buffers; growing and shrinking


@pytest.mark.parametrize("palette", [False, True])
def test_writer_pool_writes_all_four_kinds(tmp_path, golden, palette):
    out = str(tmp_path / "out")
    pool = P.PredictWriterPool(out, P.KINDS, palette=palette, writers=3, depth=2, alloc=_host_alloc, event=_Event)
    expect = {}
    for i, (H, W) in enumerate(SIZES):
        slot = pool.acquire(H, W)
        assert sorted(slot.views) == sorted(P.KINDS) and all(v.data_ptr() % 4 == slot.dev.data_ptr() % 4 for v in slot.views.values())
        name = f"img_{i}" if i % 2 else f"sub/dir/img_{i}"
        expect[name] = _fill(slot, i, H, W)
        pool.commit(slot, name)
    assert pool.finish() == len(SIZES)
    assert sorted(os.listdir(out)) == sorted(P.KINDS)
    table = golden("voc_cmap.npz")["cmap"]
    for name, data in expect.items():
        modes = {}
        for k in P.KINDS:
            with Image.open(os.path.join(out, k, name + ".png")) as im:
                modes[k] = im.mode
                if k == "prediction" and palette:                          # the same index bytes under the VOC palette
                    assert np.array_equal(np.array(im.getpalette(), np.uint8).reshape(256, 3), table)
                    assert np.array_equal(np.asarray(im.convert("RGB")), table[data[k]])
                assert np.array_equal(np.asarray(im), data[k]), (name, k)
        assert modes == {"prediction": "P" if palette else "L", "prediction_cmap": "RGB", "confidence": "L", "overlay": "RGB"}


def test_writer_pool_makes_only_the_requested_directories(tmp_path):
    out = str(tmp_path / "out")
    pool = P.PredictWriterPool(out, ("confidence", "prediction"), writers=1, alloc=_host_alloc, event=_Event)
    slot = pool.acquire(6, 10)
    assert sorted(slot.views) == ["confidence", "prediction"] and slot.layout[3] == 120
    data = _fill(slot, 0, 6, 10)
    pool.commit(slot, "one")
    assert pool.finish() == 1
    assert sorted(os.listdir(out)) == ["confidence", "prediction"]
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, "confidence", "one.png"))), data["confidence"])
    default = P.PredictWriterPool(str(tmp_path / "default"), writers=1, alloc=_host_alloc, event=_Event)
    assert default.finish() == 0 and sorted(os.listdir(str(tmp_path / "default"))) == ["prediction", "prediction_cmap"]


def test_the_parents_pool_is_unchanged(tmp_path):
    """PredictWriterPool and msc_flip_eval.WriterPool are siblings on one ring; the evaluation pool's tree and layout stay."""
    from weclip_vit_comer_amd import msc_flip_eval as E
    pool = E.WriterPool(str(tmp_path / "val"), writers=1, alloc=_host_alloc, event=_Event)
    slot = pool.acquire(5, 7)
    assert sorted(slot.views) == ["cmap", "pred"] and slot.layout == (5, 7, None, 140)
    assert pool.finish() == 0 and sorted(os.listdir(str(tmp_path / "val"))) == ["prediction", "prediction_cmap"]


# ---------------------------------------------------------------------------------------------- summary.json
def test_summary_is_strict_json_sorted_by_name():
    C = 3
    stats = np.array([[6, 0, 2, 6 * 255, 0, 300, 2],           # 10 pixels: class 0 sure, class 2 at 150 / 255, 2 ignored
                      [0, 0, 0, 0, 0, 0, 4]], np.int64)          # every pixel ignored: no class entry, nothing divides by zero
    recs = P.image_records(["b/img", "a"], [(2, 5), (2, 2)], stats, C)
    s = P.make_summary(recs, {"alpha": 0.5, "crf": None, "bad": float("nan")})
    assert json.loads(json.dumps(s, allow_nan=False)) == s
    assert s["images"] == 2 and [r["name"] for r in s["per_image"]] == ["a", "b/img"] and s["args"]["bad"] is None
    a, b = s["per_image"]
    assert a == {"name": "a", "size": [2, 2], "classes": {}, "ignored": 1.0}
    assert b["size"] == [2, 5] and b["ignored"] == 0.2 and sorted(b["classes"]) == ["0", "2"]
    assert b["classes"]["0"] == {"share": 0.6, "confidence": 1.0}
    assert b["classes"]["2"] == {"share": 0.2, "confidence": 150 / 255}
    with pytest.raises(RuntimeError, match="twice"):
        P.make_summary(recs + recs[:1], {})


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_one_class_is_sure_everywhere(golden):
    table = golden("voc_cmap.npz")["cmap"]
    src = np.random.RandomState(0).randn(1, 3, 3).astype(np.float32) * 5
    for mode, s in ((0, src), (1, np.ones((1, 5, 5), np.float32))):
        r = R.predict_finish(s, (5, 5), table, mode=mode, ignore_below=255)
        assert (r["conf"] == 255).all() and (r["pred"] == 0).all() and r["stats"].tolist() == [25, 25 * 255, 0]


def test_two_equal_logits_give_128_and_the_first_label(golden):
    table = golden("voc_cmap.npz")["cmap"]
    src = np.full((2, 2, 2), 1.75, np.float32)
    r = R.predict_finish(src, (3, 4), table)
    assert (r["conf"] == 128).all() and (r["pred"] == 0).all()            # 255 / 2 + 0.5 = 128.0
    assert r["stats"].tolist() == [12, 0, 12 * 128, 0, 0]
    r = R.predict_finish(src, (3, 4), table, ignore_below=129)             # 128 < 129: every pixel ignored, conf untouched
    assert (r["pred"] == 255).all() and (r["conf"] == 128).all() and r["stats"].tolist() == [0, 0, 0, 0, 12]
    assert (r["cmap"] == table[255]).all()
    r = R.predict_finish(src, (3, 4), table, ignore_below=128)             # the comparison is strict
    assert (r["pred"] == 0).all()


def test_known_softmax_and_rounding(golden):
    table = golden("voc_cmap.npz")["cmap"]
    src = np.zeros((3, 1, 1), np.float32)
    src[1] = np.log(2.0)                                                   # probabilities 1/4, 1/2, 1/4 (to float32 accuracy)
    r = R.predict_finish(src, (1, 1), table)
    assert r["pred"].item() == 1 and r["conf"].item() == 128 and abs(r["x"].item() - 127.5) < 1e-5
    q = np.array([0.125, 0.75, 0.125], np.float32).reshape(3, 1, 1)
    r = R.predict_finish(q, (1, 1), table, mode=1)
    assert r["pred"].item() == 1 and r["conf"].item() == 191               # 255 * 0.75 = 191.25
    assert R.predict_finish(np.array([[[1.5]], [[-2.0]]], np.float32), (1, 1), table, mode=1)["conf"].item() == 255      # clamped


def test_bilinear_grid_and_first_maximum(golden):
    table = golden("voc_cmap.npz")["cmap"]
    src = np.zeros((2, 1, 2), np.float32)
    src[0, 0] = [4.0, 0.0]
    src[1, 0] = [0.0, 4.0]
    r = R.predict_finish(src, (1, 4), table)                               # source x = -0.25 -> 0, 0.25, 0.75, 1.25 -> 1
    assert r["best"].tolist() == [[0, 0, 1, 1]]
    assert np.allclose(R.values(src, (1, 4))[0, 0], [4.0, 3.0, 1.0, 0.0])
    tie = R.predict_finish(np.zeros((2, 1, 2), np.float32), (1, 2), table)
    assert tie["best"].tolist() == [[0, 0]]


def test_overlay_ends_are_the_image_and_the_colour(golden):
    table = golden("voc_cmap.npz")["cmap"]
    rs = np.random.RandomState(3)
    src = rs.randn(21, 4, 5).astype(np.float32)
    image = rs.randint(0, 256, (9, 11, 3)).astype(np.uint8)
    r0 = R.predict_finish(src, (9, 11), table, image=image, alpha256=0)
    r256 = R.predict_finish(src, (9, 11), table, image=image, alpha256=256)
    assert np.array_equal(r0["overlay"], image) and np.array_equal(r256["overlay"], r256["cmap"])
    assert np.array_equal(r256["cmap"], table[r256["pred"]])
    half = R.predict_finish(src, (9, 11), table, image=image, alpha256=128)["overlay"].astype(int)
    assert np.abs(half - (r256["cmap"].astype(int) + image) / 2).max() <= 0.5
    assert R.predict_finish(src, (9, 11), table)["overlay"] is None
    assert r0["stats"][:21].sum() == 99 and r0["stats"][42] == 0


def test_band_is_narrow():
    x = np.array([10.5, 10.5 + 1e-3, 10.0, 254.49999])
    assert R.band(x, 21).tolist() == [True, False, False, True]            # d = 255 * 58 * 2^-24 = 8.8e-4
