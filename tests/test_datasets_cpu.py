"""CPU tests of the dataset package (weclip_vit_comer_amd.datasets): files, names, class labels, the host-side aug=False
path against the reference fixture (tests/golden/dataset_ragged_ref.npz), the loader's index plan, the packed batch, the
host-computed img_box and the opt-in `datasets` alias of install_dropin."""
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import dataset_trees as DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def voc(tmp_path, golden):
    return DT.write_voc_tree(str(tmp_path / "voc"), golden("dataset_ragged_ref.npz"))


@pytest.fixture()
def coco(tmp_path):
    return DT.write_coco_tree(str(tmp_path / "coco"))


def test_voc_names_len_labels_and_raw(voc):
    from weclip_vit_comer_amd.datasets import voc as V
    root, lists, names = voc
    assert [str(n) for n in V.load_img_name_list(os.path.join(lists, "train.txt"))] == names
    table = V.load_cls_label_list(lists)
    assert sorted(table) == sorted(names)
    ds = V.VOC12ClsDataset(root_dir=root, name_list_dir=lists, split="train", stage="train", crop_size=96)
    seg = V.VOC12SegDataset(root_dir=root, name_list_dir=lists, split="val", stage="val")
    assert len(ds) == 7 and len(seg) == 3
    sizes = set()
    for i, name in enumerate(names):
        n, img, lab, cls = ds.raw(i)
        with Image.open(os.path.join(root, "JPEGImages", name + ".jpg")) as im:
            direct = np.asarray(im.convert("RGB"))
        assert n == name and lab is None and img.dtype == np.uint8 and np.array_equal(img, direct)
        assert np.array_equal(cls, table[name])
        sizes.add(img.shape[:2])
    assert len(sizes) == 7
    for i in range(3):
        n, img, lab, cls = seg.raw(i)
        with Image.open(os.path.join(root, "SegmentationClassAug", names[i] + ".png")) as im:
            assert im.mode == ("P" if i == 1 else "L")
            direct = np.array(im)
        assert lab.dtype == np.uint8 and lab.shape == img.shape[:2] and np.array_equal(lab, direct)
        assert np.array_equal(cls, table[names[i]])
    # the base class hands out the decoded pair, a test-stage dataset the first channel as the reference does
    n, img, lab = V.VOC12Dataset(root, lists, "val", "val")[1]
    assert n == names[1] and lab.shape == img.shape[:2]
    n, img, lab = V.VOC12Dataset(root, lists, "val", "test")[0]
    assert np.array_equal(lab, img[:, :, 0])


def test_palette_label_keeps_indices(voc, golden):
    from weclip_vit_comer_amd.datasets.voc import VOC12SegDataset
    root, lists, _ = voc
    g = golden("dataset_ragged_ref.npz")
    ds = VOC12SegDataset(root_dir=root, name_list_dir=lists, split="train", stage="train")
    for i in range(6):
        _, img, lab, _ = ds.raw(i)
        assert np.array_equal(img, g[f"image_{i}"]) and np.array_equal(lab, g[f"label_{i}"]), i


def test_getitem_without_aug_equals_reference_normalize(voc, golden):
    """aug=False __getitem__ against `normalize_img` of the unmodified reference (the fixture), exactly; and through a stock
    DataLoader with batch_size=1."""
    import torch
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset, VOC12SegDataset
    root, lists, names = voc
    g = golden("dataset_ragged_ref.npz")
    cls = VOC12ClsDataset(root_dir=root, name_list_dir=lists, split="train", stage="val", aug=False)
    seg = VOC12SegDataset(root_dir=root, name_list_dir=lists, split="train", stage="val", aug=False)
    for i in (int(v) for v in g["normalize_of"]):
        name, image, cls_label = cls[i]
        assert name == names[i] and image.dtype == np.float32 and np.array_equal(image, g[f"norm_{i}"])
        name, image, label, cls_label = seg[i]
        assert np.array_equal(image, g[f"norm_{i}"]) and np.array_equal(label, g[f"label_{i}"])
    batches = list(torch.utils.data.DataLoader(seg, batch_size=1, shuffle=False, num_workers=0))
    assert len(batches) == 7
    name, inputs, labels, cls_label = batches[2]
    assert list(name) == [names[2]] and tuple(cls_label.shape) == (1, 20)
    assert np.array_equal(inputs[0].numpy(), g["norm_2"]) and np.array_equal(labels[0].numpy(), g["label_2"])


def test_getitem_with_aug_raises_and_names_the_loader(voc, coco):
    from weclip_vit_comer_amd.datasets import coco as C, voc as V
    root, lists, _ = voc
    for cls in (V.VOC12ClsDataset, V.VOC12SegDataset):
        with pytest.raises(RuntimeError, match="DeviceLoader"):
            cls(root_dir=root, name_list_dir=lists, split="train", stage="train", aug=True)[0]
    root, lists, _ = coco
    for cls in (C.CocoClsDataset, C.CocoSegDataset):
        with pytest.raises(RuntimeError, match="DeviceLoader"):
            cls(root_dir=root, name_list_dir=lists, split="train", stage="train", aug=True)[0]


def test_coco_names_grey_image_and_labels(coco):
    from weclip_vit_comer_amd.datasets import coco as C
    root, lists, names = coco
    table = C.load_cls_label_list(lists)
    tr = C.CocoSegDataset(root_dir=root, name_list_dir=lists, split="train", stage="train")
    va = C.CocoClsDataset(root_dir=root, name_list_dir=lists, split="val", stage="val")
    assert len(tr) == 4 and len(va) == 2
    for i, full in enumerate(names["train"]):
        n, img, lab, cls = tr.raw(i)
        path = os.path.join(root, "JPEGImages", "train", full + ".jpg")
        with Image.open(path) as im:
            assert im.mode == ("L" if i == 2 else "RGB")
            direct = np.asarray(im.convert("RGB"))
            if i == 2:                           # what the reference's robust_read_image makes of a grey file
                grey = np.asarray(im)
                assert np.array_equal(direct, np.stack((grey, grey, grey), axis=-1))
        assert n == full[15:] and img.shape[2] == 3 and np.array_equal(img, direct)
        with Image.open(os.path.join(root, "SegmentationClass", "train", n + ".png")) as im:
            assert np.array_equal(lab, np.asarray(im))
        assert np.array_equal(cls, table[full])
    n, image, cls = va[1]
    assert n == names["val"][1][13:] and image.shape[0] == 3 and np.array_equal(cls, table[names["val"][1]])
    full, short, img, lab = C.CocoDataset(root, lists, "val", "val")[0]
    assert full == names["val"][0] and short == full[13:] and lab.shape == img.shape[:2]


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("drop_last", [False, True])
def test_index_plan_partitions_the_epoch(voc, world, drop_last):
    """7 images, batch 2: not divisible by world * batch for any world here.  No device is touched."""
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset
    root, lists, _ = voc
    ds = VOC12ClsDataset(root_dir=root, name_list_dir=lists, split="train", stage="train", crop_size=96, aug=True)
    n, batch = len(ds), 2
    assert n % (world * batch) != 0

    def loaders(seed):
        return [DeviceLoader(ds, batch, shuffle=True, drop_last=drop_last, seed=seed, rank=r, world=world) for r in range(world)]
    first, again = loaders(5), loaders(5)
    epochs = []
    for epoch in (0, 1):
        plans = [ld.plan(epoch) for ld in first]
        assert plans == [ld.plan(epoch) for ld in again]
        full = [index_plan_full(ds, batch, 5, epoch, r, world) for r in range(world)]
        seen = sorted(i for p in full for b in p for i in b)
        assert seen == list(range(n)), "every index exactly once per epoch across the ranks, before drop_last trimming"
        for r, (p, f, ld) in enumerate(zip(plans, full, first)):
            mine = len(range(r, n, world))
            assert len(p) == len(ld) == (mine // batch if drop_last else -(-mine // batch))
            assert p == (f[:mine // batch] if drop_last else f)
            assert all(len(b) == batch for b in p[:-1]) and (not drop_last or all(len(b) == batch for b in p))
        epochs.append(plans)
    assert epochs[0] != epochs[1]
    assert loaders(6)[0].plan(0) != first[0].plan(0) or n < 3
    unshuffled = DeviceLoader(ds, batch, shuffle=False, drop_last=False, rank=0, world=world).plan(0)
    assert [i for b in unshuffled for i in b] == list(range(0, n, world))


def index_plan_full(ds, batch, seed, epoch, rank, world):
    from weclip_vit_comer_amd.datasets import index_plan
    return index_plan(len(ds), batch, shuffle=True, drop_last=False, seed=seed, epoch=epoch, rank=rank, world=world)


def test_thread_count_is_capped(voc):
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset
    root, lists, _ = voc
    ds = VOC12ClsDataset(root_dir=root, name_list_dir=lists, crop_size=96, aug=True)
    assert DeviceLoader(ds, 2, threads=64).threads == 8 and DeviceLoader(ds, 2).threads == 4
    with pytest.raises(ValueError, match="batch_size"):
        DeviceLoader(VOC12ClsDataset(root_dir=root, name_list_dir=lists, aug=False), 2)


def test_packed_batch_layout(voc):
    from weclip_vit_comer_amd.datasets import pack_batch
    from weclip_vit_comer_amd.datasets.voc import VOC12SegDataset
    root, lists, _ = voc
    ds = VOC12SegDataset(root_dir=root, name_list_dir=lists, split="train", stage="train")
    items = [ds.raw(i) for i in (4, 0, 6, 2)]
    images, labels = [it[1] for it in items], [it[2] for it in items]
    rec = np.arange(4 * 16, dtype=np.int32).reshape(4, 16)
    buf, offsets, sizes, lay = pack_batch(images, labels, (rec,))
    nbytes = [im.shape[0] * im.shape[1] * 3 for im in images]
    assert offsets.dtype == np.int64 and offsets.tolist() == [0] + np.cumsum(nbytes)[:-1].tolist()
    assert sizes.dtype == np.int32 and sizes.tolist() == [list(im.shape[:2]) for im in images]
    assert lay["images"] == (0, sum(nbytes)) and lay["labels"] == (sum(nbytes), sum(nbytes) + sum(nbytes) // 3)
    for b, (im, lab) in enumerate(zip(images, labels)):
        assert np.array_equal(buf[offsets[b]:offsets[b] + nbytes[b]].reshape(im.shape), im)
        o = lay["labels"][0] + offsets[b] // 3
        assert np.array_equal(buf[o:o + lab.size].reshape(lab.shape), lab)
    for key, arr in (("offsets", offsets), ("sizes", sizes), ("table0", rec)):
        a, e = lay[key]
        assert a % 16 == 0 and np.array_equal(buf[a:e].view(arr.dtype).reshape(arr.shape), arr)
    assert lay["total"] == buf.size
    # without labels, into a caller's buffer that is larger than needed
    big = np.full(lay["total"] + 100, 7, np.uint8)
    out, offsets2, _, lay2 = pack_batch(images, None, (), out=big)
    assert out is big and lay2["labels"][0] == lay2["labels"][1] and offsets2.tolist() == offsets.tolist()
    with pytest.raises(ValueError, match="at least"):
        pack_batch(images, labels, (rec,), out=np.empty(100, np.uint8))


def test_host_img_box_equals_reference(golden):
    from weclip_vit_comer_amd.data import DeviceAugment
    g = golden("dataset_ragged_ref.npz")
    crop = int(g["crop"])
    for i in range(int(g["n_cases"])):
        H, W = g[f"image_{i}"].shape[:2]
        box = DeviceAugment.img_box(DT.cls_draw(g["cls_draws"][i], H, W), crop)
        assert box.dtype == np.int16 and np.array_equal(box, g[f"cls_img_box_{i}"]), (i, box, g[f"cls_img_box_{i}"])


def test_labels_from_onehot():
    import torch
    from weclip_vit_comer_amd.datasets import labels_from_onehot
    v = torch.zeros(2, 20)
    v[0, [3, 7]] = 1
    v[1, 19] = 1
    assert labels_from_onehot(v) == [[3, 7], [19]]


@pytest.mark.parametrize("enable", [False, True])
def test_install_dropin_datasets_alias_is_opt_in(enable):
    """A fresh interpreter each: by default `import datasets` is none of this package's business; with datasets=True it is."""
    code = (
        "import sys, importlib.util\n"
        "import weclip_vit_comer_amd as P\n"
        f"P.install_dropin({'datasets=True' if enable else ''})\n"
        "assert P.DROPIN_NAMES == ('clip', 'pytorch_grad_cam', 'WeCLIP_model', 'utils')\n"
        "if %r:\n"
        "    import datasets\n"
        "    from datasets import voc, coco\n"
        "    import weclip_vit_comer_amd.datasets as real\n"
        "    assert datasets is real and voc is real.voc and coco is real.coco and datasets.DeviceLoader\n"
        "    print('aliased')\n"
        "else:\n"
        "    spec = None\n"
        "    try:\n"
        "        spec = importlib.util.find_spec('datasets')\n"
        "    except (ImportError, ValueError):\n"
        "        pass\n"
        "    m = None\n"
        "    if spec is not None:\n"
        "        import datasets as m\n"
        "    assert m is None or 'weclip' not in (getattr(m, '__file__', '') or ''), m\n"
        "    assert 'datasets' not in sys.modules or m is not None\n"
        "    print('untouched')\n" % enable)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=str(os.path.dirname(ROOT)))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("aliased" if enable else "untouched")
