"""GPU tests of the ragged device input pipeline and the dataset loader (csrc/augment.hip, csrc/augment_seg.hip,
weclip_vit_comer_amd.datasets): the ragged kernels against the fixture made by the unmodified reference
(tests/golden/dataset_ragged_ref.npz) and against the uniform kernels, bit for bit; wc_normalize_u8; one epoch of
DeviceLoader recomputed from raw() and the loader's own draws through the B=1 path; two TrainStep steps fed by it."""
import numpy as np
import pytest
import torch

import dataset_trees as DT
from oracle import synth

pytestmark = pytest.mark.gpu


def _pack(images, labels=None, tables=()):
    """pack_batch -> the device tensors the ragged entry points take."""
    from weclip_vit_comer_amd.datasets import pack_batch
    buf, offsets, sizes, lay = pack_batch(images, labels, tables)
    dev = torch.from_numpy(buf).cuda()
    src = dev[lay["images"][0]:lay["images"][1]]
    lab = dev[lay["labels"][0]:lay["labels"][1]] if labels is not None else None
    return src, lab, torch.from_numpy(offsets).cuda(), torch.from_numpy(sizes).cuda()


def _cls_aug(crop):
    from weclip_vit_comer_amd.data import DeviceAugment
    return DeviceAugment(crop_size=crop)


def _seg_aug(crop, **kw):
    from weclip_vit_comer_amd.data import DeviceSegAugment
    return DeviceSegAugment(crop_size=crop, **kw)


def test_ragged_cls_kernel_equals_reference_fixture(golden):
    """The six images of six sizes as ONE packed batch with the recorded draws: every value equals the reference's."""
    g = golden("dataset_ragged_ref.npz")
    crop, cases = int(g["crop"]), DT.fixture_cases(g)
    aug = _cls_aug(crop)
    draws = [DT.cls_draw(g["cls_draws"][i], *img.shape[:2]) for i, (img, _) in enumerate(cases)]
    src, _, offsets, sizes = _pack([c[0] for c in cases])
    rec = aug.pack(draws)
    aug.check_ragged(rec, [c[0].shape[:2] for c in cases])
    out = aug.ragged(src, offsets, sizes, rec.cuda()).cpu().numpy()
    for i in range(len(cases)):
        diff = np.abs(out[i] - g[f"cls_out_{i}"])
        print(f"cls case {i} {cases[i][0].shape[:2]} scale {draws[i][0]:.3f}: max abs diff {diff.max():.3e}, differing {(diff > 0).mean():.3e}")
    for i in range(len(cases)):
        assert np.array_equal(out[i], g[f"cls_out_{i}"]), i
    # each image alone through the uniform entry (B = 1, same parameters): bit-identical to its slice of the ragged batch
    for i, (img, _) in enumerate(cases):
        one = aug(torch.from_numpy(img)[None].cuda(), aug.pack([draws[i]])).cpu().numpy()[0]
        assert np.array_equal(one, out[i]), i


def test_ragged_seg_kernel_equals_reference_fixture(golden):
    """Image, label, img_box and the chosen candidate of the six-size batch against the fixture; two fillers for the
    candidates the reference did not draw; and each image alone through the uniform entry."""
    g = golden("dataset_ragged_ref.npz")
    crop, cases = int(g["crop"]), DT.fixture_cases(g)
    results = []
    for filler in ("min", "max"):
        aug = _seg_aug(crop)
        draws = [DT.seg_draw(aug, g, i, filler) for i in range(len(cases))]
        src, lab, offsets, sizes = _pack([c[0] for c in cases], [c[1] for c in cases])
        rec, cand = aug.pack(draws)
        cm = aug.check_ragged(rec, cand, [c[0].shape[:2] for c in cases])
        assert cm == max(max(c[0].shape[:2]) for c in cases)
        out, ol, box = aug.ragged(src, lab, offsets, sizes, rec.cuda(), cand.cuda(), cm)
        out, ol, box, sel = out.cpu().numpy(), ol.cpu().numpy(), box.cpu().numpy(), aug.sel.cpu().numpy()
        for i in range(len(cases)):
            diff = np.abs(out[i] - g[f"seg_out_{i}"])
            print(f"seg case {i} filler {filler}: max abs diff {diff.max():.3e}, label mismatches "
                  f"{(ol[i] != g[f'seg_out_label_{i}']).sum()}, box {box[i].tolist()} sel {sel[i].tolist()}")
        for i in range(len(cases)):
            assert np.array_equal(out[i], g[f"seg_out_{i}"]), i
            assert ol.dtype == np.int64 and np.array_equal(ol[i], g[f"seg_out_label_{i}"]), i
            assert box[i].tolist() == g[f"seg_img_box_{i}"].tolist(), i
            n_tried = len(g[f"seg_cand_{i}"])
            assert sel[i].tolist()[:3] == g[f"seg_cand_{i}"][-1].tolist() + [n_tried - 1], i
        for i, (img, l) in enumerate(cases):
            one = _seg_aug(crop)
            o1, l1, b1 = one(torch.from_numpy(img)[None].cuda(), torch.from_numpy(l)[None].cuda(), one.pack([draws[i]]))
            assert np.array_equal(o1[0].cpu().numpy(), out[i]) and np.array_equal(l1[0].cpu().numpy(), ol[i]), i
            assert b1[0].tolist() == box[i].tolist() and one.sel[0].tolist() == sel[i].tolist(), i
        results.append(out)
    assert np.array_equal(results[0], results[1])


@pytest.mark.parametrize("rescale", [None, (0.5, 2.0)])
def test_ragged_seg_mixed_sizes_equal_single_image_path(rescale):
    """Fresh draws (rescaling included, which the fixture's Seg chain does not have) on a mixed-size batch: every image
    alone through DeviceSegAugment with B = 1 gives the bits of its slice, candidates rejected and accepted alike."""
    sizes = [(70, 90), (131, 64), (64, 64), (97, 150), (50, 47)]
    crop = 64
    imgs = [(synth.make_images(1, H, W, seed=900 + i) * 58.0 + 118.0).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1)[0].contiguous()
            for i, (H, W) in enumerate(sizes)]
    labs = [synth.make_label_maps(1, H, W, regions=1 + 2 * i, seed=40 + i)[0].contiguous() for i, (H, W) in enumerate(sizes)]
    aug = _seg_aug(crop, rescale_range=rescale, seed=3)
    draws = [aug.draw_one(H, W) for H, W in sizes]
    src, lab, offsets, szs = _pack([i.numpy() for i in imgs], [l.numpy() for l in labs])
    rec, cand = aug.pack(draws)
    cm = aug.check_ragged(rec, cand, sizes)
    out, ol, box = aug.ragged(src, lab, offsets, szs, rec.cuda(), cand.cuda(), cm)
    sel = aug.sel.clone()
    assert not torch.isnan(out).any()
    for b in range(len(sizes)):
        one = _seg_aug(crop, rescale_range=rescale)
        o1, l1, b1 = one(imgs[b][None].cuda(), labs[b][None].cuda(), one.pack([draws[b]]))
        assert torch.equal(o1[0], out[b]) and torch.equal(l1[0], ol[b]) and torch.equal(b1[0], box[b]), b
        assert torch.equal(one.sel[0], sel[b]), b
    assert len({int(s) for s in sel[:, 2]}) > 1 or int(sel[:, 3].min()) == 0


def test_ragged_entries_equal_uniform_entries_on_equal_sizes():
    """A batch of equal-sized images: wc_augment_normalize_ragged / wc_seg_augment_ragged give the bits of
    wc_augment_normalize / wc_seg_augment."""
    B, H, W, crop = 5, 75, 100, 64
    imgs = (synth.make_images(B, H, W, seed=950) * 58.0 + 118.0).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    labs = synth.make_label_maps(B, H, W, regions=5, seed=51).contiguous()
    src, lab, offsets, sizes = _pack(list(imgs.numpy()), list(labs.numpy()))
    assert offsets.tolist() == [b * H * W * 3 for b in range(B)]
    aug = _cls_aug(crop)
    rec = aug.draw(B, H, W)
    assert torch.equal(aug.ragged(src, offsets, sizes, rec.cuda()), aug(imgs.cuda(), rec))
    for rescale in (None, (0.5, 2.0)):
        seg = _seg_aug(crop, rescale_range=rescale, seed=9)
        rec, cand = seg.draw(B, H, W)
        o0, l0, b0 = seg(imgs.cuda(), labs.cuda(), (rec, cand))
        s0 = seg.sel.clone()
        o1, l1, b1 = seg.ragged(src, lab, offsets, sizes, rec.cuda(), cand.cuda(), seg.canvas_max(H, W))
        assert torch.equal(o0, o1) and torch.equal(l0, l1) and torch.equal(b0, b1) and torch.equal(s0, seg.sel)


def test_ragged_image_outside_the_buffer_is_poisoned_not_read():
    """The device-side check of the tables: an extent beyond the packed buffer gives NaN / ignore for that image only."""
    crop = 32
    imgs = [np.full((40, 50, 3), 90, np.uint8), np.full((30, 36, 3), 200, np.uint8)]
    labs = [np.full((40, 50), 4, np.uint8), np.full((30, 36), 6, np.uint8)]
    src, lab, offsets, sizes = _pack(imgs, labs)
    bad = sizes.clone()
    bad[1, 0] = 4000                                                # claims far more rows than the buffer holds
    aug = _cls_aug(crop)
    draws = [(1.0, 0, 40, 50, 0, 0, 0, 0), (1.0, 0, 30, 36, 0, 0, 0, 0)]
    out = aug.ragged(src, offsets, bad, aug.pack(draws).cuda())
    assert not torch.isnan(out[0]).any() and torch.isnan(out[1]).all()
    seg = _seg_aug(crop, photometric=False, fliplr=False)
    d = [seg.draw_one(40, 50), seg.draw_one(30, 36)]
    rec, cand = seg.pack(d)
    o, l, _ = seg.ragged(src, lab, offsets, bad, rec.cuda(), cand.cuda(), 64)
    assert not torch.isnan(o[0]).any() and (l[0] == 4).all() and torch.isnan(o[1]).all() and (l[1] == 255).all()


def test_normalize_u8_equals_reference_fixture(golden):
    from weclip_vit_comer_amd.data import normalize_u8
    g = golden("dataset_ragged_ref.npz")
    for i in (int(v) for v in g["normalize_of"]):
        img, lab = torch.from_numpy(g[f"image_{i}"]).cuda(), torch.from_numpy(g[f"label_{i}"]).cuda()
        out, ol = normalize_u8(img, lab)
        diff = np.abs(out.cpu().numpy() - g[f"norm_{i}"])
        print(f"normalize case {i}: max abs diff {diff.max():.3e}")
        assert np.array_equal(out.cpu().numpy(), g[f"norm_{i}"]), i
        assert ol.dtype == torch.int64 and np.array_equal(ol.cpu().numpy(), g[f"label_{i}"])
        assert torch.equal(normalize_u8(img), out)
    # every byte value in every channel against numpy's own evaluation
    ramp = torch.arange(256, dtype=torch.uint8)[:, None, None].expand(256, 1, 3).contiguous()
    from weclip_vit_comer_amd.datasets.voc import normalize_chw
    assert np.array_equal(normalize_u8(ramp.cuda()).cpu().numpy(), normalize_chw(ramp.numpy()))


def _recompute(ds, loader, names, kind):
    """One yielded batch again from raw() + the loader's recorded draws, image by image through the B = 1 uniform path."""
    index = {str(n): i for i, n in enumerate(ds.name_list)}
    outs = []
    for name, d in zip(names, loader.last_draws):
        _, img, lab, cls = ds.raw(index[name])
        if kind == "cls":
            aug = _cls_aug(ds.crop_size)
            outs.append((aug(torch.from_numpy(img)[None].cuda(), aug.pack([d]))[0], None, cls))
        else:
            aug = _seg_aug(ds.crop_size)
            o, l, _ = aug(torch.from_numpy(img)[None].cuda(), torch.from_numpy(lab)[None].cuda(), aug.pack([d]))
            outs.append((o[0], l[0], cls))
    return outs


@pytest.mark.parametrize("kind", ["cls", "seg"])
def test_device_loader_epoch_equals_recomputation(tmp_path, golden, kind):
    """One full epoch with prefetch=2, threads=4, batches kept alive until the end and compared only then (a buffer reused
    too early would have changed an earlier batch... or the one read while the next was staged); a second loader with the
    same seed yields identical batches."""
    from weclip_vit_comer_amd.data import DeviceAugment
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset, VOC12SegDataset
    root, lists, names = DT.write_voc_tree(str(tmp_path / "voc"), golden("dataset_ragged_ref.npz"))
    cls = VOC12ClsDataset if kind == "cls" else VOC12SegDataset
    ds = cls(root_dir=root, name_list_dir=lists, split="train", stage="train", crop_size=64, aug=True)

    def epoch(loader):
        got = []
        for batch in loader:
            got.append((batch, _recompute(ds, loader, batch[0], kind), list(loader.last_draws)))
        return got
    first = epoch(DeviceLoader(ds, 2, shuffle=True, drop_last=False, seed=11, threads=4, prefetch=2))
    torch.cuda.synchronize()
    assert len(first) == 4 and sorted(n for b, _, _ in first for n in b[0]) == sorted(names)
    for batch, ref, draws in first:
        B = len(batch[0])
        inputs = batch[1]
        assert inputs.is_cuda and inputs.dtype == torch.float32 and tuple(inputs.shape) == (B, 3, 64, 64)
        assert not torch.isnan(inputs).any()
        cls_labels = batch[2] if kind == "cls" else batch[3]
        assert cls_labels.is_cuda and tuple(cls_labels.shape) == (B, 20)
        for b in range(B):
            assert torch.equal(inputs[b], ref[b][0]), (batch[0], b)
            assert np.array_equal(cls_labels[b].cpu().numpy(), ref[b][2])
            if kind == "cls":
                assert batch[3].dtype == torch.int16 and batch[3][b].tolist() == DeviceAugment.img_box(draws[b], 64).tolist()
            else:
                assert batch[2].dtype == torch.int64 and torch.equal(batch[2][b], ref[b][1])
    second = epoch(DeviceLoader(ds, 2, shuffle=True, drop_last=False, seed=11, threads=4, prefetch=2))
    assert len(second) == len(first)
    for (a, _, _), (b, _, _) in zip(first, second):
        assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    # the next epoch of the same loader is another order or other draws
    ld = DeviceLoader(ds, 2, seed=11)
    e0 = [b[1].clone() for b in ld]
    e1 = [b[1].clone() for b in ld]
    assert ld.epoch == 2 and not all(torch.equal(x, y) for x, y in zip(e0, e1))


def test_device_loader_equal_sizes_reproduce_device_augment_draws(tmp_path):
    """A tree of equal-sized images: the loader's parameters are the ones DeviceAugment(seed) draws for the batch itself."""
    import os
    from PIL import Image
    from weclip_vit_comer_amd.data import DeviceAugment
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset
    root, lists = str(tmp_path / "eq"), str(tmp_path / "eq" / "lists")
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(lists)
    names = [f"im{i}" for i in range(4)]
    for i, n in enumerate(names):
        Image.fromarray(DT.smooth_image(60, 84, i)).save(os.path.join(root, "JPEGImages", n + ".jpg"), quality=90)
    open(os.path.join(lists, "train.txt"), "w").write("\n".join(names) + "\n")
    np.save(os.path.join(lists, "cls_labels_onehot.npy"), {n: np.eye(20, dtype=np.float32)[i] for i, n in enumerate(names)})
    ds = VOC12ClsDataset(root_dir=root, name_list_dir=lists, crop_size=48, aug=True)
    ld = DeviceLoader(ds, 4, shuffle=False, seed=21)
    (got_names, inputs, cls_labels, box), = list(ld)
    ref = DeviceAugment(crop_size=48, seed=21)
    rec = ref.draw(4, 60, 84)
    assert torch.equal(DeviceAugment.pack(ld.last_draws), rec)
    imgs = torch.stack([torch.from_numpy(ds.raw(i)[1]) for i in range(4)]).cuda()
    assert got_names == names and torch.equal(inputs, ref(imgs, rec))


def test_device_loader_without_aug_yields_normalized_image(tmp_path, golden):
    from weclip_vit_comer_amd.datasets import DeviceLoader
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset, VOC12SegDataset
    g = golden("dataset_ragged_ref.npz")
    root, lists, names = DT.write_voc_tree(str(tmp_path / "voc"), g)
    seg = VOC12SegDataset(root_dir=root, name_list_dir=lists, split="val", stage="val", aug=False)
    out = list(DeviceLoader(seg, 1, shuffle=False))
    assert len(out) == 3
    for i, (name, inputs, labels, cls_label) in enumerate(out):
        host = seg[i]
        assert name == [names[i]] and tuple(inputs.shape) == (1, 3) + host[1].shape[1:] and tuple(labels.shape) == (1,) + host[2].shape
        assert np.array_equal(inputs[0].cpu().numpy(), host[1]) and np.array_equal(labels[0].cpu().numpy(), host[2])
        assert labels.dtype == torch.int64 and tuple(cls_label.shape) == (1, 20)
    assert np.array_equal(out[0][1][0].cpu().numpy(), g["norm_0"]) and np.array_equal(out[2][1][0].cpu().numpy(), g["norm_2"])
    cls = VOC12ClsDataset(root_dir=root, name_list_dir=lists, split="val", stage="val", aug=False)
    name, inputs, cls_label = next(iter(DeviceLoader(cls, 1, shuffle=False)))
    assert np.array_equal(inputs[0].cpu().numpy(), g["norm_0"])


def test_train_steps_fed_by_the_device_loader(tmp_path, golden):
    """Two TrainStep steps at a small size from files on disk: finite losses."""
    from weclip_vit_comer_amd.datasets import DeviceLoader, labels_from_onehot
    from weclip_vit_comer_amd.datasets.voc import VOC12ClsDataset
    from weclip_vit_comer_amd.train_step import TrainStep
    root, lists, _ = DT.write_voc_tree(str(tmp_path / "voc"), golden("dataset_ragged_ref.npz"))
    ds = VOC12ClsDataset(root_dir=root, name_list_dir=lists, split="train", stage="train", crop_size=64, aug=True)
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP
    sd = synth.make_clip_state_dict(**synth.TINY)
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
    model = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4,
                   dataset_root_path=None, device="cuda", text_features=(bg.cuda(), fg.cuda()))
    model.decoder_fts_fuse.load_state_dict(fuse)
    model.decoder.load_state_dict(dec)
    model.train()
    step = TrainStep(model)
    losses = []
    for names, inputs, cls_labels, box in DeviceLoader(ds, 2, drop_last=True, seed=2):
        labels = labels_from_onehot(cls_labels)
        assert all(len(ids) >= 1 for ids in labels)
        out = step(inputs, labels=labels)
        losses.append([float(v) for v in out])
        print("step", len(losses), names, labels, losses[-1])
        if len(losses) == 2:
            break
    torch.cuda.synchronize()
    assert len(losses) == 2 and all(np.isfinite(v) for vals in losses for v in vals), losses
