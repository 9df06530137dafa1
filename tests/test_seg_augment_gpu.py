"""GPU tests of the label-aware device input pipeline (data.DeviceSegAugment, csrc/augment_seg.hip): the reference fixture,
the tie to the pinned image-only `DeviceAugment`, OpenCV's 8-bit HSV restatement on all 2^24 colours, the loader's real
geometry against the tests' numpy restatement (tests/segaug_ref.py, itself pinned to the fixture on the CPU), graph capture
with device-resident parameters, and three SupervisedTrainStep steps fed by the seg loader."""
import ctypes

import numpy as np
import pytest
import torch

import photo_ref
import segaug_ref
from oracle import synth

pytestmark = pytest.mark.gpu


def _u8_images(n, H, W, seed):
    f = synth.make_images(n, H, W, seed=seed)
    return (f * 58.0 + 118.0).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _check(aug, imgs, labs, draws, crop, tag=""):
    """Run `aug` on the batch with `draws` and compare everything with the numpy restatement.  -> chosen indices, accepted."""
    out, lab, box = aug(imgs.cuda(), labs.cuda(), aug.pack(draws))
    out, lab, box, sel = out.cpu().numpy(), lab.cpu().numpy(), box.cpu().numpy(), aug.sel.cpu().numpy()
    assert out.shape == (len(draws), 3, crop, crop) and lab.dtype == np.int64 and box.dtype == np.int32
    for b, d in enumerate(draws):
        r_out, r_lab, r_box, chosen, ok = segaug_ref.chain(imgs[b].numpy(), labs[b].numpy(), d, crop)
        assert sel[b].tolist() == [d[11][chosen][0], d[11][chosen][1], chosen, int(ok)], (tag, b, sel[b], chosen, ok)
        assert np.array_equal(box[b], r_box), (tag, b, box[b], r_box)
        assert np.array_equal(lab[b], r_lab), (tag, b, (lab[b] != r_lab).mean())
        diff = np.abs(out[b] - r_out)
        assert np.array_equal(out[b], r_out), (tag, b, d[:11], diff.max(), (diff > 0).mean())
    return sel[:, 2], sel[:, 3]


def test_seg_pipeline_equals_reference_fixture(golden):
    """Image (to the last bit), label, img_box and chosen candidate index against the fixture made by the reference's own
    transforms (tests/golden/make_segaug_golden.py), the recorded draws fed through DeviceSegAugment's host side.  Where the
    reference stopped drawing candidates early the device path gets the recorded candidates plus filler ones: two different
    fillers give the same, reference-equal result."""
    from weclip_vit_comer_amd.data import DeviceSegAugment
    g = golden("seg_augment_ref.npz")
    crop = int(g["crop"])
    n_filled = 0
    for i in range(int(g["n_cases"])):
        group = int(g["group"][i])
        img, lab = torch.from_numpy(g[f"image_{i}"]), torch.from_numpy(g[f"label_{i}"])
        names, vals = [str(n) for n in g[f"draw_names_{i}"]], g[f"draw_vals_{i}"]
        for filler in ("min", "max"):
            aug = DeviceSegAugment(crop_size=crop, rescale_range=(0.5, 2.0) if group == 2 else None)
            d, filled = segaug_ref.replay_draw(aug, names, vals, *lab.shape, filler=filler)
            n_filled += filled
            out, ol, box = aug(img[None].cuda(), lab[None].cuda(), aug.pack([d]))
            diff = np.abs(out[0].cpu().numpy() - g[f"out_{i}"])
            print(f"case {i} group {group} filler {filler}: max abs diff {diff.max():.3e}, chosen {aug.sel[0].tolist()}")
            assert np.array_equal(out[0].cpu().numpy(), g[f"out_{i}"]), (i, diff.max(), (diff > 0).mean())
            assert np.array_equal(ol[0].cpu().numpy(), g[f"out_label_{i}"]), i
            assert box[0].tolist() == g[f"img_box_{i}"].tolist(), i
            n_tried = len(g[f"cand_{i}"])
            assert aug.sel[0].tolist()[:3] == g[f"cand_{i}"][-1].tolist() + [n_tried - 1], i
    assert n_filled > 0


@pytest.mark.parametrize("rescale", [None, (0.5, 2.0)])
def test_seg_gather_without_photometric_equals_device_augment(rescale):
    """photometric=False and the same geometry draws: the image is DeviceAugment's output bit for bit."""
    from weclip_vit_comer_amd.data import DeviceAugment, DeviceSegAugment
    for (H, W, crop, B) in [(54, 76, 64, 6), (375, 500, 512, 4)]:
        imgs = _u8_images(B, H, W, seed=40 + H)
        labs = synth.make_label_maps(B, H, W, seed=3)
        ref = DeviceAugment(crop_size=crop, rescale_range=rescale, seed=17)
        draws = [ref.draw_one(H, W) for _ in range(B)]
        want = ref(imgs.cuda(), ref.pack(draws))
        aug = DeviceSegAugment(crop_size=crop, rescale_range=rescale, photometric=False, seed=1)
        mine = [(s, flip, rh, rw, py, px, 0, 0.0, 1.0, 1.0, 0, [(cy, cx)] * 10) for s, flip, rh, rw, py, px, cy, cx in draws]
        got, lab, _ = aug(imgs.cuda(), labs.cuda(), aug.pack(mine))
        assert torch.equal(got, want), (H, W, (got - want).abs().max().item())
        assert aug.sel[:, :2].tolist() == [[d[6], d[7]] for d in draws]
        _check(aug, imgs, labs, mine, crop, "tie")


def test_hsv_kernels_equal_restatement_on_all_colours():
    from weclip_vit_comer_amd import _lib as L
    rgb = photo_ref.all_colours()
    src = torch.from_numpy(rgb).cuda()
    dst = torch.empty_like(src)
    for inverse, fn in ((0, photo_ref.bgr2hsv), (1, photo_ref.hsv2bgr)):
        L.lib().wc_hsv8_convert(L.ptr(src, torch.uint8), L.ptr(dst, torch.uint8), ctypes.c_long(src.shape[0]), inverse, L.stream())
        got, want = dst.cpu().numpy(), fn(rgb)
        bad = (got != want).any(axis=1)
        print(f"hsv8 inverse={inverse}: {int(bad.sum())} of {len(bad)} triples differ")
        assert not bad.any(), (inverse, rgb[bad][:5], got[bad][:5], want[bad][:5])


def test_seg_pipeline_full_geometry_against_restatement():
    """375 x 500 sources, crop 512, B = 16 with the class's own draws; a batch of single-class maps where every image
    exhausts its candidates; a rescaled batch (Pillow BILINEAR image / NEAREST label)."""
    from weclip_vit_comer_amd.data import DeviceSegAugment
    B, H, W, crop = 16, 375, 500, 512
    imgs = _u8_images(B, H, W, seed=77)
    labs = synth.make_label_maps(B, H, W, regions=8, seed=31)
    aug = DeviceSegAugment(crop_size=crop, seed=5)
    chosen, ok = _check(aug, imgs, labs, [aug.draw_one(H, W) for _ in range(B)], crop, "full")
    print("full geometry: chosen", chosen.tolist(), "accepted", ok.tolist())
    one = synth.make_label_maps(B, H, W, regions=1, seed=2)
    chosen, ok = _check(aug, imgs, one, [aug.draw_one(H, W) for _ in range(B)], crop, "single class")
    assert chosen.tolist() == [9] * B and not ok.any()
    aug = DeviceSegAugment(crop_size=crop, rescale_range=(0.5, 2.0), seed=6)
    draws = [aug.draw_one(H, W) for _ in range(4)]
    assert min(d[0] for d in draws) < 0.95 and max(d[0] for d in draws) > 1.1
    _check(aug, imgs[:4], labs[:4], draws, crop, "rescaled")
    assert aug(imgs.cuda(), labs.cuda())[1].shape == (B, crop, crop)      # fresh draw path
    with pytest.raises(RuntimeError):                                     # beyond the 4x down-scaling the tables hold
        bad = (0.2, 0, 75, 100, 0, 0, 0, 0.0, 1.0, 1.0, 0, [(0, 0)])
        aug(imgs[:1].cuda(), labs[:1].cuda(), aug.pack([bad]))
    with pytest.raises(RuntimeError, match="n_cand"):
        DeviceSegAugment(crop_size=crop, n_cand=17)(imgs.cuda(), labs.cuda(), (torch.zeros(B, 16, dtype=torch.int32).cuda(),
                                                                             torch.zeros(B, 17, 2, dtype=torch.int32).cuda()))


def test_seg_pipeline_graph_capture_with_device_params():
    """Device-resident records and candidates: the call is captured as a graph (nothing in it may synchronise with the host)
    and replayed with new parameters and new sources in the static buffers; equal to eager."""
    from weclip_vit_comer_amd.data import DeviceSegAugment
    B, H, W, crop = 4, 96, 120, 64
    aug = DeviceSegAugment(crop_size=crop, seed=9)
    batches = []
    for k in range(3):
        imgs, labs = _u8_images(B, H, W, seed=90 + k).cuda(), synth.make_label_maps(B, H, W, seed=60 + k).cuda()
        rec, cand = aug.draw(B, H, W)
        batches.append((imgs, labs, rec.cuda(), cand.cuda()))
    eager = []
    for imgs, labs, rec, cand in batches:
        o = aug(imgs, labs, (rec, cand))
        eager.append([t.clone() for t in o] + [aug.sel.clone()])
    s_img, s_lab, s_rec, s_cand = (t.clone() for t in batches[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = aug(s_img, s_lab, (s_rec, s_cand))
        g_sel = aug.sel
    for k in (1, 2, 0):
        for dst, src in zip((s_img, s_lab, s_rec, s_cand), batches[k]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(list(g_out) + [g_sel], eager[k]):
            assert torch.equal(got, want), k
    assert not torch.equal(eager[0][0], eager[1][0])


def test_supervised_steps_fed_by_the_seg_loader():
    """Three SupervisedTrainStep steps on the seg loader's (image, label) crops; the losses are finite and equal those of a
    second, identically initialised model fed the same crops prepared on the CPU by the tests' restatement."""
    from test_seg_variant_gpu import _seg_model
    from weclip_vit_comer_amd.data import DeviceSegAugment, SyntheticVOCLoader
    from weclip_vit_comer_amd.train_step import SupervisedTrainStep
    B, crop, hw, seed = 2, 64, (48, 80), 300

    def run(feed):
        torch.manual_seed(0)
        step = SupervisedTrainStep(_seg_model())
        return [step(*feed(k)).item() for k in range(3)]

    loader = SyntheticVOCLoader(B, crop, seed=seed, pool=2, source="seg", src_hw=hw)
    got = run(lambda k: loader.next())
    twin = SyntheticVOCLoader(B, crop, seed=seed, pool=2, source="seg", src_hw=hw)
    host = DeviceSegAugment(crop_size=crop, seed=seed)

    def cpu_feed(k):
        imgs, labs = twin.images[k % 2].cpu().numpy(), twin.labels[k % 2].cpu().numpy()
        res = [segaug_ref.chain(imgs[b], labs[b], host.draw_one(*hw), crop) for b in range(B)]
        return (torch.from_numpy(np.stack([r[0] for r in res])).cuda(), torch.from_numpy(np.stack([r[1] for r in res])).cuda())
    want = run(cpu_feed)
    print("seg loader losses", got, "restatement-fed", want)
    assert all(np.isfinite(got)) and got == want
