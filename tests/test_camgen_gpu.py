"""Stand-alone CAM generation on the MI355X: wc_clip_preprocess against Pillow's recorded output, the output
kernel against the reference's recorded scale_cam_image, CamGenerator against the per-image API and against itself across
bucket sizes, GradCAM(target_size=...), the driver's files.  GPU tests read only committed fixtures."""
import os
import signal
import sys

import numpy as np
import pytest
import torch

from oracle import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

# CAM map on [0, 1] in the same precision mode: tests/test_gradcam_gpu.py:48 (8e-3, measured 1.7e-3 / 2.9e-3)
CAM_TOL = 8e-3


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own limit."""
    def boom(*_):
        raise TimeoutError("test exceeded its 180 s limit")
    old = signal.signal(signal.SIGALRM, boom)
    signal.alarm(180)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def test_clip_preprocess_equals_pillow_bit_for_bit(golden):
    from weclip_vit_comer_amd.clip.generate_cams import ClipPreprocess
    g = golden("clip_preprocess.npz")
    pre = ClipPreprocess()
    for i in range(int(g["n_cases"])):
        src = torch.from_numpy(g[f"c{i}_src"]).cuda()
        out, flip, u8 = pre(src, scale=float(g[f"c{i}_scale"]), flip=True, return_u8=True)
        u8, out, flip = u8[0].cpu().numpy(), out[0].cpu().numpy(), flip[0].cpu().numpy()
        bad8 = np.count_nonzero(u8 != g[f"c{i}_u8"])
        bad = np.count_nonzero(out.view(np.uint32) != g[f"c{i}_out"].view(np.uint32))
        badf = np.count_nonzero(flip.view(np.uint32) != g[f"c{i}_flip"].view(np.uint32))
        print(f"case {i} {tuple(src.shape)} -> {u8.shape}: differing uint8 {bad8}, f32 {bad}, flipped f32 {badf}")
        assert bad8 == 0 and bad == 0 and badf == 0, f"case {i}"


def test_clip_preprocess_batch_equals_single_images():
    from weclip_vit_comer_amd.clip.generate_cams import ClipPreprocess
    src = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (3, 37, 50, 3), dtype=np.uint8)).cuda()
    pre = ClipPreprocess()
    both = pre(src)
    assert both.shape == (3, 3, 48, 64)
    for b in range(3):
        assert torch.equal(both[b], pre(src[b])[0])
        ref = PR.clip_normalize(PR.bicubic_resize_u8(src[b].cpu().numpy(), 48, 64))
        assert np.array_equal(both[b].cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_clip_preprocess_at_the_8x_table_limit():
    """128 x 160 -> 16 x 20 is exactly 8x, the largest ratio the host accepts (its tap bound is 33 = PREP_KMAX): the widest windows
    the shared coefficient routine (csrc/resample.h) sees from a valid call, 32 taps of the 33 the table holds.  The uint8 image
    equals the restatement of Pillow's BICUBIC."""
    import ctypes
    from weclip_vit_comer_amd import _lib as L
    from weclip_vit_comer_amd.clip.generate_cams import CLIP_MEAN, CLIP_STD
    img = np.random.default_rng(8).integers(0, 256, (128, 160, 3), dtype=np.uint8)
    src = torch.from_numpy(img).cuda()
    n = ctypes.c_long(0)
    L.lib().wc_clip_preprocess_workspace_bytes(1, 128, 160, 16, 20, ctypes.byref(n))
    ws = torch.empty(n.value, device="cuda", dtype=torch.uint8)
    dst = torch.empty(1, 3, 16, 20, device="cuda", dtype=torch.float32)
    u8 = torch.empty(1, 16, 20, 3, device="cuda", dtype=torch.uint8)
    L.lib().wc_clip_preprocess(L.ptr(src, torch.uint8, "images"), L.ptr(dst), None, L.ptr(u8), L.ptr(ws), ws.numel(), 1, 128, 160, 16, 20,
                               (ctypes.c_float * 3)(*CLIP_MEAN), (ctypes.c_float * 3)(*CLIP_STD), L.stream())
    ref = PR.bicubic_resize_u8(img, 16, 20)
    got = u8[0].cpu().numpy()
    assert np.array_equal(got, ref), np.count_nonzero(got != ref)


def test_output_kernel_within_one_fp16_ulp_of_the_reference(golden):
    from weclip_vit_comer_amd.clip.generate_cams import resize_cam_f32, scale_cam_f16
    g = golden("cam_scale_resize.npz")
    grids = {}
    for i in range(int(g["n_pairs"])):
        grids.setdefault(g[f"p{i}_cam"].shape, []).append(i)
    assert max(len(v) for v in grids.values()) >= 3                   # one launch serves pairs of different target sizes
    for (gh, gw), idx in grids.items():
        cams = torch.from_numpy(np.stack([g[f"p{i}_cam"].reshape(-1) for i in idx])).cuda()
        sizes = [g[f"p{i}_out"].shape for i in idx]
        for i, hi, plain in zip(idx, scale_cam_f16(cams, gh, gw, sizes), resize_cam_f32(cams, gh, gw, sizes)):
            hi, plain = hi.cpu().numpy(), plain.cpu().numpy()
            assert hi.dtype == np.float16 and hi.shape == g[f"p{i}_out"].shape
            d = PR.f16_ulp_distance(hi, g[f"p{i}_out"])
            e = np.abs(plain - g[f"p{i}_plain"]).max()
            print(f"pair {i} {(gh, gw)} -> {hi.shape}: max fp16 ulp distance {d.max()}, differing {np.count_nonzero(d)}; plain resize abs {e:.2e}")
            assert d.max() <= 1
            # fp32 bilinear: 2 subtractions for the weights, 6 products and 3 sums, each rounded once (<= eps / 2 of a value
            # bounded by the map's maximum) in both implementations, fused or not: 8 eps of the maximum bounds the difference
            assert e <= 8 * np.finfo(np.float32).eps * np.abs(g[f"p{i}_plain"]).max()


def _tiny_generator(thr, max_bucket=16):
    from weclip_vit_comer_amd import clip
    from weclip_vit_comer_amd.clip.generate_cams import CamGenerator
    model, _ = clip.load(synth.make_clip_state_dict(**synth.TINY), device="cuda")
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    return CamGenerator(model, fg.cuda(), bg.cuda(), thr, max_bucket=max_bucket), model, bg, fg


def _tiny_images():
    rng = np.random.default_rng(21)
    sizes = [(60, 90), (64, 96), (60, 90), (49, 81), (60, 90)]
    labels = [[3, 7], [0], [14, 2, 5], [9, 1], []]
    base = (synth.make_images(1, 64, 96)[0].permute(1, 2, 0).numpy())
    base = (255 * (base - base.min()) / (base.max() - base.min())).astype(np.uint8)
    imgs = [torch.from_numpy(np.clip(base[:h, :w].astype(np.int64) + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8))
            for h, w in sizes]
    return imgs, labels


@pytest.mark.parametrize("thr", [0.4, 0.7])
def test_cam_generator_payload_and_per_image_api(thr):
    """keys / dtypes / shapes of the dumpers' payload, and the maps against the per-image API that already exists
    (perform_single_voc_cam with the refinement of the training model's normal branch) + the numpy output stage."""
    from weclip_vit_comer_amd.clip import clip_tool as CT
    from weclip_vit_comer_amd.pytorch_grad_cam import GradCAM
    gen, model, bg, fg = _tiny_generator(thr)
    imgs, labels = _tiny_images()
    res = gen(imgs, labels)
    assert res[4] is None and gen.skipped == [4]
    cam = GradCAM(model=model, target_layers=[model.visual.transformer.resblocks[-1].ln_1])
    single = CT.perform_single_voc_cam if thr == 0.4 else CT.perform_single_coco_cam
    for i in range(4):
        r, (H0, W0) = res[i], imgs[i].shape[:2]
        assert r["keys"].dtype == np.int64 and r["keys"].tolist() == labels[i]
        assert r["attn_highres"].dtype == np.float16 and r["attn_highres"].shape == (len(labels[i]), H0, W0)
        x = gen.pre(imgs[i].cuda())
        h, w = x.shape[-2:]
        assert (h, w) == PR.target_size(H0, W0)
        fts, attns = model.encode_image(x, h, w, require_all_fts=True)
        refined, ids, _, _ = single(None, x[0], fts[-1], [a[0] for a in attns], None, bg.cuda(), fg.cuda(), cam, mode="val",
                                    labels=labels[i])
        assert ids == labels[i]
        for k, rc in enumerate(refined):
            want = PR.scale_cam_resize_f16(rc.cpu().numpy(), H0, W0).astype(np.float32)
            err = np.abs(r["attn_highres"][k].astype(np.float32) - want).max()
            print(f"thr {thr} image {i} class {labels[i][k]}: attn_highres abs {err:.2e}")
            assert err < CAM_TOL


@pytest.mark.parametrize("flavour,thr", [("voc", 0.4), ("coco", 0.7)])
def test_cam_generator_end_to_end_against_the_reference_perform(golden, flavour, thr):
    """CamGenerator against the reference's `perform` recorded in camgen_tiny.npz (tests/golden/make_camgen_golden.py).
    keys, boxes and the preprocessed tensor: exact.  grayscale_cam: 8e-3 abs on [0, 1] (tests/test_gradcam_gpu.py:48).
    cam_refined has no counterpart there; its bound is composed from the cited ones: cam_refined = T_sym^2 (mask * cam) with
    T_sym rows of non-negative weights, so an error of 8e-3 of the CAM's maximum (1) passes through as at most 8e-3 of the
    refined map's scale, and each of the two applications of T adds the attention tolerance of tests/test_gradcam_gpu.py:47
    (2e-3 relative): 8e-3 + 2 * 2e-3 = 1.2e-2 of the refined map's maximum.  attn_highres = (refined - min) / (max - min),
    interpolated with weights in [0, 1] and rounded to fp16: the same 1.2e-2 scaled by max / (max - min) of the RECORDED
    refined map (a property of the input, not of the code under test), plus one fp16 ulp at 1 (9.8e-4)."""
    g = golden("camgen_tiny.npz")
    n = int(g["n_images"])
    gen, _, _, _ = _tiny_generator(thr)
    imgs = [torch.from_numpy(g[f"img{i}_src"]) for i in range(n)]
    labels = [g[f"img{i}_labels"].tolist() for i in range(n)]
    from weclip_vit_comer_amd.clip.generate_cams import bucket_images, resize_cam_f32
    buckets, _ = bucket_images([im.shape[:2] for im in imgs], labels, 16)
    assert any(len(b) == 2 for b in buckets)
    for idx in buckets:                       # bucket by bucket, so that the intermediates of each one can be read
        res = gen([imgs[i] for i in idx], [labels[i] for i in idx])
        st, boxes = gen.last, gen.last_boxes()
        p = 0
        for j, i in enumerate(idx):
            assert res[j]["keys"].dtype == np.int64 and res[j]["keys"].tolist() == g[f"{flavour}{i}_keys"].tolist()
            assert np.array_equal(st["input"][j].cpu().numpy().view(np.uint32), g[f"img{i}_input"].view(np.uint32))
            for k in range(len(labels[i])):
                gray, ref = st["grayscale_cam"][p].cpu().numpy(), st["cam_refined"][p].cpu().numpy()
                want_ref = g[f"{flavour}{i}_refined"][k]
                e_gray = np.abs(gray - g[f"{flavour}{i}_gray"][k]).max()
                e_ref = np.abs(ref - want_ref).max() / want_ref.max()
                amp = want_ref.max() / (want_ref.max() - want_ref.min())
                e_hi = np.abs(res[j]["attn_highres"][k].astype(np.float32) - g[f"{flavour}{i}_attn_highres"][k].astype(np.float32)).max()
                print(f"[{flavour}] image {i} class {labels[i][k]}: grayscale_cam abs {e_gray:.2e}, cam_refined rel-to-max {e_ref:.2e}, "
                      f"attn_highres abs {e_hi:.2e} (bound {1.2e-2 * amp + 9.8e-4:.2e}), boxes {boxes[p]}")
                assert boxes[p] == sorted(map(tuple, g[f"{flavour}{i}_boxes{k}"].tolist()))
                assert e_gray < CAM_TOL                          # measured on the MI355X (fast): 3.6e-4 .. 1.7e-3
                assert e_ref < 1.2e-2                            # measured: 1.0e-6 .. 1.4e-3
                assert e_hi < 1.2e-2 * amp + 9.8e-4              # measured: 9.5e-7 .. 1.5e-3 (bound 1.3e-2 for every pair)
                assert res[j]["attn_highres"].dtype == np.float16
                # the dumpers' "highres" map, cv2.resize(grayscale_cam, (ori_w, ori_h)): convex weights, so the CAM bound holds
                gh, gw = st["grid"]
                hr = resize_cam_f32(st["grayscale_cam"][p].reshape(1, -1), gh, gw, [tuple(imgs[i].shape[:2])])[0].cpu().numpy()
                assert np.abs(hr - g[f"{flavour}{i}_highres"][k]).max() < CAM_TOL
                p += 1


@pytest.mark.parametrize("precision", ["fast", "exact"])
def test_bucket_of_same_size_images_equals_images_run_alone(precision):
    from weclip_vit_comer_amd import config
    old = config.precision
    config.precision = precision
    try:
        imgs, labels = _tiny_images()
        together = _tiny_generator(0.4)[0](imgs, labels)
        alone = _tiny_generator(0.4, max_bucket=1)[0](imgs, labels)
        for i in range(4):
            assert together[i]["keys"].tolist() == alone[i]["keys"].tolist() == labels[i]
            err = np.abs(together[i]["attn_highres"].astype(np.float32) - alone[i]["attn_highres"].astype(np.float32)).max()
            print(f"[{precision}] image {i}: bucket vs alone abs {err:.2e}")
            assert err < CAM_TOL
    finally:
        config.precision = old


def test_gradcam_target_size():
    from weclip_vit_comer_amd import clip
    from weclip_vit_comer_amd.clip.clip_tool import ClipOutputTarget
    from weclip_vit_comer_amd.pytorch_grad_cam import GradCAM
    model, _ = clip.load(synth.make_clip_state_dict(**synth.TINY), device="cuda")
    H, W = synth.TINY_HW
    fts, _ = model.encode_image(synth.make_images(1, H, W).cuda(), H, W, require_all_fts=True)
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    text = torch.cat([fg[[3, 7]], bg], 0).cuda()
    cam = GradCAM(model=model, target_layers=[model.visual.transformer.resblocks[-1].ln_1])
    low, _, _ = cam(input_tensor=[fts[-1], text, H, W], targets=[ClipOutputTarget(1)], target_size=None)
    hi, probs, attn = cam(input_tensor=[fts[-1], text, H, W], targets=[ClipOutputTarget(1)], target_size=(91, 59))
    assert hi.dtype == np.float32 and hi.shape == (1, 59, 91) and probs.shape[0] == 1
    want = PR.bilinear_resize_f32(low[0], 59, 91)       # pinned to the recorded cv2.resize in tests/test_camgen_cpu.py
    want = want - want.min()
    want = want / (np.float32(1e-7) + want.max())
    assert np.abs(hi[0] - want).max() < 1e-6
    with pytest.raises(NotImplementedError):
        cam(input_tensor=[fts[-1], text, H, W], targets=[ClipOutputTarget(1)], aug_smooth=True)


def test_worker_writes_the_reference_payload(tmp_path, monkeypatch):
    from weclip_vit_comer_amd.clip import generate_cams as G
    imgs, labels = _tiny_images()
    names = [f"img_{i}.jpg" for i in range(len(imgs))]
    table = dict(zip(names, zip(imgs, labels)))
    monkeypatch.setattr(G, "load_image", lambda path: table[os.path.basename(path)][0])
    out = tmp_path / "cams"
    out.mkdir()
    rc = G.run_worker(0, G.split_dataset(names, 1), str(tmp_path), str(out), lambda: _tiny_generator(0.4)[0],
                      lambda name: (name, table[name][1]), chunk=3)
    assert rc == 0 and sorted(os.listdir(out)) == [f"img_{i}.npy" for i in range(4)]         # the image without labels is skipped
    for i in range(4):
        d = np.load(out / f"img_{i}.npy", allow_pickle=True).item()
        assert sorted(d) == ["attn_highres", "keys"]
        assert d["keys"].dtype == np.int64 and d["keys"].tolist() == labels[i]
        assert d["attn_highres"].dtype == np.float16 and d["attn_highres"].shape == (len(labels[i]),) + tuple(imgs[i].shape[:2])
        assert np.isfinite(d["attn_highres"].astype(np.float32)).all() and d["attn_highres"].max() <= 1
