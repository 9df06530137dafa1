"""Generate tests/golden/clip_preprocess.npz by RUNNING THE UNMODIFIED REFERENCE's preprocessing on the CPU.

Build-container only (needs the reference checkout, see oracle/refharness.py, and Pillow):
    python tests/golden/make_camgen_golden.py
`_transform_resize`, `_convert_image_to_rgb` and `img_ms_and_flip` are compiled from the source of the reference's
clip/generate_cams_voc12.py without running the script.  oracle/refharness.py stubs torchvision's transforms as identities,
which is useless here, so the functions are compiled against functional stand-ins: Compose, Resize (= PIL.Image.resize),
ToTensor (uint8 HWC -> float32 CHW / 255) and Normalize (sub_(mean).div_(std) in float32), the documented arithmetic of
torchvision.  Inputs are synthetic PNG files in a temporary directory (no JPEG: the fixture must not depend on a libjpeg).

Cases `c<i>`: (a) no resize (both sides multiples of 16); (b) +1..+15 pixels on one side and on both; (c) scale 0.5 and 2.0
of an odd size; (d) a 1-pixel-wide and a 3-pixel-high image.  Per case: src (H0,W0,3) uint8, scale, u8 (h,w,3) uint8 = the
image after Pillow's resize, out (3,h,w) f32 and flip (3,h,w) f32 = the two tensors img_ms_and_flip returns.
Noise images plus images of saturated 0 / 255 blocks; the generator asserts that the unclipped cubic overshoots below 0
and above 255 in at least one case, so the clip to [0, 255] is exercised at both ends.

tests/golden/cam_scale_resize.npz: the reference's own `scale_cam_image([cam], (ori_w, ori_h))[0]` + `.astype(np.float16)`
(pytorch_grad_cam/utils/image.py:51-61, generate_cams_voc12.py:198,215) on random refined-CAM-like maps `p<i>_cam` (gh, gw) f32
-> `p<i>_out` (ori_h, ori_w) float16, and `p<i>_plain` = `cv2.resize(cam, (ori_w, ori_h))` f32 (voc12:159).  cv2 is the
harness's stand-in (oracle/refharness.py), so this step is pinned to a restatement, unverified against real OpenCV.
Maps whose maximum after the shift is below 1e-3 are rejected (none was: 0 seeds rejected).

tests/golden/camgen_tiny.npz: the reference `perform` of generate_cams_voc12.py (threshold 0.4) and generate_cams_coco14.py
(threshold 0.7), compiled from their source and run on the tiny synthetic CLIP of oracle/synth.py over four synthetic images
(PNG data; two share a size, two have sizes that are no multiples of 16 in different ways; 1, 2 and 3 labels) with annotation
XML files in a temporary directory.  Recorded by wrapping the functions `perform` calls, not by editing it: the preprocessed
tensor (`img<i>_input`), per class `grayscale_cam`, the boxes of scoremap2bbox, `cam_refined`, the `cv2.resize` "highres" map,
and the saved payload (`keys`, `attn_highres`), per flavour `voc_` / `coco_`.  `.to("cuda:0")` is mapped to the CPU and
`torch.cuda.device_count()` to 1 for the run; lxml.etree.fromstring is the standard library's.
The box step is discrete (threshold on the CAM quantised to uint8), so an image is rejected and drawn again with the next
seed when, in either flavour, a quantised CAM value of one of its classes lies within 1 of int(thr * max), or a refined CAM's
maximum is below 1e-3; the committed set is asserted to satisfy this.  Seeds rejected for the committed set: see
`seeds_rejected` in the fixture (printed by the generator; 8 when this file was last run)."""
import ast
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refharness  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 11
# (H0, W0, scale, kind)
CASES = [(32, 48, 1.0, "noise"), (48, 32, 1.0, "blocks"),
         (33, 48, 1.0, "noise"), (32, 63, 1.0, "blocks"), (47, 49, 1.0, "noise"), (40, 35, 1.0, "blocks"), (17, 31, 1.0, "blocks"),
         (45, 37, 0.5, "noise"), (45, 37, 2.0, "noise"), (45, 37, 0.5, "blocks"), (45, 37, 2.0, "blocks"),
         (20, 1, 1.0, "noise"), (3, 25, 1.0, "blocks")]


def _functional_transforms():
    from PIL import Image

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    class Resize:
        def __init__(self, size, interpolation=Image.BICUBIC):
            self.size, self.interpolation = size, interpolation

        def __call__(self, img):
            h, w = self.size
            return img.resize((w, h), self.interpolation)

    class ToTensor:
        def __call__(self, img):
            return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)

        def __call__(self, t):
            return t.clone().sub_(self.mean[:, None, None]).div_(self.std[:, None, None])
    return dict(Compose=Compose, Resize=Resize, ToTensor=ToTensor, Normalize=Normalize, Image=Image, BICUBIC=Image.BICUBIC)


def dumper_functions(names=("_convert_image_to_rgb", "_transform_resize", "img_ms_and_flip")):
    src = open(os.path.join(refharness.REF, "clip", "generate_cams_voc12.py")).read()
    ns = {"np": np, "torch": torch}
    ns.update(_functional_transforms())
    nodes = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(nodes) == len(names)
    exec(compile(ast.Module(nodes, []), "generate_cams_voc12.py", "exec"), ns)
    return ns


def make_image(rng, H0, W0, kind):
    if kind == "noise":
        return rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)
    img = np.zeros((H0, W0, 3), np.uint8)
    for _ in range(6):          # saturated rectangles, edges anywhere: the cubic overshoots next to every edge
        y, x = rng.integers(0, H0), rng.integers(0, W0)
        img[y:y + rng.integers(1, 9), x:x + rng.integers(1, 9)] = 255 * rng.integers(0, 2, 3)
    img[::5, ::3] = 255 - img[::5, ::3]
    return img


def main():
    ns = dumper_functions()
    Image = ns["Image"]
    rng = np.random.default_rng(SEED)
    out = {"n_cases": np.int64(len(CASES))}
    under = over = False
    with tempfile.TemporaryDirectory() as tmp:
        for i, (H0, W0, scale, kind) in enumerate(CASES):
            src = make_image(rng, H0, W0, kind)
            path = os.path.join(tmp, f"c{i}.png")
            Image.fromarray(src).save(path)
            image, flip = ns["img_ms_and_flip"](path, H0, W0, scales=[scale])
            h, w = image.shape[-2:]
            u8 = np.asarray(Image.open(path).resize((w, h), Image.BICUBIC))
            # the reference's own tensor is ToTensor + Normalize of exactly this uint8 image
            redo = ns["Normalize"]((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))(ns["ToTensor"]()(u8))
            assert torch.equal(redo, image)
            for c in range(3):      # unclipped cubic of the same channel (Pillow's float path)
                f = np.asarray(Image.fromarray(src[..., c].astype(np.float32), "F").resize((w, h), Image.BICUBIC))
                under |= bool((f < -0.5).any() and (u8[..., c] == 0).any())
                over |= bool((f > 255.5).any() and (u8[..., c] == 255).any())
            out[f"c{i}_src"], out[f"c{i}_scale"], out[f"c{i}_u8"] = src, np.float64(scale), u8
            out[f"c{i}_out"], out[f"c{i}_flip"] = image.numpy(), flip.numpy()
    assert under and over, "no fixture pixel clips at 0 / at 255"
    np.savez_compressed(os.path.join(OUT, "clip_preprocess.npz"), **out)
    print("clip_preprocess.npz:", os.path.getsize(os.path.join(OUT, "clip_preprocess.npz")), "bytes,", len(CASES), "cases")


# (gh, gw, ori_h, ori_w): three pairs share a token grid (one launch serves them), sizes that are no multiples of 16
PAIRS = [(4, 6, 64, 96), (4, 6, 50, 83), (4, 6, 61, 90), (3, 2, 33, 17), (12, 16, 150, 199), (2, 2, 2, 2)]


def make_cam_fixture():
    refharness.install()
    import cv2
    from pytorch_grad_cam.utils.image import scale_cam_image
    rng = np.random.default_rng(SEED + 1)
    out = {"n_pairs": np.int64(len(PAIRS))}
    for i, (gh, gw, oh, ow) in enumerate(PAIRS):
        cam = (rng.random((gh, gw)) ** 3 * rng.uniform(0.01, 0.2) + rng.uniform(0, 0.01)).astype(np.float32)
        assert (cam - cam.min()).max() >= 1e-3
        hi = scale_cam_image([cam], (ow, oh))[0]
        assert hi.dtype == np.float32 and hi.shape == (oh, ow)
        out[f"p{i}_cam"], out[f"p{i}_out"] = cam, hi.astype(np.float16)
        out[f"p{i}_plain"] = cv2.resize(cam, (ow, oh)).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "cam_scale_resize.npz"), **out)
    print("cam_scale_resize.npz:", os.path.getsize(os.path.join(OUT, "cam_scale_resize.npz")), "bytes")


PERFORM_SIZES = [(60, 90), (64, 96), (60, 90), (49, 81)]
PERFORM_LABELS = [[3, 7], [0], [14, 2, 5], [9, 1]]


def _perform_ns(script, extra):
    """The functions of one dumper script, compiled against recording stand-ins."""
    import importlib.util
    import xml.etree.ElementTree as ET
    import cv2
    import types
    from pytorch_grad_cam.utils.image import scale_cam_image
    spec = importlib.util.spec_from_file_location("_ref_clip_utils", os.path.join(refharness.REF, "clip", "utils.py"))
    U = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(U)
    T = importlib.util.spec_from_file_location("_ref_clip_text", os.path.join(refharness.REF, "clip", "clip_text.py"))
    names = importlib.util.module_from_spec(T)
    T.loader.exec_module(names)
    rec = {"boxes": [], "refined": [], "highres": [], "input": []}

    def scoremap2bbox(scoremap, threshold, multi_contour_eval=False):
        box, cnt = U.scoremap2bbox(scoremap=scoremap, threshold=threshold, multi_contour_eval=multi_contour_eval)
        rec["boxes"].append(np.asarray(box)[:cnt].copy())
        return box, cnt

    def scale(cams, size=None):
        rec["refined"].append(np.asarray(cams[0]).copy())
        return scale_cam_image(cams, size)
    cv = types.SimpleNamespace(**{k: getattr(cv2, k) for k in dir(cv2) if not k.startswith("__")})

    def resize(src, dsize, *a, **k):
        out = cv2.resize(src, dsize, *a, **k)
        rec["highres"].append(np.asarray(out).copy())
        return out
    cv.resize, cv.__version__ = resize, cv2.__version__
    ns = {"np": np, "torch": torch, "os": os, "cv2": cv, "tqdm": lambda x, *a, **k: x,
          "etree": types.SimpleNamespace(fromstring=ET.fromstring), "parse_xml_to_dict": U.parse_xml_to_dict,
          "scoremap2bbox": scoremap2bbox, "scale_cam_image": scale}
    ns.update({k: getattr(names, k) for k in dir(names) if not k.startswith("_")})
    ns.update(_functional_transforms())
    src = open(os.path.join(refharness.REF, "clip", script)).read()
    want = ("reshape_transform", "ClipOutputTarget", "_convert_image_to_rgb", "_transform_resize", "img_ms_and_flip", "perform")
    nodes = [n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in want]
    assert len(nodes) == len(want)
    exec(compile(ast.Module(nodes, []), script, "exec"), ns)
    inner = ns["img_ms_and_flip"]

    def ms(*a, **k):
        out = inner(*a, **k)
        rec["input"].append(out[0].numpy().copy())
        return out
    ns["img_ms_and_flip"] = ms
    ns.update(extra)
    return ns, rec, names


def _near_threshold(cam, thr):
    q = (cam * 255).astype(np.uint8).astype(np.int64)
    t = int(thr * q.max())
    return bool((np.abs(q - t) <= 1).any())


def make_perform_fixture():
    import types
    from oracle import synth
    refharness.install()
    from pytorch_grad_cam import GradCAM
    torch.cuda.device_count = lambda: 1
    t_to, m_to = torch.Tensor.to, torch.nn.Module.to

    def cpu(a):
        return tuple("cpu" if isinstance(x, str) and x.startswith("cuda") else x for x in a)
    torch.Tensor.to = lambda self, *a, **k: t_to(self, *cpu(a), **k)
    torch.nn.Module.to = lambda self, *a, **k: m_to(self, *cpu(a), **k)
    Image = _functional_transforms()["Image"]
    model = refharness.build_clip(synth.make_clip_state_dict(**synth.TINY))
    for name, p in model.named_parameters():
        p.requires_grad = "11" in name
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])

    def run(flavour, tmp, imgs):
        script = "generate_cams_voc12.py" if flavour == "voc" else "generate_cams_coco14.py"
        ns, rec, names = _perform_ns(script, {})
        cam = GradCAM(model=model, target_layers=[model.visual.transformer.resblocks[-1].ln_1], reshape_transform=ns["reshape_transform"])
        gray = []

        def cam_rec(**k):
            out = cam(**k)
            gray.append(np.asarray(out[0][0]).copy())
            return out
        root = os.path.join(tmp, flavour, "JPEGImages")
        os.makedirs(root, exist_ok=True)
        os.makedirs(os.path.join(tmp, flavour, "Annotations"), exist_ok=True)
        out_dir = os.path.join(tmp, flavour, "out")
        os.makedirs(out_dir, exist_ok=True)
        files = []
        for i, (a, ids) in enumerate(zip(imgs, PERFORM_LABELS)):
            f = f"img_{i}.jpg"
            Image.fromarray(a).save(os.path.join(root, f), format="PNG")
            objs = "".join(f"<object><name>{names.class_names[j]}</name></object>" for j in ids + ids[:1])
            with open(os.path.join(tmp, flavour, "Annotations", f"img_{i}.xml"), "w") as fh:
                fh.write(f"<annotation><size><width>{a.shape[1]}</width><height>{a.shape[0]}</height><depth>3</depth></size>{objs}</annotation>")
            files.append(f)
        args = types.SimpleNamespace(img_root=root, cam_out_dir=out_dir)
        if flavour == "voc":
            rc = ns["perform"](0, [files], args, model, bg, fg, cam_rec)
        else:
            rc = ns["perform"](0, [files], args, model, bg, fg, cam_rec, [[[str(j) for j in ids] for ids in PERFORM_LABELS]])
        assert rc == 0
        res, p = [], 0
        for i, ids in enumerate(PERFORM_LABELS):
            d = np.load(os.path.join(out_dir, f"img_{i}.npy"), allow_pickle=True).item()
            k = len(ids)
            res.append(dict(input=rec["input"][i], gray=np.stack(gray[p:p + k]), boxes=rec["boxes"][p:p + k],
                            refined=np.stack(rec["refined"][p:p + k]), highres=np.stack(rec["highres"][p:p + k]),
                            keys=d["keys"], attn_highres=d["attn_highres"]))
            p += k
        assert p == len(gray) == len(rec["boxes"]) == len(rec["refined"])
        return res

    def ok(r, thr):
        return not any(_near_threshold(g, thr) for g in r["gray"]) and all(x.max() >= 1e-3 for x in r["refined"])

    seeds, rejected, nxt = [None] * 4, 0, 100
    imgs = [None] * 4
    with tempfile.TemporaryDirectory() as tmp:
        while True:
            for i, (h, w) in enumerate(PERFORM_SIZES):
                if seeds[i] is None:
                    seeds[i], nxt = nxt, nxt + 1
                    imgs[i] = np.random.default_rng(seeds[i]).integers(0, 256, (h // 4 + 1, w // 4 + 1, 3), dtype=np.uint8) \
                        .repeat(4, 0).repeat(4, 1)[:h, :w].copy()
            voc, coco = run("voc", tmp, imgs), run("coco", tmp, imgs)
            bad = [i for i in range(4) if not (ok(voc[i], 0.4) and ok(coco[i], 0.7))]
            if not bad:
                break
            for i in bad:
                seeds[i] = None
                rejected += 1
    out = {"n_images": np.int64(4), "seeds": np.asarray(seeds), "seeds_rejected": np.int64(rejected)}
    for i in range(4):
        out[f"img{i}_src"], out[f"img{i}_labels"] = imgs[i], np.asarray(PERFORM_LABELS[i], np.int64)
        out[f"img{i}_input"] = voc[i]["input"]
        assert np.array_equal(voc[i]["input"], coco[i]["input"])
        for tag, res, thr in (("voc", voc, 0.4), ("coco", coco, 0.7)):
            r = res[i]
            assert ok(r, thr) and r["keys"].tolist() == PERFORM_LABELS[i]
            out[f"{tag}{i}_gray"], out[f"{tag}{i}_refined"], out[f"{tag}{i}_highres"] = r["gray"], r["refined"], r["highres"]
            out[f"{tag}{i}_keys"], out[f"{tag}{i}_attn_highres"] = r["keys"], r["attn_highres"]
            for k, b in enumerate(r["boxes"]):
                out[f"{tag}{i}_boxes{k}"] = np.asarray(b, np.int64).reshape(-1, 4)
    path = os.path.join(OUT, "camgen_tiny.npz")
    np.savez_compressed(path, **out)
    print("camgen_tiny.npz:", os.path.getsize(path), "bytes; seeds", seeds, "rejected", rejected)


if __name__ == "__main__":
    if "--perform-only" not in sys.argv:
        main()
        make_cam_fixture()
    make_perform_fixture()
