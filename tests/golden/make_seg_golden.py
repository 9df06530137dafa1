"""Generate the fixtures of the fully supervised WeCLIP variant by RUNNING THE UNMODIFIED REFERENCE (build container
only, like make_golden.py; the reference is imported on CPU through oracle/refharness.py).

    python tests/golden/make_seg_golden.py

tiny_voc_segonly.npz      reference WeCLIP_model/model_attn_aff_voc_seg.WeCLIP on the synth tiny config, same weight and
                          image seeds as tiny_voc.npz, eval mode:
                            seg; a synthetic ground-truth map `gt` (several classes, an ignore border, 37 x 53 -- not
                            16h x 16w) and ce_loss = F.cross_entropy(F.interpolate(seg, gt size, bilinear), gt,
                            ignore_index=255) -- the variant's loss as this package defines it; the norm of
                            every decoder / decoder_fts_fuse gradient after ce_loss.backward() (grad_names, grad_norms)
                            and the small ones in full ("grad:<name>", tiny_voc.npz's list);
                            the state_dict key list as constructed and after a forward (the reference's forward adds
                            encoder.visual.positional_embedding_new), the encoder's requires_grad flags as constructed, weight and
                            image checksums.
tiny_voc_segonly_msc.npz  the reference's own `validate` of test_msc_flip_seg.py (compiled from the script's source; its
                          np.save of the logits goes to a temporary directory) on three synthetic images of different
                          sizes (one odd), 21 classes, scales (1, 0.75): per-image predictions, both histograms, scores.
"""
import ast
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refharness, synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
TINY, TINY_HW, checksum = synth.TINY, synth.TINY_HW, synth.checksum
GT_HW = (37, 53)
MSC_SIZES = [(80, 112), (96, 64), (71, 100)]      # synthetic "original" image sizes (the last one is odd on purpose)
MSC_LONG = 96                                     # --resize_long
KEEP = ["linear_pred.weight", "linear_pred.bias", "transformer.resblocks.2.attn.in_proj_bias",
        "transformer.resblocks.0.ln_1.weight", "transformer.resblocks.0.mlp.c_fc.bias",
        "linears_modulelist.10.proj_2.bias", "linears_modulelist.0.proj.bias", "linear_fuse.bias"]


def gt_map(B=2, hw=GT_HW, seed=21):
    """(B, H, W) int64 ground truth: 4 x 4 blocks of classes 0..20, a 2-pixel ignore border."""
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    lab = torch.randint(0, 21, (B, (H + 3) // 4, (W + 3) // 4), generator=g)
    lab = lab.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()
    lab[:, :2, :] = 255
    lab[:, :, -2:] = 255
    return lab


def msc_inputs():
    """(name, image (3,H,W), label (H,W) uint8) triples shared by the generator and the tests."""
    out = []
    for i, (H, W) in enumerate(MSC_SIZES):
        img = synth.make_images(1, H, W, seed=800 + i)[0]
        g = torch.Generator().manual_seed(900 + i)
        lab = torch.randint(0, 21, (max(H // 8, 1), max(W // 8, 1)), generator=g)
        lab = lab.repeat_interleave(8, 0).repeat_interleave(8, 1)[:H, :W].contiguous()
        lab[:3, :5] = 255
        out.append((f"im{i}", img, lab.to(torch.uint8)))
    return out


def _build(tmp, WeCLIP, sd, fuse_sd, dec_sd):
    ck = os.path.join(tmp, "clip_tiny.pt")
    torch.save(sd, ck)                    # clip.load: torch.jit.load fails -> torch.load state-dict branch
    bg, fg = synth.make_text_features(20, 25, TINY["embed_dim"])
    import WeCLIP_model.model_attn_aff_voc_seg as M
    # the constructor encodes the class names with the text tower; the tiny synth model has none: feed the synth rows
    orig = M.zeroshot_classifier
    M.zeroshot_classifier = lambda names, templates, model: bg if len(names) == bg.shape[0] else fg
    try:
        model = WeCLIP(num_classes=21, clip_model=ck, embedding_dim=256, in_channels=[TINY["width"]] * 4,
                       dataset_root_path=tmp, device="cpu")
    finally:
        M.zeroshot_classifier = orig
    model.decoder_fts_fuse.load_state_dict(fuse_sd)
    model.decoder.load_state_dict(dec_sd)
    return model


def make_tiny_segonly():
    from WeCLIP_model.model_attn_aff_voc_seg import WeCLIP
    sd = synth.make_clip_state_dict(**TINY)
    H, W = TINY_HW
    img = synth.make_images(2, H, W)
    fuse_sd, dec_sd = synth.make_head_state_dicts(width=TINY["width"])
    with tempfile.TemporaryDirectory() as tmp:
        model = _build(tmp, WeCLIP, sd, fuse_sd, dec_sd)
        model.eval()
        keys0 = list(model.state_dict().keys())
        frozen0 = [p.requires_grad for p in model.encoder.parameters()]
        seg = model(img, ["a", "b"])
    gt = gt_map()
    loss = F.cross_entropy(F.interpolate(seg, size=GT_HW, mode="bilinear", align_corners=False), gt, ignore_index=255)
    loss.backward()
    out = dict(weights_ck=checksum(sd.values()), img_ck=checksum([img]), head_ck=checksum(list(fuse_sd.values()) + list(dec_sd.values())),
               seg=seg.detach().numpy(), gt=gt.numpy().astype(np.uint8), ce_loss=np.float64(loss.item()),
               state_keys=np.array(keys0), state_keys_after_forward=np.array(list(model.state_dict().keys())),
               encoder_requires_grad=np.array(frozen0))
    # every gradient as its norm, the small ones in full (tiny_voc.npz's rule: the full set is 24 MB)
    grads = dict(model.decoder.named_parameters())
    grads.update(dict(model.decoder_fts_fuse.named_parameters()))
    out.update(grad_names=np.array(sorted(grads)), grad_norms=np.array([float(grads[n].grad.norm()) for n in sorted(grads)]))
    for n in KEEP:
        out["grad:" + n] = grads[n].grad.numpy()
    np.savez_compressed(os.path.join(OUT, "tiny_voc_segonly.npz"), **out)
    print("tiny_voc_segonly.npz written; loss", loss.item(), "gt classes", np.unique(out["gt"]))


def _seg_script_fn(name, ns):
    """One function of test_msc_flip_seg.py, compiled from the script's source without importing the script (it parses
    argv and imports omegaconf / joblib / imageio / pydensecrf at import time)."""
    src = open(os.path.join(refharness.REF, "test_msc_flip_seg.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            exec(compile(ast.Module([node], []), "test_msc_flip_seg.py", "exec"), ns)
            return ns[name]
    raise KeyError(name)


def make_tiny_segonly_msc():
    from WeCLIP_model.model_attn_aff_voc_seg import WeCLIP
    from utils import evaluate
    sd = synth.make_clip_state_dict(**TINY)
    fuse_sd, dec_sd = synth.make_head_state_dicts(width=TINY["width"])
    data = msc_inputs()

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return len(data)

        def __getitem__(self, i):
            n, img, lab = data[i]
            return n, img, lab.long(), torch.zeros(20)

    with tempfile.TemporaryDirectory() as tmp:
        model = _build(tmp, WeCLIP, sd, fuse_sd, dec_sd)
        model.eval()
        os.makedirs(os.path.join(tmp, "logit"))
        tu = types.SimpleNamespace(data=types.SimpleNamespace(
            DataLoader=lambda ds, **kw: torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)))
        tproxy = types.SimpleNamespace(**{k: getattr(torch, k) for k in ("cat", "mean", "stack", "argmax")}, utils=tu)
        ns = {"np": np, "torch": tproxy, "F": F, "tqdm": lambda it, **kw: it, "evaluate": evaluate,
              "args": types.SimpleNamespace(resize_long=MSC_LONG, work_dir=tmp)}
        validate = _seg_script_fn("validate", ns)
        with torch.no_grad():
            gts, preds, msc_preds, cams, h1, h2, h3 = validate(model, DS(), test_scales=[1, 0.75])
    assert len(preds) == len(data) and not h1.any()          # the script folds its lists into the histograms every 100 images
    hist, score = evaluate.scores(gts, preds, np.zeros((21, 21)), 21)
    msc_hist, msc_score = evaluate.scores(gts, msc_preds, np.zeros((21, 21)), 21)
    out = dict(weights_ck=checksum(sd.values()), head_ck=checksum(list(fuse_sd.values()) + list(dec_sd.values())),
               img_ck=checksum([d[1] for d in data]), sizes=np.array(MSC_SIZES), resize_long=np.int64(MSC_LONG),
               hist=hist.astype(np.int64), msc_hist=msc_hist.astype(np.int64),
               miou=np.float64(score["miou"]), msc_miou=np.float64(msc_score["miou"]),
               pacc=np.float64(score["pAcc"]), msc_pacc=np.float64(msc_score["pAcc"]))
    for i in range(len(data)):
        out[f"pred{i}"] = np.asarray(preds[i]).astype(np.uint8)
        out[f"msc_pred{i}"] = np.asarray(msc_preds[i]).astype(np.uint8)
    np.savez_compressed(os.path.join(OUT, "tiny_voc_segonly_msc.npz"), **out)
    print("tiny_voc_segonly_msc.npz written; mIoU", score["miou"], "msc mIoU", msc_score["miou"])


def main():
    refharness.install()
    torch.manual_seed(0)
    make_tiny_segonly()
    make_tiny_segonly_msc()


if __name__ == "__main__":
    main()
