"""GPU tests of the CLIP text tower (csrc/text.hip, clip/text_engine.py): the causal attention kernel against fp64,
CLIP.encode_text and the zero-shot rows against the reference fixture (tests/golden/text_tower.npz) and the fp64 text
oracle, the truncated run, WeCLIP's constructor computing its text rows, and the argument refusals."""
import gzip
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import text_ref as TR  # noqa: E402
from oracle import synth  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "text_tower.npz")
F16, F32 = torch.float16, torch.float32


def _lib():
    from weclip_vit_comer_amd import _lib as L
    return L


def causal_call(qkv, N, L, H, DH, mean=True):
    """Outputs NaN-filled before the call: every element the kernel owes must be written."""
    Lb = _lib()
    E = H * DH
    dev = qkv.device
    o16 = torch.full((N * L, E), float("nan"), device=dev, dtype=F16)
    o32 = torch.full((N * L, E), float("nan"), device=dev, dtype=F32)
    lse = torch.full((N, H, L), float("nan"), device=dev, dtype=F32)
    m = torch.full((N, L, L), float("nan"), device=dev, dtype=F32) if mean else None
    Lb.lib().wc_attn_fwd_causal(Lb.ptr(qkv), Lb.ptr(o16), Lb.ptr(o32), Lb.ptr(lse), Lb.ptr(m), N, L, H, DH, Lb.stream())
    torch.cuda.synchronize()
    return o16.cpu(), o32.cpu(), lse.cpu(), (m.cpu() if mean else None)


@pytest.mark.parametrize("L", [1, 2, 13, 64, 77, 128])
@pytest.mark.parametrize("N,H", [(1, 1), (1, 8), (103, 1), (103, 8)])
def test_causal_attention_against_fp64(L, N, H):
    DH = 64
    qkv = TR.make_causal_inputs(N, L, H, DH, seed=L + N + H)
    o16, o32, lse, m = causal_call(qkv.cuda(), N, L, H, DH)
    O, lse64, M, bO, blse, bM = TR.causal_fwd(qkv, N, L, H, DH)
    assert torch.isfinite(o16).all() and torch.isfinite(o32).all() and torch.isfinite(lse).all() and torch.isfinite(m).all()
    e32 = (o32.double() - O).abs()
    assert (e32 <= bO).all(), f"o32 worst excess {(e32 - bO).max().item():.3e}"
    e16 = (o16.double() - O).abs()
    assert (e16 <= bO + TR.ulp16(O)).all(), f"o16 worst excess {(e16 - bO - TR.ulp16(O)).max().item():.3e}"
    assert ((lse.double() - lse64).abs() <= blse).all()
    assert (m.triu(1) == 0).all(), "map above the diagonal must be exactly 0"
    assert ((m.double() - M).abs() <= bM + 2.0 ** -40).all()
    assert ((m.double().sum(-1) - 1).abs() <= (L + 4) * 2.0 ** -23 + bM.sum(-1)).all()
    # without the mask these outputs would be far off: the planted keys above the diagonal carry > half of each row
    if L > 2:
        assert (O.view(N, L, H * DH)[:, :-2] - TR.fwd_exact_nomask(qkv, N, L, H, DH).view(N, L, -1)[:, :-2]).abs().max() > 0.1


def test_causal_attention_without_map_or_extras():
    Lb = _lib()
    N, L, H, DH = 3, 77, 8, 64
    qkv = TR.make_causal_inputs(N, L, H, DH, seed=5).cuda()
    o16 = torch.full((N * L, H * DH), float("nan"), device="cuda", dtype=F16)
    Lb.lib().wc_attn_fwd_causal(Lb.ptr(qkv), Lb.ptr(o16), None, None, None, N, L, H, DH, Lb.stream())
    ref, _, _, _ = causal_call(qkv, N, L, H, DH, mean=False)
    assert torch.equal(o16.cpu(), ref)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def text_model(gold):
    from weclip_vit_comer_amd.clip import load
    sd = synth.make_clip_state_dict(seed=0, text_width=512, text_layers=12)
    keys = sorted(k for k in sd if not k.startswith("visual.") and k != "logit_scale")
    assert synth.checksum([sd[k] for k in keys]) == gold["checksum"]
    model, _ = load(sd, device="cuda")
    return model, sd


def rel_rows(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1)).max().item()


@pytest.mark.parametrize("precision,bound", [("fast", 2e-3), ("exact", 1e-3)])
def test_encode_text_against_the_reference(text_model, gold, precision, bound):
    from weclip_vit_comer_amd import config
    model, sd = text_model
    old = config.precision
    config.precision = precision
    try:
        for tag in ("voc", "coco"):
            ids = torch.from_numpy(gold[f"ids_{tag}"])
            f = model.encode_text(ids)
            assert f.dtype == F32 and f.device.type == "cuda" and f.shape == (ids.shape[0], 512)
            e_ref = rel_rows(f, gold[f"feat_{tag}"])
            e64 = rel_rows(f, TR.encode_text(ids, sd, L_used=int(ids.long().argmax(-1).max()) + 1))
            print(f"encode_text {precision} {tag}: max row rel err vs reference {e_ref:.2e}, vs fp64 {e64:.2e}")
            assert e_ref < bound and e64 < bound, (e_ref, e64)
            f64ids = model.encode_text(ids.long().cuda())            # int64 on the GPU: same values
            assert torch.equal(f64ids, f)
    finally:
        config.precision = old


def test_truncated_run_matches_the_full_context(text_model, gold):
    model, _ = text_model
    ids = torch.from_numpy(gold["ids_coco"])
    a = model.encode_text(ids)
    b = model.encode_text(ids, full_context=True)
    assert rel_rows(a, b) < 1e-3


def test_zeroshot_rows_and_torch_op(text_model, gold):
    import weclip_vit_comer_amd as pkg
    from weclip_vit_comer_amd import ops
    from weclip_vit_comer_amd.clip import text_engine as TE
    pkg.register_torch_ops()
    model, _ = text_model
    for tag in ("voc", "coco"):
        ids = torch.from_numpy(gold[f"ids_{tag}"])
        nb = int(gold[f"n_bg_{tag}"])
        f = model.encode_text(ids)
        bg = ops.text_zeroshot(f[:nb].contiguous(), nb, 1)
        fg = ops.text_zeroshot(f[nb:].contiguous(), f.shape[0] - nb, 1)
        assert rel_rows(bg, gold[f"zs_bg_{tag}"]) < 2e-3 and rel_rows(fg, gold[f"zs_fg_{tag}"]) < 2e-3
        z64 = TR.zeroshot(f[nb:].cpu(), f.shape[0] - nb, 1)
        assert rel_rows(fg, z64) < 1e-6
    two = ops.text_zeroshot(f[:6].contiguous(), 3, 2)          # T = 2 templates per class
    assert rel_rows(two, TR.zeroshot(f[:6].cpu(), 3, 2)) < 1e-6
    tr = model.transformer
    blocks = [dict(b.named_parameters())[k] for b in tr.resblocks for k in TE.BLOCK_KEYS]
    via_op = torch.ops.weclip.encode_text(torch.from_numpy(gold["ids_voc"]).cuda(), model.token_embedding.weight,
                                          model.positional_embedding, blocks, tr.resblocks[0].attn.num_heads,
                                          model.ln_final.weight, model.ln_final.bias, model.text_projection)
    assert torch.equal(via_op, model.encode_text(torch.from_numpy(gold["ids_voc"])))


def test_weclip_builds_its_text_rows(tmp_path):
    """TINY WeCLIP without text_features: rows from a names module and a hand-written vocabulary in tmp_path."""
    import weclip_vit_comer_amd as pkg
    from weclip_vit_comer_amd.clip import tokenizer as TK
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import TEMPLATES, WeCLIP, zeroshot_classifier
    (tmp_path / "clip").mkdir()
    fg = [f"thing {chr(97 + i)}" for i in range(20)]
    bg = ["ground", "sky", "wall", "lower tree", "new water"]
    (tmp_path / "clip" / "clip_text.py").write_text(f"new_class_names = {fg!r}\nBACKGROUND_CATEGORY = {bg!r}\n")
    with gzip.open(tmp_path / "clip" / TK.BPE_NAME, "wt", encoding="utf-8") as fh:
        fh.write("#version: test\nl o\nlo w</w>\ne r</w>\nn e\nne w\n")
    C = sys.modules["weclip_vit_comer_amd.clip"]
    old_path, old_bpe = list(C.__path__), TK._bpe_path
    sd = synth.make_clip_state_dict(**synth.TINY)
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
    kw = dict(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4, dataset_root_path=None,
              device="cuda")
    try:
        TK._bpe_path = None
        C.__path__[:] = old_path[:1]                 # the package's own directory only
        none = WeCLIP(**kw)
        assert none.bg_text_features is None and none.fg_text_features is None       # unknown checkout: today's behaviour
        pkg.install_dropin(reference_root=str(tmp_path))
        m = WeCLIP(**kw)
        assert m.bg_text_features.shape == (5, synth.TINY["embed_dim"]) and m.fg_text_features.shape == (20, synth.TINY["embed_dim"])
        ebg = zeroshot_classifier(bg, TEMPLATES, m.encoder)
        efg = zeroshot_classifier(fg, TEMPLATES, m.encoder)
        explicit = WeCLIP(**kw, text_features=(ebg, efg))
        assert torch.equal(m.bg_text_features, explicit.bg_text_features)
        assert torch.equal(m.fg_text_features, explicit.fg_text_features)
        feat = m.encoder.encode_text(TK.tokenize([t.format(c) for c in fg for t in TEMPLATES]))
        assert rel_rows(m.fg_text_features, TR.zeroshot(feat.cpu(), 20, 1)) < 1e-6
        m.decoder_fts_fuse.load_state_dict(fuse)
        m.decoder.load_state_dict(dec)
        m.eval()
        H, W = synth.TINY_HW
        seg, labels, ap = m(synth.make_images(2, H, W).cuda(), ["a", "b"], labels=synth.TINY_LABELS)
        assert torch.isfinite(seg).all() and labels.shape == (2, H, W)
    finally:
        C.__path__[:] = old_path
        TK._bpe_path = old_bpe
        for k in [k for k in sys.modules if k.endswith("clip.clip_text")]:
            del sys.modules[k]


def test_refusals(text_model):
    from weclip_vit_comer_amd import ops
    model, _ = text_model
    bad = torch.zeros(2, 77, dtype=torch.int32)
    bad[0, :3] = torch.tensor([49406, 5, 49407])
    bad[1, :3] = torch.tensor([49406, 49408, 49407])
    with pytest.raises(RuntimeError, match="outside"):
        model.encode_text(bad)
    bad[1, 1] = -1
    with pytest.raises(RuntimeError, match="outside"):
        model.encode_text(bad)
    with pytest.raises(RuntimeError, match="int32 or int64"):
        model.encode_text(bad.float())
    qkv = torch.zeros(129 * 2, 3 * 128, device="cuda", dtype=F16)
    with pytest.raises(RuntimeError, match="L <= 128"):
        ops.attention_causal(qkv, 2, 129, 2, 64)
    with pytest.raises(RuntimeError, match="head dim"):
        ops.attention_causal(torch.zeros(10, 3 * 64, device="cuda", dtype=F16), 1, 10, 2, 32)
    Lb = _lib()
    big = torch.zeros(10 * 3 * 64 + 8, device="cuda", dtype=F16)
    out = torch.zeros(10 * 64, device="cuda", dtype=F16)
    with pytest.raises(RuntimeError, match="aligned"):
        Lb.lib().wc_attn_fwd_causal(Lb.ptr(big[1:]), Lb.ptr(out), None, None, None, 1, 10, 1, 64, Lb.stream())
    with pytest.raises(RuntimeError, match="H >= 1|bad argument"):
        Lb.lib().wc_attn_fwd_causal(Lb.ptr(big), Lb.ptr(out), None, None, None, 1, 10, 0, 64, Lb.stream())
