"""CPU tests of the text tower's host side: the BPE tokenizer, the fp64 text oracle, the drop-in path of clip.clip_text,
and the ISA scan of csrc/text.hip."""
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
import weclip_vit_comer_amd as pkg  # noqa: E402
from weclip_vit_comer_amd.clip import tokenizer as TK  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "text_tower.npz")
REF_BPE = os.path.join("/root/reference", "clip", TK.BPE_NAME)
needs_bpe = pytest.mark.skipif(not os.path.isfile(REF_BPE), reason="needs the reference checkout's BPE merges file")


@pytest.fixture
def bpe(request):
    """Point the tokenizer at a merges file for one test and restore the previous state afterwards."""
    old = TK._bpe_path

    def use(path):
        TK.set_bpe_path(path)
    yield use
    TK._bpe_path = old


def write_vocab(path, merges):
    with gzip.open(path, "wt", encoding="utf-8") as fh:
        fh.write("#version: test\n" + "".join(f"{a} {b}\n" for a, b in merges))
    return str(path)


FIVE = [("l", "o"), ("lo", "w</w>"), ("e", "r</w>"), ("n", "e"), ("ne", "w")]


def test_five_merge_vocabulary_pins_the_bpe(tmp_path, bpe):
    bpe(write_vocab(tmp_path / "v.txt.gz", FIVE))
    tok = TK.get_tokenizer()
    sym = dict(TK.byte_symbols())
    ids = lambda *s: [tok.encoder[x] for x in s]
    assert len(tok.encoder) == 512 + 5 + 2
    assert tok.encoder["<|startoftext|>"] == 517 and tok.encoder["<|endoftext|>"] == 518
    # byte symbols: printable ASCII first in byte order, then the rest; then the same with </w>
    assert tok.encoder["!"] == 0 and tok.encoder["a"] == ord("a") - 0x21 and tok.encoder["a</w>"] == 256 + ord("a") - 0x21
    assert sym[0x20] == chr(256 + 32) and tok.encoder[sym[0x20]] == 188 + 32
    assert tok.encode("low") == ids("low</w>")                       # l+o, then lo+w</w>
    assert tok.encode("lower") == ids("lo", "w", "er</w>")          # lo+w</w> cannot fire inside the word
    assert tok.encode("newer") == ids("new", "er</w>")              # ranks: e+r</w> before n+e before ne+w
    assert tok.encode("  LOW,\tlow  ") == ids("low</w>", ",</w>", "low</w>")
    assert tok.encode("&amp;amp;") == ids("&</w>")                  # double unescape
    t = TK.tokenize(["low", "newer"], context_length=5)
    assert t.dtype == torch.int32 and t.tolist() == [[517] + ids("low</w>") + [518, 0, 0], [517] + ids("new", "er</w>") + [518, 0]]
    with pytest.raises(RuntimeError, match="too long"):
        TK.tokenize("low low low low", context_length=5)
    cut = TK.tokenize("low low low low", context_length=5, truncate=True)
    assert cut.tolist() == [[517] + ids("low</w>") * 3 + [518]]


def test_missing_vocabulary_raises_with_a_hint(bpe, monkeypatch):
    monkeypatch.setattr(TK, "_bpe_path", None)
    import weclip_vit_comer_amd.clip as C
    monkeypatch.setattr(C, "__path__", [os.path.dirname(C.__file__)])
    with pytest.raises(RuntimeError, match="set_bpe_path"):
        TK.tokenize("a")


@needs_bpe
def test_tokenizer_matches_the_recorded_reference_ids(bpe):
    bpe(REF_BPE)
    g = np.load(GOLD)
    for tag in ("voc", "coco"):
        got = TK.tokenize([str(p) for p in g[f"prompts_{tag}"]])
        assert np.array_equal(got.numpy(), g[f"ids_{tag}"]), tag


EXTRA = ["Hello, World!!  How's it going?", "a  b\t\tc\n\nd", "tom & jerry &amp; co &lt;3 &amp;amp;", "1234567 apples, 3.14 pies",
         "state-of-the-art CLIP's tokenizer; (test) [x] {y} #hash @user", "naïve café — ünïcödé ✓ 日本語", "   padded   ",
         "<|startoftext|> inner <|endoftext|>", "don't won't I'll we've they're I'm he'd"]


@needs_bpe
def test_tokenizer_matches_the_live_reference(bpe):
    """Against the reference's own SimpleTokenizer (loaded from its file, ftfy stubbed like oracle/refharness.py)."""
    import importlib.util
    from oracle import refharness
    refharness.install()
    spec = importlib.util.spec_from_file_location("_ref_simple_tokenizer", os.path.join(refharness.REF, "clip", "simple_tokenizer.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rt = ref.SimpleTokenizer(bpe_path=REF_BPE)
    sot, eot = rt.encoder["<|startoftext|>"], rt.encoder["<|endoftext|>"]
    bpe(REF_BPE)
    for t in EXTRA:
        ids = [sot] + rt.encode(t) + [eot]
        assert TK.tokenize(t).tolist() == [ids + [0] * (77 - len(ids))], t
    long_text = "a very long prompt with 123 digits, punctuation! " * 10
    ids = [sot] + rt.encode(long_text) + [eot]
    assert len(ids) > 77
    with pytest.raises(RuntimeError, match="too long"):
        TK.tokenize(long_text)
    assert TK.tokenize(long_text, truncate=True).tolist() == [ids[:76] + [eot]]


def test_text_ref_agrees_with_the_fixture():
    from oracle import synth
    g = np.load(GOLD)
    sd = synth.make_clip_state_dict(seed=0, text_width=512, text_layers=12)
    keys = sorted(k for k in sd if not k.startswith("visual.") and k != "logit_scale")
    assert synth.checksum([sd[k] for k in keys]) == g["checksum"]
    ids = torch.from_numpy(g["ids_voc"])
    eot = ids.long().argmax(-1)
    f = TR.encode_text(ids, sd, L_used=int(eot.max()) + 1)
    r = torch.from_numpy(g["feat_voc"]).double()
    rel = ((f - r).norm(dim=-1) / r.norm(dim=-1)).max().item()
    assert rel < 2e-3, rel            # measured 4.0e-4: the reference's fp32 CPU GEMMs vs fp64, fp16 out-projection flips
    assert torch.equal(TR.encode_text(ids[:3], sd), TR.encode_text(ids[:3], sd, L_used=int(eot.max()) + 1))
    nb = int(g["n_bg_voc"])
    zs = TR.zeroshot(r[:nb], nb, 1)
    assert (zs - torch.from_numpy(g["zs_bg_voc"]).double()).abs().max().item() < 2e-4


def test_causal_ref_masks_and_bounds():
    qkv = TR.make_causal_inputs(2, 13, 2, 64)
    O, lse, M, bO, blse, bM = TR.causal_fwd(qkv, 2, 13, 2, 64)
    assert torch.all(M.triu(1) == 0)
    assert torch.allclose(M.sum(-1), torch.ones(2, 13, dtype=torch.float64))
    assert torch.all(bO > 0) and torch.all(bO < 1e-2) and torch.all(blse < 1e-3)
    # without the mask the planted keys (i + 1 and L - 1) would take most of each row: a missing mask moves O by O(|v|)
    qs, k, _ = TR.heads(qkv, 2, 13, 2, 64)
    P = torch.softmax((qs @ k.transpose(-1, -2)) * TR.LN2, -1)
    above = P.diagonal(offset=1, dim1=-2, dim2=-1)[..., :-1] + P[..., :-2, -1]
    assert above.min() > 0.5


def test_dropin_resolves_clip_text_from_the_reference_root(tmp_path, bpe):
    import importlib
    (tmp_path / "clip").mkdir()
    (tmp_path / "clip" / "clip_text.py").write_text("new_class_names = ['zorb', 'quux']\nBACKGROUND_CATEGORY = ['flarn']\n")
    write_vocab(tmp_path / "clip" / TK.BPE_NAME, FIVE)
    C = importlib.import_module("weclip_vit_comer_amd.clip")
    old_path = list(C.__path__)
    try:
        pkg.install_dropin(reference_root=str(tmp_path))
        from clip.clip_text import BACKGROUND_CATEGORY, new_class_names
        assert new_class_names == ["zorb", "quux"] and BACKGROUND_CATEGORY == ["flarn"]
        import clip
        assert clip is C and clip.tokenize is TK.tokenize
        assert TK.bpe_path() == str(tmp_path / "clip" / TK.BPE_NAME)
        assert clip.tokenize("low").tolist()[0][:3] == [517, TK.get_tokenizer().encoder["low</w>"], 518]
        from clip import model as M                      # the package's own modules keep precedence
        assert M.__file__.startswith(os.path.dirname(C.__file__))
    finally:
        C.__path__[:] = old_path
        for k in [k for k in sys.modules if k.endswith("clip.clip_text")]:
            del sys.modules[k]


def test_causal_mask_is_a_plain_attribute():
    from weclip_vit_comer_amd.clip import model as M
    m = M.CLIP(32, 64, 1, 64, 16, 77, 10, 64, 1, 2)
    assert m.transformer.causal and not m.visual.transformer.causal
    assert m.build_attention_mask().shape == (77, 77) and M.is_causal_mask(m.build_attention_mask())
    assert not any("attn_mask" in k for k in m.state_dict())
    with pytest.raises(NotImplementedError):
        M.Transformer(64, 1, 1, attn_mask=torch.zeros(4, 4))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_text_kernels_issue_their_loads_together(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_scan
    rows = isa_scan.report([os.path.join(ROOT, "weclip-vit-comer_amd", "csrc", "text.hip")], threshold=4, out_dir=str(tmp_path))
    assert not rows, rows
