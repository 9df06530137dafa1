"""CPU tests of the fully supervised WeCLIP variant (WeCLIP_model/model_attn_aff_voc_seg.py): the reference
test_msc_flip_seg.py import lines resolve after install_dropin(), the model's state-dict / frozen-encoder contract
against the reference fixture, the fused cross-entropy's host-side argument checks, and its kernels' load issue."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_seg_variant_import_lines_resolve_after_install_dropin():
    code = """
        import weclip_vit_comer_amd
        weclip_vit_comer_amd.install_dropin()
        from WeCLIP_model.model_attn_aff_voc_seg import WeCLIP
        from WeCLIP_model.segformer_head_seg import SegFormerHead
        from WeCLIP_model.Decoder.TransDecoder_seg import DecoderTransformer
        import weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc_seg as M
        import weclip_vit_comer_amd.WeCLIP_model.segformer_head as S
        import weclip_vit_comer_amd.WeCLIP_model.Decoder.TransDecoder as D
        assert WeCLIP is M.WeCLIP and SegFormerHead is S.SegFormerHead and DecoderTransformer is D.DecoderTransformer
        print("ok")
    """
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def _cpu_model():
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc_seg import WeCLIP
    sd = synth.make_clip_state_dict(**synth.TINY)
    return WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4,
                  dataset_root_path="/data/VOC", device="cpu")


def test_seg_variant_contract_against_reference_fixture(golden):
    g = golden("tiny_voc_segonly.npz")
    m = _cpu_model()
    keys = list(m.state_dict().keys())
    assert keys == [str(k) for k in g["state_keys"]]
    assert not any(k.startswith("par.") for k in keys)
    flags = [p.requires_grad for p in m.encoder.parameters()]
    assert flags == [bool(f) for f in g["encoder_requires_grad"]] and not any(flags)
    # a reference-layout state dict loads strict -- also one saved after a reference forward, which carries the
    # resized positional embedding the reference stores as an attribute
    sd = {k: v.clone() + 1 for k, v in m.state_dict().items()}
    after = [str(k) for k in g["state_keys_after_forward"]]
    assert set(after) - set(sd) == {"encoder.visual.positional_embedding_new"}
    sd["encoder.visual.positional_embedding_new"] = torch.zeros(5, synth.TINY["width"])
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.decoder.linear_pred.bias, sd["decoder.linear_pred.bias"])
    # text rows stay None without a reference checkout; API-parity attributes
    assert m.bg_text_features is None and m.fg_text_features is None
    assert m.root_path == os.path.join("/data/VOC", "JPEGImages") and m.cam_bg_thres == 1 and m.iter_num == 0
    assert m.require_all_fts is True and m.grad_cam is not None and len(m.target_layers) == 1
    groups = m.get_param_groups()
    assert [len(x) for x in groups[:3]] == [0, 0, 0]
    assert len(groups[3]) == len(list(m.decoder.parameters())) + len(list(m.decoder_fts_fuse.parameters()))
    assert m.head_engine.attn_pred is False


@pytest.mark.parametrize("seg,label,err", [
    (torch.zeros(2, 21, 3, 4, dtype=torch.int64), torch.zeros(2, 37, 53, dtype=torch.int64), TypeError),      # int logits
    (torch.zeros(2, 21, 3, 4), torch.zeros(2, 37, 53), TypeError),                                           # float labels
    (torch.zeros(21, 3, 4), torch.zeros(2, 37, 53, dtype=torch.int64), ValueError),                          # seg rank 3
    (torch.zeros(2, 21, 3, 4), torch.zeros(2, 1, 37, 53, dtype=torch.int64), ValueError),                   # label rank 4
    (torch.zeros(2, 21, 3, 4), torch.zeros(3, 37, 53, dtype=torch.int64), ValueError),                      # batch mismatch
    (torch.zeros(2, 0, 3, 4), torch.zeros(2, 37, 53, dtype=torch.int64), ValueError),                       # nc = 0
    (torch.zeros(2, 129, 3, 4), torch.zeros(2, 37, 53, dtype=torch.int64), ValueError),                     # nc = 129
])
def test_ce_loss_host_checks_refuse_before_launch(seg, label, err):
    from weclip_vit_comer_amd.utils.losses import get_ce_loss_fused
    with pytest.raises(err):
        get_ce_loss_fused(seg, label)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_ce_loss_kernels_issue_their_loads_together(tmp_path):
    import isa_scan
    src = os.path.join(ROOT, "weclip-vit-comer_amd", "csrc", "losses.hip")
    rows = isa_scan.report([src], threshold=4, out_dir=str(tmp_path))
    bad = [(alone, loads, name) for alone, loads, _, name, _ in rows if "ce_loss" in name or "seg_bwd_x2" in name]
    assert not bad, "loads waited for one at a time (see tools/isa_scan.py): %s" % bad
    asm = open(os.path.join(str(tmp_path), "losses.hip.s")).read()
    assert asm.count("ce_loss_fused_kernel") > 0
    # nc > 24 loops over classes in registers: no scratch (private segment) in any instantiation
    for name, lines in isa_scan.kernels(os.path.join(str(tmp_path), "losses.hip.s")):
        if "ce_loss_fused_kernel" in name:
            assert not any("scratch_store" in l or "buffer_store" in l for l in lines), name
