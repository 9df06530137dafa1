"""The affinity weight straight from the layers' Q / K (attn_affw_kernel, wc_attn_aff_weight in csrc/attention.hip) against the
path it replaces outside the seg-trans branch -- wc_attn_mean per layer, then wc_aff_weight_c1 -- and against fp64.

W and c1 must be BIT-identical to the two-kernel path (same MFMA chain per score, same head / layer / row summation order).
Outputs and workspaces are NaN-filled before every call.  The fp64 check holds W on the smallest shape (one layer, weight 1:
W is then the cropped head-mean map itself) to the bound of tests/attn_ref.mean, the attention-map pin's."""
import ctypes

import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16


def _L():
    from weclip_vit_comer_amd import _lib as L
    return L


def _nan(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(255)
    return t


def _timed(fn):
    """Run fn with the kernel timers on; -> (fn's result, names of the kernels it launched, group tags stripped)."""
    from weclip_vit_comer_amd import ops
    ops.KernelTimer.enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = {n.split("@")[0] for n in ops.KernelTimer.summary()}
    finally:
        ops.KernelTimer.enable(0)
    return out, names


def _weights(B, nmaps, uniform):
    if uniform:
        return torch.full((B, nmaps), 1.0 / nmaps, dtype=F32, device="cuda")
    g = torch.Generator().manual_seed(B * 16 + nmaps)
    w = torch.rand(B, nmaps, generator=g, dtype=F32) + 0.05
    w[0, 0] = 0.0                                   # a dropped layer, as the seg-trans selection produces
    return (w / w.sum(1, keepdim=True)).cuda().contiguous()


_CASES = {}


def _case(B, H, DH, L, nmaps, uniform):
    """Inputs of one shape, its layers through ops.attention (old path's maps included), both weights: computed once."""
    key = (B, H, DH, L, nmaps, uniform)
    if key in _CASES:
        return _CASES[key]
    from weclip_vit_comer_amd import ops
    Lb = _L()
    hw = L - 1
    layers, maps, host = [], [], []
    for l in range(nmaps):
        qkv, _ = R.make_inputs(B, L, H, DH, seed=1000 * l + B * 131 + L)
        host.append(qkv)
        qd = qkv.cuda().contiguous()
        _, lse, mean = ops.attention(qd, B, L, H, DH, want_mean=True)
        layers.append(ops.AttnOperands(qd, lse, B, L, H, DH))
        maps.append(mean)
    wgt = _weights(B, nmaps, uniform)
    nblk = -(-hw // 8)
    # today's path
    W0, c0, ws0 = _nan((B, hw, hw), F32), _nan((B, hw), F32), _nan((B * nblk * hw,), F32)
    marr = (ctypes.c_void_p * nmaps)(*[m.data_ptr() for m in maps])
    _, names0 = _timed(lambda: Lb.lib().wc_aff_weight_c1(marr, nmaps, Lb.ptr(wgt), None, Lb.ptr(W0), Lb.ptr(c0), Lb.ptr(ws0), B, L,
                                                         Lb.stream()))
    # one launch from Q / K
    W1, c1, ws1 = _nan((B, hw, hw), F32), _nan((B, hw), F32), _nan((B * nblk * hw,), F32)
    qarr = (ctypes.c_void_p * nmaps)(*[x.qkv.data_ptr() for x in layers])
    larr = (ctypes.c_void_p * nmaps)(*[x.lse.data_ptr() for x in layers])
    _, names1 = _timed(lambda: Lb.lib().wc_attn_aff_weight(qarr, larr, nmaps, Lb.ptr(wgt), Lb.ptr(W1), Lb.ptr(c1), Lb.ptr(ws1), B,
                                                           L, H, DH, Lb.stream()))
    out = dict(layers=layers, maps=maps, host=host, wgt=wgt, old=(W0, c0, ws0, names0), new=(W1, c1, ws1, names1))
    _CASES.clear()                                  # one case's device tensors at a time
    _CASES[key] = out
    return out


# (B, H, DH, L, nmaps, uniform weights): one / two tiles per side, the full eight layers with per-image weights, the second
# group of eight images of the XCD order (B = 9), ragged tiles (hw = 196: the last 8-row block holds 4 rows; hw = 400, DH = 32)
EQUAL_CASES = [(2, 2, 64, 1 + 256, 1, True), (2, 3, 64, 1 + 256, 8, False), (9, 2, 64, 1 + 128, 3, True),
               (1, 2, 64, 1 + 196, 2, True), (1, 2, 32, 1 + 400, 2, True)]


@pytest.mark.parametrize("B,H,DH,L,nmaps,uniform", EQUAL_CASES)
def test_bit_identical_to_maps_path(B, H, DH, L, nmaps, uniform):
    c = _case(B, H, DH, L, nmaps, uniform)
    W0, c0, ws0, names0 = c["old"]
    W1, c1, ws1, names1 = c["new"]
    assert "aff_weight_colpart_kernel" in names0 and f"attn_affw_kernel<{DH}>" in names1, (names0, names1)
    assert not any(n.startswith(("attn_mean_kernel", "aff_weight_colpart_kernel")) for n in names1), names1
    for name, t in (("W", W1), ("c1", c1), ("column partials", ws1)):
        assert torch.isfinite(t).all(), f"{name}: {int((~torch.isfinite(t)).sum())} elements not written (still NaN)"
    assert torch.equal(ws1, ws0), "column partials differ from aff_weight_colpart_kernel's"
    assert torch.equal(W1, W0), f"W differs at {int((W1 != W0).sum())} of {W0.numel()} elements"
    assert torch.equal(c1, c0), f"c1 differs at {int((c1 != c0).sum())} of {c0.numel()} elements"


def test_pipeline_form_and_switch():
    """cam_pipeline.affinity_weight takes the operand list (uniform weights) and returns the same (W, c1); with per-image weights
    affinity_weight_qk does."""
    from weclip_vit_comer_amd import cam_pipeline as CP
    c = _case(2, 3, 64, 1 + 256, 8, False)
    W, c1 = CP.affinity_weight_qk(c["layers"], c["wgt"])
    assert torch.equal(W, c["old"][0]) and torch.equal(c1, c["old"][1])
    (Wq, cq), names = _timed(lambda: CP.affinity_weight(c["layers"], return_c1=True))
    assert "attn_affw_kernel<64>" in names and not any(n.startswith("attn_mean") for n in names), names
    Wm, cm = CP.affinity_weight(c["maps"], return_c1=True)
    assert torch.equal(Wq, Wm) and torch.equal(cq, cm)


def test_fp64_reference_smallest_shape():
    """One layer with weight 1: W = fmaf(1, map, 0) is the cropped head-mean map, held to the attention-map pin's bound
    (tests/attn_ref.mean: exponent error, the two-part -lse, the H-head sum and the 1/H scale), nothing added."""
    B, H, DH, L, nmaps = 2, 2, 64, 1 + 256, 1
    c = _case(B, H, DH, L, nmaps, True)
    assert torch.equal(c["wgt"], torch.ones_like(c["wgt"]))
    rows = torch.arange(L)
    M, bM = R.mean(c["host"][0], B, L, H, DH, list(range(B)), rows)
    ref, bound = M[:, 1:, 1:], bM[:, 1:, 1:]
    got = c["new"][0].double().cpu()
    err = (got - ref).abs()
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print(f"attn_affw_kernel<64> W vs fp64: worst err / bound {ratio:.3g}, worst abs err {err.max().item():.3g}")
    assert (err <= bound).all(), f"{int((err > bound).sum())} of {err.numel()} elements outside the bound, worst err / bound {ratio:.3g}"


def test_argument_errors():
    Lb = _L()
    c = _case(2, 2, 64, 1 + 256, 1, True)
    x = c["layers"][0]
    W1, c1, ws1, _ = c["new"]
    q = (ctypes.c_void_p * 1)(x.qkv.data_ptr())
    ls = (ctypes.c_void_p * 1)(x.lse.data_ptr())
    call = lambda **k: Lb.lib().wc_attn_aff_weight(k.get("q", q), ls, k.get("nmaps", 1), Lb.ptr(c["wgt"]), Lb.ptr(W1), Lb.ptr(c1),
                                                   Lb.ptr(ws1), 2, k.get("L", 257), 2, k.get("DH", 64), Lb.stream())
    with pytest.raises(RuntimeError, match="bad argument"):
        call(nmaps=13)
    with pytest.raises(RuntimeError, match="head dim"):
        call(DH=48)
    with pytest.raises(RuntimeError, match="patch tokens"):
        call(L=1 + 255)
    with pytest.raises(RuntimeError, match="16-byte"):
        call(q=(ctypes.c_void_p * 1)(x.qkv.data_ptr() + 2))
    with pytest.raises(RuntimeError, match="no operands"):
        call(q=(ctypes.c_void_p * 1)(None))


# ---------------------------------------------------------------------------------------------------------------------
# routing

@pytest.fixture(scope="module")
def model():
    from oracle import synth
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP
    sd = synth.make_clip_state_dict(**synth.TINY)            # 12 blocks, width 64: one head of 64
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
    m = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4, dataset_root_path=None,
               device="cuda", text_features=(bg.cuda(), fg.cuda()))
    m.decoder_fts_fuse.load_state_dict(fuse)
    m.decoder.load_state_dict(dec)
    return m.eval()


def _forward(m, img, labels, iter_num):
    m.iter_num = iter_num
    with torch.no_grad():
        return m(img, [""] * img.shape[0], labels=labels)


OLD = ("attn_mean_kernel", "aff_weight_colpart_kernel")


def test_routing_and_unchanged_results(model, monkeypatch):
    """WeCLIP.forward outside the seg-trans branch takes the one-launch path and gives what the maps path gives; the seg-trans
    branch and an encode() call that asks for maps keep the old kernels."""
    from oracle import synth
    from weclip_vit_comer_amd import cam_pipeline as CP
    B, S = 2, 192                                    # hw = 144: two ragged tiles per side
    img = synth.make_images(B, S, S, seed=3).cuda()
    labels = synth.make_label_lists(B, 2, seed=7)
    assert CP.FUSED_QK_WEIGHT
    (seg1, lab1, ap1), names = _timed(lambda: _forward(model, img, labels, 0))
    assert "attn_affw_kernel<64>" in names and not any(n.startswith(OLD) for n in names), sorted(names)
    monkeypatch.setattr(CP, "FUSED_QK_WEIGHT", False)
    (seg0, lab0, ap0), names = _timed(lambda: _forward(model, img, labels, 0))
    assert "attn_affw_kernel<64>" not in names and all(any(n.startswith(o) for n in names) for o in OLD), sorted(names)
    assert torch.equal(lab1, lab0) and torch.equal(seg1, seg0) and torch.equal(ap1, ap0)
    monkeypatch.setattr(CP, "FUSED_QK_WEIGHT", True)
    # the seg-trans branch (iterations past the switch) reads attn_pred and selects layers from their maps
    (_, labs, _), names = _timed(lambda: _forward(model, img, labels, 20000))
    assert "attn_affw_kernel<64>" not in names and all(any(n.startswith(o) for n in names) for o in OLD), sorted(names)
    monkeypatch.setattr(CP, "FUSED_QK_WEIGHT", False)
    labs0 = _forward(model, img, labels, 20000)[1]
    assert torch.equal(labs, labs0)
    monkeypatch.setattr(CP, "FUSED_QK_WEIGHT", True)
    # encode() hands back maps unless asked otherwise
    with torch.no_grad():
        (_, maps, _, Lq), names = _timed(lambda: model.encode(img, False))
    assert any(n.startswith("attn_mean_kernel") for n in names) and "attn_affw_kernel<64>" not in names, sorted(names)
    assert [m is None for m in maps] == [True] * 4 + [False] * 7
    assert all(torch.is_tensor(m) and m.shape == (B, Lq, Lq) for m in maps[4:])
