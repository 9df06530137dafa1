"""GPU tests of the fully supervised WeCLIP variant: the model against the reference fixture, bit-identity with the VOC
path and with the default head engine, the fused cross-entropy kernel against fp64 torch, SupervisedTrainStep (eager vs
graph replay, and against a stock-torch step) and the msc-flip evaluator against the reference's own `validate`."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth

pytestmark = pytest.mark.gpu
H, W = synth.TINY_HW
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


def _seg_model(head="hip", train=False):
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc_seg import WeCLIP
    sd = synth.make_clip_state_dict(**synth.TINY)
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
    m = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4, device="cuda")
    m.decoder_fts_fuse.load_state_dict(fuse)
    m.decoder.load_state_dict(dec)
    m.head_impl = head
    return m.train() if train else m.eval()


def _voc_model():
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP
    sd = synth.make_clip_state_dict(**synth.TINY)
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
    m = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4,
               dataset_root_path=None, device="cuda", text_features=(bg.cuda(), fg.cuda()))
    m.decoder_fts_fuse.load_state_dict(fuse)
    m.decoder.load_state_dict(dec)
    return m.eval()


@pytest.mark.parametrize("head", ["hip", "torch"])
def test_seg_variant_matches_reference(golden, head):
    from weclip_vit_comer_amd import config
    from weclip_vit_comer_amd.utils.losses import get_ce_loss_fused
    g = golden("tiny_voc_segonly.npz")
    m = _seg_model(head)
    img = synth.make_images(2, H, W).cuda()
    assert synth.checksum([img.cpu()]) == pytest.approx(float(g["img_ck"]), rel=1e-12)
    seg = m(img, ["a", "b"])
    assert isinstance(seg, torch.Tensor) and tuple(seg.shape) == (2, 21, H // 16, W // 16) and seg.dtype == torch.float32
    assert m.iter_num == 1
    e_seg = np.abs(seg.detach().cpu().numpy() - g["seg"]).max() / np.abs(g["seg"]).max()
    gt = torch.from_numpy(g["gt"].astype(np.int64)).cuda()
    loss = get_ce_loss_fused(seg, gt, 255)
    e_loss = abs(loss.item() - float(g["ce_loss"])) / abs(float(g["ce_loss"]))
    print(f"[{head}] seg rel {e_seg:.2e}  ce loss rel {e_loss:.2e}")
    assert e_seg < (1e-3 if config.exact() else 3e-3)
    assert e_loss < 1e-3
    loss.backward()
    grads = dict(m.decoder.named_parameters())
    grads.update(dict(m.decoder_fts_fuse.named_parameters()))
    entry = {k: float(np.abs(grads[k[5:]].grad.cpu().numpy() - g[k]).max() / (np.abs(g[k]).max() + 1e-12))
             for k in g.files if k.startswith("grad:")}
    names = [str(n) for n in g["grad_names"]]
    norms = np.array([float(grads[n].grad.norm()) for n in names])
    worst = np.abs(norms - g["grad_norms"]).max() / g["grad_norms"].max()
    print(f"[{head}] worst gradient entry error {max(entry.values()):.2e} of its tensor's largest ({max(entry, key=entry.get)}); "
          f"worst grad-norm deviation {worst:.2e} of the largest norm")
    # test_weclip_gpu.py's rule.  The first adapter's bias gradient reads the output of encoder block 1 through the whole
    # head: measured 3.1e-2 of its largest entry with the HIP and the module head alike (so the encoder's fp16 block outputs,
    # not the head, set it), hence 5e-2 here instead of that test's 3e-2; every other tensor stays far below
    for k, e in entry.items():
        assert e <= (5e-2 if k == "grad:linears_modulelist.0.proj.bias" else 3e-2), (k, e)
    assert worst < 2e-4, worst
    np.testing.assert_allclose(norms, g["grad_norms"], rtol=1e-2, atol=1e-6)
    assert all(p.grad is None and not p.requires_grad for p in m.encoder.parameters())
    assert list(m.state_dict().keys()) == [str(k) for k in g["state_keys"]]


def test_seg_variant_equals_voc_seg_bit_identical():
    img = synth.make_images(2, H, W).cuda()
    seg = _seg_model()(img, ["a", "b"], mode="val")
    seg_voc, _, _ = _voc_model()(img, ["a", "b"], mode="val", labels=synth.TINY_LABELS)
    assert torch.equal(seg.detach(), seg_voc.detach())


def test_seg_only_engine_bit_identical_to_default_engine():
    from weclip_vit_comer_amd.clip import vit_engine as VE
    from weclip_vit_comer_amd.head_engine import HeadEngine, HeadFunction
    m = _seg_model(train=True)
    img = synth.make_images(2, H, W).cuda()
    x16 = VE.X16Stack(m.encoder.visual.transformer.layers - 1)
    with torch.no_grad():
        _, B, Lq = m.encode(img, x16)
    drop = ((torch.rand(B, 256, device="cuda", generator=torch.Generator("cuda").manual_seed(5)) >= 0.1).float() / 0.9).contiguous()
    w = torch.randn(2, 21, H // 16, W // 16, device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    out = {}
    for mode in (True, False):
        eng = HeadEngine(m.decoder_fts_fuse, m.decoder, attn_pred=mode)
        for p in eng.params():
            p.grad = None
        seg, ap = HeadFunction.apply(eng, x16, B, Lq, H // 16, W // 16, drop, *eng.params())
        assert (ap is None) == (not mode)
        (seg * w).sum().backward()
        out[mode] = (seg.detach().clone(), [p.grad.clone() for p in eng.params()])
    assert torch.equal(out[True][0], out[False][0])
    for a, b in zip(out[True][1], out[False][1]):
        assert torch.equal(a, b)


def _ce_ref64(seg, label, ignore=255):
    x = seg.detach().double().cpu().requires_grad_(True)
    up = F.interpolate(x, size=tuple(label.shape[1:]), mode="bilinear", align_corners=False)
    loss = F.cross_entropy(up, label.cpu(), ignore_index=ignore)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("nc", [1, 2, 21, 81, 128])
@pytest.mark.parametrize("hw,HW", [((3, 4), (37, 53)), ((4, 6), (64, 96)), ((9, 7), (5, 6)), ((1, 1), (7, 9))])
def test_ce_loss_matches_fp64_torch(nc, hw, HW):
    from weclip_vit_comer_amd.utils.losses import ce_loss_counts, get_ce_loss_fused
    g = torch.Generator().manual_seed(nc * 100 + HW[0])
    B = 2
    seg = torch.randn(B, nc, *hw, generator=g) * 3
    label = torch.randint(0, nc, (B, *HW), generator=g)
    label[:, : max(1, HW[0] // 5), :] = 255                         # an ignore band
    label[0, -1, -1] = 255
    x = seg.cuda().requires_grad_(True)
    loss = get_ce_loss_fused(x, label.cuda(), 255)
    loss.backward()
    ref, gref = _ce_ref64(seg, label)
    n_valid, n_bad = ce_loss_counts()
    assert int(n_valid.item()) == int((label != 255).sum()) and int(n_bad.item()) == 0
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()) + 1e-7, (loss.item(), ref.item())
    err = (x.grad.double().cpu() - gref).abs().max().item()
    assert err <= 1e-5 * gref.abs().max().item() + 1e-9, (err, gref.abs().max().item())


def test_ce_loss_all_ignored_matches_torch():
    from weclip_vit_comer_amd.utils.losses import get_ce_loss_fused
    seg = torch.randn(2, 21, 3, 4)
    label = torch.full((2, 37, 53), 255, dtype=torch.int64)
    x = seg.cuda().requires_grad_(True)
    loss = get_ce_loss_fused(x, label.cuda(), 255)
    loss.backward()
    ref, gref = _ce_ref64(seg, label)
    assert torch.isnan(loss).item() and torch.isnan(ref).item()
    assert torch.equal(x.grad.cpu(), torch.zeros_like(seg)) and torch.equal(gref, torch.zeros_like(gref))     # zero, as torch


def test_ce_loss_out_of_range_labels_are_counted_and_ignored():
    from weclip_vit_comer_amd.utils.losses import ce_loss_counts, get_ce_loss_fused
    g = torch.Generator().manual_seed(3)
    seg = torch.randn(2, 21, 4, 6, generator=g)
    label = torch.randint(0, 21, (2, 64, 96), generator=g)
    label[:, :4] = 255
    bad = label.clone()
    bad[0, 10, :7] = 21
    bad[1, 20, :5] = -3
    bad[1, 30, 0] = 1 << 40
    x = seg.cuda().requires_grad_(True)
    loss = get_ce_loss_fused(x, bad.cuda(), 255)
    loss.backward()
    n_valid, n_bad = ce_loss_counts()
    assert int(n_bad.item()) == 13
    ok = label.clone()
    ok[bad != label] = 255                                            # == treating the bad labels as ignored
    ref, gref = _ce_ref64(seg, ok)
    assert int(n_valid.item()) == int((ok != 255).sum())
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert (x.grad.double().cpu() - gref).abs().max().item() <= 1e-5 * gref.abs().max().item()


def test_ce_loss_is_deterministic_and_refuses_bad_arguments():
    from weclip_vit_comer_amd import _lib as L
    from weclip_vit_comer_amd.utils.losses import get_ce_loss_fused
    g = torch.Generator().manual_seed(4)
    seg = torch.randn(4, 81, 8, 8, generator=g).cuda()
    label = torch.randint(0, 81, (4, 128, 128), generator=g).cuda()
    outs = []
    for _ in range(2):
        x = seg.clone().requires_grad_(True)
        loss = get_ce_loss_fused(x, label, 255)
        loss.backward()
        outs.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # the C entry refuses before launching anything: the output buffer stays as it was
    f32 = torch.float32
    part, sums = torch.empty(4096, device="cuda"), torch.full((4,), 7.0, device="cuda")
    tmp, grad = torch.empty(2 * 4 * 129 * 8 * 128, device="cuda"), torch.full((4, 129, 8, 8), 7.0, device="cuda")
    for nc in (0, 129):
        with pytest.raises(RuntimeError, match="bad size"):
            L.lib().wc_ce_loss_fwd_bwd(L.ptr(seg, f32), L.ptr(label, torch.int64), L.ptr(part), L.ptr(sums), L.ptr(tmp), L.ptr(grad),
                                       4, nc, 8, 8, 128, 128, 255, L.stream())
    with pytest.raises(RuntimeError, match="null"):
        L.lib().wc_ce_loss_fwd_bwd(L.ptr(seg, f32), None, L.ptr(part), L.ptr(sums), L.ptr(tmp), L.ptr(grad), 4, 81, 8, 8, 128, 128,
                                   255, L.stream())
    import ctypes
    mis = ctypes.c_void_p(label.data_ptr() + 4)
    with pytest.raises(RuntimeError, match="misaligned"):
        L.lib().wc_ce_loss_fwd_bwd(L.ptr(seg, f32), mis, L.ptr(part), L.ptr(sums), L.ptr(tmp), L.ptr(grad), 4, 81, 8, 8, 128, 64,
                                   255, L.stream())
    torch.cuda.synchronize()
    assert (sums == 7.0).all().item() and (grad == 7.0).all().item()


def test_ce_loss_torch_op():
    import weclip_vit_comer_amd as W
    W.register_torch_ops()
    g = torch.Generator().manual_seed(8)
    seg = torch.randn(2, 21, 3, 4, generator=g)
    label = torch.randint(0, 21, (2, 37, 53), generator=g)
    out = torch.ops.weclip.ce_loss(seg.cuda(), label.cuda(), 255)
    ref, _ = _ce_ref64(seg, label)
    assert abs(out.item() - ref.item()) <= 1e-5 * ref.item()


BATCHES = [11, 12, 13]


def _labels(seed, hw=(37, 53)):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, 21, (2, *hw), generator=g)
    lab[:, :3] = 255
    return lab


def _run_steps(graph, batches=tuple((s, (37, 53)) for s in BATCHES), make_step=None):
    from weclip_vit_comer_amd.train_step import SupervisedTrainStep
    torch.manual_seed(0)
    m = _seg_model()                 # eval: no Dropout2d, so eager and replayed steps see the same arithmetic
    step = (make_step or SupervisedTrainStep)(m, graph=graph)
    losses = []
    for s, hw in batches:
        img = synth.make_images(2, H, W, seed=s).cuda()
        losses.append(step(img, _labels(s, hw).cuda()).item())
    params = torch.cat([p.detach().flatten() for p in m.get_param_groups()[3]])
    return losses, params, step, m


def test_supervised_step_graph_replay_is_bit_identical_to_eager():
    le, pe, _, me = _run_steps(False)
    lg, pg, step, mg = _run_steps(True)
    assert len(step._graphs) == 1 and next(iter(step._graphs.values()))["graph"] is not None
    assert me.iter_num == mg.iter_num == 3
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg)
    assert len(set(le)) == 3 and all(np.isfinite(le))


def test_supervised_step_second_signature_gets_its_own_graph():
    """Two label sizes: two graphs out of one pool, `iter_num` counted once per step across both, all of it as in eager."""
    batches = [(11, (37, 53)), (12, (37, 53)), (13, (40, 48)), (14, (40, 48)), (15, (40, 48))]
    le, pe, _, me = _run_steps(False, batches)
    lg, pg, step, mg = _run_steps(True, batches)
    assert len(step._graphs) == 2 and all(ent["graph"] is not None for ent in step._graphs.values())
    assert me.iter_num == mg.iter_num == 5
    assert all(np.isfinite(lg)) and le == lg, (le, lg)
    assert torch.equal(pe, pg)


def test_supervised_step_subclass_loss_override_is_captured():
    """A `loss` override that also writes to a device buffer runs inside the captured region: every replay refreshes the
    buffer (what train.LoggedTrainStep.losses relies on for the weak class)."""
    from weclip_vit_comer_amd.train_step import SupervisedTrainStep
    buf = torch.full((), -1.0, device="cuda")

    class Marked(SupervisedTrainStep):
        def loss(self, seg, label):
            loss = super().loss(seg, label)
            buf.copy_(loss.detach())
            return loss

    losses, _, step, _ = _run_steps(True, make_step=Marked)
    assert next(iter(step._graphs.values()))["graph"] is not None
    assert len(set(losses)) == 3 and buf.item() == losses[2]


def test_supervised_step_matches_stock_torch_step():
    from weclip_vit_comer_amd.train_step import SupervisedTrainStep, make_optimizer
    img = synth.make_images(2, H, W, seed=11).cuda()
    lab = _labels(11).cuda()
    m = _seg_model()
    loss = SupervisedTrainStep(m)(img, lab).item()
    grads = {n: p.grad.detach().clone() for n, p in list(m.decoder.named_parameters()) + list(m.decoder_fts_fuse.named_parameters())}
    params = torch.cat([p.detach().flatten() for p in m.get_param_groups()[3]])
    r = _seg_model(head="torch")                 # module head + stock torch CE + the same optimizer settings
    opt = make_optimizer(r)
    seg = r(img)
    rl = F.cross_entropy(F.interpolate(seg, size=lab.shape[1:], mode="bilinear", align_corners=False), lab, ignore_index=255)
    opt.zero_grad()
    rl.backward()
    opt.step()
    assert abs(loss - rl.item()) <= 1e-3 * abs(rl.item())
    rg = {n: p.grad.detach() for n, p in list(r.decoder.named_parameters()) + list(r.decoder_fts_fuse.named_parameters())}
    a = np.array([float(grads[n].norm()) for n in sorted(rg)])
    b = np.array([float(rg[n].norm()) for n in sorted(rg)])
    assert np.abs(a - b).max() / b.max() < 2e-3
    rparams = torch.cat([p.detach().flatten() for p in r.get_param_groups()[3]])
    assert (params - rparams).abs().max().item() < 1e-5


def test_msc_flip_evaluator_on_seg_variant_matches_reference_validate(golden):
    from make_seg_golden import msc_inputs
    from weclip_vit_comer_amd.msc_flip import MscFlipEvaluator
    from weclip_vit_comer_amd.utils.dcrf import DenseCRF
    g = golden("tiny_voc_segonly_msc.npz")
    m = _seg_model()
    ev = MscFlipEvaluator(m, 21, scales=(1.0, 0.75), resize_long=int(g["resize_long"]),
                          crf=DenseCRF(iter_max=10, pos_w=3, pos_xy_std=3, bi_w=4, bi_xy_std=64, bi_rgb_std=5))
    worst = 0.0
    for i, (_, img, lab) in enumerate(msc_inputs()):
        p, mp_ = ev.add(img[None].cuda(), lab[None].cuda())
        assert tuple(p.shape) == tuple(lab.shape)
        worst = max(worst, float((p.cpu().numpy().astype(np.uint8) != g[f"pred{i}"]).mean()),
                    float((mp_.cpu().numpy().astype(np.uint8) != g[f"msc_pred{i}"]).mean()))
    dh = np.abs(ev.hist.cpu().numpy() - g["hist"]).sum() / g["hist"].sum()
    dm = np.abs(ev.msc_hist.cpu().numpy() - g["msc_hist"]).sum() / g["msc_hist"].sum()
    print(f"seg variant msc+flip vs reference validate: worst arg-max mismatch {worst:.3%}; histogram L1 {dh:.3%} / {dm:.3%}")
    assert worst < 1.5e-2 and dh < 1.2e-2 and dm < 1.2e-2        # test_msc_flip_driver_matches_reference_validate's thresholds
    assert int(ev.hist.sum()) == int(g["hist"].sum()) and int(ev.msc_hist.sum()) == int(g["msc_hist"].sum())
    # the CRF leg on the same images
    for _, img, lab in msc_inputs():
        rgb = (torch.rand(lab.shape[0], lab.shape[1], 3, generator=torch.Generator().manual_seed(1)) * 255).to(torch.uint8)
        s, ms, c = ev.add_with_crf(img[None].cuda(), lab[None].cuda(), rgb.numpy())
        assert tuple(c.shape) == tuple(lab.shape) and int(c.min()) >= 0 and int(c.max()) < 21
    assert int(ev.crf_hist.sum()) == int(g["hist"].sum()) and ev.images == 6
    s1, s2 = ev.scores()
    assert 0.0 <= s2["pAcc"] <= 1.0 and 0.0 <= ev.crf_scores()["pAcc"] <= 1.0
