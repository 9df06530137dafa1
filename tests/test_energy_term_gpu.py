"""The dense energy loss as a term of the training step on the MI355X (csrc/energy_prep.hip, utils.losses.get_energy_loss_fused,
TrainStep / SupervisedTrainStep reg=...) against the fp64 restatement tests/energy_term_ref.py, the stock f32 torch chain and
the reference's own numbers in tests/golden/energy_loss.npz.

Bounds.  Prep forward: images_s, rois_s, unlabel_u8 bit-equal to the stock f32 chain; |P_s - P64| <= (16 M + K + 16) 2^-24 per
element (energy_term_ref.p_bound; tests/test_energy_term_cpu.py shows that the stock chain meets it on the same inputs).  Prep
backward: error over the largest entry <= 2^-10 (EPS of tests/test_energy_gpu.py) and <= max(8 x the stock f32 chain's own error,
2^-20).  Whole term: loss and gradient within EPS of fp64 and of the recorded reference.

Every test prints its measured figures before it asserts; DESIGN.md section 15.2 records the worst of them."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_term_ref as R  # noqa: E402

EPS = 2.0 ** -10                      # this loss's tolerance against fp64 (tests/test_energy_gpu.py)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "energy_loss.npz")
CFG = (1e-7, 15, 100)                 # weight, sigma_rgb, sigma_xy: the lineage's (tests/golden/make_energy_golden.py:27)


def _losses():
    from weclip_vit_comer_amd.utils import losses
    return losses


def _dev_box(box, dtype=torch.int32):
    return None if box is None else torch.tensor(box, dtype=dtype).cuda()


def _prep_fwd(img, seg, lab, box, e):
    return _losses().energy_prep_forward(img.cuda().contiguous(), seg.cuda().contiguous(), lab.cuda().long().contiguous(), _dev_box(box),
                                         e, R.MEAN, R.STD)


# ------------------------------------------------------------------------------------------------ prep forward
def _check_prep_forward(hw, HW, K, N, e, seed, mag=3.0):
    img, seg, lab, box = R.make_case(hw, HW, K, N, seed, mag)
    s = 2.0 ** -e
    images_s, P_s, rois_s, unl = (t.cpu() for t in _prep_fwd(img, seg, lab, box, e))
    ri, rP, rr, ru = R.prep_forward(img, seg, lab, box, s, torch.float32)           # the stock f32 chain
    assert images_s.dtype == rois_s.dtype == P_s.dtype == torch.float32 and unl.dtype == torch.uint8
    assert images_s.shape == ri.shape and P_s.shape == rP.shape and rois_s.shape == rr.shape and unl.shape == ru.shape
    assert torch.equal(images_s, ri), "images_s differs from img * std + mean at the nearest source"
    assert torch.equal(rois_s, rr), "rois_s"
    assert torch.equal(unl != 0, ru), "unlabel_u8"
    P64 = R.prep_forward(img, seg, lab, box, s, R.F64)[1]
    assert torch.isfinite(P_s).all().item()
    return R.worst_p_ratio(P_s, P64, seg, HW, K)


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("e", R.ES)
@pytest.mark.parametrize("si", range(len(R.SHAPES)))
def test_prep_forward(si, e, K):
    hw, HW = R.SHAPES[si]
    for N in R.NS:
        ratio = _check_prep_forward(hw, HW, K, N, e, R.case_seed(si, e, K, N))
        print(f"{hw}->{HW} e={e} K={K} N={N}: worst |P - P64| / ((16 M + K + 16) 2^-24) = {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("e", R.ES)
@pytest.mark.parametrize("si", range(len(R.SHAPES)))
def test_prep_forward_logits_of_magnitude_30(si, e):
    hw, HW = R.SHAPES[si]
    ratio = _check_prep_forward(hw, HW, 21, 1, e, R.case_seed(si, e, 21, 1), mag=30.0)
    print(f"{hw}->{HW} e={e} K=21 logits x 30: worst ratio {ratio:.3f}")
    assert ratio <= 1.0


def test_prep_forward_box_dtypes_and_label_dtypes_agree():
    """A device box of any integer type, a host tensor and rows give the same ROI; uint8 and int64 labels the same mask."""
    LS = _losses()
    (hw, HW), K, N = R.SHAPES[1], 21, 3
    img, seg, lab, _ = R.make_case(hw, HW, K, N, seed=2)              # seed 2: int64 labels with a patch
    box = R.boxes("border", N, *HW)
    layer = LS.DenseEnergyLoss(*CFG, 0.5)
    outs = []
    for b in (box, torch.tensor(box), _dev_box(box, torch.int16), _dev_box(box, torch.int64), _dev_box(box, torch.uint8)):
        outs.append(LS.get_energy_loss_fused(img.cuda(), seg.cuda(), lab.cuda(), b, layer))
    outs.append(LS.get_energy_loss_fused(img.cuda(), seg.cuda(), lab.to(torch.uint8).cuda(), box, layer))
    assert all(torch.equal(outs[0], o) for o in outs[1:]) and outs[0].item() != 0


# ------------------------------------------------------------------------------------------------ prep backward
def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("K", [1, 21, 33, 128])
@pytest.mark.parametrize("e", R.ES)
@pytest.mark.parametrize("si", range(len(R.SHAPES)))
def test_prep_backward(si, e, K):
    LS = _losses()
    (h, w), (H, W) = R.SHAPES[si]
    N, s, coef = 3, 2.0 ** -e, -0.37
    g = torch.Generator().manual_seed(50 + R.case_seed(si, e, K, N))
    seg = 3 * torch.randn(N, K, h, w, generator=g)
    A = torch.randn(N, K, H >> e, W >> e, generator=g)
    roi = (torch.rand(N, H >> e, W >> e, generator=g) > 0.3).float()
    got = LS.energy_prep_backward(A.cuda(), roi.cuda(), seg.cuda(), coef, (H, W), e).cpu()
    ref = R.prep_backward(seg, (H, W), s, A, roi, coef, R.F64)
    stock = R.prep_backward(seg.cuda(), (H, W), s, A.cuda(), roi.cuda(), coef, torch.float32).cpu()
    assert got.shape == seg.shape and torch.isfinite(got).all().item()
    if ref.abs().max().item() == 0:            # K = 1: the soft-max is constant
        assert got.abs().max().item() == 0
        return
    e_got, e_stock = _rel(got, ref), _rel(stock, ref)
    print(f"{(h, w)}->{(H, W)} e={e} K={K}: error / largest entry: kernel {e_got:.3e}, stock f32 chain {e_stock:.3e}")
    assert e_got <= EPS
    assert e_got <= max(8 * e_stock, 2.0 ** -20)


# ------------------------------------------------------------------------------------------------ the whole term
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("i", range(4))
def test_pinned_to_the_reference_fixture(gold, i):
    """seg_lowres = the recorded full-resolution logits (the up-sample is the identity): loss and logit gradient against the
    unmodified reference's recorded numbers and against fp64, as test_energy_loss_vs_fixture_and_fp64 asserts for the stock path."""
    LS = _losses()
    t = lambda k: torch.from_numpy(gold[f"c{i}_{k}"])
    weight, srgb, sxy, s = gold[f"c{i}_cfg"].tolist()
    box = gold[f"c{i}_box"].tolist()
    lg = t("logit").cuda().requires_grad_(True)
    loss = LS.get_energy_loss_fused(t("img").cuda(), lg, t("label").cuda(), box, LS.DenseEnergyLoss(weight, srgb, sxy, s))
    assert loss.is_cuda and tuple(loss.shape) == (1,)
    loss.backward()
    ref_loss, ref_grad = t("loss").double(), t("grad").double()
    r64 = R.energy_term(t("img"), t("logit"), t("label"), box, weight, srgb, sxy, s)
    e_loss, e_grad = _rel(loss.detach().cpu(), ref_loss), _rel(lg.grad.cpu(), ref_grad)
    e_loss64, e_grad64 = _rel(loss.detach().cpu(), r64["loss"]), _rel(lg.grad.cpu(), r64["grad"])
    print(f"case {i}: vs the reference: loss rel {e_loss:.3e}, gradient / largest {e_grad:.3e}; vs fp64: {e_loss64:.3e}, {e_grad64:.3e}")
    assert max(e_loss, e_loss64) <= EPS and max(e_grad, e_grad64) <= EPS


@pytest.mark.parametrize("e", [0, 1])
@pytest.mark.parametrize("hw,HW", [((2, 3), (26, 22)), ((3, 4), (40, 36))])
def test_end_to_end_with_real_upsampling(hw, HW, e):
    """Against fp64: EPS.  Against the stock get_energy_loss on the same card: both are within EPS of fp64, so 2 EPS."""
    LS = _losses()
    N, K, s = 2, 21, 2.0 ** -e
    img, seg, lab, _ = R.make_case(hw, HW, K, N, seed=2 + e)          # labels with a patch of 255: int64 (e = 0), uint8 (e = 1)
    box = R.boxes("border", N, *HW)
    layer = LS.DenseEnergyLoss(*CFG, s)
    sg = seg.cuda().requires_grad_(True)
    loss = LS.get_energy_loss_fused(img.cuda(), sg, lab.cuda(), _dev_box(box), layer)
    loss.backward()
    r64 = R.energy_term(img, seg, lab, box, *CFG, s)
    st = seg.cuda().requires_grad_(True)
    stock = LS.get_energy_loss(img.cuda(), R.upsample(st, HW), lab.cuda(), box, layer)
    stock.backward()
    e_loss, e_grad = _rel(loss.detach().cpu(), r64["loss"]), _rel(sg.grad.cpu(), r64["grad"])
    s_loss, s_grad = _rel(stock.detach().cpu(), r64["loss"]), _rel(st.grad.cpu(), r64["grad"])
    d_loss, d_grad = _rel(loss.detach().cpu(), stock.detach().cpu().double()), _rel(sg.grad.cpu(), st.grad.cpu().double())
    print(f"{hw}->{HW} e={e}: vs fp64: loss {e_loss:.3e}, gradient {e_grad:.3e} (stock: {s_loss:.3e}, {s_grad:.3e}); "
          f"vs stock: {d_loss:.3e}, {d_grad:.3e}")
    assert r64["loss"].item() != 0 and r64["grad"].abs().max().item() > 0
    assert e_loss <= EPS and e_grad <= EPS
    assert d_loss <= 2 * EPS and d_grad <= 2 * EPS


# ------------------------------------------------------------------------------------------------ behaviour
def test_run_to_run_no_sync_and_opcheck():
    import weclip_vit_comer_amd
    LS = _losses()
    weclip_vit_comer_amd.register_torch_ops()
    (hw, HW), K, N = R.SHAPES[1], 33, 3
    img, seg, lab, _ = R.make_case(hw, HW, K, N, seed=2)
    img, seg, lab = img.cuda(), seg.cuda(), lab.cuda()
    box = _dev_box(R.boxes("border", N, *HW), torch.int16)
    layer = LS.DenseEnergyLoss(*CFG, 0.5)
    w = torch.tensor([0.37], device="cuda")

    def run(fn):
        p = seg.clone().requires_grad_(True)
        loss = fn(p)
        (loss * w).sum().backward()
        return loss.detach(), p.grad

    fused = lambda p: LS.get_energy_loss_fused(img, p, lab, box, layer)
    op = lambda p: torch.ops.weclip.energy_term(img, p, lab, box, 1e-7, 15.0, 100.0, 0.5, list(R.MEAN), list(R.STD))[0]
    l1, g1 = run(fused)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            l2, g2 = run(fused)
            l3, g3 = run(op)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert not [str(c.message) for c in caught if "called a synchronizing" in str(c.message)], [str(c.message) for c in caught]
    assert torch.equal(l1, l2) and torch.equal(g1, g2)                 # bit-identical from run to run
    assert torch.equal(l1, l3) and torch.equal(g1, g3)                 # the registered op gives the Function's tensors
    assert l1.item() != 0 and g1.abs().max().item() > 0
    torch.library.opcheck(torch.ops.weclip.energy_term, (img, seg.clone().requires_grad_(True), lab, box.int(), 1e-7, 15.0, 100.0, 0.5,
                                                        list(R.MEAN), list(R.STD)))
    torch.library.opcheck(torch.ops.weclip.energy_term, (img, seg.clone().requires_grad_(True), lab, None, 1e-7, 15.0, 100.0, 1.0,
                                                        list(R.MEAN), list(R.STD)))


def test_zero_roi_and_all_unlabelled():
    LS = _losses()
    (hw, HW), K, N = R.SHAPES[2], 21, 2
    img, seg, lab, _ = R.make_case(hw, HW, K, N, seed=0)
    layer = LS.DenseEnergyLoss(*CFG, 0.5)
    sg = seg.cuda().requires_grad_(True)
    loss = LS.get_energy_loss_fused(img.cuda(), sg, lab.cuda(), [[5, 5, 0, HW[1]], [0, HW[0], 7, 7]], layer)     # empty boxes
    loss.backward()
    assert loss.item() == 0 and sg.grad.abs().max().item() == 0
    sg = seg.cuda().requires_grad_(True)
    loss = LS.get_energy_loss_fused(img.cuda(), sg, torch.full_like(lab, 255).cuda(), None, layer)
    loss.backward()
    assert torch.isfinite(loss).all().item() and torch.isfinite(sg.grad).all().item() and sg.grad.abs().max().item() > 0
    r64 = R.energy_term(img, seg, torch.full_like(lab, 255), None, *CFG, 0.5)
    assert _rel(loss.detach().cpu(), r64["loss"]) <= EPS and _rel(sg.grad.cpu(), r64["grad"]) <= EPS


# ------------------------------------------------------------------------------------------------ the steps
H, W = synth.TINY_HW
REG = {"coef": 0.5, "weight": 1e-3}          # a weight at which the term moves the parameters of the tiny model visibly
BATCHES = [(11, [[3, 7], [0, 14]]), (12, [[1, 2], [5, 19]]), (13, [[4, 6], [8, 9]]), (14, [[3, 7], [10, 11]]), (15, [[0, 1], [2, 3]])]


def _boxes(seed):
    """Per-image boxes that change from batch to batch, as a device tensor of the loader's type (int16)."""
    return torch.tensor([[seed % 5, H - 3, 2, W - seed % 7], [1, H - seed % 4, seed % 6, W]], dtype=torch.int16).cuda()


def _voc_model():
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP
    sd = synth.make_clip_state_dict(**synth.TINY)
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
    m = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4,
               dataset_root_path=None, device="cuda", text_features=(bg.cuda(), fg.cuda()))
    m.decoder_fts_fuse.load_state_dict(fuse)
    m.decoder.load_state_dict(dec)
    return m.eval()                  # eval: no Dropout2d, so eager and replayed steps see the same arithmetic


def _run(graph, reg, with_box=True):
    from weclip_vit_comer_amd.train_step import TrainStep
    torch.manual_seed(0)
    m = _voc_model()
    step = TrainStep(m, graph=graph, reg=reg)
    losses, grads = [], []
    for seed, labels in BATCHES:
        img = synth.make_images(2, H, W, seed=seed).cuda()
        out = step(img, labels=labels, img_box=_boxes(seed)) if with_box else step(img, labels=labels)
        losses.append([o.item() for o in out])
        grads.append(step.bucket.flat.clone())
    return losses, grads, torch.cat([p.detach().flatten() for p in m.get_param_groups()[3]]), step


@pytest.fixture(scope="module")
def plain_step():
    return _run(False, None, with_box=False)


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    assert torch.equal(a[2], b[2])


def test_step_graph_replay_equals_eager_with_the_term(plain_step):
    eager, graph = _run(False, REG), _run(True, REG)
    step = graph[3]
    assert len(step._graphs) == 1 and next(iter(step._graphs.values()))["graph"] is not None
    _same(eager, graph)
    assert all(len(l) == 4 and l[3] != 0 for l in eager[0])
    assert len({l[3] for l in eager[0]}) == len(BATCHES)          # boxes and batches really differ
    assert not torch.equal(eager[2], plain_step[2])               # the term reached the parameters
    # the loss is seg_loss + 0.1 attn_loss + coef * energy
    for loss, seg_loss, attn_loss, energy in eager[0]:
        terms = (seg_loss, 0.1 * attn_loss, REG["coef"] * energy)
        assert abs(loss - sum(terms)) <= 1e-5 * sum(abs(t) for t in terms)


def test_step_start_iter_gives_two_graphs_and_a_zero_before(plain_step):
    reg = dict(REG, start_iter=2)
    eager, graph = _run(False, reg), _run(True, reg)
    step = graph[3]
    assert len(step._graphs) == 2 and all(ent["graph"] is not None for ent in step._graphs.values())
    _same(eager, graph)
    assert [l[3] == 0 for l in graph[0]] == [True, True, False, False, False]
    assert eager[0][0][:3] == plain_step[0][0] and eager[0][1][:3] == plain_step[0][1]      # before the start: the plain step
    for a, b in zip(eager[1][:2], plain_step[1][:2]):
        assert torch.equal(a, b)


def test_step_without_reg_is_unchanged(plain_step):
    """reg=None returns three values; a term that never starts leaves losses, gradients and parameters bit-identical to it, in
    eager and in graph mode, and so does passing img_box to a step without the term."""
    assert all(len(l) == 3 for l in plain_step[0])
    never = dict(REG, start_iter=10 ** 9)
    for graph in (False, True):
        r = _run(graph, never)
        assert all(l[3] == 0 for l in r[0])
        _same(([l[:3] for l in r[0]], r[1], r[2]), plain_step)
    _same(_run(True, None, with_box=False), plain_step)


def _seg_model():
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc_seg import WeCLIP
    sd = synth.make_clip_state_dict(**synth.TINY)
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
    m = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4, device="cuda")
    m.decoder_fts_fuse.load_state_dict(fuse)
    m.decoder.load_state_dict(dec)
    return m.eval()


def _run_supervised(graph, reg):
    from weclip_vit_comer_amd.train_step import SupervisedTrainStep
    torch.manual_seed(0)
    m = _seg_model()
    step = SupervisedTrainStep(m, graph=graph, reg=reg)
    losses = []
    for seed, _ in BATCHES:
        img = synth.make_images(2, H, W, seed=seed).cuda()
        lab = torch.randint(0, 21, (2, H, W), generator=torch.Generator().manual_seed(seed))
        lab[:, :3] = 255
        out = step(img, lab.cuda(), _boxes(seed)) if reg is not None else step(img, lab.cuda())
        losses.append([o.item() for o in out] if reg is not None else [out.item()])
    return losses, [], torch.cat([p.detach().flatten() for p in m.get_param_groups()[3]]), step


@pytest.fixture(scope="module")
def plain_supervised():
    return _run_supervised(False, None)


def test_supervised_step_graph_replay_equals_eager_with_the_term(plain_supervised):
    eager, graph = _run_supervised(False, REG), _run_supervised(True, REG)
    assert len(graph[3]._graphs) == 1 and next(iter(graph[3]._graphs.values()))["graph"] is not None
    _same(eager, graph)
    assert all(len(l) == 2 and l[1] != 0 for l in eager[0]) and not torch.equal(eager[2], plain_supervised[2])


def test_supervised_step_start_iter_and_no_reg(plain_supervised):
    reg = dict(REG, start_iter=2)
    eager, graph = _run_supervised(False, reg), _run_supervised(True, reg)
    assert len(graph[3]._graphs) == 2 and all(ent["graph"] is not None for ent in graph[3]._graphs.values())
    _same(eager, graph)
    assert [l[1] == 0 for l in graph[0]] == [True, True, False, False, False]
    assert [l[0] for l in eager[0][:2]] == [l[0] for l in plain_supervised[0][:2]]
    never = _run_supervised(True, dict(REG, start_iter=10 ** 9))
    _same(([l[:1] for l in never[0]], [], never[2]), plain_supervised)


# ------------------------------------------------------------------------------------------------ the training entry point
def _driver(tmp_path, *flags):
    """Six graph-replayed iterations of train.Trainer on the synthetic VOC tree of tests/test_train_driver_gpu.py (crop 64)."""
    import test_train_driver_gpu as D
    from weclip_vit_comer_amd import train as T
    root, lists = D._write_voc(str(tmp_path / "voc"))
    path, cfg = D._cfg(str(tmp_path), root, lists)
    tr = T.Trainer(cfg, D._args(path, "--graph", *flags), model=D._model(), timestamp="t")
    for _ in range(3):
        tr.step_once()
    recs = [tr.log()]
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            tr.step_once()
            tr.step_once()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    tr.step_once()
    recs.append(tr.log())
    tr.close()
    return recs, T.read_metrics(tr.metrics_path), [str(c.message) for c in caught if "called a synchronizing" in str(c.message)], tr


def test_train_driver_with_and_without_reg_loss(tmp_path, caplog):
    import logging
    plain_keys = ["iter", "lr", "seg_loss", "attn_loss", "pseudo_seg_mAcc"]
    with caplog.at_level(logging.INFO, logger="weclip.train"):
        # active from the first step: the signatures are captured at the steps at which the plain driver captures them, so the
        # counted steps 4 and 5 are replays, as in tests/test_train_driver_gpu.py
        recs, lines, syncs, tr = _driver(tmp_path / "reg", "--reg_loss", "--reg_start", "0")
    assert tr.step.reg.start_iter == 0 and tr.step.reg.step_num == 6 and not syncs, syncs
    assert [list(r) for r in lines] == [plain_keys + ["reg_loss"]] * 2 and lines == recs
    assert all(np.isfinite(r["reg_loss"]) and r["reg_loss"] != 0 for r in recs)
    assert sum(", reg_loss: " in r.getMessage() for r in caplog.records) == 2
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="weclip.train"):
        recs, lines, syncs, tr = _driver(tmp_path / "plain")
    assert tr.step.reg is None and not syncs and [list(r) for r in lines] == [plain_keys] * 2
    assert not any("reg_loss" in r.getMessage() for r in caplog.records)
    # without --reg_start the term waits for train.cam_iters
    from weclip_vit_comer_amd import train as T
    args = T.build_parser().parse_args(["--config", "c.yaml", "--reg_loss"])
    assert T.reg_settings(tr.cfg, args)["start_iter"] == tr.cfg.train.cam_iters == 2000
