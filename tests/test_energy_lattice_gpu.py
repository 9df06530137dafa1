"""The lattice form of the dense energy loss on the MI355X (csrc/energy_lattice.hip, utils.losses bilateral="lattice", TrainStep /
SupervisedTrainStep reg={"bilateral": "lattice"}, train.py --reg_bilateral lattice) against the composed fp64 restatement
tests/energy_lattice_ref.py.

Bounds (none of them new).  Filter: the header's |AS - AS64| <= eps * filter64(|S|) + 2^-24 with eps = 2^-10, per element, and the
device's vertex count M equal to the restatement's.  Loss and gradients: eps relative (the gradient: of its largest entry), the
tolerance of tests/test_energy_gpu.py.  Gate: bit-equal to the f32 definition.  Capture: bit-equal to eager.

Every test prints its measured figures before it asserts; DESIGN.md section 15.3 records the worst of them."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_lattice_ref as LE  # noqa: E402
import energy_ref as E  # noqa: E402
import energy_term_ref as R  # noqa: E402
import test_energy_gpu as TE  # noqa: E402      (its image and probability makers)
import test_energy_term_gpu as TG  # noqa: E402 (its tiny-model steps and its driver run)

EPS = 2.0 ** -10
ABS = 2.0 ** -24
GOLD = TE.GOLD
CFG = TG.CFG


def _losses():
    from weclip_vit_comer_amd.utils import losses
    return losses


def _constant(H, W, seed):
    return torch.full((3, H, W), 0.0) + torch.tensor([90.0 + seed % 50, 120.0, 33.5])[:, None, None]


def _ramp(H, W, seed):
    """tests/test_energy_gpu.py's ramp with its offset folded into 0..30, so that every colour stays inside [0, 256)."""
    return TE._ramp(H, W, seed % 7)


def _images(N, H, W, kind, seed):
    """N different images: 'noise', 'ramp', 'mixed' (image n alternates, so a batch-index slip shows), or 'constant': one
    constant image (its 6 vertices carry H W entries each) before noise images."""
    pick = {"noise": lambda n: TE._noise, "ramp": lambda n: _ramp, "mixed": lambda n: (TE._noise, _ramp)[n % 2],
            "constant": lambda n: _constant if n == 0 else TE._noise}[kind]
    return torch.stack([pick(n)(H, W, seed + 17 * n) for n in range(N)])


def _check_filter(img, seg, srgb, sxy, what):
    """bilateral_filter_batch(bilateral="lattice") against the restatement, per element, and M of every image."""
    LS = _losses()
    N, K, H, W = seg.shape
    wsp = LS._lattice_workspace(N, K, H, W, torch.device("cuda"))
    got = LS.bilateral_filter_batch(img.cuda(), seg.cuda(), srgb, sxy, bilateral="lattice", workspace=wsp)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == seg.shape
    flag, M = LS.lattice_vertex_counts(wsp[0], N)
    counts = []
    ref, scale = LE.lattice_filter_batch(img, seg, srgb, sxy, want_abs=True, counts=counts)
    got = got.cpu().double()
    assert torch.isfinite(got).all().item(), what
    ratio = ((got - ref).abs() / (EPS * scale + ABS)).max().item()
    print(f"{what}: worst |AS - AS64| / (eps filter64(|S|) + 2^-24) = {ratio:.3e}; M / pixel = {[round(m / (H * W), 2) for m in counts]}")
    assert flag.item() == 0 and M.tolist() == counts, (what, flag.item(), M.tolist(), counts)
    assert ratio <= 1.0, f"{what}: {ratio:.3e}"
    return got


SHAPES = [(5, 7), (13, 11), (37, 53), (40, 36)]      # 35 pixels: one slice workgroup and a bit; 1961, 1440: many, ragged
KS = [1, 21, 33, 128]                                # 33: the first second column tile; 128: the limit


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("hw", SHAPES)
def test_filter_vs_restatement(hw, K, N):
    H, W = hw
    kind = "mixed" if N == 3 else ("ramp" if K in (21, 128) else "noise")
    _check_filter(_images(N, H, W, kind, seed=H + K), TE._probs(N, K, H, W, seed=K + W), 15.0, 50.0, f"{H}x{W} K={K} N={N} {kind}")


def _smallest_sigma_xy(H, W, srgb):
    """The smallest f32 sigma_xy whose keys fit at H x W (the host's own bound, by bisection)."""
    from weclip_vit_comer_amd import _lib
    fn = ctypes.CDLL(_lib.LIB_PATH).wc_dcrf_lattice_key_bound
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_double)]
    b = ctypes.c_double()
    lo, hi = np.float32(1e-3), np.float32(50.0)
    assert fn(H, W, lo, srgb, ctypes.byref(b)) != 0 and fn(H, W, hi, srgb, ctypes.byref(b)) == 0
    for _ in range(64):
        mid = np.float32((lo + hi) / 2)
        if mid == lo or mid == hi:
            break
        if fn(H, W, mid, srgb, ctypes.byref(b)) == 0:
            hi = mid
        else:
            lo = mid
    return float(hi)


@pytest.mark.parametrize("kind", ["noise", "ramp"])
@pytest.mark.parametrize("hw,sxy", [(hw, sxy) for hw in SHAPES for sxy in (50.0, 25.0, 100.0)] + [((37, 53), "smallest")])
def test_filter_sigma_pairs(hw, sxy, kind):
    H, W = hw
    if sxy == "smallest":                            # the smallest sigma_xy the key bound admits: nearly every pixel its own vertices
        sxy = _smallest_sigma_xy(H, W, 15.0)
    _check_filter(_images(3, H, W, kind, seed=5), TE._probs(3, 21, H, W, seed=6), 15.0, sxy, f"{H}x{W} sxy={sxy:.4g} srgb=15 {kind}")


def test_filter_constant_image_takes_the_chunk_path():
    """A constant image puts all 1440 pixels on 6 vertices: segments of 1440 entries, five extra 256-entry chunks each."""
    H, W, K, N = 40, 36, 33, 3
    img = _images(N, H, W, "constant", seed=3)
    counts = []
    LE.lattice_filter_batch(img[:1], torch.zeros(1, 1, H, W), 15.0, 50.0, counts=counts)
    assert counts[0] * 256 < 6 * H * W                 # some segment is longer than a chunk
    _check_filter(img, TE._probs(N, K, H, W, seed=4), 15.0, 50.0, "constant 40x36 K=33 N=3")


def test_filter_signed_segs():
    H, W, K, N = 13, 11, 33, 3
    seg = torch.randn(N, K, H, W, generator=torch.Generator().manual_seed(8))
    _check_filter(_images(N, H, W, "mixed", seed=9), seg, 15.0, 50.0, "signed 13x11 K=33 N=3")
    H, W = 40, 36
    seg = torch.randn(N, K, H, W, generator=torch.Generator().manual_seed(9))
    _check_filter(_images(N, H, W, "constant", seed=9), seg, 15.0, 25.0, "signed constant 40x36 K=33 N=3")


@pytest.mark.parametrize("hw,K", [((13, 11), 21), ((40, 36), 33)])
def test_filter_images_of_a_batch_are_isolated(hw, K):
    """Image n of a batched call is bit-equal to the same image filtered alone (one shared structure, image after image)."""
    LS = _losses()
    H, W = hw
    img = _images(3, H, W, "constant" if H == 40 else "mixed", seed=11).cuda()
    seg = torch.randn(3, K, H, W, generator=torch.Generator().manual_seed(12)).cuda()
    batch = LS.bilateral_filter_batch(img, seg, 15.0, 50.0, bilateral="lattice")
    for n in range(3):
        alone = LS.bilateral_filter_batch(img[n:n + 1], seg[n:n + 1], 15.0, 50.0, bilateral="lattice")
        assert torch.equal(batch[n], alone[0]), n
    assert torch.equal(batch, LS.bilateral_filter_batch(img, seg, 15.0, 50.0, bilateral="lattice"))
    exact = LS.bilateral_filter_batch(img, seg, 15.0, 50.0)
    assert not torch.equal(batch, exact)


@pytest.mark.parametrize("hw,K,kind", [((13, 11), 21, "noise"), ((40, 36), 33, "constant")])
def test_filter_is_the_crf_lattice_filter(hw, K, kind):
    """The dense CRF and the energy loss run one lattice filter: one image through bilateral_filter_batch(bilateral="lattice")
    (no ROI, no gate) is bit-equal to utils.dcrf.lattice_filter on the same image in HWC form and the same planes.  Both build
    with lat_point, splat and blur with the same kernels on the same operand values, and end in 1 * (acc * alpha)."""
    from weclip_vit_comer_amd.utils import dcrf
    H, W = hw
    img = _images(1, H, W, kind, seed=7)[0].cuda()
    seg = TE._probs(1, K, H, W, seed=8).cuda()
    got = _losses().bilateral_filter_batch(img[None], seg, 15.0, 50.0, bilateral="lattice")[0]
    crf = dcrf.lattice_filter(img.permute(1, 2, 0).contiguous(), seg[0], 50.0, 15.0)
    assert got.abs().max().item() > 0 and torch.equal(got, crf)


def test_colours_outside_the_range_are_clamped_and_flagged():
    """A colour above 256 is clamped for the key and OR-ed into the device flag; the other images of the batch are untouched."""
    LS = _losses()
    H, W, K = 13, 11, 5
    img = _images(3, H, W, "mixed", seed=2)
    seg = TE._probs(3, K, H, W, seed=3)
    bad = img.clone()
    bad[1, 0, 4, 5] = 300.0
    wsp = LS._lattice_workspace(3, K, H, W, torch.device("cuda"))
    good = LS.bilateral_filter_batch(img.cuda(), seg.cuda(), 15.0, 50.0, bilateral="lattice", workspace=wsp)
    assert LS.lattice_vertex_counts(wsp[0], 3)[0].item() == 0
    got = LS.bilateral_filter_batch(bad.cuda(), seg.cuda(), 15.0, 50.0, bilateral="lattice", workspace=wsp)
    assert LS.lattice_vertex_counts(wsp[0], 3)[0].item() == 1
    assert torch.isfinite(got).all().item() and torch.equal(got[0], good[0]) and torch.equal(got[2], good[2])


def test_filter_refuses_keys_that_do_not_fit():
    LS = _losses()
    img, seg = torch.zeros(1, 3, 37, 53).cuda(), torch.zeros(1, 2, 37, 53).cuda()
    with pytest.raises(Exception, match="key bound"):
        LS.bilateral_filter_batch(img, seg, 15.0, 0.5 * _smallest_sigma_xy(37, 53, 15.0), bilateral="lattice")


# ------------------------------------------------------------------------------------------------ the loss
def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _gold_case(gold, i):
    t = lambda k: torch.from_numpy(gold[f"c{i}_{k}"])
    return t("img"), t("logit"), t("label"), gold[f"c{i}_box"].tolist(), gold[f"c{i}_cfg"].tolist()


@pytest.mark.parametrize("i", range(4))
def test_function_on_the_fixture_inputs(gold, i):
    """DenseEnergyLossFunction(..., "lattice") on the Function's inputs of fixture case i (as f32): Gate bit-equal to the f32
    definition, A per element within the filter's bound, loss and gradient within eps of the restatement on the same inputs."""
    LS = _losses()
    img, logit, label, box, (weight, srgb, sxy, s) = _gold_case(gold, i)
    r0 = E.energy_loss(img, logit, label, box, weight, srgb, sxy, s)
    im, P, roi, unl = r0["images"].float(), r0["segs"].float(), r0["rois"].float(), r0["unlabel"]
    Pd = P.cuda().requires_grad_(True)
    loss = LS.DenseEnergyLossFunction.apply(im.cuda(), Pd, srgb, sxy * s, roi.cuda(), unl.cuda(), "lattice")
    assert loss.is_cuda and tuple(loss.shape) == (1,) and loss.dtype == torch.float32
    (3.0 * loss).sum().backward()
    loss2, A, gate = LS.dense_energy_forward(im.cuda(), P.cuda(), srgb, sxy * s, roi.cuda(), unl.cuda(), "lattice")
    r = LE.energy_function(im, P, srgb, sxy * s, roi, unl)
    assert torch.equal(gate.cpu(), E.gate(P, roi, unl))
    assert torch.equal(loss.detach(), loss2)                                   # two calls: the same bits
    _, scale = LE.lattice_filter_batch(im, r["S"], srgb, sxy * s, want_abs=True)
    ratio = ((A.cpu().double() - r["A"]).abs() / (EPS * r["gate"][:, None] * scale + ABS)).max().item()
    e_loss, e_grad = _rel(loss.detach().cpu(), r["loss"]), _rel(Pd.grad.cpu(), 3.0 * r["grad"])
    exact = LS.DenseEnergyLossFunction.apply(im.cuda(), P.cuda(), srgb, sxy * s, roi.cuda(), unl.cuda())
    print(f"case {i}: A worst ratio {ratio:.3e}, loss rel {e_loss:.3e}, gradient / largest {e_grad:.3e}; "
          f"lattice loss / exact loss = {(loss / exact).item():.3f}")
    assert r["loss"].item() < 0 and ratio <= 1.0 and e_loss <= EPS and e_grad <= EPS
    assert not torch.equal(loss.detach(), exact)


@pytest.mark.parametrize("i", range(4))
def test_fused_term_on_the_fixture_inputs(gold, i):
    LS = _losses()
    img, logit, label, box, (weight, srgb, sxy, s) = _gold_case(gold, i)
    lg = logit.cuda().requires_grad_(True)
    loss = LS.get_energy_loss_fused(img.cuda(), lg, label.cuda(), box, LS.DenseEnergyLoss(weight, srgb, sxy, s, bilateral="lattice"))
    assert loss.is_cuda and tuple(loss.shape) == (1,)
    loss.backward()
    r64 = LE.energy_term(img, logit, label, box, weight, srgb, sxy, s)
    e_loss, e_grad = _rel(loss.detach().cpu(), r64["loss"]), _rel(lg.grad.cpu(), r64["grad"])
    print(f"case {i}: vs the lattice restatement: loss rel {e_loss:.3e}, logit gradient / largest {e_grad:.3e}")
    assert r64["loss"].item() < 0 and e_loss <= EPS and e_grad <= EPS


@pytest.mark.parametrize("e", [0, 1])
@pytest.mark.parametrize("hw,HW", [((2, 3), (26, 22)), ((3, 4), (40, 36))])
def test_end_to_end_with_real_upsampling(hw, HW, e):
    """The cases of tests/test_energy_term_gpu.py, through the fused term and through the stock layer around the Function."""
    LS = _losses()
    N, K, s = 2, 21, 2.0 ** -e
    img, seg, lab, _ = R.make_case(hw, HW, K, N, seed=2 + e)
    box = R.boxes("border", N, *HW)
    layer = LS.DenseEnergyLoss(*CFG, s, bilateral="lattice")
    sg = seg.cuda().requires_grad_(True)
    loss = LS.get_energy_loss_fused(img.cuda(), sg, lab.cuda(), TG._dev_box(box), layer)
    loss.backward()
    r64 = LE.energy_term(img, seg, lab, box, *CFG, s)
    st = seg.cuda().requires_grad_(True)
    stock = LS.get_energy_loss(img.cuda(), R.upsample(st, HW), lab.cuda(), box, layer)       # DenseEnergyLoss.forward -> the Function
    stock.backward()
    e_loss, e_grad = _rel(loss.detach().cpu(), r64["loss"]), _rel(sg.grad.cpu(), r64["grad"])
    s_loss, s_grad = _rel(stock.detach().cpu(), r64["loss"]), _rel(st.grad.cpu(), r64["grad"])
    print(f"{hw}->{HW} e={e}: vs the lattice restatement: fused loss {e_loss:.3e}, gradient {e_grad:.3e}; stock layer {s_loss:.3e}, {s_grad:.3e}")
    assert r64["loss"].item() != 0 and r64["grad"].abs().max().item() > 0
    assert e_loss <= EPS and e_grad <= EPS and s_loss <= EPS and s_grad <= EPS


def test_run_to_run_no_sync_and_opcheck():
    import weclip_vit_comer_amd
    LS = _losses()
    weclip_vit_comer_amd.register_torch_ops()
    (hw, HW), K, N = R.SHAPES[1], 33, 3
    img, seg, lab, _ = R.make_case(hw, HW, K, N, seed=2)
    img, seg, lab = img.cuda(), seg.cuda(), lab.cuda()
    box = TG._dev_box(R.boxes("border", N, *HW), torch.int16)
    layer = LS.DenseEnergyLoss(*CFG, 0.5, bilateral="lattice")
    w = torch.tensor([0.37], device="cuda")

    def run(fn):
        p = seg.clone().requires_grad_(True)
        loss = fn(p)
        (loss * w).sum().backward()
        return loss.detach(), p.grad

    fused = lambda p: LS.get_energy_loss_fused(img, p, lab, box, layer)
    op = lambda p: torch.ops.weclip.energy_term_lattice(img, p, lab, box, 1e-7, 15.0, 100.0, 0.5, list(R.MEAN), list(R.STD))[0]
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
    torch.library.opcheck(torch.ops.weclip.energy_term_lattice, (img, seg.clone().requires_grad_(True), lab, box.int(), 1e-7, 15.0, 100.0,
                                                                0.5, list(R.MEAN), list(R.STD)))
    im, P = TE._images(2, 13, 11, "mixed", 3).cuda(), TE._probs(2, 5, 13, 11, 4).cuda()
    roi, unl = (torch.rand(2, 13, 11) > 0.3).float().cuda(), (torch.rand(2, 13, 11) > 0.8).cuda()
    la, A = torch.ops.weclip.dense_energy_lattice(im, P, roi, unl, 15.0, 50.0)
    lb, Ab, _ = LS.dense_energy_forward(im, P, 15.0, 50.0, roi, unl, "lattice")
    assert torch.equal(la, lb) and torch.equal(A, Ab)
    torch.library.opcheck(torch.ops.weclip.dense_energy_lattice, (im, P.clone().requires_grad_(True), roi, unl, 15.0, 50.0))


# ------------------------------------------------------------------------------------------------ capture
def _content(kind, seed, N, HW, hw, K):
    """One batch for the captured term: a normalised image of the kind (its lattice has its own M), logits, labels, a box."""
    H, W = HW
    g = torch.Generator().manual_seed(seed)
    raw = {"noise": TE._noise, "ramp": _ramp, "constant": _constant}
    img = torch.stack([raw[kind](H, W, seed + n) for n in range(N)])
    img = (img - torch.tensor(R.MEAN)[None, :, None, None]) / torch.tensor(R.STD)[None, :, None, None]
    seg = 3 * torch.randn(N, K, *hw, generator=g)
    lab = torch.randint(0, K, (N, H, W), generator=g)
    lab[:, seed % 5:seed % 5 + 6, 2:9] = 255
    box = torch.tensor([[seed % 4, H - seed % 3, n, W - 1 - seed % 5] for n in range(N)], dtype=torch.int32)
    return img, seg, lab, box


def test_captured_term_replays_on_other_contents():
    """The test that matters most: the lattice term captured once on static buffers, replayed on image / seg / box contents whose
    vertex counts differ, gives the bits of an eager call on the same contents.  M never crossed to the host."""
    LS = _losses()
    N, K, hw, HW, e = 2, 21, (5, 6), (40, 36), 1
    args = (1e-3, 15.0, 100.0, 0.5, list(R.MEAN), list(R.STD))
    cache = {}
    contents = [_content(kind, seed, N, HW, hw, K) for kind, seed in (("noise", 1), ("ramp", 2), ("constant", 3), ("noise", 4))]
    st = [t.cuda() for t in contents[0]]
    st[2] = st[2].long()

    def term(img, seg, lab, box, cache):
        return LS.energy_term(img, seg, lab, box, *args, bilateral="lattice", workspace_cache=cache)

    term(*st, cache)                                     # warms every lazy initialisation; allocates the workspace once
    assert len(cache) == 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = term(*st, cache)
    assert len(cache) == 1                               # the capture reused it
    lat = next(iter(cache.values()))[0]
    Ms = []
    for c in contents[1:] + contents[:1]:
        for buf, t in zip(st, c):
            buf.copy_(t)
        g.replay()
        flag, M = LS.lattice_vertex_counts(lat, N)
        Ms.append(tuple(M.tolist()))
        loss, grad = out[0].clone(), out[1].clone()
        eager = term(*[t.cuda() for t in c[:2]], c[2].cuda().long(), c[3].cuda(), None)
        print(f"replay: M = {Ms[-1]}, loss {loss.item():.6e}")
        assert flag.item() == 0 and torch.equal(loss, eager[0]) and torch.equal(grad, eager[1])
        assert loss.item() != 0 and grad.abs().max().item() > 0
    assert len(set(Ms)) == len(Ms) and len(Ms) >= 3, Ms  # the vertex counts really differed between replays


LAT = dict(TG.REG, bilateral="lattice")


def test_step_graph_replay_equals_eager_with_the_lattice_term():
    eager, graph = TG._run(False, LAT), TG._run(True, LAT)
    step = graph[3]
    assert len(step._graphs) == 1 and next(iter(step._graphs.values()))["graph"] is not None
    TG._same(eager, graph)                               # losses, gradient bucket, parameters: five batches
    assert all(len(l) == 4 and l[3] != 0 for l in eager[0]) and len({l[3] for l in eager[0]}) == len(TG.BATCHES)
    assert len(step.reg.layer.workspace_cache) == 1      # allocated once per signature, not per step
    exact = TG._run(False, TG.REG)
    assert [l[3] for l in exact[0]] != [l[3] for l in eager[0]] and not torch.equal(exact[2], eager[2])
    # "exact" spelled out and no key at all are the step as it was, eager and replayed
    TG._same(TG._run(False, dict(TG.REG, bilateral="exact")), exact)
    TG._same(TG._run(True, dict(TG.REG, bilateral="exact")), exact)


def test_supervised_step_graph_replay_equals_eager_with_the_lattice_term():
    eager, graph = TG._run_supervised(False, LAT), TG._run_supervised(True, LAT)
    assert len(graph[3]._graphs) == 1 and next(iter(graph[3]._graphs.values()))["graph"] is not None
    TG._same(eager, graph)
    assert all(len(l) == 2 and l[1] != 0 for l in eager[0])
    exact = TG._run_supervised(False, TG.REG)
    assert [l[1] for l in exact[0]] != [l[1] for l in eager[0]] and not torch.equal(exact[2], eager[2])
    TG._same(TG._run_supervised(True, dict(TG.REG, bilateral="exact")), exact)


def test_train_driver_with_the_lattice_term(tmp_path, caplog):
    import logging
    keys = ["iter", "lr", "seg_loss", "attn_loss", "pseudo_seg_mAcc", "reg_loss"]
    with caplog.at_level(logging.INFO, logger="weclip.train"):
        recs, lines, syncs, tr = TG._driver(tmp_path / "lat", "--reg_loss", "--reg_start", "0", "--reg_bilateral", "lattice")
    assert tr.step.reg.bilateral == "lattice" and tr.step.reg.step_num == 6 and not syncs, syncs
    assert [list(r) for r in lines] == [keys] * 2 and lines == recs
    assert all(np.isfinite(r["reg_loss"]) and r["reg_loss"] != 0 for r in recs)
    assert sum(", reg_loss: " in r.getMessage() for r in caplog.records) == 2
