"""The multi-job weight-gradient launch (wc_gemm_km_f16_multi, csrc/gemm_km.hip gemm_km_multi_kernel) against the same jobs
launched one at a time (wc_gemm_km_f16_grouped through ops.wgrad_partials: same slice plan, same kernel form): partials and
reduced gradients bit-identical, every reduced gradient against fp64 at the bound of tests/test_backward_ops_gpu.py
(2e-6 of the largest entry); then both explicit backward engines with the deferred sink against `defer_wgrads = False`."""
import ctypes

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
TOL = 2e-6          # tests/test_backward_ops_gpu.py test_weight_gradient_gemm_row_major_operands


def _case(g, M, N, K, slices, *, lda=None, xmap=None, groups=1):
    """One job: operands on the CPU (fp16) + the keyword arguments of ops.wgrad_partials / GradSink.wgrad."""
    kw = dict(slices=slices)
    if groups > 1:                       # dY = column slices of one (M, groups * N + pad) matrix: lda > N
        lda = groups * N + 8
        kw.update(groups=groups, gA=N)
    if lda is not None:
        kw["lda"] = lda
    dy = torch.zeros(M, lda or N).half()
    dy[:, :groups * N] = torch.randn(M, groups * N, generator=g).half()
    if xmap is not None:                 # X = the patch rows of (groups, B, 1 + hw, K) tokens, CLS rows skipped
        hw, Lq, _ = xmap
        B = M // hw
        x = torch.randn(groups, B, Lq, K, generator=g).half()
        kw["xmap"] = xmap
        if groups > 1:
            kw["gX"] = B * Lq * K
        xd = x[:, :, 1:].reshape(groups, M, K)
    else:
        x = torch.randn(M, K, generator=g).half()
        xd = x.view(1, M, K)
    ref = [(dy[:, i * N:(i + 1) * N].double().t() @ xd[i].double(), dy[:, i * N:(i + 1) * N].double().sum(0)) for i in range(groups)]
    return dict(M=M, N=N, K=K, dy=dy.cuda(), x=x.view(-1, K).cuda(), kw=kw, groups=groups, ref=ref)


@pytest.fixture(scope="module")
def cases():
    g = torch.Generator().manual_seed(2024)
    cs = [
        _case(g, 1000, 21, 256, 4, lda=64),                  # the class head: N = 21 in 64-column rows; ragged last slice (232 of 256)
        _case(g, 2048, 256, 256, 8),                         # bias edge (K % 128 == 0); 8 units: XCD-aware order
        _case(g, 1100, 128, 320, 3),                         # K % 128 != 0: the bias column has a tile of its own; 3 units: plain order
        _case(g, 600, 64, 128, 1),                           # M smaller than one slice (640)
        _case(g, 672, 64, 192, 2, xmap=(224, 225, 1)),       # CLS-skipping row map
        _case(g, 640, 64, 192, 3, xmap=(160, 161, 1), groups=3),     # grouped, lda > N, 9 units
        _case(g, 2048, 256, 1024, 32),                       # 64-token slices, 512 workgroups: the 4-wave form
        _case(g, 2100, 130, 200, 33, lda=136),               # 64-token slices, ragged everything, 33 units
        _case(g, 1024, 21, 256, 16, lda=64),                 # 16 units of 64 tokens
    ]
    # enough small jobs to overflow one 32-job argument chunk in BOTH kernel forms (slices of 64 tokens: four waves; longer: eight)
    for i in range(34):
        cs.append(_case(g, 640 + 64 * (i % 3), 32, 64, 10 + i % 3))       # 64-token slices
        cs.append(_case(g, 600 + 8 * i, 32 + 8 * (i % 2), 64, 1 + i % 3))
    return cs


def _sink_run(cases, defer):
    from weclip_vit_comer_amd import ops
    from weclip_vit_comer_amd.grad_sink import GradSink
    outs, parts, calls = [], [], []
    real = ops.wgrad_partials

    def spy(*a, **kw):
        r = real(*a, **kw)
        parts.append(r[0])
        return r

    ops.wgrad_partials = spy
    try:
        with GradSink(defer=defer) as sink:
            for c in cases:
                G, N, K = c["groups"], c["N"], c["K"]
                sw, sb = N * K + 24, N + 8
                dw = torch.full((G * sw,), 7.0, device="cuda")
                db = torch.full((G * sb,), 7.0, device="cuda")
                kw = dict(c["kw"])
                ns = kw.pop("slices")
                sink.wgrad(c["dy"], c["x"], c["M"], N, K, 0.5, [(dw[:N * K].view(N, K), db[:N])], ns=ns, sw=sw, sb=sb, **kw)
                outs.append((dw, db, sw, sb))
            calls.append(len(sink._gemms))
    finally:
        ops.wgrad_partials = real
    torch.cuda.synchronize()
    return outs, parts, calls[0]


def test_multi_launch_equals_single_launches_and_fp64(cases):
    from weclip_vit_comer_amd import _lib as L
    single, sparts, q0 = _sink_run(cases, defer=False)
    multi, mparts, q1 = _sink_run(cases, defer=True)
    assert q0 == 0 and q1 == len(cases)          # nothing queued in immediate mode, every GEMM queued in deferred mode
    # the plan of this job list: several launches, both kernel forms, more than one chunk per form
    from weclip_vit_comer_amd import ops
    queue = []
    for c in cases:
        ops.wgrad_partials(c["dy"], c["x"], c["M"], c["N"], c["K"], bias=True, queue=queue, **c["kw"])
    n = len(queue)
    flat = (ctypes.c_int64 * (16 * n))(*[v for _, f in queue for v in f])
    launch, first, pos = ((ctypes.c_int * n)() for _ in range(3))
    grids, forms, nl = (ctypes.c_int * 8)(), (ctypes.c_int * 8)(), ctypes.c_int(0)
    L.lib().wc_gemm_km_multi_plan(flat, n, 0, launch, first, pos, grids, forms, 8, ctypes.byref(nl))
    forms = list(forms)[:nl.value]
    print(f"{n} jobs -> {nl.value} launches, forms {forms}, grids {list(grids)[:nl.value]}")
    assert forms.count(1) >= 2 and forms.count(2) >= 2
    units = [c["groups"] * (ps.shape[-3]) for c, ps in zip(cases, sparts)]
    assert any(u % 8 == 0 for u in units) and any(u % 8 for u in units)
    worst = 0.0
    for c, ps, pm, (dw0, db0, sw, sb), (dw1, db1, _, _) in zip(cases, sparts, mparts, single, multi):
        assert ps.shape == pm.shape and torch.equal(ps, pm), (c["M"], c["N"], c["K"], c["kw"])
        assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
        N, K = c["N"], c["K"]
        dw, db = dw1.cpu().double(), db1.cpu().double()
        for gi, (ref, refb) in enumerate(c["ref"]):
            ew = (dw[gi * sw:gi * sw + N * K].view(N, K) - 0.5 * ref).abs().max() / (0.5 * ref).abs().max()
            eb = (db[gi * sb:gi * sb + N] - 0.5 * refb).abs().max() / (0.5 * refb).abs().max()
            worst = max(worst, ew.item(), eb.item())
            assert ew < TOL and eb < TOL, (c["M"], N, K, c["kw"], ew.item(), eb.item())
            assert (dw[gi * sw + N * K:(gi + 1) * sw] == 7.0).all() and (db[gi * sb + N:(gi + 1) * sb] == 7.0).all()     # nothing else touched
    print(f"worst error against fp64: {worst:.2e} of the largest entry")


def _head_step(defer, monkeypatch):
    from weclip_vit_comer_amd.head_engine import HeadEngine
    from weclip_vit_comer_amd.WeCLIP_model.model_attn_aff_voc import WeCLIP
    from weclip_vit_comer_amd.train_step import TrainStep
    monkeypatch.setattr(HeadEngine, "defer_wgrads", defer)
    torch.manual_seed(0)
    sd = synth.make_clip_state_dict(**synth.TINY)
    bg, fg = synth.make_text_features(20, 25, synth.TINY["embed_dim"])
    fuse, dec = synth.make_head_state_dicts(width=synth.TINY["width"])
    m = WeCLIP(num_classes=21, clip_model=sd, embedding_dim=256, in_channels=[synth.TINY["width"]] * 4, dataset_root_path=None,
               device="cuda", text_features=(bg.cuda(), fg.cuda()))
    m.decoder_fts_fuse.load_state_dict(fuse)
    m.decoder.load_state_dict(dec)
    m.train()
    step = TrainStep(m, bucket=True)
    torch.manual_seed(1)
    step(synth.make_images(3, *synth.TINY_HW, seed=11).cuda(), labels=[[1], [2, 5], [0, 3]])
    return step.bucket.flat.clone(), {id(p): n for n, p in m.named_parameters()}, step.bucket


def test_head_engine_deferred_equals_immediate(monkeypatch):
    """HeadEngine.backward at the tiny geometry of tests/test_weclip_gpu.py: the slice plan is unchanged and every job keeps its
    kernel form, so the whole gradient bucket must be bit-identical."""
    flat_d, names, bucket = _head_step(True, monkeypatch)
    flat_i, _, _ = _head_step(False, monkeypatch)
    assert flat_d.abs().max().item() > 0
    for p, o in zip(bucket.params, bucket.offsets):
        assert torch.equal(flat_d[o:o + p.numel()], flat_i[o:o + p.numel()]), names.get(id(p))
    assert torch.equal(flat_d, flat_i)


def test_comer_engine_deferred_equals_immediate(monkeypatch):
    """The insert engine at its smallest tested geometry (tests/test_comer_gpu.py, adapters inside the engine): output and
    every parameter gradient bit-identical between the deferred sink and `defer_wgrads = False`."""
    from types import SimpleNamespace
    import torch.nn as nn
    from weclip_vit_comer_amd.comer_engine import ComerEngine
    from weclip_vit_comer_amd.WeCLIP_model.comer import CoMerInteraction
    from weclip_vit_comer_amd.WeCLIP_model.segformer_head import MLP
    B, H, W, dim, Cin = 2, 64, 96, 256, 128
    h, w = H // 16, W // 16
    Lq = h * w + 1
    torch.manual_seed(0)
    net = CoMerInteraction(dim).cuda()
    ads = nn.ModuleList([MLP(Cin, dim) for _ in range(11)]).cuda()
    with torch.no_grad():
        for t in net.cti:
            t.gamma.fill_(0.4)
    g = torch.Generator().manual_seed(3)
    img = torch.randn(B, 3, H, W, generator=g).cuda()
    xs = [torch.randn(B * Lq, Cin, generator=g).half().cuda() for _ in range(11)]
    gy = torch.randn(B, dim, h, w, generator=g).cuda()
    res = {}
    for defer in (True, False):
        monkeypatch.setattr(ComerEngine, "defer_wgrads", defer)
        for p in list(net.parameters()) + list(ads.parameters()):
            p.grad = None
        y = net.forward_tokens(img, [SimpleNamespace(hi=x) for x in xs], Lq, ads, (h, w))
        y.backward(gy)
        res[defer] = (y.detach().clone(), {n: p.grad.clone() for n, p in list(ads.named_parameters()) + list(net.named_parameters())
                                           if p.grad is not None})
    assert net._engine is not None and torch.equal(res[True][0], res[False][0])
    assert set(res[True][1]) == set(res[False][1]) and len(res[True][1]) > 50
    assert any(v.abs().max().item() > 0 for v in res[True][1].values())
    for n, v in res[True][1].items():
        assert torch.equal(v, res[False][1][n]), n
