"""utils.mmdloss on the GPU (csrc/mmd.hip) against the fp64 restatement tests/mmd_ref.py.

Error model (include/weclip_hip.h wc_mmd_*), every reference computed in fp64 from the very values the kernels read:
    |loss - loss64| <= EPS * A + 2^-24           A    = (1/B^2) sum_ij K_ij
    |K - K64|       <= EPS * K64 + 2^-24         per element
    |g - g64|       <= EPS * G + 2^-24           G_ic = (4/B^2) (sum_j W_ij |x_ic| + sum_j W_ij |x_jc|)
Each check prints its worst ratio r = max (|error| - 2^-24) / scale, so EPS is met when r <= EPS.

EPS: the starting bound was 2^-10 (what tests/test_energy_gpu.py accepts for an f32-input-MFMA filter).  After the first runs
on the MI355X it was tightened to the smallest power of two at least 8 x the worst ratio seen over all cases of this file
(the margin covers input draws not tried): 2^-16, see MEASURED below.  fp16 gradients are rounded once to fp16 (2^-11 of |g| <= G), so
they keep EPS16 = 2^-10, which the number format sets, whatever EPS is.
"""
import warnings

import numpy as np
import pytest
import torch

import mmd_ref

pytestmark = pytest.mark.gpu

# MEASURED on the MI355X (worst ratio over every case of this file, per quantity), and the bound chosen from it:
#   loss 5.2e-8 (normal, B = 2, d = 7); gradient, fp32 inputs, 1.1e-7 (golden B2_d3); K 1.9e-6 (target == source, B = 130, d = 768,
#   fixed bandwidth); gradient, fp16 inputs, 2.0e-4 (B = 33, d = 40: the fp16 rounding of the result).
#   8 x 1.895e-6 = 1.516e-5 <= 2^-16 = 1.526e-5, the smallest such power of two: EPS = 2^-16.
#   (With the rows centred on one common mean, the first design, the "far" inputs measured K 2.8e-4 at d = 768; centring each
#   block on its own mean brought them to 2.8e-7, and the bound was chosen only after that.)
EPS = 2.0 ** -16
EPS16 = 2.0 ** -10
FLOOR = 2.0 ** -24

BS = [1, 2, 5, 16, 33, 64, 65, 130]
DS = [1, 2, 3, 7, 64, 129, 768]          # 129 is also the gradient chunk width (128) + 1


def _mod():
    import weclip_vit_comer_amd
    weclip_vit_comer_amd.register_torch_ops()
    from weclip_vit_comer_amd.utils import mmdloss
    return mmdloss


def _inputs(kind, B, d, seed=0):
    """(source, target) contiguous CPU tensors of the kind's dtype ("noncontig": the "normal" values; _check strides them)."""
    g = torch.Generator().manual_seed(7919 * B + 31 * d + seed)
    src = torch.randn(B, d, generator=g)
    tgt = 1.3 * torch.randn(B, d, generator=g) + 0.5            # scaled and shifted against the source
    if kind == "shift100":
        src, tgt = src + 100.0, tgt + 100.0                     # pins the centring
    elif kind == "same":
        tgt = src.clone()
    elif kind == "far":
        tgt = torch.randn(B, d, generator=g) + 30.0             # cross blocks underflow with a bandwidth of the blocks' own size
    elif kind == "fp16":
        src, tgt = src.half(), tgt.half()
    return src, tgt


def _within_block_sigma(src, d):
    """A fixed bandwidth near the mean squared distance inside a block, so that off-diagonal entries carry weight."""
    return round(1.6 * d * float(src.float().var().item() if src.numel() > 1 else 1.0) + 0.5, 3)


def _ratio(got, want, scale):
    err = (got.double().cpu() - want.cpu()).abs() - FLOOR
    scale = scale.cpu()
    r = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return max(r.max().item(), 0.0)


def _check(kind, B, d, kernel_mul=2.0, kernel_num=5, fix_sigma=None, matrix=None, seed=0, tag=""):
    M = _mod()
    src, tgt = _inputs(kind, B, d, seed)
    ref = mmd_ref.mmd(src, tgt, kernel_mul, kernel_num, fix_sigma, want_K=2 * B <= 260)
    s, t = src.cuda().requires_grad_(True), tgt.cuda().requires_grad_(True)
    if kind == "noncontig":                                      # the same values behind strided views
        s = torch.zeros(B, 2 * d + 1, device="cuda")[:, 1::2].copy_(src).requires_grad_(True)
        t = torch.zeros(2 * B, d, device="cuda")[::2].copy_(tgt).requires_grad_(True)
        assert (not s.is_contiguous() or d == 1) and (not t.is_contiguous() or B == 1)
    loss = M.mmd_rbf(s, t, kernel_mul, kernel_num, fix_sigma)
    assert loss.shape == () and loss.dtype == torch.float32
    gs, gt = torch.autograd.grad(loss, (s, t))
    assert gs.dtype == src.dtype and gt.dtype == src.dtype and gs.shape == src.shape
    with torch.no_grad():
        loss_ng = M.mmd_rbf(s, t, kernel_mul, kernel_num, fix_sigma)     # the loss-only kernel (upper triangle of tiles)
    r_loss = max(_ratio(loss, ref["loss"], ref["A"]), _ratio(loss_ng, ref["loss"], ref["A"]))
    r_grad = max(_ratio(gs, ref["grad_source"], ref["G_source"]), _ratio(gt, ref["grad_target"], ref["G_target"]))
    r_K = 0.0
    if ref["K"] is not None and matrix is not False:
        K = M.rbf_kernel(s.detach(), t.detach(), kernel_mul, kernel_num, fix_sigma)
        assert K.dtype == torch.float32 and tuple(K.shape) == (2 * B, 2 * B)
        assert torch.equal(K, K.T)                                       # symmetric bit for bit
        assert torch.equal(K.diagonal(), torch.full((2 * B,), float(kernel_num), device="cuda"))
        r_K = _ratio(K, ref["K"], ref["K"])
    eg = EPS16 if src.dtype == torch.float16 else EPS
    print(f"MMD-RATIO {tag or kind} B={B} d={d} mul={kernel_mul} num={kernel_num} fix={fix_sigma}: loss {r_loss:.3e} grad {r_grad:.3e} "
          f"K {r_K:.3e} (eps {EPS:.3e})")
    assert np.isfinite(loss.item())
    assert r_loss <= EPS, (r_loss, loss.item(), ref["loss"].item(), ref["A"].item())
    assert r_grad <= eg, r_grad
    assert r_K <= EPS, r_K
    return ref, loss


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("B", BS)
def test_shapes(B, d):
    _check("normal", B, d)


@pytest.mark.parametrize("B,d", [(5, 7), (33, 40), (65, 129), (130, 768)])
@pytest.mark.parametrize("kind", ["normal", "shift100", "same", "far", "fp16", "noncontig"])
def test_input_kinds(kind, B, d):
    src, _ = _inputs(kind, B, d)
    for fix in (None, _within_block_sigma(src, d)):
        if kind == "far" and fix is None:
            continue      # a bandwidth taken from the data grows with the distance: nothing underflows, the "normal" kind again
        ref, loss = _check(kind, B, d, fix_sigma=fix)
        if kind == "same":
            assert abs(loss.item()) <= EPS * ref["A"].item() + FLOOR and abs(ref["loss"].item()) < 1e-12
        if kind == "far":                        # the cross blocks are gone: the loss is the two diagonal blocks' mean
            K = mmd_ref.mmd(*_inputs(kind, B, d), 2.0, 5, fix, want_K=True, want_grad=False)["K"]
            assert K[:B, B:].max().item() < 1e-30
            diag_mean = (K[:B, :B].sum() + K[B:, B:].sum()).item() / (B * B)
            assert abs(ref["loss"].item() - diag_mean) < 1e-12
            assert abs(loss.item() - diag_mean) <= EPS * ref["A"].item() + FLOOR


@pytest.mark.parametrize("B,d", [(33, 40), (65, 129)])
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("kernel_mul", [2.0, 1.5])
@pytest.mark.parametrize("kernel_num", [1, 3, 5])
def test_parameters(kernel_num, kernel_mul, fixed, B, d):
    src, _ = _inputs("normal", B, d)
    _check("normal", B, d, kernel_mul, kernel_num, _within_block_sigma(src, d) if fixed else None, tag="params")


def test_golden_cases_through_the_device(golden):
    """The reference's own fp64 run (tests/golden/mmd_rbf.npz).  The device reads the fp32 rounding of the recorded inputs, which
    moves the fp64 result by at most sum_ic |g_ic| |x_ic| 2^-24 <= sum_ic G_ic |x_ic| 2^-24 to first order; K and the gradient
    are therefore compared through tests/mmd_ref.py on the rounded inputs (test_mmd_ref_cpu.py ties that to the golden)."""
    M = _mod()
    gold = golden("mmd_rbf.npz")
    for name in [str(n) for n in gold["names"]]:
        src, tgt = torch.from_numpy(gold[f"{name}_source"]), torch.from_numpy(gold[f"{name}_target"])
        fix = float(gold[f"{name}_fix"]) or None
        s, t = src.float().cuda().requires_grad_(True), tgt.float().cuda().requires_grad_(True)
        loss = M.mmd_rbf(s, t, fix_sigma=fix)
        gs, gt = torch.autograd.grad(loss, (s, t))
        ref = mmd_ref.mmd(src.float(), tgt.float(), 2.0, 5, fix, want_K=True)
        moved = ((ref["G_source"] * src.abs()).sum() + (ref["G_target"] * tgt.abs()).sum()).item() * FLOOR
        err = abs(loss.item() - float(gold[f"{name}_loss"]))
        r = [_ratio(loss, ref["loss"], ref["A"]), _ratio(gs, ref["grad_source"], ref["G_source"]), _ratio(gt, ref["grad_target"], ref["G_target"]),
             _ratio(M.rbf_kernel(s.detach(), t.detach(), fix_sigma=fix), ref["K"], ref["K"])]
        print(f"MMD-RATIO golden {name}: loss {r[0]:.3e} grad {max(r[1:3]):.3e} K {r[3]:.3e}; |loss - golden| {err:.3e} (allowed "
              f"{EPS * ref['A'].item() + FLOOR + moved:.3e})")
        assert max(r) <= EPS, (name, r)
        assert err <= EPS * ref["A"].item() + FLOOR + moved, (name, err)


def test_autograd_upstream_gradient_and_single_input():
    M = _mod()
    src, tgt = _inputs("normal", 33, 40)
    ref = mmd_ref.mmd(src, tgt)
    s, t = src.cuda().requires_grad_(True), tgt.cuda().requires_grad_(True)
    (M.mmd_rbf(s, t) * -2.5).backward()
    assert _ratio(s.grad / -2.5, ref["grad_source"], ref["G_source"]) <= EPS + 2.0 ** -23     # (+ the rounding of the scaling)
    assert _ratio(t.grad / -2.5, ref["grad_target"], ref["G_target"]) <= EPS + 2.0 ** -23
    s1, t1 = src.cuda().requires_grad_(True), tgt.cuda()
    M.mmd_rbf(s1, t1).backward()
    assert t1.grad is None and _ratio(s1.grad, ref["grad_source"], ref["G_source"]) <= EPS
    s2, t2 = src.cuda(), tgt.cuda().requires_grad_(True)
    M.mmd_rbf(s2, t2).backward()
    assert s2.grad is None and _ratio(t2.grad, ref["grad_target"], ref["G_target"]) <= EPS
    assert not M.mmd_rbf(src.cuda(), tgt.cuda()).requires_grad


def test_run_to_run_no_sync_and_opcheck():
    M = _mod()
    src, tgt = _inputs("normal", 65, 129)

    sd, td = src.cuda(), tgt.cuda()                                      # (a pageable host-to-device copy synchronises)

    def run():
        s, t = sd.clone().requires_grad_(True), td.clone().requires_grad_(True)
        loss = M.mmd_rbf(s, t)
        return (loss.detach(),) + torch.autograd.grad(loss, (s, t)) + (M.rbf_kernel(s.detach(), t.detach()),)
    a = run()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            b = run()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert not [str(c.message) for c in caught if "called a synchronizing" in str(c.message)], [str(c.message) for c in caught]
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                         # bit-identical from run to run
    s, t = _inputs("normal", 5, 7)
    torch.library.opcheck(torch.ops.weclip.mmd_rbf, (s.cuda().requires_grad_(True), t.cuda().requires_grad_(True), 2.0, 5, 0.0, True))
    torch.library.opcheck(torch.ops.weclip.mmd_rbf, (s.cuda(), t.cuda(), 1.5, 3, 7.0, False))
    torch.library.opcheck(torch.ops.weclip.rbf_kernel, (s.cuda(), t.cuda(), 2.0, 5, 0.0))


def test_graph_capture_replays_on_new_contents():
    M = _mod()
    src, tgt = _inputs("normal", 65, 129)
    s, t = src.cuda().requires_grad_(True), tgt.cuda().requires_grad_(True)

    def step():
        loss = M.mmd_rbf(s, t, 1.5, 3)
        return (loss,) + torch.autograd.grad(loss, (s, t))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                           # warms lazy initialisation and the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    src2, tgt2 = _inputs("normal", 65, 129, seed=11)
    with torch.no_grad():
        s.copy_(src2.cuda())
        t.copy_(0.5 * tgt2.cuda())
    g.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in out]
    eager = step()
    for x, y in zip(replayed, eager):
        assert torch.equal(x, y)
    ref = mmd_ref.mmd(src2, 0.5 * tgt2, 1.5, 3)
    assert _ratio(replayed[0], ref["loss"], ref["A"]) <= EPS and _ratio(replayed[1], ref["grad_source"], ref["G_source"]) <= EPS


def test_many_workgroups_against_the_host_restatement():
    M = _mod()
    B, d = 1024, 256
    src, tgt = _inputs("normal", B, d)
    ref = mmd_ref.mmd(src, tgt, chunk=256)
    s, t = src.cuda().requires_grad_(True), tgt.cuda().requires_grad_(True)
    loss = M.mmd_rbf(s, t)
    gs, gt = torch.autograd.grad(loss, (s, t))
    with torch.no_grad():
        loss_ng = M.mmd_rbf(s, t)
    r = [_ratio(loss, ref["loss"], ref["A"]), _ratio(loss_ng, ref["loss"], ref["A"]), _ratio(gs, ref["grad_source"], ref["G_source"]),
         _ratio(gt, ref["grad_target"], ref["G_target"])]
    print(f"MMD-RATIO many-workgroups B={B} d={d}: loss {max(r[:2]):.3e} grad {max(r[2:]):.3e}")
    assert max(r) <= EPS, r


def test_memory_stays_linear_in_the_rows():
    """B = 4096, d = 256: the (N, N) fp32 matrix alone would be 256 MiB; loss + gradient must stay below 64 MiB over the inputs."""
    M = _mod()
    B, d = 4096, 256
    src, tgt = _inputs("normal", B, d)
    s, t = src.cuda().requires_grad_(True), tgt.cuda().requires_grad_(True)
    from weclip_vit_comer_amd import ops
    ops._mmd_ws.pop((2 * B, d, str(s.device)), None)                     # the workspace counts
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = M.mmd_rbf(s, t)
    gs, gt = torch.autograd.grad(loss, (s, t))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ref = mmd_ref.mmd(s, t, chunk=1024, device="cuda")                   # fp64 stock ops on the device, 1024 rows at a time
    r = [_ratio(loss, ref["loss"], ref["A"]), _ratio(gs, ref["grad_source"], ref["G_source"]), _ratio(gt, ref["grad_target"], ref["G_target"])]
    print(f"MMD-RATIO memory B={B} d={d}: loss {r[0]:.3e} grad {max(r[1:]):.3e}; peak over the inputs {peak / 2**20:.1f} MiB")
    assert peak < 64 * 2 ** 20, peak
    assert max(r) <= EPS, r


def test_width_limit_is_refused():
    M = _mod()
    x = torch.zeros(2, 8193, device="cuda")
    with pytest.raises(ValueError, match="bad argument"):
        M.mmd_rbf(x, x)
    from weclip_vit_comer_amd import _lib
    with pytest.raises(RuntimeError, match="bad argument"):
        _lib.lib().wc_mmd_rbf(_lib.ptr(x), _lib.ptr(x), 0, _lib.ptr(x), None, _lib.ptr(x), 2, 8193, 5, 2.0, 0.0, _lib.stream())
    y = torch.randn(2, 8192, device="cuda")
    assert np.isfinite(M.mmd_rbf(y, y + 1.0).item())
