"""CPU tests of grad_sink (no GPU): the split-K slice counts of every weight-gradient call site, the packed
wc_sum_slices_wb_multi job array and the destination policy.  The library and the partials GEMM are recording fakes;
the tensors are CPU tensors (only their addresses matter here)."""
import struct
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from weclip_vit_comer_amd import _lib, ops
from weclip_vit_comer_amd.grad_sink import GradSink, handback, slices

INV = 1.0 / 4096.0
ABITS = struct.unpack("<I", struct.pack("<f", INV))[0]


def _old_loop(M, tiles, budget):
    """The slice-count loop as each call site had it inline."""
    ns = 1
    while ns * 2 * tiles <= budget and M // (ns * 2) >= 256:
        ns *= 2
    return ns


def _ns_of(M, requested):
    """The slice count ops.wgrad_partials returns for `requested` slices (64-row aligned slices)."""
    mslice = (-(-M // requested) + 63) // 64 * 64
    return -(-M // mslice)


@pytest.fixture
def fakes(monkeypatch):
    """Recording stand-ins for the library and the partials GEMM: -> (partials calls, reduction launches)."""
    partials, launches = [], []

    def wgrad_partials(dy16, x16, M, N, K, *, slices=1, bias=True, groups=1, **kw):
        partials.append(dict(M=M, N=N, K=K, slices=slices, bias=bias, groups=groups, **kw))
        ns = _ns_of(M, slices)
        return torch.empty(groups * ns * N * (K + bias)), ns

    class Lib:
        def wc_sum_slices_wb_multi(self, arr, count, stream):
            launches.append((count, list(arr)))

        def __getattr__(self, name):       # any other entry point: a no-op
            return lambda *a: None

    monkeypatch.setattr(ops, "wgrad_partials", wgrad_partials)
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    monkeypatch.setattr(_lib, "stream", lambda: None)
    return partials, launches


# (M, N, K, budget) of the bench step's weight gradients (batch 16 at 512x512: 32x32 patch grid, 64x64 / 32x32 / 16x16 pyramid)
HEAD = [(16384, n, k, 512) for n, k in [(21, 256), (256, 2816), (256, 256), (256, 768), (256, 1024), (1024, 256), (768, 256)]]
INSERTS = [(m, n, k, 256) for m, n, k in [(16384, 256, 2048), (86016, 256, 256), (86016, 96, 256), (16384, 256, 256),
                                          (16384, 288, 256), (16384, 256, 768), (86016, 256, 128), (86016, 128, 256)]]
TORCH_OPS = [(m, n, k, 512) for m, n, k in [(16384, 256, 768), (16384, 256, 256), (512, 21, 256), (300, 64, 64)]]


@pytest.mark.parametrize("M,N,K,budget", HEAD + INSERTS + TORCH_OPS)
def test_slices_match_the_inline_loops(M, N, K, budget):
    tiles = ops.wgrad_tiles(N, K)
    ns = slices(M, tiles, budget)
    assert ns == _old_loop(M, tiles, budget)
    assert ns & (ns - 1) == 0 and ns * tiles <= max(budget, tiles) and (ns == 1 or M // ns >= 256)


def test_head_grouped_adapters_keep_their_slice_formula(fakes):
    """The grouped adapter weight gradients use max(1, min(512 // tiles, M // 256)), not the power-of-two loop, and write
    group g at the bucket stride between consecutive adapters."""
    from weclip_vit_comer_amd.head_engine import HeadEngine
    from weclip_vit_comer_amd.train_step import GradBucket
    partials, launches = fakes
    n, E, C, B, h, w = 11, 256, 768, 16, 32, 32
    M, Lq = B * h * w, h * w + 1
    torch.manual_seed(0)
    mods = [SimpleNamespace(proj=nn.Linear(C, E), proj_2=nn.Linear(E, E)) for _ in range(n)]
    bucket = GradBucket([q for m in mods for q in (m.proj.weight, m.proj.bias, m.proj_2.weight, m.proj_2.bias)])
    eng = HeadEngine.__new__(HeadEngine)
    eng.index, eng.E, eng.fuse = n, E, SimpleNamespace(linears_modulelist=mods)
    lo = bucket.flat.data_ptr()
    sink = GradSink((lo, lo + 4 * bucket.flat.numel()))
    op = torch.empty(8, dtype=torch.float16)  # operands only travel to the (fake) GEMM
    ctx = dict(h=h, w=w, t1b=SimpleNamespace(hi=op))
    xs = SimpleNamespace(big=op[:1].expand(n, B * Lq, C))
    assert eng._adapter_wgrads_grouped(ctx, SimpleNamespace(hi=op), op, xs, B, Lq, C, M, INV, sink)
    sink.flush()
    assert [(c["N"], c["K"], c["groups"]) for c in partials] == [(E, E, n), (E, C, n)]
    for c in partials:
        assert c["slices"] == max(1, min(512 // (ops.wgrad_tiles(c["N"], c["K"]) * n), M // 256))
    (count, arr), = launches
    assert count == 2 * n
    jobs = [arr[8 * j:8 * j + 8] for j in range(count)]
    stride = [(mods[1].proj_2.weight.grad.data_ptr() - mods[0].proj_2.weight.grad.data_ptr()),
              (mods[1].proj_2.bias.grad.data_ptr() - mods[0].proj_2.bias.grad.data_ptr())]
    for g, j in enumerate(jobs[:n]):           # proj_2 first
        ns = _ns_of(M, partials[0]["slices"])
        assert j[1] == mods[g].proj_2.weight.grad.data_ptr() == mods[0].proj_2.weight.grad.data_ptr() + g * stride[0]
        assert j[2] == mods[g].proj_2.bias.grad.data_ptr() == mods[0].proj_2.bias.grad.data_ptr() + g * stride[1]
        assert j[3:] == [ns, E, E, ABITS, E * (E + 1)]
        assert j[0] - jobs[0][0] == 4 * g * ns * E * (E + 1)
    assert all(j[1] == mods[g].proj.weight.grad.data_ptr() for g, j in enumerate(jobs[n:]))
    g = handback([q for m in mods for q in (m.proj.weight, m.proj_2.bias)], sink.grads)
    assert g == (None,) * (2 * n)             # all written into the bucket


def _conv_stem_slices(monkeypatch, fakes, N, H, W, C, O, stride):
    """Slice count _Conv3x3Fn.backward requests for the weight gradient of one stem layer."""
    from weclip_vit_comer_amd import hip_functional as HF
    partials, _ = fakes
    monkeypatch.setattr(ops, "colscale_split", lambda *a, **k: (None, ops.Split(torch.empty(8, dtype=torch.float16), None)))
    monkeypatch.setattr(_lib, "ptr", lambda *a, **k: None)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M, Kp = N * Ho * Wo, (9 * C + 63) // 64 * 64
    ctx = SimpleNamespace(saved_tensors=(torch.empty(8, dtype=torch.float16), torch.empty(O, Kp)),
                          meta=(N, H, W, C, O, stride, Kp, M, False, (O, C, 3, 3)), needs_input_grad=(False, True))
    partials.clear()
    HF._Conv3x3Fn.backward(ctx, torch.empty(M, O))
    (c,) = partials
    assert (c["M"], c["N"], c["K"], c["bias"]) == (M, O, Kp, False)
    return M, Kp, c["slices"]


@pytest.mark.parametrize("C,O,H", [(3, 32, 512), (32, 32, 256), (32, 64, 128), (64, 128, 64), (128, 128, 32)])
def test_conv_stem_keeps_its_tile_count(monkeypatch, fakes, C, O, H):
    """The stem counts ((O+127)//128) * ((Kp+1+127)//128) tiles although it has no bias column (not ops.wgrad_tiles(O, Kp,
    bias=False) when Kp % 128 == 0): kept, a different slice count would change the fp32 summation order."""
    M, Kp, ns = _conv_stem_slices(monkeypatch, fakes, 16, H, H, C, O, 2)
    assert ns == _old_loop(M, ((O + 127) // 128) * ((Kp + 1 + 127) // 128), 512)


def test_job_array_row_ranges_and_single(fakes):
    """Two Linears stacked along N (the insert engine's sampling_offsets | attention_weights) reduce row ranges of one
    partial matrix; the slice stride is the whole matrix's."""
    partials, launches = fakes
    M, K, rows = 16384, 256, (192, 96)
    N = sum(rows)
    outs = [(torch.empty(r, K), torch.empty(r)) for r in rows]
    single = (torch.empty(21, 256), torch.empty(21))
    with GradSink() as sink:
        sink.wgrad(None, None, M, N, K, INV, outs, ns=8, lda=320)
        sink.wgrad(None, None, M, 21, 256, 0.5, [single], ns=4)
        assert not launches                   # queued until the context exits
    (count, arr), = launches
    assert count == 3 and len(arr) == 24
    j0, j1, j2 = arr[:8], arr[8:16], arr[16:]
    assert partials[0]["lda"] == 320 and partials[0]["slices"] == 8
    assert j1[0] - j0[0] == 4 * rows[0] * (K + 1)
    assert j0[1:] == [outs[0][0].data_ptr(), outs[0][1].data_ptr(), 8, rows[0], K, ABITS, N * (K + 1)]
    assert j1[1:] == [outs[1][0].data_ptr(), outs[1][1].data_ptr(), 8, rows[1], K, ABITS, N * (K + 1)]
    assert j2[1:] == [single[0].data_ptr(), single[1].data_ptr(), 4, 21, 256, 0x3F000000, 21 * 257]
    with pytest.raises(ValueError):           # destinations must cover the N rows exactly
        GradSink().wgrad(None, None, M, N + 1, K, INV, outs, ns=8)


def test_job_array_groups(fakes):
    _, launches = fakes
    M, N, K, G, sw, sb = 4096, 64, 128, 3, 9000, 100
    dw, db = torch.empty(G * sw), torch.empty(G * sb)
    with GradSink() as sink:
        sink.wgrad(None, None, M, N, K, INV, [(dw[:N * K], db[:N])], ns=4, groups=G, sw=sw, sb=sb, gA=64, gX=128)
    (count, arr), = launches
    ns = _ns_of(M, 4)
    jobs = [arr[8 * g:8 * g + 8] for g in range(count)]
    assert count == G
    for g, j in enumerate(jobs):
        assert j[0] - jobs[0][0] == 4 * g * ns * N * (K + 1)
        assert j[1:] == [dw.data_ptr() + 4 * g * sw, db.data_ptr() + 4 * g * sb, ns, N, K, ABITS, N * (K + 1)]


def test_no_launch_without_jobs_or_on_error(fakes):
    _, launches = fakes
    with GradSink():
        pass
    with pytest.raises(RuntimeError):
        with GradSink() as sink:
            sink.wgrad(None, None, 1024, 8, 8, INV, [(torch.empty(8, 8), torch.empty(8))], ns=1)
            raise RuntimeError("backward failed")
    assert not launches


def _bucket_params():
    ps = [nn.Parameter(torch.zeros(s)) for s in [(4, 6), (6,), (21,), (4,), (4,)]]
    flat = torch.zeros(64)
    offs = [0, 24, 32, 56, 60]
    for p, o in zip(ps, offs):
        p.grad = flat[o:o + p.numel()].view_as(p)
    return ps, flat


def test_dest_inside_outside_misaligned():
    (w, b, odd, lw, lb), flat = _bucket_params()
    lo = flat.data_ptr()
    sink = GradSink((lo, lo + 4 * flat.numel()))
    assert sink.dest(w) is w.grad and sink.dest(b) is b.grad
    outside = nn.Parameter(torch.zeros(4))
    outside.grad = torch.zeros(4)
    g = sink.dest(outside)
    assert g is not outside.grad and g.shape == outside.shape and g.dtype == torch.float32
    mis = nn.Parameter(torch.zeros(3))
    mis.grad = flat[1:4]                      # inside the bucket, 4 bytes past a 16-byte boundary
    assert sink.direct(mis) is None and sink.dest(mis).data_ptr() != mis.grad.data_ptr()
    assert GradSink((lo, lo + 4 * 58)).direct(lw) is None      # [56, 60) runs past the end of the range
    assert GradSink(None).direct(w) is None
    assert sink.grads[id(w)] is w.grad and sink.grads[id(outside)] is g
    hb = handback([w, outside, odd], sink.grads)          # odd: no gradient produced
    assert hb[0] is None and hb[1].data_ptr() == g.data_ptr() and hb[2] is None


def test_ln_dest_adjacent_and_not():
    (w, b, odd, lw, lb), flat = _bucket_params()
    lo = flat.data_ptr()
    sink = GradSink((lo, lo + 4 * flat.numel()))
    d = sink.ln_dest(lw, lb)                   # lw [56, 60), lb [60, 64): back to back
    assert d.shape == (2, 4) and d.data_ptr() == lw.grad.data_ptr() and d[1].data_ptr() == lb.grad.data_ptr()
    assert sink.ln_dest(w, odd) is None        # w [0, 24), odd [32, 53): padding between
    assert GradSink(None).ln_dest(lw, lb) is None
