"""Where the explicit backward engines (head_engine, comer_engine) put their parameter gradients.

One decision, shared by both: this step's flat all-reduce bucket (train_step.GradBucket, zeroed every step) is WRITTEN in
place, each gradient exactly once per backward, and the weight-gradient GEMMs and their split-K reductions are QUEUED: nothing
in a backward pass reads a weight gradient, so all GEMMs go out as one grid per kernel form (wc_gemm_km_f16_multi: launched
alone, each of them has to fill the chip by itself and pays its own ramp, prologue and tail) and all reductions as ONE
launch behind them (wc_sum_slices_wb_multi, instead of one launch of 5-7 us at the launch floor per weight gradient).  A
`.grad` outside the bucket (gradient accumulation, a TrainStep without a bucket, a harness calling backward twice) gets a
fresh tensor that autograd accumulates as usual.

The queue holds references to dY, X and the partials until the launch, so the caching allocator cannot hand their memory
out again; what it cannot see is a caller that WRITES an operand again before the sink exits (an in-place kernel, a scratch
buffer used twice, a view of a buffer that is rewritten).  Such a gradient has to be launched at once
(`GradSink(defer=False)`, or a `flush()` in front of the overwrite); the engines have none.
"""
import ctypes
import struct

import torch

from . import _lib as L
from . import ops
from .ops import F32


def slices(M, tiles, budget):
    """Split-K slice count of a weight-gradient GEMM with `tiles` output tiles over M tokens: the largest power of two that
    keeps the launch within `budget` workgroups and every slice at >= 256 tokens."""
    ns = 1
    while ns * 2 * tiles <= budget and M // (ns * 2) >= 256:
        ns *= 2
    return ns


def handback(params, grads):
    """What `Function.backward` returns for `params`: the gradient of each from `grads` ({id(param): tensor}), None where
    it was written into `p.grad` itself (or not produced)."""
    out = []
    for p in params:
        g = grads.get(id(p))
        if g is not None and p.grad is not None and g.data_ptr() == p.grad.data_ptr():
            g = None
        out.append(g.reshape(p.shape) if g is not None else None)
    return tuple(out)


class GradSink:
    """The parameter gradients of one backward pass: `bucket` is the (lo, hi) byte address range of the gradient bucket
    that may be written in place, or None.  Use as a context manager around the backward: the queued GEMMs and reductions
    are launched on a clean exit.  defer=False launches every GEMM where it is requested (tests, A/B): same partials."""

    def __init__(self, bucket=None, defer=True):
        self.bucket = bucket
        self.defer = defer
        self._gemms = []            # ops.wgrad_partials(queue=...) jobs: ((dY, X, partials kept alive), [16 int64 job fields])
        self.grads = {}             # id(param) -> gradient tensor
        self._jobs = []             # ((tensors kept alive until the launch), [8 int64 job fields])

    def __enter__(self):
        return self

    def __exit__(self, exc, *_):
        if exc is None:
            self.flush()

    def direct(self, p):
        """`p.grad` when it is a contiguous, fp32, 16-byte aligned view inside the bucket, else None."""
        g = p.grad
        if self.bucket is None or g is None or not g.is_contiguous() or g.dtype != F32 or g.data_ptr() % 16:
            return None
        lo, hi = self.bucket
        return g if lo <= g.data_ptr() and g.data_ptr() + 4 * g.numel() <= hi else None

    def dest(self, p):
        """The tensor p's gradient is written into (`direct(p)`, else a fresh one of p's shape), recorded for `handback`."""
        g = self.direct(p)
        if g is None:
            g = torch.empty(p.shape, device=p.device, dtype=F32)
        self.grads[id(p)] = g
        return g

    def put(self, params, grads):
        """Record gradients produced elsewhere (a LayerNorm's [dgamma; dbeta] rows)."""
        for p, g in zip(params, grads):
            self.grads[id(p)] = g

    def ln_dest(self, weight, bias):
        """(2, D) destination of a LayerNorm's [dgamma; dbeta]: the two bucket views when they lie back to back, else None."""
        gw, gb = self.direct(weight), self.direct(bias)
        if gw is None or gb is None or gb.data_ptr() != gw.data_ptr() + 4 * gw.numel():
            return None
        return torch.as_strided(gw, (2, gw.numel()), (gw.numel(), 1))

    def wgrad(self, dy16, x16, M, N, K, alpha, outs, *, ns, groups=1, sw=0, sb=0, **kw):
        """Split-K partials of dY^T [X | 1] (ops.wgrad_partials with `ns` slices; kw: lda, ldx, xmap, gA, gX) and their
        reduction, alpha * the slice sum, both queued until `flush`, into outs = [(dw, db)]:
          * one Linear: dw (N, K), db (N);
          * Linears stacked along N (one GEMM over their columns): each pair takes the next db.numel() rows of the partials;
          * groups > 1: `groups` gradients of one shape in one GEMM, outs holds group 0's and group g's lie at dw + g * sw,
            db + g * sb (elements)."""
        if sum(db.numel() for _, db in outs) != N:
            raise ValueError("GradSink.wgrad: the destinations do not cover the N gradient rows")
        if self.defer:
            kw["queue"] = self._gemms
        part, ns = ops.wgrad_partials(dy16, x16, M, N, K, slices=ns, bias=True, groups=groups, **kw)
        abits = struct.unpack("<I", struct.pack("<f", alpha))[0]
        stride = N * (K + 1)                # elements between two slices
        r0 = 0
        for dw, db in outs:
            rows = db.numel()
            for g in range(groups):
                self._jobs.append(((part, dw, db), [part.data_ptr() + 4 * (g * ns * stride + r0 * (K + 1)),
                                                    dw.data_ptr() + 4 * g * sw, db.data_ptr() + 4 * g * sb,
                                                    ns, rows, K, abits, stride]))
            r0 += rows

    def flush(self):
        """Every queued GEMM in one grid per kernel form, then every queued reduction in ONE launch."""
        ops.wgrad_launch(self._gemms)
        jobs, self._jobs = self._jobs, []
        if jobs:
            flat = [v for _, fields in jobs for v in fields]
            L.lib().wc_sum_slices_wb_multi((ctypes.c_int64 * len(flat))(*flat), len(jobs), L.stream())
