"""CPU checks of the SGD path (utils.optimizer.PolyWarmupSGD, csrc/sgd_ops.hip wc_sgd_multi, make_optimizer(type=...), the
driver's optimizer.type): the fp64 restatement of tests/sgd_ref.py against torch.optim.SGD, its derived bounds against an fp32
evaluation and four planted faults, the lr schedule and a CPU trajectory against values recorded from the reference's own class
(tests/golden/sgd_schedule.npz; against the live class too where the reference checkout is present), the entry points, the
C entry's refusals and the load schedule of the kernel.  No GPU."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest
import torch

import weclip_vit_comer_amd  # noqa: F401
from tests import sgd_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = S.F64, S.F32


# ---------------------------------------------------------------------------------------------------------------------
# the restatement is torch.optim.SGD

def _torch_sgd_steps(p, grads, buf, grp, steps):
    """`steps` steps of torch.optim.SGD in fp64 from (p, buf) (buf None: fresh) -> states before the last step and after it."""
    q = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.SGD([q], lr=grp["lr"], momentum=S.MOMENTUM, weight_decay=grp["weight_decay"], foreach=False)
    if buf is not None:
        opt.state[q]["momentum_buffer"] = buf.double().clone()
    before = None
    for it in range(steps):
        mb = opt.state[q].get("momentum_buffer")
        before = (q.detach().clone(), torch.zeros_like(q) if mb is None else mb.clone())
        q.grad = grads[it].double().clone()
        opt.step()
    return before, (q.detach().clone(), opt.state[q]["momentum_buffer"].clone())


@pytest.mark.parametrize("gi", [0, 1])
@pytest.mark.parametrize("case", ["fresh", "step3"])
def test_restatement_is_torch_sgd_in_fp64(gi, case):
    """8 ulp of fp64 on the magnitudes: both sides round every operation once in fp64 (torch may fuse a multiply-add)."""
    grp = S.SGD_GROUPS[gi]
    n = 2 * 16384 + 5
    p, g, buf = S.sgd_inputs(n, seed=gi)
    gen = torch.Generator().manual_seed(7 + gi)
    grads = [g] + [torch.randn(n, generator=gen) for _ in range(2)]
    steps = 1 if case == "fresh" else 3
    (pb, bb), (pt, bt) = _torch_sgd_steps(p, grads, None, grp, steps)
    po, bo, A_p, A_buf = S.sgd(pb, grads[steps - 1].double(), bb, **grp)
    assert ((po - pt).abs() <= 8 * 2.0 ** -53 * A_p).all() and ((bo - bt).abs() <= 8 * 2.0 ** -53 * A_buf).all()
    assert (bt != 0).any() and not torch.equal(pt, pb)
    if case == "fresh":                           # torch's first step: buf = clone(g'); a zero buffer gives the same values
        assert torch.equal(bo, grads[0].double() + grp["weight_decay"] * pb)


# ---------------------------------------------------------------------------------------------------------------------
# the bounds hold for an fp32 evaluation and do not hold for a wrong update

def _ratios(got, ref):
    bp, bb = S.sgd_bounds(ref[2], ref[3])
    return ((got[0].double() - ref[0]).abs() / bp.clamp(min=1e-300)), ((got[1].double() - ref[1]).abs() / bb.clamp(min=1e-300))


@pytest.mark.parametrize("fresh", [False, True])
@pytest.mark.parametrize("gi", [0, 1])
def test_fp32_evaluation_is_inside_the_derived_bounds(gi, fresh):
    worst = [0.0, 0.0]
    for n in S.SGD_SIZES:
        p, g, buf = S.sgd_inputs(n, seed=gi, fresh=fresh)
        rp, rb = _ratios(S.sgd(p, g, buf, dt=F32, **S.SGD_GROUPS[gi]), S.sgd(p, g, buf, **S.SGD_GROUPS[gi]))
        worst = [max(worst[0], rp.max().item()), max(worst[1], rb.max().item())]
    print(f"group {gi} fresh {fresh}: worst err / bound p {worst[0]:.3g} buf {worst[1]:.3g}")
    assert worst[0] <= 1 and worst[1] <= 1


def _faulty(fault, p, g, buf, lr, weight_decay, mu=S.MOMENTUM):
    p, g, buf = p.double(), g.double(), buf.double()
    if fault == "decoupled_decay":                # AdamW-style: p *= 1 - lr*wd, the gradient without the decay term
        bo = mu * buf + g
        return p * (1 - lr * weight_decay) - lr * bo, bo
    gd = g + weight_decay * p
    if fault == "lr_on_gradient":                 # the momentum left out of the parameter update
        return p - lr * gd, mu * buf + gd
    if fault == "dampening_is_momentum":
        bo = mu * buf + (1 - mu) * gd
        return p - lr * bo, bo
    if fault == "nesterov":
        bo = mu * buf + gd
        return p - lr * (gd + mu * bo), bo
    raise KeyError(fault)


@pytest.mark.parametrize("fault", ["decoupled_decay", "lr_on_gradient", "dampening_is_momentum", "nesterov"])
def test_planted_faults_break_a_bound_on_four_elements(fault):
    """On the 4-element tensor, from a non-zero buffer, in both groups: some element of p' or buf' leaves its bound (an element
    whose gradient is zero may hide a fault; not all four do)."""
    for gi in (0, 1):
        p, g, buf = S.sgd_inputs(4, seed=gi)
        rp, rb = _ratios(_faulty(fault, p, g, buf, **S.SGD_GROUPS[gi]), S.sgd(p, g, buf, **S.SGD_GROUPS[gi]))
        print(f"{fault} group {gi}: err / bound p {rp.max().item():.3g} buf {rb.max().item():.3g}")
        # (one step of the decoupled decay moves p exactly as the coupled one does: that fault shows in the buffer alone, and
        #  in the parameters from the second step on)
        assert rp.max().item() > 1 or rb.max().item() > 1, "the planted fault is admissible"
        if fault != "decoupled_decay":
            assert rp.max().item() > 1, "the planted fault leaves the parameters inside their bound"


# ---------------------------------------------------------------------------------------------------------------------
# schedule and CPU trajectory: the reference's class, recorded (and live where its checkout is present)

def _ours():
    from weclip_vit_comer_amd.utils.optimizer import PolyWarmupSGD
    return PolyWarmupSGD


def _live_reference_class():
    """The reference's own class from its file, or None where the checkout is absent."""
    from oracle import refharness
    path = os.path.join(refharness.REF, "utils", "optimizer.py")
    if not (refharness.available() and os.path.isfile(path)):
        return None
    spec = importlib.util.spec_from_file_location("_ref_optimizer_live", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PolyWarmupSGD


@pytest.mark.parametrize("power", S.SCHED_POWER)
@pytest.mark.parametrize("warmup_iter", S.SCHED_WARMUP)
def test_schedule_equals_the_recorded_reference_values(golden, warmup_iter, power):
    rec = golden("sgd_schedule.npz")[S.sched_key(warmup_iter, power)]
    assert rec.shape == (S.SCHED_MAX_ITER + 3, 2) and rec.dtype == np.float64
    ours = S.run_schedule(_ours(), warmup_iter, power)
    current = list(S.SCHED_BASE)
    for s, row in enumerate(ours):
        for gi, base in enumerate(S.SCHED_BASE):
            assert row[gi] == float(rec[s, gi]), (s, gi, row[gi], float(rec[s, gi]))
            current[gi] = S.sgd_lr(base, s, warmup_iter, S.SCHED_MAX_ITER, power, current[gi])      # the restatement as well
            assert current[gi] == row[gi], (s, gi)
    assert ours[-1] == ours[S.SCHED_MAX_ITER - 1]                  # s >= max_iter: the lr is left as it is
    if warmup_iter:
        assert ours[0] == [b * 1.0 * 10 for b in S.SCHED_BASE] and ours[warmup_iter] == list(S.SCHED_BASE)
    live = _live_reference_class()
    if live is not None:
        assert S.run_schedule(live, warmup_iter, power) == ours


def test_cpu_parameters_reproduce_the_reference_class_bit_for_bit(golden):
    """Six steps across the warm-up boundary on CPU parameters (stock torch under the schedule): parameters and momentum buffers
    after every step equal the recorded ones of the reference's class in their bits."""
    rec = golden("sgd_schedule.npz")
    ours = S.run_trajectory(_ours())
    assert len(ours) == S.TRAJ["steps"] > S.TRAJ["warmup_iter"]
    for it, row in enumerate(ours):
        for gi in range(2):
            assert torch.equal(row[gi], torch.from_numpy(rec[f"traj_p{gi}"][it])), (it, gi, "p")
            assert torch.equal(row[2 + gi], torch.from_numpy(rec[f"traj_buf{gi}"][it])), (it, gi, "momentum_buffer")
    live = _live_reference_class()
    if live is not None:
        for a, b in zip(S.run_trajectory(live), ours):
            assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_constructor_keeps_the_references_attributes():
    p = torch.nn.Parameter(torch.zeros(3))
    opt = _ours()([p], lr=1e-3, weight_decay=0.02, betas=[0.5, 0.6], warmup_iter=2, max_iter=9, warmup_ratio=1e-6, power=0.9)
    assert isinstance(opt, torch.optim.SGD) and opt.global_step == 0
    g = opt.param_groups[0]
    assert (g["momentum"], g["weight_decay"], g["dampening"], g["nesterov"], g["lr"]) == (0.9, 0.02, 0, False, 1e-3)
    assert (opt.warmup_iter, opt.max_iter, opt.power, opt.warmup_lr) == (2, 9, 0.9, 1e-6) and "betas" not in g
    # the state of a CPU run is torch.optim.SGD's and loads into one; a loaded buffer of None counts as absent
    p.grad = torch.ones(3)
    opt.step()
    assert set(opt.state[p]) == {"momentum_buffer"} and opt.global_step == 1
    q = torch.nn.Parameter(torch.zeros(3))
    plain = torch.optim.SGD([q], lr=1e-3, momentum=0.9, weight_decay=0.02)
    plain.load_state_dict(opt.state_dict())
    assert torch.equal(plain.state[q]["momentum_buffer"], opt.state[p]["momentum_buffer"])
    sd = opt.state_dict()
    sd["state"][0]["momentum_buffer"] = None
    opt.load_state_dict(sd)
    opt.step()
    assert torch.is_tensor(opt.state[p]["momentum_buffer"])


# ---------------------------------------------------------------------------------------------------------------------
# entry points

class _Groups:
    def __init__(self):
        self.groups = [[torch.nn.Parameter(torch.zeros(2))] if k in (0, 3) else [] for k in range(4)]

    def get_param_groups(self):
        return self.groups


def test_make_optimizer_types():
    from weclip_vit_comer_amd.train_step import OPTIMIZER_TYPES, make_optimizer
    from weclip_vit_comer_amd.utils.optimizer import PolyWarmupAdamW, PolyWarmupSGD
    assert OPTIMIZER_TYPES == ("AdamW", "SGD")
    kw = dict(lr=3e-4, weight_decay=0.02, warmup_iter=5, max_iter=70, warmup_ratio=1e-5, power=0.8)
    default, adamw = make_optimizer(_Groups(), **kw), make_optimizer(_Groups(), type="adamw", **kw)
    assert type(default) is type(adamw) is PolyWarmupAdamW
    for name in ("SGD", "sgd", "Sgd"):
        m = _Groups()
        sgd = make_optimizer(m, type=name, **kw)
        assert type(sgd) is PolyWarmupSGD
        assert [g["lr"] for g in sgd.param_groups] == [g["lr"] for g in default.param_groups] == [3e-4, 0.0, 3e-4 * 10, 3e-4 * 10]
        assert [g["weight_decay"] for g in sgd.param_groups] == [g["weight_decay"] for g in default.param_groups]
        assert [len(g["params"]) for g in sgd.param_groups] == [1, 0, 0, 1] and sgd.param_groups[3]["params"][0] is m.groups[3][0]
        assert all(g["momentum"] == 0.9 for g in sgd.param_groups)
        assert (sgd.warmup_iter, sgd.max_iter, sgd.power) == (default.warmup_iter, default.max_iter, default.power) == (5, 70, 0.8)
    for bad in ("Adam", "", None, "momentum"):
        with pytest.raises(ValueError, match="AdamW, SGD"):
            make_optimizer(_Groups(), type=bad)


def _cfg(**optimizer):
    from weclip_vit_comer_amd import train as T
    return T._wrap({"optimizer": dict(learning_rate=2e-4, weight_decay=0.01, **optimizer)})


def test_driver_argument_and_yaml_precedence():
    from weclip_vit_comer_amd import train as T
    parse = lambda *a: T.build_parser().parse_args(["--config", "c.yaml", *a])      # noqa: E731
    assert parse().optimizer is None and parse("--optimizer", "SGD").optimizer == "SGD"
    with pytest.raises(SystemExit):
        parse("--optimizer", "Adam")
    assert T.optimizer_type(_cfg(), parse()) == "AdamW"                          # a missing key means AdamW
    assert T.optimizer_type(_cfg(type="AdamW"), parse()) == T.optimizer_type(_cfg(type="adamw"), parse()) == "AdamW"
    assert T.optimizer_type(_cfg(type="SGD"), parse()) == T.optimizer_type(_cfg(type="sgd"), parse()) == "SGD"
    assert T.optimizer_type(_cfg(type="SGD"), parse("--optimizer", "AdamW")) == "AdamW"        # the flag overrides the YAML
    assert T.optimizer_type(_cfg(type="AdamW"), parse("--optimizer", "SGD")) == "SGD"
    assert T.optimizer_type(_cfg(type="SGD"), types.SimpleNamespace()) == "SGD"               # arguments from before the flag
    with pytest.raises(ValueError, match="AdamW, SGD"):
        T.optimizer_type(_cfg(type="RMSprop"), parse())


def test_resume_refuses_a_state_of_the_other_optimizer():
    from weclip_vit_comer_amd import train as T
    T.check_state_optimizer({"optimizer": {}, "optimizer_type": "SGD"}, "SGD")
    T.check_state_optimizer({"optimizer": {}, "optimizer_type": "AdamW"}, "AdamW")
    T.check_state_optimizer({"optimizer": {}}, "AdamW")                          # files from before the key: AdamW
    with pytest.raises(RuntimeError, match="optimizer SGD.*configured for AdamW"):
        T.check_state_optimizer({"optimizer": {}, "optimizer_type": "SGD"}, "AdamW", "train_state_iter_2.pth")
    with pytest.raises(RuntimeError, match="optimizer AdamW.*configured for SGD"):
        T.check_state_optimizer({"optimizer": {}}, "SGD")


def test_dropin_import_line_resolves():
    """`from utils.optimizer import PolyWarmupSGD` after install_dropin(), in a fresh process (as tests/test_boundary_cpu.py)."""
    code = """
        import weclip_vit_comer_amd
        weclip_vit_comer_amd.install_dropin()
        from utils.optimizer import PolyWarmupSGD, PolyWarmupAdamW
        import torch
        import weclip_vit_comer_amd.utils.optimizer as real
        assert PolyWarmupSGD is real.PolyWarmupSGD and issubclass(PolyWarmupSGD, torch.optim.SGD)
        print("DROPIN-OK")
    """
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and "DROPIN-OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------------------------
# the C entry refuses bad arguments before any launch (the table pointer is never dereferenced)

_VALID = dict(table=ctypes.c_void_p(4096), count=2, lr=1e-3, momentum=0.9, weight_decay=0.01, blocks_per_tensor=64)
_NAN, _INF = float("nan"), float("inf")
_BAD = [dict(table=None), dict(count=0), dict(count=-1), dict(count=65536), dict(blocks_per_tensor=0), dict(blocks_per_tensor=-3),
        dict(momentum=-0.1), dict(momentum=1.0), dict(momentum=1.5), dict(momentum=_NAN), dict(lr=-1e-3), dict(lr=_INF), dict(lr=_NAN),
        dict(weight_decay=-0.01), dict(weight_decay=_INF), dict(weight_decay=_NAN)]


def test_entry_is_declared_as_the_refusals_assume():
    from weclip_vit_comer_amd import _lib
    protos = {name: args for name, _, args in _lib.parse_header()}
    assert [n for _, n in protos["wc_sgd_multi"]] == list(_VALID) + ["stream"]
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "sgd_ops.hip")).read()
    assert set(re.findall(r'extern "C" int (wc_\w+)\(', src)) == {"wc_sgd_multi"}


@pytest.mark.parametrize("kw", _BAD, ids=lambda kw: ",".join(f"{k}={'NULL' if v is None else v}" for k, v in kw.items()))
def test_sgd_multi_refusals(kw):
    from weclip_vit_comer_amd import _lib
    a = dict(_VALID)
    assert set(kw) <= set(a)
    a.update(kw)
    with pytest.raises(RuntimeError, match="wc_sgd_multi: bad argument"):
        _lib.lib().wc_sgd_multi(*a.values(), None)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's loads are global ones and none of them is waited for alone

def test_isa_scan_lists_nothing_for_the_kernel(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_scan
    finally:
        sys.path.pop(0)
    src = os.path.join(ROOT, "weclip-vit-comer_amd", "csrc", "sgd_ops.hip")
    assert isa_scan.report([src], threshold=1, out_dir=str(tmp_path)) == []
    found = {name: isa_scan.scan(lines) for name, lines in isa_scan.kernels(os.path.join(str(tmp_path), "sgd_ops.hip.s"))}
    assert len(found) == 1
    (name, (loads, alone, seq)), = found.items()
    # three loads per path (p, g, buf), each path's three issued back to back ahead of the first wait, two stores behind them
    assert "sgd_multi_kernel" in name and (loads, alone) == (6, 0) and seq.count("LLL") == 2 and seq.count("SS") == 2, seq
