"""fp64 restatement of the momentum-SGD step behind `wc_sgd_multi` / `utils.optimizer.PolyWarmupSGD`, with the magnitudes its
error bounds are stated in, and the lr schedule of the reference's PolyWarmupSGD (utils/optimizer.py:35-65) restated.

The step (torch.optim.SGD with dampening 0, no Nesterov, no maximize):

    g' = g + wd p;    buf' = mu buf + g';    p' = p - lr buf'

Bounds of an fp32 evaluation against the fp64 one from the same fp32 inputs (u = 2^-24; lr, mu and wd each rounded once to
fp32, a relative error of at most u each; every fp32 operation rounds once; first order, times 1 + 2^-20 for the rest):

    buf':  wd p carries two relative errors (wd's rounding, the product's) and the add one; mu buf carries two; the final add one:
           |buf'_32 - buf'_64| <= 4 u A_buf,   A_buf = mu |buf| + |g| + wd |p|
    p':    lr buf' carries the buffer's four and two of its own (lr's rounding, the product's); the subtraction one:
           |p'_32 - p'_64|   <= 7 u A_p,       A_p = |p| + lr A_buf

A contraction into FMA only removes roundings.  The factors are counted, not measured."""
import torch

from tests.trainops_ref import adamw_inputs

F64, F32 = torch.float64, torch.float32
EPS = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -20
K_BUF, K_P = 4, 7
MOMENTUM = 0.9

SGD_SIZES = (4, 65536, 2 * 65536 + 148, 2 * 16384 + 5, 4096)      # the last one: grad a view at a 4-byte offset
SGD_VECTOR = (True, True, True, False, False)                     # the kernel path each of them takes
SGD_GROUPS = (dict(lr=2e-3, weight_decay=0.01), dict(lr=5e-4, weight_decay=0.3))


def sgd_inputs(n, seed=0, fresh=False):
    """p, g, buf fp32 (every 7th g zero); fresh: a zero buffer, the state before a first step."""
    p, g, m, _ = adamw_inputs(n, seed=seed)
    return p, g, torch.zeros_like(m) if fresh else m


def sgd_path(k):
    return "sgd_multi_kernel (" + ("vector" if SGD_VECTOR[k] else "scalar") + ")"


def sgd(p, g, buf, lr, weight_decay, momentum=MOMENTUM, dt=F64):
    """One step in dtype dt, the three scalars rounded to dt once.  -> p', buf', A_p, A_buf (the magnitudes in dt as well)."""
    sc = lambda val: torch.tensor(val, dtype=F64).to(dt)      # noqa: E731
    lr_, mu, wd = sc(lr), sc(momentum), sc(weight_decay)
    p, g, buf = (t.to(dt) for t in (p, g, buf))
    gd = g + wd * p
    bo = mu * buf + gd
    po = p - lr_ * bo
    A_buf = mu * buf.abs() + g.abs() + wd * p.abs()
    return po, bo, p.abs() + lr_ * A_buf, A_buf


def sgd_bounds(A_p, A_buf):
    """(bound of p', bound of buf') of an fp32 step against the fp64 one whose magnitudes these are."""
    return K_P * EPS * SECOND_ORDER * A_p.double(), K_BUF * EPS * SECOND_ORDER * A_buf.double()


def sgd_lr_mult(step, warmup_iter, max_iter, power):
    """The schedule at global step `step` (from 0) -> (mult, gain): lr = base * mult * gain, multiplied in that order so that
    the Python floats are the reference's; None once step >= max_iter, where the lr is left as it stands.  During the warm-up
    the polynomial runs DOWN from 1 at ten times the base lr (gain 10); behind it the decay restarts at the base lr."""
    if step < warmup_iter:
        return (1 - step / warmup_iter) ** power, 10
    if step < max_iter:
        return (1 - (step - warmup_iter) / (max_iter - warmup_iter)) ** power, 1
    return None


def sgd_lr(base, step, warmup_iter, max_iter, power, current=None):
    """The lr of a group with base lr `base` at `step`; `current` is what it held before (returned once step >= max_iter)."""
    m = sgd_lr_mult(step, warmup_iter, max_iter, power)
    return current if m is None else base * m[0] * m[1]


# ---------------------------------------------------------------------------------------------------------------------
# the schedule / trajectory fixture (tests/golden/sgd_schedule.npz, written by tests/golden/make_sgd_golden.py)

SCHED_BASE = (2e-3, 5e-4)                       # base lr of the two groups
SCHED_WARMUP = (0, 3)
SCHED_MAX_ITER = 40
SCHED_POWER = (1.0, 0.9)
TRAJ = dict(warmup_iter=3, max_iter=40, power=0.9, steps=6, sizes=(5, 3), weight_decay=(0.01, 0.3))


def sched_key(warmup_iter, power):
    return f"lr_w{warmup_iter}_p{str(power).replace('.', '_')}"


def traj_inputs():
    """The CPU trajectory's fp32 start values, one tensor per group, and its gradients per step (seeded)."""
    gen = torch.Generator().manual_seed(4242)
    p0 = [torch.randn(n, generator=gen) for n in TRAJ["sizes"]]
    grads = [[torch.randn(n, generator=gen) * (0.5 + it) for n in TRAJ["sizes"]] for it in range(TRAJ["steps"])]
    return p0, grads


def run_schedule(cls, warmup_iter, power):
    """lr of both groups before every step s = 0 .. max_iter + 2 of optimizer class `cls` on CPU -> (steps, 2) float64 list."""
    ps = [torch.nn.Parameter(torch.ones(2)) for _ in SCHED_BASE]
    opt = cls([dict(params=[p], lr=b) for p, b in zip(ps, SCHED_BASE)], lr=SCHED_BASE[0], weight_decay=0.0, betas=[0.9, 0.999],
              warmup_iter=warmup_iter, max_iter=SCHED_MAX_ITER, warmup_ratio=1e-6, power=power)
    rows = []
    for _ in range(SCHED_MAX_ITER + 3):
        for p in ps:
            p.grad = torch.zeros(2)
        opt.step()
        rows.append([g["lr"] for g in opt.param_groups])
    return rows


def run_trajectory(cls):
    """Six CPU steps of optimizer class `cls` across the warm-up boundary -> per step [p of group 0, p of group 1, their momentum
    buffers], fp32."""
    p0, grads = traj_inputs()
    ps = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = cls([dict(params=[p], lr=b, weight_decay=wd) for p, b, wd in zip(ps, SCHED_BASE, TRAJ["weight_decay"])],
              lr=SCHED_BASE[0], weight_decay=0.01, betas=[0.9, 0.999], warmup_iter=TRAJ["warmup_iter"], max_iter=TRAJ["max_iter"],
              warmup_ratio=1e-6, power=TRAJ["power"])
    out = []
    for it in range(TRAJ["steps"]):
        for p, g in zip(ps, grads[it]):
            p.grad = g.clone()
        opt.step()
        out.append([p.detach().clone() for p in ps] + [opt.state[p]["momentum_buffer"].clone() for p in ps])
    return out
