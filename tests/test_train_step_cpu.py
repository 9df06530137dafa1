"""CPU tests of the host side that `TrainStep` and `SupervisedTrainStep` share through their common base in train_step.py:
the eager path of the supervised step against a hand-written loop, the shape of the returned values with and without a
`reg` term, graph mode declining CPU tensors, the `direct_grads` wiring, and the single code path behind both classes."""
import pytest
import torch
import torch.nn.functional as F

from weclip_vit_comer_amd.train_step import SupervisedTrainStep, TrainStep, make_optimizer

NC = 5
NEVER = {"start_iter": 10 ** 9}         # a term that never becomes active: nothing of the GPU library is called


class _Engine:
    """Dummy owner of a `direct_grads` range (HeadEngine / CoMerInteraction stand-in)."""
    direct_grads = "unset"


class _StubSeg(torch.nn.Module):
    """CPU stand-in for the supervised model: forward(img, mode="train") -> seg only."""

    def __init__(self, engine=False):
        super().__init__()
        self.body = torch.nn.Conv2d(3, 8, 16, stride=16)
        self.pred = torch.nn.Conv2d(8, NC, 1)
        self.iter_num = 0
        if engine:
            self.head_engine = _Engine()

    def get_param_groups(self):
        return [[], [], [], list(self.parameters())]

    def forward(self, img, mode="train"):
        self.iter_num += 1
        return self.pred(self.body(img))


class _StubWeak(_StubSeg):
    """CPU stand-in with WeCLIP's contract (seg, cam_labels, attn_pred), as tests/test_boundary_cpu.py::_StubWeCLIP."""
    seg_trans_after = 15000

    def __init__(self, engine=False, comer=False):
        super().__init__(engine)
        if comer:
            self.comer = _Engine()

    def forward(self, img, names=None, mode="train", labels=None):
        self.iter_num += 1
        f = self.body(img)
        B, C, h, w = f.shape
        ff = f.reshape(B, C, h * w)
        return self.pred(f), (img[:, 0] > 0).long() * 2, torch.sigmoid(ff.transpose(2, 1).bmm(ff))


def _batches(n=3):
    g = torch.Generator().manual_seed(7)
    out = []
    for _ in range(n):
        label = torch.randint(0, NC, (2, 37, 53), generator=g)
        label[:, 10:14] = 255
        out.append((torch.randn(2, 3, 64, 64, generator=g), label))
    return out


def _flat(m):
    return torch.cat([p.detach().flatten() for p in m.parameters()])


def _model(cls, **kw):
    torch.manual_seed(0)
    return cls(**kw)


@pytest.fixture(scope="module")
def hand_loop():
    """Parameters and losses of three steps written out by hand."""
    m = _model(_StubSeg)
    opt = make_optimizer(m)
    losses = []
    for img, label in _batches():
        segs = F.interpolate(m(img), size=label.shape[1:], mode="bilinear", align_corners=False)
        loss = F.cross_entropy(segs, label, ignore_index=255)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return _flat(m), losses


@pytest.mark.parametrize("bucket", [True, False])
def test_three_eager_supervised_steps_equal_the_hand_written_loop(hand_loop, bucket):
    ref, ref_losses = hand_loop
    m = _model(_StubSeg)
    step = SupervisedTrainStep(m, bucket=bucket)
    losses = [step(img, label).item() for img, label in _batches()]
    assert all(torch.isfinite(torch.tensor(losses))) and len(set(losses)) == 3
    assert torch.allclose(torch.tensor(losses), torch.tensor(ref_losses), rtol=1e-5, atol=1e-7)
    assert torch.allclose(_flat(m), ref, rtol=1e-5, atol=1e-7), (_flat(m) - ref).abs().max()
    assert m.iter_num == 3 and (step.bucket is not None) == bucket


def test_return_shapes_with_and_without_a_reg_term():
    (img, label), = _batches(1)
    sup = [SupervisedTrainStep(_model(_StubSeg), reg=reg) for reg in (None, NEVER)]
    weak = [TrainStep(_model(_StubWeak), reg=reg) for reg in (None, NEVER)]
    for n in (1, 2):        # two calls: the same step of both runs sees the same parameters
        plain, (loss, energy) = sup[0](img, label), sup[1].step(img, label)
        assert isinstance(plain, torch.Tensor) and plain.dim() == 0 and not plain.requires_grad
        assert energy.dim() == 0 and energy.item() == 0 and loss.item() == plain.item()
        three, four = weak[0](img, labels=[[0], [1]]), weak[1](img, labels=[[0], [1]], img_box=None)
        assert isinstance(three, tuple) and len(three) == 3 and isinstance(four, tuple) and len(four) == 4
        assert all(t.dim() == 0 and not t.requires_grad for t in three + four)
        assert four[3].item() == 0 and [t.item() for t in four[:3]] == [t.item() for t in three]
        assert sup[0].reg is None and weak[0].reg is None and sup[1].reg.step_num == n and weak[1].reg.step_num == n


def test_graph_mode_takes_the_eager_path_on_cpu_tensors():
    (img, label), = _batches(1)
    sup = SupervisedTrainStep(_model(_StubSeg), graph=True)
    weak = TrainStep(_model(_StubWeak), graph=True)
    ref_s, ref_w = SupervisedTrainStep(_model(_StubSeg)), TrainStep(_model(_StubWeak))
    for _ in range(2):      # the second step of a signature is the one that would capture
        assert sup(img, label).item() == ref_s(img, label).item()
        assert weak(img, labels=[[0], [1]])[0].item() == ref_w(img, labels=[[0], [1]])[0].item()
    assert sup.graph and weak.graph and sup._graphs == {} and weak._graphs == {}
    assert sup.model.iter_num == 2 and weak.model.iter_num == 2


@pytest.mark.parametrize("cls,stub,owners", [(SupervisedTrainStep, _StubSeg, ["head_engine"]),
                                             (TrainStep, _StubWeak, ["head_engine"]),
                                             (TrainStep, _StubWeak, ["head_engine", "comer"])])
def test_direct_grads_is_the_bucket_byte_range(cls, stub, owners, monkeypatch):
    monkeypatch.delenv("WECLIP_DIRECT_GRADS", raising=False)
    kw = dict(engine=True, comer=True) if "comer" in owners else dict(engine=True)
    m = _model(stub, **kw)
    step = cls(m)
    flat = step.bucket.flat
    for name in owners:
        assert getattr(m, name).direct_grads == (flat.data_ptr(), flat.data_ptr() + 4 * flat.numel())
    cls(m, bucket=False)
    for name in owners:
        assert getattr(m, name).direct_grads is None
    monkeypatch.setenv("WECLIP_DIRECT_GRADS", "0")
    assert cls(m).bucket is not None
    for name in owners:
        assert getattr(m, name).direct_grads is None


def test_both_classes_run_one_shared_code_path():
    shared = [c for c in TrainStep.__mro__ if c in SupervisedTrainStep.__mro__ and c is not object]
    assert len(shared) == 1, shared
    base = shared[0]
    assert not issubclass(TrainStep, SupervisedTrainStep) and not issubclass(SupervisedTrainStep, TrainStep)
    assert SupervisedTrainStep._reduce_grads is TrainStep._reduce_grads is base.__dict__["_reduce_grads"]
    for cls in (TrainStep, SupervisedTrainStep):
        own = set(cls.__dict__)
        assert "_reduce_grads" not in own and "_backward" not in own
        # the capture / replay sequence is whatever the base's __call__ reaches; no class carries one of its own
        assert not [n for n in own if "graphed" in n or "capture" in n or "replay" in n], own
    assert SupervisedTrainStep.step is base.__call__ is SupervisedTrainStep.__call__
    graph_side = [n for n, f in base.__dict__.items() if callable(f) and "graph" in n]
    assert graph_side and all(getattr(TrainStep, n) is getattr(SupervisedTrainStep, n) for n in graph_side)
