"""CPU tests of the shared host machinery: the writer ring (utils/writer_ring.py) on its own and under train.PanelWriter, behind
host stand-ins for the device buffers and the copy event; `msc_flip.shard_batches`; `evaluate.range_flag`.  The ring's other three
subclasses are covered where they live (test_msc_flip_eval_cpu.py, test_predict_cpu.py, test_camseed_cpu.py)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import weclip_vit_comer_amd  # noqa: F401
from weclip_vit_comer_amd import msc_flip, validate
from weclip_vit_comer_amd import train as T
from weclip_vit_comer_amd.utils import evaluate
from weclip_vit_comer_amd.utils.writer_ring import WriterRing

SHAPES = {"images": (5, 7), "seg_conf": (6, 3), "attn_pred_0": (1, 1)}      # odd sizes: no section ends 4-byte aligned; and a 1x1


class _Event:
    """Stands in for torch.cuda.Event: the host 'copy' is complete when copy_ returns."""

    def record(self):
        pass

    def synchronize(self):
        pass


def _host_alloc(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8), torch.empty(nbytes, dtype=torch.uint8)


def _paint(slot, seed):
    rs = np.random.RandomState(seed)
    data = {}
    for name, view in slot.views.items():
        data[name] = rs.randint(0, 256, tuple(view.shape)).astype(np.uint8)
        view.copy_(torch.from_numpy(data[name]))
    return data


def _panel(out, n, name):
    with Image.open(os.path.join(out, f"iter_{n}_{name}.png")) as im:
        return im.mode, np.asarray(im)


# ---------------------------------------------------------------------------------------------- PanelWriter
def test_panel_writer_writes_every_canvas_and_hands_it_on(tmp_path):
    out, seen = str(tmp_path / "panels"), []
    pw = T.PanelWriter(out, depth=2, on_image=lambda name, chw, n: seen.append((n, name, chw.copy())),
                       alloc=_host_alloc, event=_Event)
    assert (pw.writers, pw.depth, len(pw.slots), pw.jobs.maxsize) == (2, 2, 2, 2)
    expect = {}
    for i in range(5):                                                       # more sets than buffers
        slot = pw.acquire(SHAPES)
        assert {k: tuple(v.shape) for k, v in slot.views.items()} == {k: (3,) + hw for k, hw in SHAPES.items()}
        assert all(v.data_ptr() % 4 == slot.dev.data_ptr() % 4 for v in slot.views.values())
        expect[10 * i] = _paint(slot, i)
        pw.commit(slot, 10 * i)
    assert pw.finish() == 5
    assert sorted(os.listdir(out)) == sorted(f"iter_{n}_{name}.png" for n in expect for name in SHAPES)
    for n, data in expect.items():
        for name, chw in data.items():
            mode, pixels = _panel(out, n, name)
            assert mode == "RGB" and np.array_equal(pixels, chw.transpose(1, 2, 0))
    assert sorted((n, name) for n, name, _ in seen) == sorted((n, name) for n in expect for name in SHAPES)
    assert all(np.array_equal(chw, expect[n][name]) for n, name, chw in seen)


def test_panel_writer_zeroes_the_bytes_a_smaller_set_reuses(tmp_path):
    out = str(tmp_path / "panels")
    pw = T.PanelWriter(out, writers=1, depth=1, alloc=_host_alloc, event=_Event)
    slot = pw.acquire(SHAPES)
    for v in slot.views.values():
        v.fill_(255)
    pw.commit(slot, 1)
    small = {"images": (3, 5), "seg_conf": (2, 2)}
    again = pw.acquire(small)                                                # waits for the writer of set 1
    assert again is slot and all(int(v.max()) == 0 for v in again.views.values())
    pw.commit(again, 2)
    assert pw.finish() == 2
    assert all(_panel(out, 1, name)[1].min() == 255 for name in SHAPES)
    assert all(_panel(out, 2, name)[1].max() == 0 and _panel(out, 2, name)[1].shape == hw + (3,) for name, hw in small.items())


def test_panel_writer_keeps_turning_after_on_image_raises(tmp_path):
    out = str(tmp_path / "panels")

    def on_image(name, chw, n):
        if n == 2:
            raise ValueError("tensorboard refused set 2")
    pw = T.PanelWriter(out, depth=2, on_image=on_image, alloc=_host_alloc, event=_Event)
    for n in range(5):                                                       # the failed set frees its buffer
        slot = pw.acquire(SHAPES)
        _paint(slot, n)
        pw.commit(slot, n)
    with pytest.raises(ValueError, match="set 2"):
        pw.finish()
    assert pw.written == 4 and all(not t.is_alive() for t in pw.threads)
    assert all(os.path.isfile(os.path.join(out, f"iter_{n}_{name}.png")) for n in (0, 1, 3, 4) for name in SHAPES)


# ---------------------------------------------------------------------------------------------- the ring alone
class _Keep(WriterRing):
    def _write(self, slot, job):
        self.seen.append(job if job != "bad" else 1 // 0)


def test_commit_hands_write_the_job_it_was_given():
    ring = _Keep(writers=1, depth=2, alloc=_host_alloc, event=_Event)
    ring.seen = []
    jobs = ["2007_000033", ["a", "b"], 400]
    for job in jobs:
        slot = ring.next_slot()
        assert ring.carve(slot, [("x", (3,), torch.uint8), ("y", (2,), torch.float32)]) == 12 and slot.used == 12
        assert slot.views["y"].data_ptr() - slot.views["x"].data_ptr() == 4
        ring.commit(slot, job)
    assert ring.drain() is None and ring.written == 3
    assert len(ring.seen) == 3 and all(a is b for a, b in zip(ring.seen, jobs))


def test_drain_returns_what_finish_raises():
    rings = [_Keep(writers=1, alloc=_host_alloc, event=_Event) for _ in range(2)]
    for ring in rings:
        ring.seen = []
        for job in ("ok", "bad", "ok"):
            slot = ring.next_slot()
            ring.carve(slot, [("x", (1,), torch.uint8)])
            ring.commit(slot, job)
    with pytest.raises(ZeroDivisionError) as raised:
        rings[0].finish()
    error = rings[1].drain()
    assert type(error) is type(raised.value) and error is rings[1].error and rings[1].written == 2


# ---------------------------------------------------------------------------------------------- shard_batches
class _Loader:
    def __init__(self, **attrs):
        vars(self).update(attrs)

    def __iter__(self):
        return iter(range(7))


def test_shard_batches_gives_every_batch_to_one_rank():
    for rank in range(3):
        assert list(msc_flip.shard_batches(_Loader(world=3, rank=rank), rank, 3)) == list(range(7))      # its share already
        assert list(msc_flip.shard_batches(_Loader(), rank, 3)) == list(range(rank, 7, 3))
        assert list(msc_flip.shard_batches(_Loader(world=3, rank=(rank + 1) % 3), rank, 3)) == list(range(rank, 7, 3))
    assert sorted(b for rank in range(3) for b in msc_flip.shard_batches(_Loader(), rank, 3)) == list(range(7))
    assert list(msc_flip.shard_batches(_Loader(), 0, 1)) == list(range(7))


# ---------------------------------------------------------------------------------------------- range_flag
def test_range_flag_is_one_tensor_per_indexed_device(monkeypatch):
    made, zeros = [], torch.zeros
    monkeypatch.setattr(evaluate, "_flags", {})
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
    monkeypatch.setattr(torch, "zeros", lambda *a, device, **kw: made.append(device) or zeros(*a, **kw))      # a host tensor
    flag = evaluate.range_flag("cuda")                                       # index-less: the current device
    assert validate._flag is evaluate.range_flag
    assert evaluate.range_flag(torch.device("cuda", 3)) is flag and evaluate.range_flag("cuda:1") is not flag
    assert made == [torch.device("cuda", 3), torch.device("cuda", 1)] and sorted(evaluate._flags, key=str) == made[::-1]
    assert flag.dtype == torch.int32 and evaluate.check_predictions_in_range("cuda")
    flag.fill_(1)
    assert not evaluate.check_predictions_in_range("cuda:3") and evaluate.check_predictions_in_range("cuda:1")
    assert evaluate.check_predictions_in_range("cuda:2")                     # never used: nothing to read
