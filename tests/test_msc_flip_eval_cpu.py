"""CPU tests of the evaluation entry point (weclip_vit_comer_amd.msc_flip_eval): the command line against the reference's
three scripts, the output tree, and the writer pool behind a stand-in for the device copy."""
import os
import queue
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import weclip_vit_comer_amd  # noqa: F401  (import alias for the hyphenated package dir)
from weclip_vit_comer_amd import _lib
from weclip_vit_comer_amd import msc_flip_eval as E


def test_parser_defaults_are_the_references():
    a = E.parse_args([])                                  # test_msc_flip_voc.py:20-28
    assert (a.config, a.work_dir, a.bkg_score, a.resize_long, a.eval_set, a.model_path) == (
        "configs/voc_attn_reg.yaml", "results", 0.45, 512, "val", "/your/path/WeCLIP/WeCLIP_model_iter_30000.pth")
    assert (a.dataset, a.scales, a.crf, a.save_logits, a.writers) == ("voc", [1.0, 0.75], False, False, 4)      # :199, :213
    c = E.parse_args(["--dataset", "coco"])               # test_msc_flip_coco.py:20-29
    assert (c.config, c.model_path) == ("configs/coco_attn_reg.yaml", "/your/path/WeCLIP/WeCLIP_model_iter_80000.pth")
    s = E.parse_args(["--dataset", "seg", "--model_path", "m.pth", "--config", "x.yaml"])
    assert (s.config, s.model_path, s.work_dir, s.resize_long) == ("x.yaml", "m.pth", "results", 512)
    assert E.CRF_PARAMS == dict(iter_max=10, pos_xy_std=3, pos_w=3, bi_xy_std=64, bi_rgb_std=5, bi_w=4)          # :126-133


def test_scales_and_switches_parse():
    a = E.parse_args(["--scales", "1,0.75,1.25", "--crf", "--save_logits", "--bkg_score", "0.3"])
    assert a.scales == [1.0, 0.75, 1.25] and a.crf is True and a.save_logits is True and a.bkg_score == 0.3
    assert E.parse_args(["--scales", "1"]).scales == [1.0] and E.parse_args(["--no-crf"]).crf is False
    assert E.parse_scales("0.5, 1 ,2") == [0.5, 1.0, 2.0]


def test_output_tree_is_work_dir_eval_set(tmp_path):
    out, dirs = E.output_dirs(str(tmp_path / "results"), "val")
    assert out == os.path.join(str(tmp_path), "results", "val")
    assert dirs == {k: os.path.join(out, k) for k in ("logit", "prediction", "prediction_cmap")}
    pool = E.WriterPool(out, writers=1, alloc=_host_alloc, event=_Event)
    assert pool.finish() == 0
    assert sorted(os.listdir(out)) == ["prediction", "prediction_cmap"]      # logit/ only with save_logits


class _Event:
    """Stands in for torch.cuda.Event: the host 'copy' below is complete when copy_ returns."""

    def record(self):
        pass

    def synchronize(self):
        pass


def _host_alloc(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8), torch.empty(nbytes, dtype=torch.uint8)


def _fill(slot, seed, H, W, shape=None):
    rs = np.random.RandomState(seed)
    pred = rs.randint(0, 256, (H, W)).astype(np.uint8)
    cmap = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    slot.views["pred"].copy_(torch.from_numpy(pred))
    slot.views["cmap"].copy_(torch.from_numpy(cmap))
    logits = None
    if shape:
        logits = rs.randn(2, *shape).astype(np.float32)
        slot.views["segs"].copy_(torch.from_numpy(logits[0]))
        slot.views["msc_segs"].copy_(torch.from_numpy(logits[1]))
    return pred, cmap, logits


def test_writer_pool_writes_the_files_under_their_names(tmp_path):
    out = str(tmp_path / "val")
    pool = E.WriterPool(out, writers=3, depth=2, save_logits=True, alloc=_host_alloc, event=_Event)
    sizes = [(7, 9), (33, 17), (5, 5), (64, 3), (9, 40), (33, 17), (12, 13)]      # more images than buffers; growing and shrinking
    expect = {}
    for i, (H, W) in enumerate(sizes):
        slot = pool.acquire(H, W, (3, 2 + i, 4))
        expect[f"2007_{i:06d}"] = _fill(slot, i, H, W, (3, 2 + i, 4))
        pool.commit(slot, f"2007_{i:06d}")
    assert pool.finish() == len(sizes)
    for k in ("prediction", "prediction_cmap", "logit"):
        assert sorted(os.listdir(os.path.join(out, k))) == sorted(n + (".npy" if k == "logit" else ".png") for n in expect)
    for name, (pred, cmap, logits) in expect.items():
        p = Image.open(os.path.join(out, "prediction", name + ".png"))
        c = Image.open(os.path.join(out, "prediction_cmap", name + ".png"))
        assert (p.mode, c.mode) == ("L", "RGB")
        assert np.array_equal(np.asarray(p), pred) and np.array_equal(np.asarray(c), cmap)
        d = np.load(os.path.join(out, "logit", name + ".npy"), allow_pickle=True).item()
        assert sorted(d) == ["msc_segs", "segs"] and d["segs"].dtype == np.float32 and d["segs"].shape == (1,) + logits[0].shape
        assert np.array_equal(d["segs"][0], logits[0]) and np.array_equal(d["msc_segs"][0], logits[1])


def test_writer_pool_bounds_its_queue(tmp_path):
    """At most `depth` images are in flight: with every writer held, the next acquire finds no free buffer."""
    gate = threading.Event()

    class Held(_Event):
        def synchronize(self):
            gate.wait()
    pool = E.WriterPool(str(tmp_path / "val"), writers=2, depth=3, alloc=_host_alloc, event=Held)
    for i in range(3):
        slot = pool.acquire(4, 6)
        _fill(slot, i, 4, 6)
        pool.commit(slot, f"n{i}")
    with pytest.raises(queue.Full):
        pool.acquire(4, 6, block=False)
    assert pool.jobs.maxsize == 3 and len(pool.slots) == 3
    gate.set()
    assert pool.finish() == 3
    assert sorted(os.listdir(os.path.join(str(tmp_path / "val"), "prediction"))) == ["n0.png", "n1.png", "n2.png"]


def test_writer_exception_is_raised_by_finish(tmp_path):
    out = str(tmp_path / "val")
    pool = E.WriterPool(out, writers=2, alloc=_host_alloc, event=_Event)
    names = ["ok_0", os.path.join("no_such_dir", "x"), "ok_1", "ok_2", "ok_3", "ok_4"]      # the second cannot be written
    for i, name in enumerate(names):
        slot = pool.acquire(6, 8)                             # the failed job frees its buffer: the ring keeps turning
        _fill(slot, i, 6, 8)
        pool.commit(slot, name)
    with pytest.raises(OSError):
        pool.finish()
    assert sorted(os.listdir(os.path.join(out, "prediction"))) == ["ok_0.png", "ok_1.png", "ok_2.png", "ok_3.png", "ok_4.png"]
    assert all(not t.is_alive() for t in pool.threads) and pool.written == 5


def test_new_symbols_are_declared():
    protos = {name: args for name, _, args in _lib.parse_header()}
    assert [n for _, n in protos["wc_eval_finish"]] == ["seg1", "msc", "cam", "gt", "pred1_u8", "predm_u8", "cmap_rgb", "hist",
                                                        "msc_hist", "cam_hist", "flag", "C", "Hs", "Ws", "Hl", "Wl", "nc", "stream"]
    assert [n for _, n in protos["wc_label_finish"]] == ["pred", "gt", "out_u8", "cmap_rgb", "hist", "flag", "H", "W", "nc", "stream"]
    src = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "evalfinish.hip")
    assert os.path.isfile(src)


def test_to_json_is_strict():
    import json
    r = {"cam": None, "seg": {"pAcc": np.float64(0.5), "miou": float("nan"), "iou": {0: np.float64(1.0), 1: np.float64("nan")}},
         "pixels": {"seg": np.int64(7)}, "images": 3}
    j = E.to_json(r)
    assert j == {"cam": None, "seg": {"pAcc": 0.5, "miou": None, "iou": {"0": 1.0, "1": None}}, "pixels": {"seg": 7}, "images": 3}
    assert json.loads(json.dumps(j, allow_nan=False)) == j
