"""CPU checks of the supervised variant's training driver (`python -m weclip_vit_comer_amd.train --dataset seg`): the command
line, the log line and metrics.jsonl record built from one host read, and the C entry behind the step's confusion counts."""
import json
import math
import subprocess

import numpy as np
import pytest

import weclip_vit_comer_amd  # noqa: F401
from weclip_vit_comer_amd import _lib
from weclip_vit_comer_amd import train as T
from weclip_vit_comer_amd.utils.evaluate import scores_from_hist

HIST = np.array([[50, 3, 0], [4, 20, 1], [0, 0, 0]], dtype=np.int64)       # class 2 never appears as ground truth


def test_parser_accepts_the_seg_dataset():
    a = T.build_parser().parse_args(["--config", "x.yaml", "--dataset", "seg", "--seg_detach", "--radius", "4", "--reg_loss"])
    assert (a.dataset, a.seg_detach, a.radius, a.reg_loss) == ("seg", True, 4, True)
    assert T.build_parser().parse_args(["--config", "x.yaml"]).dataset == "voc"
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--config", "x.yaml", "--dataset", "ade"])


def test_save_after_of_the_seg_dataset():
    assert T.SAVE_AFTER["seg"] == 26000 and T.SAVE_AFTER["voc"] == 26000 and T.SAVE_AFTER["coco"] == 40000


def test_seg_record_and_log_line_from_one_host_array():
    """host = the window sums (loss, seg_loss) followed by the 3 x 3 confusion matrix, as Trainer reads them in one `.cpu()`."""
    host = [4.5, 3.0] + [float(v) for v in HIST.flatten()]
    rec = T.seg_log_record(6, 2e-3, host, 3, 3)
    ref = scores_from_hist(HIST)
    assert rec == {"iter": 6, "lr": 2e-3, "seg_loss": 1.0, "pAcc": ref["pAcc"], "mAcc": ref["mAcc"], "miou": ref["miou"]}
    assert rec["pAcc"] == 70 / 78 and all(isinstance(rec[k], float) for k in ("pAcc", "mAcc", "miou"))
    line = T.format_seg_log_line(rec["iter"], "0:00:01", "0:00:02", rec["lr"], rec["seg_loss"], rec["pAcc"], rec["mAcc"], rec["miou"])
    assert line == ("Iter: 6; Elasped: 0:00:01; ETA: 0:00:02; LR: 2.000e-03;, seg_loss: 1.0000, seg_pAcc: %.4f, seg_mAcc: %.4f, "
                    "seg_mIoU: %.4f" % (ref["pAcc"], ref["mAcc"], ref["miou"]))
    assert "reg_loss" not in line and "pseudo" not in line and "attn_loss" not in line


def test_seg_record_has_reg_loss_only_with_its_sum():
    """With --reg_loss the sums are (loss, seg_loss, reg_loss): one more than without (the weak variant's fourth sum; this
    variant has no attn_loss, so it is the third here)."""
    cells = [float(v) for v in HIST.flatten()]
    assert "reg_loss" not in T.seg_log_record(3, 1e-3, [4.5, 3.0] + cells, 3, 3)
    rec = T.seg_log_record(3, 1e-3, [4.5, 3.0, 6e-3] + cells, 3, 3)
    assert rec["reg_loss"] == 2e-3 and rec["seg_loss"] == 1.0 and rec["pAcc"] == scores_from_hist(HIST)["pAcc"]
    line = T.format_seg_log_line(3, "a", "b", 1e-3, rec["seg_loss"], rec["pAcc"], rec["mAcc"], rec["miou"], rec["reg_loss"])
    assert line.endswith(", reg_loss: 2.0000e-03")
    for bad in ([4.5] + cells, [1.0, 2.0, 3.0, 4.0] + cells):
        with pytest.raises(ValueError):
            T.seg_log_record(3, 1e-3, bad, 3, 3)


def test_seg_record_non_finite_values_go_through_strict_json(tmp_path):
    """An empty window matrix (every label ignored) gives NaN scores, a NaN loss sum a NaN loss: null in the file."""
    rec = T.seg_log_record(3, 1e-3, [float("nan"), float("nan")] + [0.0] * 9, 3, 3)
    assert all(math.isnan(rec[k]) for k in ("seg_loss", "pAcc", "mAcc", "miou"))
    path = str(tmp_path / "metrics.jsonl")
    T.append_metrics(path, rec)
    with open(path) as f:
        text = f.read()
    assert "NaN" not in text
    assert json.loads(text) == {"iter": 3, "lr": 1e-3, "seg_loss": None, "pAcc": None, "mAcc": None, "miou": None}
    assert T.read_metrics(path) == [T.strict_json(rec)]


def test_step_pair_hist_is_declared_and_exported():
    protos = {name: args for name, _, args in _lib.parse_header()}
    assert "wc_step_pair_hist" in protos
    assert [n for _, n in protos["wc_step_pair_hist"]] == ["seg", "label", "hist", "flag", "B", "C", "Hs", "Ws", "H", "W", "nc", "stream"]
    _lib.lib()                                    # raises if the library is not built
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert any(l.split()[-1] == "wc_step_pair_hist" and " T " in l for l in out.splitlines())
    with pytest.raises(RuntimeError, match="bad argument"):
        _lib.lib().wc_step_pair_hist(None, None, None, None, 1, 1, 1, 1, 1, 1, 1, None)
