"""CPU checks of the training driver's host side (weclip_vit_comer_amd.train): the YAML loader, the work_dir tree and the
file names, the log line, metrics.jsonl and the argument parser.  No GPU."""
import os

import weclip_vit_comer_amd  # noqa: F401
from weclip_vit_comer_amd import train as T

YAML = """\
dataset:
  root_dir: /data/VOC2012
  name_list_dir: /data/lists
  num_classes: 21
  crop_size: 320
  resize_range: [512, 2048]
  rescale_range: [0.5, 2.0]
  ignore_index: 255

work_dir:
  dir: {work_dir}
  ckpt_dir: checkpoints
  pred_dir: predictions
  segs_dir: segs
  tb_logger_dir: tb_logger

train:
  split: train_aug
  samples_per_gpu: 4 #4 #2
  max_iters: 30000
  cam_iters: 2000
  eval_iters: 2000
  log_iters: 200

val:
  split: train

optimizer:
  type: AdamW
  learning_rate: 2e-4 #2e-4
  betas: [0.9, 0.999]
  weight_decay: 0.01

scheduler:
  warmup_iter: 50 #1500
  warmup_ratio: 1e-6
  power: 1.0

clip_init:
  clip_pretrain_path: /data/ViT-B-16.pt
  embedding_dim: 256
  in_channels: [768, 768,768,768]
"""


def _write(tmp_path):
    path = tmp_path / "voc_attn_reg.yaml"
    path.write_text(YAML.format(work_dir=str(tmp_path / "work")))
    return str(path)


def test_load_config_coerces_yaml11_floats_and_gives_attribute_access(tmp_path):
    import yaml
    path = _write(tmp_path)
    raw = yaml.safe_load(open(path))
    assert isinstance(raw["optimizer"]["learning_rate"], str)              # what PyYAML makes of `2e-4`: the reason for the coercion
    cfg = T.load_config(path)
    assert isinstance(cfg.optimizer.learning_rate, float) and cfg.optimizer.learning_rate == 2e-4
    assert isinstance(cfg.scheduler.warmup_ratio, float) and cfg.scheduler.warmup_ratio == 1e-6
    assert cfg.optimizer.betas == [0.9, 0.999] and all(isinstance(b, float) for b in cfg.optimizer.betas)
    assert cfg.optimizer.weight_decay == 0.01 and cfg.scheduler.power == 1.0 and cfg.scheduler.warmup_iter == 50
    assert cfg.dataset.crop_size == 320 and cfg.dataset.resize_range == [512, 2048] and cfg.train.split == "train_aug"
    assert cfg.clip_init.in_channels == [768] * 4 and cfg["val"]["split"] == "train"
    assert cfg.optimizer.type == "AdamW" and cfg.dataset.root_dir == "/data/VOC2012"       # strings stay strings
    over = T.load_config(path, crop_size=512, work_dir="elsewhere")
    assert over.dataset.crop_size == 512 and over.work_dir.dir == "elsewhere"
    cfg.train.max_iters = 7
    assert cfg["train"]["max_iters"] == 7


def test_work_dir_tree_and_checkpoint_names(tmp_path):
    cfg = T.load_config(_write(tmp_path))
    log = T.prepare_work_dir(cfg, timestamp="2024-01-02-03-04")
    work = str(tmp_path / "work")
    assert log == os.path.join(work, "2024-01-02-03-04.log")
    assert cfg.work_dir.ckpt_dir == os.path.join(work, "checkpoints", "2024-01-02-03-04")
    assert cfg.work_dir.pred_dir == os.path.join(work, "predictions")
    assert cfg.work_dir.tb_logger_dir == os.path.join(work, "tb_logger", "2024-01-02-03-04")
    assert all(os.path.isdir(d) for d in (cfg.work_dir.ckpt_dir, cfg.work_dir.pred_dir, cfg.work_dir.tb_logger_dir))
    model, state = T.checkpoint_paths(cfg.work_dir.ckpt_dir, 28000)
    assert os.path.basename(model) == "WeCLIP_model_iter_28000.pth" and os.path.basename(state) == "train_state_iter_28000.pth"
    assert T.state_path_of(model) == state
    # another rank resolves the same names and creates nothing
    cfg2 = T.load_config(_write(tmp_path), work_dir=str(tmp_path / "other"))
    T.prepare_work_dir(cfg2, timestamp="t", create=False)
    assert not os.path.exists(str(tmp_path / "other"))
    assert T.SAVE_AFTER == {"voc": 26000, "coco": 40000}


def test_log_line_is_the_references_character_for_character():
    line = T.format_log_line(200, "0:02:11", "5:25:19", 1.9867e-4, 0.123449, 0.98765, 0.87654)
    assert line == ("Iter: 200; Elasped: 0:02:11; ETA: 5:25:19; LR: 1.987e-04;, pseudo_seg_loss: 0.1234, attn_loss: 0.9877, "
                    "pseudo_seg_mAcc: 0.8765")


def test_metrics_jsonl_round_trips(tmp_path):
    path = str(tmp_path / "metrics.jsonl")
    recs = [{"iter": 200, "lr": 1.9867e-4, "seg_loss": 0.5, "attn_loss": 0.25, "pseudo_seg_mAcc": 0.875},
            {"iter": 400, "lr": 1.97e-4, "seg_loss": 0.1 + 0.2, "attn_loss": 1e-9, "pseudo_seg_mAcc": 1.0 / 3.0}]
    for r in recs:
        T.append_metrics(path, r)
    assert T.read_metrics(path) == recs
    assert len(open(path).read().splitlines()) == 2
    # a NaN window mean (a batch without foreground pseudo labels, as in the reference) is written as strict JSON: null
    T.append_metrics(path, {"iter": 600, "lr": 1e-4, "seg_loss": float("nan"), "attn_loss": 0.5, "pseudo_seg_mAcc": 0.25})
    last = open(path).read().splitlines()[-1]
    assert "NaN" not in last and T.read_metrics(path)[-1] == {"iter": 600, "lr": 1e-4, "seg_loss": None, "attn_loss": 0.5,
                                                               "pseudo_seg_mAcc": 0.25}


def test_parser_accepts_the_references_options():
    a = T.build_parser().parse_args(["--config", "c.yaml", "--work_dir", "w", "--radius", "4", "--crop_size", "512", "--seg_detach"])
    assert (a.config, a.work_dir, a.radius, a.crop_size, a.seg_detach) == ("c.yaml", "w", 4, 512, True)
    d = T.build_parser().parse_args(["--config", "c.yaml"])
    assert (d.radius, d.crop_size, d.seg_detach, d.work_dir) == (8, 320, False, None)      # the reference's defaults
    assert d.graph is True and d.dataset == "voc" and d.max_iters is None and d.save_after is None and d.resume is None
    n = T.build_parser().parse_args(["--config", "c.yaml", "--no-graph", "--dataset", "coco", "--max_iters", "10", "--save_after", "0",
                                     "--threads", "2", "--prefetch", "1", "--reference_root", "r", "--resume", "x.pth"])
    assert n.graph is False and n.dataset == "coco" and (n.max_iters, n.save_after, n.threads, n.prefetch) == (10, 0, 2, 1)
