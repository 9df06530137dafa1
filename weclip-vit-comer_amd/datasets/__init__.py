"""Datasets on disk for the device input pipeline: the reference's `datasets` package (datasets/voc.py, datasets/coco.py)
with its class names and constructor arguments, and `DeviceLoader` in place of `DistributedSampler` + `DataLoader`.
`install_dropin(datasets=True)` makes `import datasets`, `from datasets import voc` and `from datasets import coco` resolve
here."""
from . import coco, folder, voc  # noqa: F401
from .loader import DeviceLoader, index_plan, labels_from_onehot, pack_batch  # noqa: F401
