"""MS COCO 2014 datasets with the reference's names and constructor arguments (datasets/coco.py); see voc.py for what the
classes offer.  Layout, as the reference's: `<root_dir>/JPEGImages/{train,val}/<full name>.jpg`,
`<root_dir>/SegmentationClass/{train,val}/<short name>.png`, `<name_list_dir>/<split>.txt`, `cls_labels_onehot.npy` keyed by
the FULL name.  The short name drops the `COCO_train2014_` (15 characters, stage "train") or `COCO_val2014_` (13, stage "val")
prefix (datasets/coco.py:61-69); items are yielded under the short name.

`CocoSegDataset(aug=True)` runs the chain of `VOC12SegDataset`: the reference's own version of it (datasets/coco.py:199-230)
unpacks the three results of random_crop into two names and cannot run.
"""
import os

from .voc import (VOC12Dataset, _ClsMixin, _SegMixin, load_cls_label_list, load_img_name_list,  # noqa: F401
                  read_image)

_PREFIX = {"train": 15, "val": 13}


def robust_read_image(image_name):
    """RGB uint8 (H,W,3) also for the grey JPEGs of COCO (datasets/coco.py:20-24)."""
    return read_image(image_name)


class CocoDataset(VOC12Dataset):
    def __init__(self, root_dir=None, name_list_dir=None, split="train", stage="train"):
        self.root_dir, self.stage = root_dir, stage
        self.img_dir = os.path.join(root_dir, "JPEGImages")
        self.label_dir = os.path.join(root_dir, "SegmentationClass")
        self.name_list_dir = os.path.join(name_list_dir, split + ".txt")
        self.name_list = load_img_name_list(self.name_list_dir)
        sub = "train" if "train" in split else ("val" if "val" in split else None)
        if sub is not None:
            self.img_dir, self.label_dir = os.path.join(self.img_dir, sub), os.path.join(self.label_dir, sub)

    def _files(self, idx):
        full = str(self.name_list[idx])
        img_path = os.path.join(self.img_dir, full + ".jpg")
        if self.stage not in _PREFIX:
            return full, full, img_path, None
        short = full[_PREFIX[self.stage]:]
        return short, full, img_path, os.path.join(self.label_dir, short + ".png")

    def __getitem__(self, idx):
        name, full, image, label = self.read(idx)
        return full, name, image, label


class CocoClsDataset(_ClsMixin, CocoDataset):
    def __init__(self, root_dir=None, name_list_dir=None, split="train", stage="train", resize_range=[512, 640],
                 rescale_range=[0.5, 2.0], crop_size=512, img_fliplr=True, ignore_index=255, num_classes=21, aug=False, **kwargs):
        super().__init__(root_dir, name_list_dir, split, stage)
        self._init_cls(resize_range, rescale_range, crop_size, img_fliplr, ignore_index, num_classes, aug, name_list_dir)


class CocoSegDataset(_SegMixin, CocoDataset):
    def __init__(self, root_dir=None, name_list_dir=None, split="train", stage="train", resize_range=[512, 640],
                 rescale_range=[0.5, 2.0], crop_size=512, img_fliplr=True, ignore_index=255, aug=False, **kwargs):
        super().__init__(root_dir, name_list_dir, split, stage)
        self._init_seg(resize_range, rescale_range, crop_size, img_fliplr, ignore_index, aug, name_list_dir)
