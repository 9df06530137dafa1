"""PASCAL VOC 2012 datasets with the reference's names and constructor arguments (datasets/voc.py), feeding the device
input pipeline: the files are decoded on the host with Pillow, everything after that runs in HIP kernels (data.py).

Directory layout, as the reference's: `<root_dir>/JPEGImages/<name>.jpg`, `<root_dir>/SegmentationClassAug/<name>.png`,
`<name_list_dir>/<split>.txt` and `<name_list_dir>/cls_labels_onehot.npy` (a pickled dict name -> one-hot vector).

  raw(idx)                  (name, uint8 image (H,W,3), uint8 label (H,W) or None, cls_label): what DeviceLoader packs
  __getitem__, aug=False    the reference's tuple computed on the host (normalize_img + CHW, datasets/voc.py:137-143), so a
                            stock `DataLoader(val_dataset, batch_size=1)` keeps working
  __getitem__, aug=True     raises: the augmentation exists on the device only -- iterate a `datasets.DeviceLoader`
"""
import os

import numpy as np
from torch.utils.data import Dataset

from ..data import MEAN, STD


def load_img_name_list(img_name_list_path):
    """The names of `<split>.txt`, one per line, as an array of str (datasets/voc.py:19-21)."""
    return np.loadtxt(img_name_list_path, dtype=str, ndmin=1)


def load_cls_label_list(name_list_dir):
    """The dict name -> one-hot class vector of `cls_labels_onehot.npy` (datasets/voc.py:23-25)."""
    return np.load(os.path.join(name_list_dir, "cls_labels_onehot.npy"), allow_pickle=True).item()


def read_image(path):
    """RGB uint8 (H,W,3), whatever the file's mode (a grey or CMYK JPEG is converted: datasets/coco.py:20-24)."""
    from ..clip.generate_cams import load_image
    return load_image(path).numpy()


def read_label(path):
    """The stored indices of a label PNG, uint8 (H,W): mode L as is, mode P WITHOUT palette expansion."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "P"):
            raise RuntimeError(f"{path}: label maps must be 8-bit index images (mode L or P), got mode {im.mode}")
        return np.array(im, dtype=np.uint8)


def normalize_chw(image_u8, mean=MEAN, std=STD):
    """normalize_img (datasets/transforms.py:8-15) + HWC -> CHW on the host.  The image is uint8 here, so numpy evaluates
    (x - mean) / std in double precision and rounds once on the store into the float32 array."""
    out = np.empty((3,) + image_u8.shape[:2], np.float32)
    for c in range(3):
        out[c] = (image_u8[..., c] - mean[c]) / std[c]
    return out


def _device_only(cls):
    raise RuntimeError(f"{cls}(aug=True): the train-time augmentation runs on the device only; wrap the dataset in "
                       "datasets.DeviceLoader instead of indexing it (or of a torch DataLoader)")


class VOC12Dataset(Dataset):
    """Names and files of one split (datasets/voc.py:28-67).  `stage` "train" / "val" read the label PNG, "test" does not."""

    def __init__(self, root_dir=None, name_list_dir=None, split="train", stage="train"):
        self.root_dir, self.stage = root_dir, stage
        self.img_dir = os.path.join(root_dir, "JPEGImages")
        self.label_dir = os.path.join(root_dir, "SegmentationClassAug")
        self.name_list_dir = os.path.join(name_list_dir, split + ".txt")
        self.name_list = load_img_name_list(self.name_list_dir)

    def __len__(self):
        return len(self.name_list)

    def _files(self, idx):
        """(name under which the item is yielded, key of the class-label dict, image path, label path or None)."""
        name = str(self.name_list[idx])
        label = os.path.join(self.label_dir, name + ".png") if self.stage in ("train", "val") else None
        return name, name, os.path.join(self.img_dir, name + ".jpg"), label

    def read(self, idx, with_label=True):
        """(name, key, image uint8 (H,W,3), label uint8 (H,W) or None)."""
        name, key, img_path, label_path = self._files(idx)
        image = read_image(img_path)
        if not with_label:
            return name, key, image, None
        # stage "test": the reference hands out the first image channel as a stand-in label (datasets/voc.py:64-65)
        label = read_label(label_path) if label_path is not None else np.ascontiguousarray(image[:, :, 0])
        return name, key, image, label

    def __getitem__(self, idx):
        name, _, image, label = self.read(idx)
        return name, image, label


class _ClsMixin:
    """Image-level labels: `VOC12ClsDataset` / `CocoClsDataset`.  kind = "cls" tells DeviceLoader which chain to run
    (random_scaling -> random_fliplr -> random_crop -> normalize_img, datasets/voc.py:109-144)."""
    kind = "cls"

    def _init_cls(self, resize_range, rescale_range, crop_size, img_fliplr, ignore_index, num_classes, aug, name_list_dir):
        self.aug, self.ignore_index, self.resize_range, self.rescale_range = aug, ignore_index, resize_range, rescale_range
        self.crop_size, self.img_fliplr, self.num_classes = crop_size, img_fliplr, num_classes
        self.label_list = load_cls_label_list(name_list_dir=name_list_dir)

    def raw(self, idx):
        name, key, image, _ = self.read(idx, with_label=False)
        return name, image, None, self.label_list[key]

    def __getitem__(self, idx):
        if self.aug:
            _device_only(type(self).__name__)
        name, image, _, cls_label = self.raw(idx)
        return name, normalize_chw(image), cls_label

    @staticmethod
    def _to_onehot(label_mask, num_classes, ignore_index):
        """One-hot vector of the classes in a label map, background and ignore excluded (datasets/voc.py:146-158)."""
        present = np.unique(label_mask).astype(np.int16)
        present = present[(present != ignore_index) & (present != 0)]
        onehot = np.zeros(shape=(num_classes), dtype=np.uint8)
        onehot[present] = 1
        return onehot


class _SegMixin:
    """Pixel-level labels: `VOC12SegDataset` / `CocoSegDataset`.  kind = "seg": random_fliplr(image, label) ->
    PhotoMetricDistortion -> random_crop(image, label) -> normalize_img (datasets/voc.py:216-251; the reference has the
    rescale of this chain commented out, so `rescale_range` is stored and not applied)."""
    kind = "seg"

    def _init_seg(self, resize_range, rescale_range, crop_size, img_fliplr, ignore_index, aug, name_list_dir):
        self.aug, self.ignore_index, self.resize_range, self.rescale_range = aug, ignore_index, resize_range, rescale_range
        self.crop_size, self.img_fliplr = crop_size, img_fliplr
        # stage "test" never looks a class label up (raw() below): a tree without any label file, such as VOC's test set, opens
        if self.stage == "test" and not os.path.exists(os.path.join(name_list_dir, "cls_labels_onehot.npy")):
            self.label_list = {}
        else:
            self.label_list = load_cls_label_list(name_list_dir=name_list_dir)

    def raw(self, idx):
        name, key, image, label = self.read(idx)
        return name, image, label, (0 if self.stage == "test" else self.label_list[key])

    def __getitem__(self, idx):
        if self.aug:
            _device_only(type(self).__name__)
        name, image, label, cls_label = self.raw(idx)
        return name, normalize_chw(image), label, cls_label


class VOC12ClsDataset(_ClsMixin, VOC12Dataset):
    def __init__(self, root_dir=None, name_list_dir=None, split="train", stage="train", resize_range=[512, 640],
                 rescale_range=[0.5, 2.0], crop_size=512, img_fliplr=True, ignore_index=255, num_classes=21, aug=False, **kwargs):
        super().__init__(root_dir, name_list_dir, split, stage)
        self._init_cls(resize_range, rescale_range, crop_size, img_fliplr, ignore_index, num_classes, aug, name_list_dir)


class VOC12SegDataset(_SegMixin, VOC12Dataset):
    def __init__(self, root_dir=None, name_list_dir=None, split="train", stage="train", resize_range=[512, 640],
                 rescale_range=[0.5, 2.0], crop_size=512, img_fliplr=True, ignore_index=255, aug=False, **kwargs):
        super().__init__(root_dir, name_list_dir, split, stage)
        self._init_seg(resize_range, rescale_range, crop_size, img_fliplr, ignore_index, aug, name_list_dir)
