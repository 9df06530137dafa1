"""Images without any label: a directory, a glob or a list file as a dataset for `DeviceLoader` (the predict entry point,
predict.py).  No reference counterpart: the reference's datasets all need a VOC / COCO tree.

  raw(idx)     (name, uint8 image (H,W,3), None, zeros(1, uint8)): what DeviceLoader packs for a kind = "cls", aug = False dataset
  sizes()      [(H, W)] read from the file headers alone (no pixel is decoded)

Files are read with the package's own `read_image`: RGB, whatever the file's mode.  The EXIF orientation tag is NOT applied, as
everywhere else in this package (and in the reference, which decodes with `imageio` / Pillow without it): a photograph stored
rotated is predicted rotated, and the outputs have the stored size.
"""
import glob as _glob
import os

import numpy as np
from torch.utils.data import Dataset

from .voc import normalize_chw, read_image

EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".webp")       # what Pillow reads here, lower case


def _is_image(path):
    return os.path.splitext(path)[1].lower() in EXTENSIONS


def list_images(source, recursive=False):
    """-> (base directory, sorted image paths) of `source`: a directory (its own files; with `recursive` those of its
    sub-directories too), a glob pattern (`recursive` lets `**` cross directories), or a text file of paths, one per line
    (relative paths count from the list file's directory; empty lines and lines starting with # are skipped).  The base is the
    directory itself, else the deepest directory all the files share."""
    source = os.fspath(source)
    if os.path.isdir(source):
        if recursive:
            paths = [os.path.join(d, f) for d, _, files in os.walk(source) for f in files]
        else:
            paths = [os.path.join(source, f) for f in os.listdir(source)]
        paths = sorted(p for p in paths if _is_image(p) and os.path.isfile(p))
        return source, paths
    if os.path.isfile(source) and not _is_image(source):
        here = os.path.dirname(os.path.abspath(source))
        with open(source) as f:
            lines = [ln.strip() for ln in f]
        paths = [ln if os.path.isabs(ln) else os.path.join(here, ln) for ln in lines if ln and not ln.startswith("#")]
        missing = [p for p in paths if not os.path.isfile(p)]
        if missing:
            raise FileNotFoundError(f"ImageFolderDataset: {source} lists {len(missing)} missing file(s), first: {missing[0]}")
        bad = [p for p in paths if not _is_image(p)]
        if bad:
            raise ValueError(f"ImageFolderDataset: {source} lists a file that is no {'/'.join(EXTENSIONS)} image: {bad[0]}")
    else:
        paths = [p for p in _glob.glob(source, recursive=recursive) if _is_image(p) and os.path.isfile(p)]
    paths = sorted(paths)
    if not paths:
        return os.path.dirname(source) or ".", []
    base = os.path.commonpath([os.path.dirname(os.path.abspath(p)) for p in paths])
    return base, [os.path.abspath(p) for p in paths]


class ImageFolderDataset(Dataset):
    """`ImageFolderDataset(source, recursive=False)`: see `list_images` for what `source` may be.  An item's name is its path
    relative to the base directory without the extension ("sub/img_3" for base/sub/img_3.jpg), so outputs written under the names
    mirror the sub-directories.  Two files with one name (a.jpg next to a.png) raise here, before anything runs."""
    kind, aug = "cls", False

    def __init__(self, source, recursive=False):
        self.source, self.recursive = source, bool(recursive)
        self.base, self.paths = list_images(source, recursive)
        if not self.paths:
            raise FileNotFoundError(f"ImageFolderDataset: no {'/'.join(EXTENSIONS)} file in {source!r}")
        self.name_list = [os.path.splitext(os.path.relpath(p, self.base))[0].replace(os.sep, "/") for p in self.paths]
        seen = {}
        for name, path in zip(self.name_list, self.paths):
            if name in seen:
                raise ValueError(f"ImageFolderDataset: {seen[name]} and {path} would both be written as {name!r}")
            seen[name] = path

    def __len__(self):
        return len(self.paths)

    def raw(self, idx):
        return self.name_list[idx], read_image(self.paths[idx]), None, np.zeros(1, np.uint8)

    def __getitem__(self, idx):
        name, image, _, cls_label = self.raw(idx)
        return name, normalize_chw(image), cls_label

    def sizes(self):
        """[(H, W)] in dataset order, from the headers."""
        from PIL import Image
        out = []
        for p in self.paths:
            with Image.open(p) as im:
                out.append((int(im.size[1]), int(im.size[0])))
        return out
