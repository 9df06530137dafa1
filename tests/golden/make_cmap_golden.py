"""Generate tests/golden/voc_cmap.npz: the 256 x 3 uint8 PASCAL VOC label colour table the reference's prediction_cmap/*.png
files are painted with (`utils.imutils.encode_cmap` -> `colormap()`, utils/imutils.py:136-154).  Build container only.

    python tests/golden/make_cmap_golden.py

The table is RECORDED FROM THE REFERENCE'S OWN `colormap()` (imported through oracle/refharness.py, whose stubs stand in for
the torchvision import at the top of that module).  Where that module does not import (no matplotlib, no reference checkout),
the table is recorded from the VOC devkit definition instead (VOCdevkit/VOCcode/VOClabelcolormap.m: for j = 0..7, bit 0 / 1 /
2 of the label are or-ed into bit 7 - j of r / g / b and the label is shifted right by 3) and `source` says so.  When both
are available they are checked against each other.

Contents (data only):
  cmap     (256, 3) uint8, row v = (r, g, b) of label v
  source   "reference colormap()" or "VOC devkit definition"
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def devkit_table():
    t = np.zeros((256, 3), np.uint8)
    for v in range(256):
        c = v
        for j in range(8):
            for ch in range(3):
                t[v, ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
    return t


def reference_table():
    from oracle import refharness
    refharness.install()
    from utils import imutils
    return np.asarray(imutils.colormap(), dtype=np.uint8)


def main():
    dev = devkit_table()
    try:
        cmap, source = reference_table(), "reference colormap()"
        assert cmap.shape == (256, 3) and np.array_equal(cmap, dev), "the reference's table differs from the devkit definition"
    except (ImportError, RuntimeError) as e:
        print(f"reference colormap() not importable here ({e}); recording the VOC devkit definition")
        cmap, source = dev, "VOC devkit definition"
    assert cmap[[0, 1, 2, 15, 255]].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [192, 128, 128], [224, 224, 192]]
    out = os.path.join(ROOT, "tests", "golden", "voc_cmap.npz")
    np.savez(out, cmap=cmap, source=np.array(source))
    print(f"wrote {out}: {source}")


if __name__ == "__main__":
    main()
