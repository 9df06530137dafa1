"""The resampling arithmetic is written down once, in csrc/resample.h: no kernel file restates the ATen half-pixel source index
or Pillow's coefficient window.  A new consumer includes the header instead of copying."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "weclip-vit-comer_amd", "csrc")


def _files_with(*parts):
    """Sources under csrc/ with a line that holds every part, in this order."""
    hits = set()
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        for line in open(os.path.join(CSRC, name)):
            pos = 0
            for part in parts:
                pos = line.find(part, pos)
                if pos < 0:
                    break
                pos += len(part)
            else:
                hits.add(name)
    return sorted(hits)


def test_source_index_is_defined_once():
    assert _files_with("fmaxf(", "+ 0.5f) - 0.5f, 0.f)") == ["resample.h"]


def test_pillow_window_is_defined_once():
    assert _files_with("center - support + 0.5") == ["resample.h"]
