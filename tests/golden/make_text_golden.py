"""Generate tests/golden/text_tower.npz by RUNNING THE UNMODIFIED REFERENCE (build container only, like make_golden.py).

    python tests/golden/make_text_golden.py

Contents (data only):
  prompts_voc / prompts_coco   the WeCLIP prompts 'a clean origami {}.' of BACKGROUND_CATEGORY + new_class_names (45) and of
                               BACKGROUND_CATEGORY_COCO + new_class_names_coco (103), background first
  n_bg_voc / n_bg_coco         how many of them are background names
  ids_voc / ids_coco           the reference `clip.tokenize` of those prompts, (n, 77) int32
  feat_voc / feat_coco         the reference `CLIP.encode_text` (CPU fp32) of those ids on
                               synth.make_clip_state_dict(seed=0, text_width=512, text_layers=12)
  zs_{bg,fg}_{voc,coco}        the reference's own `zeroshot_classifier` rows for each list
  checksum                     synth.checksum of the text tower's tensors (RNG drift guard)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import refharness, synth  # noqa: E402

TEXT_SD = dict(seed=0, text_width=512, text_layers=12)
TEMPLATE = "a clean origami {}."


def text_keys(sd):
    return sorted(k for k in sd if not k.startswith("visual.") and k != "logit_scale")


def main():
    refharness.install()
    torch.manual_seed(0)
    import clip
    from clip.clip_text import BACKGROUND_CATEGORY, BACKGROUND_CATEGORY_COCO, new_class_names, new_class_names_coco
    from WeCLIP_model.model_attn_aff_voc import zeroshot_classifier
    sd = synth.make_clip_state_dict(**TEXT_SD)
    model = refharness.build_clip(sd)
    out = {"checksum": synth.checksum([sd[k] for k in text_keys(sd)])}
    for tag, bg, fg in (("voc", BACKGROUND_CATEGORY, new_class_names), ("coco", BACKGROUND_CATEGORY_COCO, new_class_names_coco)):
        prompts = [TEMPLATE.format(c) for c in list(bg) + list(fg)]
        ids = clip.tokenize(prompts)
        with torch.no_grad():
            feat = model.encode_text(ids)
            zbg = zeroshot_classifier(bg, [TEMPLATE], model)
            zfg = zeroshot_classifier(fg, [TEMPLATE], model)
        out[f"prompts_{tag}"] = np.array(prompts)
        out[f"n_bg_{tag}"] = np.int64(len(bg))
        out[f"ids_{tag}"] = ids.numpy().astype(np.int32)
        out[f"feat_{tag}"] = feat.float().numpy()
        out[f"zs_bg_{tag}"] = zbg.float().numpy()
        out[f"zs_fg_{tag}"] = zfg.float().numpy()
        print(tag, ids.shape, "eot max", int(ids.argmax(-1).max()), feat.shape)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "text_tower.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
