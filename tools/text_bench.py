"""Time CLIP.encode_text on the GPU (csrc/text.hip + the block GEMMs): the VOC (45) and COCO (103) prompt counts, truncated
to max(eot) + 1 = 13 positions (what the WeCLIP prompts need) and at the full 77, ViT-B/16-shaped text tower
(width 512, 12 layers, 8 heads) from synth seed 0.  Median of --reps timed calls after --warmup, HIP events.
    python tools/text_bench.py [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from weclip_vit_comer_amd import config, synth
    from weclip_vit_comer_amd.clip import load
    model, _ = load(synth.make_clip_state_dict(seed=0, text_width=512, text_layers=12), device="cuda")
    rows = []
    for prec in ("fast", "exact"):
        config.precision = prec
        for n in (45, 103):
            ids = torch.zeros(n, 77, dtype=torch.int32)
            ids[:, 0] = 49406
            ids[:, 1:12] = torch.randint(1, 49000, (n, 11), generator=torch.Generator().manual_seed(n))
            ids[:, 12] = 49407                        # EOT at index 12: 13 positions, like the longest WeCLIP prompt
            ids = ids.cuda()
            for full in (False, True):
                for _ in range(a.warmup):
                    model.encode_text(ids, full_context=full)
                ts = []
                for _ in range(a.reps):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    s.record()
                    model.encode_text(ids, full_context=full)
                    e.record()
                    torch.cuda.synchronize()
                    ts.append(s.elapsed_time(e))
                ts.sort()
                L = 77 if full else 13
                flop = n * L * 12 * (2 * 512 * 512 * 12) + n * 12 * 8 * 2 * 2 * L * (L + 1) / 2 * 64
                rows.append(dict(precision=prec, prompts=n, positions=L, ms_median=round(ts[len(ts) // 2], 3),
                                 ms_min=round(ts[0], 3), gflop=round(flop / 1e9, 1)))
                print(json.dumps(rows[-1]), flush=True)


if __name__ == "__main__":
    main()
