#!/usr/bin/env python3
"""Time the crop kernel of data.crop_batch (k_image_crop, both crop sizes from one launch) at B = 256 on 1000 x 1000 frames.

    python tools/image_crop_time.py [--batch 256] [--out profiles/image_crop_time.json]

Device events around the launches after a warm-up, over at least 0.5 s of work.  Prints ms per batch and
(block bytes read + bytes written) / time beside the 6.29 TB/s copy rate of an MI355X.  The bytes read are the uploaded blocks
(regions of interest), counted once: a workgroup re-reads source rows that its neighbours read too, from cache.  Bounding boxes:
the seeded classes of tests/image_cases.py (`mixed`) and, separately, full-frame boxes (`full`: every sample reads its whole frame).
No threshold: the number is recorded for what it is."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
COPY_RATE_TBS = 6.29


def measure(d, frames, bboxes, dev, min_seconds):
    B = len(frames)
    rois = d.crop_roi(bboxes, 1000, 1000)
    pix, desc = d.pack_frames(frames, rois)
    pix, desc, bb = pix.to(dev), desc.to(dev), bboxes.to(dev).contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    run = lambda: d.image_crop(pix, desc, bb, (224, 256), d.SPIN_NORMALIZE, status)      # noqa: E731
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, ms = 20, 0.0
    while True:
        start.record()
        for _ in range(reps):
            run()
        stop.record()
        stop.synchronize()
        ms = start.elapsed_time(stop)
        if ms >= 1000 * min_seconds:
            break
        reps *= 4
    assert int(status.item()) == 0
    written = B * 3 * 4 * (224 ** 2 + 256 ** 2)
    per = ms / reps
    return {'batch': B, 'launches_timed': reps, 'ms_per_batch': per, 'block_bytes_read': int(pix.numel()), 'bytes_written': written,
            'tb_per_s': (pix.numel() + written) / (per * 1e-3) / 1e12, 'copy_rate_tb_per_s': COPY_RATE_TBS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--min_seconds', type=float, default=0.5)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'image_crop_time.json'))
    a = ap.parse_args()
    import image_cases as ic
    d = importlib.import_module('joint-regressor-refinement_amd.data')
    dev = 'cuda:0'
    big = ic.large_frames()
    frames = [(big['noise'] if i % 2 else big['smooth'])[:1000, :1000] for i in range(a.batch)]
    classes = torch.from_numpy(ic.large_bboxes()[:35])
    res = {'device': torch.cuda.get_device_name(0), 'kernel': 'k_image_crop, sizes 224 + 256 in one launch, normalised 224 crop'}
    res['mixed'] = measure(d, frames, classes[torch.arange(a.batch) % 35], dev, a.min_seconds)
    res['full'] = measure(d, frames, torch.tensor([[0., 0., 1000., 1000.]]).repeat(a.batch, 1), dev, a.min_seconds)
    for k in ('mixed', 'full'):
        r = res[k]
        print(f"{k:<6s} B={r['batch']}: {r['ms_per_batch']:.4f} ms per batch, {r['block_bytes_read'] / 1e6:.1f} MB read + {r['bytes_written'] / 1e6:.1f} MB "
              f"written -> {r['tb_per_s']:.3f} TB/s (copy rate {COPY_RATE_TBS} TB/s)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
