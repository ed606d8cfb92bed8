#!/usr/bin/env python
"""Kernel times of the rotating augmentation policies: the crop-resize, affine and colour-jitter launches at the two sizes of
scripts/augment_bench.py (32 frames of 256 x 256 under 'pi0', 48 frames of 728 x 728 under 'dm0'), 3 warm-up calls and 20
traced ones each.  Run it under the profiler, in a run of its own, then summarise the trace per kernel and grid:
    rocprofv3 --kernel-trace --stats -d DIR -o kt --output-format csv -- python scripts/augment_kernel_trace.py
    python scripts/augment_kernel_trace.py --summarise DIR"""
import argparse
import collections
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOADS = (("pi0", 32, 256), ("dm0", 48, 728))
KERNELS = ("affine_k", "crop_hpass_k", "crop_vpass_k", "jitter_k")
WARMUP, CALLS = 3, 20


def workload():
    import torch
    from dexbotic_amd import kernels as K
    from dexbotic_amd.data.dataset.augmentations import DeviceAug
    if not torch.cuda.is_available():
        raise SystemExit("augment_kernel_trace needs the GPU")
    for policy, n, side in WORKLOADS:
        frames = torch.from_numpy(np.random.RandomState(side).randint(0, 256, (n, side, side, 3)).astype(np.uint8)).cuda()
        aug = DeviceAug(policy, p=1.0, seed=1)
        par = aug.sample(n, side, side)
        for _ in range(WARMUP + CALLS):
            resized = K.image_crop_resize(frames, par.box, aug.crop_size)
            turned = K.image_rotate(resized, par.angle)
            K.image_color_jitter(turned, par.apply_jitter, par.order, par.factors, par.hue)
        torch.cuda.synchronize()


def summarise(directory):
    rows = collections.defaultdict(list)
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if any(k in r["Kernel_Name"] for k in KERNELS):
                key = (r["Kernel_Name"][:72], r.get("Grid_Size_X", "?"), r.get("Grid_Size_Y", "?"))
                rows[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for key, v in sorted(rows.items()):
        v = v[WARMUP:]
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        print(f"{key[0]:74s} grid {key[1]:>8s} x {key[2]:>4s}  n={len(v):3d}  median {med:8.1f} us  ({q1:.1f} - {q3:.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise", default=None, metavar="DIR")
    a = ap.parse_args()
    summarise(a.summarise) if a.summarise else workload()
