#!/usr/bin/env python
"""Device-event time of dxa_cross_entropy_fwd and _bwd at [512, 152064] bf16 (the LM head's loss at 512 label rows), cold: 512 MB
are written between samples, more than the 256 MB last-level cache.  One JSON line.
    python scripts/ce_bench.py [--root TREE]      # TREE: another checkout with its own built library (old against new in one job)"""
import argparse
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from dexbotic_amd import kernels as K  # noqa: E402

dev = torch.device("cuda", 0)
rows, V = 512, 152064
g = torch.Generator().manual_seed(1)
logits = (torch.randn((rows, V), generator=g) * 3.0).to(device=dev, dtype=torch.bfloat16)
labels = torch.randint(0, V, (rows,), generator=g).to(dev)
out = torch.empty_like(logits)
gs = torch.ones(1, device=dev)
big = torch.empty(512 << 20, device=dev, dtype=torch.uint8)


def once():
    big.zero_()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record()
    _, lse = K.cross_entropy_fwd(logits, labels)
    e1.record()
    K.cross_entropy_bwd(logits, labels, lse, gs, 1.0 / rows, out=out)
    e2.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, e1.elapsed_time(e2) * 1e3


for _ in range(10):
    once()
xs = [once() for _ in range(50)]
f, b = sorted(x[0] for x in xs), sorted(x[1] for x in xs)
print(json.dumps({"ce_fwd_us_median": round(f[25], 2), "ce_bwd_us_median": round(b[25], 2), "ce_fwd_us_min": round(f[0], 2),
                  "ce_bwd_us_min": round(b[0], 2), "ce_fwd_us_p90": round(f[45], 2), "ce_bwd_us_p90": round(b[45], 2),
                  "samples": 50, "shape": [rows, V], "dtype": "bf16", "cold": True}))
