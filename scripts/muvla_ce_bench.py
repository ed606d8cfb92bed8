#!/usr/bin/env python
"""MuVLA's weighted LM loss backward at the real shapes, [16 x 850, 152064] bf16: ONE launch of dxa_cross_entropy_rows_bwd (the
per-row weight w_b / (n_b B) inside the kernel) against dxa_cross_entropy_bwd followed by a second pass that scales every row
(``dz.mul_(row_w[:, None])``, the simplest form of that pass), both on this tree's library.  Device-event times, the three variants
alternating sample by sample; each call streams 2 x 4.1 GB, far more than the 256 MB last-level cache, so every sample is cold.
The unweighted backward is timed beside them: what the extra factor costs the shared kernel.  One JSON line.
    python scripts/muvla_ce_bench.py [--rows 13600] [--samples 20]"""
import argparse
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=16 * 850)
ap.add_argument("--vocab", type=int, default=152064)
ap.add_argument("--samples", type=int, default=20)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dexbotic_amd import kernels as K  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("muvla_ce_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda", 0)
rows, V, B = args.rows, args.vocab, 16
assert rows % B == 0
g = torch.Generator(device=dev).manual_seed(1)
logits = torch.empty((rows, V), device=dev, dtype=torch.bfloat16)
for lo in range(0, rows, 1024):                                  # filled in slabs: no fp32 copy of the whole matrix
    hi = min(rows, lo + 1024)
    logits[lo:hi] = torch.randn((hi - lo, V), generator=g, device=dev) * 3.0
labels = torch.randint(0, V, (rows,), generator=g, device=dev)
labels[torch.rand(rows, generator=g, device=dev) < 0.9] = -100    # ~768 of a sample's 850 rows are image rows without a label
reward = torch.randn(B, generator=g, device=dev)
out = torch.empty_like(logits)
gs = torch.ones(1, device=dev)
row_loss, lse = K.cross_entropy_fwd(logits, labels)
_, row_w = K.ce_sample_reduce(row_loss, labels, reward, B, V)
row_w_bf16 = row_w.to(torch.bfloat16)[:, None]


def fused():
    K.cross_entropy_rows_bwd(logits, labels, lse, gs, 1.0, row_w, out=out)


def two_pass():
    K.cross_entropy_bwd(logits, labels, lse, gs, 1.0, out=out)
    out.mul_(row_w_bf16)


def unweighted():
    K.cross_entropy_bwd(logits, labels, lse, gs, 1.0 / rows, out=out)


def timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


variants = {"fused_rows_bwd": fused, "bwd_then_row_scale": two_pass, "unweighted_bwd": unweighted}
for _ in range(3):
    for fn in variants.values():
        timed(fn)
xs = {k: [] for k in variants}
for _ in range(args.samples):
    for k, fn in variants.items():
        xs[k].append(timed(fn))
res = {"shape": [rows, V], "dtype": "bf16", "samples": args.samples, "logits_gb": round(rows * V * 2 / 1e9, 2)}
for k, v in xs.items():
    v = sorted(v)
    res[k + "_us"] = {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}
print(json.dumps(res))
