#!/usr/bin/env python
"""The fused 2x2 token merge + LayerNorm (dxa_downsample_layernorm_fwd/bwd) against the unfused alternative — a device gather into
the merged layout, dxa_layernorm_fwd/bwd on it, a gather back — at the NaVILA projector's real shape (N = 64 frames, 27 x 27 grid,
C = 1152, bf16), in one process, the two alternating round by round (device events around 20 calls each; median and spread over
the rounds).  Also counts the kernel launches of one NaVILA training step at the shapes of tests/golden/navila_t1.npz.

    python scripts/navila_downsample_bench.py [out.txt]
"""
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexbotic_amd import kernels as K  # noqa: E402

DEV = "cuda"


def merged(x, G):
    N, _, C_ = x.shape
    Gp = G + (G & 1)
    h = Gp // 2
    g = F.pad(x.view(N, G, G, C_), (0, 0, 0, Gp - G, 0, Gp - G))
    return g.view(N, h, 2, h, 2, C_).permute(0, 3, 1, 2, 4, 5).reshape(N, h * h, 4 * C_)          # the gather (a copy)


def unmerged(dm, N, G, C_):
    Gp = G + (G & 1)
    h = Gp // 2
    g = dm.view(N, h, h, 2, 2, C_).permute(0, 2, 3, 1, 4, 5).reshape(N, Gp, Gp, C_)
    return g[:, :G, :G].reshape(N, G * G, C_)                                                      # the gather back (a copy)


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def bench(lines):
    N, G, C_ = 64, 27, 1152
    h = (G + 1) // 2
    torch.manual_seed(0)
    x = torch.randn(N, G * G, C_, device=DEV).bfloat16()
    w = (1 + 0.1 * torch.randn(4 * C_, device=DEV)).bfloat16()
    b = (0.1 * torch.randn(4 * C_, device=DEV)).bfloat16()
    dy = torch.randn(N, h * h, 4 * C_, device=DEV).bfloat16()
    y, mean, rstd = K.downsample_layernorm_fwd(x, w, b, 1e-5)
    xm = merged(x, G)
    y2, mean2, rstd2 = K.layernorm_fwd(xm, w, b, 1e-5)
    lines.append(f"outputs: y max |fused - unfused| {(y.float() - y2.float()).abs().max().item():.3e}")

    def fused_fwd():
        K.downsample_layernorm_fwd(x, w, b, 1e-5)

    def unfused_fwd():
        K.layernorm_fwd(merged(x, G), w, b, 1e-5)

    def fused_bwd():
        dx, part = K.downsample_layernorm_bwd(dy, x, w, mean, rstd)
        K.colsum(part)

    def unfused_bwd():
        dm, part = K.layernorm_bwd(dy, merged(x, G), w, mean2, rstd2, return_part=True)
        K.colsum(part)
        unmerged(dm, N, G, C_)

    dx1, _ = K.downsample_layernorm_bwd(dy, x, w, mean, rstd)
    dm, _ = K.layernorm_bwd(dy, xm, w, mean2, rstd2, return_part=True)
    lines.append(f"outputs: dx max |fused - unfused| {(dx1.float() - unmerged(dm, N, G, C_).float()).abs().max().item():.3e}")
    fns = dict(fused_fwd=fused_fwd, unfused_fwd=unfused_fwd, fused_bwd=fused_bwd, unfused_bwd=unfused_bwd)
    for f in fns.values():
        timed(f, 5)                                                    # warm up every shape
    t = {k: [] for k in fns}
    for _ in range(15):                                                # alternate the candidates round by round
        for k, f in fns.items():
            t[k].append(timed(f))
    byt = N * G * G * C_ * 2
    out_b = N * h * h * 4 * C_ * 2
    need = dict(fused_fwd=byt + out_b, unfused_fwd=byt + out_b, fused_bwd=2 * byt + out_b, unfused_bwd=2 * byt + out_b)
    lines.append(f"N={N} G={G} C={C_} bf16: us per call (device events, 20 calls per round, 15 alternating rounds)")
    for k, v in t.items():
        med = statistics.median(v)
        lines.append(f"  {k:12s} median {med:8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}   "
                     f"(bytes the operation needs: {need[k] / 1e6:.0f} MB -> {need[k] / med / 1e6:.2f} TB/s at the median)")


def launches(lines):
    """kernel launches of one training step at the golden fixture's shapes (torch's profiler, device activity)"""
    from torch.profiler import ProfilerActivity, profile
    sys.path.insert(0, os.path.join(ROOT))
    from tests.test_navila_gpu import batch, build, load
    g, w = load(os.path.join(ROOT, "tests", "golden"))
    m = build(g, w, "bfloat16")
    m.train()

    def step():
        m.store.begin_step()
        out = m(**batch(g))
        out.loss.backward()
        torch.cuda.synchronize()

    step()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
    n = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.key
            and "Memset" not in e.key)
    lines.append(f"kernel launches of one NaVILA training step (forward + backward, bf16, fixture shapes): {n}")


def main():
    lines = []
    bench(lines)
    try:
        launches(lines)
    except Exception as e:                                             # the profiler is optional: say so, do not guess
        lines.append(f"kernel launches of one NaVILA training step: not measured ({type(e).__name__}: {e})")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
