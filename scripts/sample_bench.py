#!/usr/bin/env python
"""One token choice over the full vocabulary — a [1, 152064] bf16 row, T = 0.7, top_k = 50 — three ways in one process:
dxa_sample_rows, the ATen sequence generate() used before it (softmax(logits.float() / T) + multinomial: the full-vocabulary
distribution, no top-k), and dxa_argmax_rows as an anchor (the sampler reads the row several times, argmax once).  Each call is
timed by a pair of device events; 20 warm-up calls, 200 timed calls per candidate, the candidates alternating call by call;
median, min and max.

    python scripts/sample_bench.py [out.txt]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexbotic_amd import kernels as K  # noqa: E402

DEV = "cuda"
V, T_, TOP_K = 152064, 0.7, 50
WARM, TIMED = 20, 200


def main():
    assert torch.cuda.is_available(), "sample_bench.py measures on the GPU; there is nothing to report without one"
    g = torch.Generator(device=DEV).manual_seed(0)
    logits = (2.5 * torch.randn(1, V, device=DEV, generator=g)).bfloat16()
    u = torch.rand(1, device=DEV, generator=g)

    def hip_sample():
        return K.sample_rows(logits, u, T_, TOP_K, 1.0)

    def aten_sample():
        probs = torch.softmax(logits.float() / T_, dim=-1)
        return torch.multinomial(probs, 1, generator=g).view(-1)

    def hip_argmax():
        return K.argmax_rows(logits)

    fns = {"dxa_sample_rows (T 0.7, top_k 50)": hip_sample, "ATen softmax + multinomial (T 0.7)": aten_sample,
           "dxa_argmax_rows": hip_argmax}
    for f in fns.values():
        for _ in range(WARM):
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(TIMED)] for k in fns}
    for i in range(TIMED):
        for k, f in fns.items():
            e0, e1 = ev[k][i]
            e0.record()
            f()
            e1.record()
    torch.cuda.synchronize()
    tok, kept, thresh, prob = K.sample_rows(logits, u, T_, TOP_K, 1.0, return_info=True)
    lines = [f"one token choice over [1, {V}] bf16 logits: us per call (a device-event pair per call, {WARM} warm-up + {TIMED} timed "
             f"calls per candidate, alternating call by call, one process)",
             f"  dxa_sample_rows kept {int(kept)} entries, smallest kept logit {float(thresh):.4f}, returned token {int(tok)} "
             f"with probability {float(prob):.4f}"]
    stats = {}
    for k in fns:
        t = [1e3 * a.elapsed_time(b) for a, b in ev[k]]
        stats[k] = (statistics.median(t), min(t), max(t))
        lines.append(f"  {k:36s} median {stats[k][0]:8.1f}  min {stats[k][1]:8.1f}  max {stats[k][2]:8.1f}")
    (ms, mns, _), (ma, mna, _) = (stats[k] for k in list(fns)[:2])
    spread = max(ms - mns, ma - mna)
    lines.append(f"  bar: the kernel's median must not exceed ATen's beyond the run's own min-to-median spread ({spread:.1f} us): "
                 f"{ms:.1f} vs {ma:.1f} -> {'met' if ms <= ma + spread else 'MISSED: the kernel is slower than ATen'}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
