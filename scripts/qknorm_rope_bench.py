#!/usr/bin/env python
"""The fused per-head q/k RMSNorm + RoPE + split pass (dxa_qknorm_rope_split / dxa_qknorm_rope_merge) against the unfused sequence
built from the kernels that existed before it — q and k column blocks copied out of the token-major qkv, dxa_rmsnorm_fwd / _bwd on
them as [B*S*H, D] rows, the blocks copied back beside v, dxa_rope_split / dxa_rope_merge — at the shape of one Qwen3-8B layer
(B*S = 16 x 287 tokens, 32 query heads, 8 kv heads, head_dim 128, bf16), in one process, the two alternating round by round (device
events around 20 calls each; median and spread over the rounds).  The copies of the unfused form are torch's (slice + cat).

    python scripts/qknorm_rope_bench.py [out.txt]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexbotic_amd import kernels as K  # noqa: E402

DEV = "cuda"
EPS = 1e-6


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def main():
    B, S, Hq, Hkv, D = 16, 287, 32, 8, 128
    M, nq, nk = B * S, Hq * D, Hkv * D
    torch.manual_seed(0)
    qkv = torch.randn(M, (Hq + 2 * Hkv) * D, device=DEV).bfloat16()
    wq = (0.5 + torch.rand(D, device=DEV)).bfloat16()
    wk = (0.5 + torch.rand(D, device=DEV)).bfloat16()
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    fr = torch.arange(S, dtype=torch.float32)[:, None] * inv[None]
    cos_t, sin_t = fr.cos().to(DEV).contiguous(), fr.sin().to(DEV).contiguous()
    dq = torch.randn(B, Hq, S, D, device=DEV).bfloat16()
    dk = torch.randn(B, Hkv, S, D, device=DEV).bfloat16()
    dv = torch.randn(B, Hkv, S, D, device=DEV).bfloat16()
    geo = (B, S, Hq, Hkv, D)

    def fused_fwd():
        return K.qknorm_rope_split(qkv, wq, wk, EPS, cos_t, sin_t, None, *geo)

    def unfused_fwd():
        xq, xk = qkv[:, :nq].contiguous().view(M * Hq, D), qkv[:, nq:nq + nk].contiguous().view(M * Hkv, D)
        yq, rq = K.rmsnorm_fwd(xq, wq, EPS)
        yk, rk = K.rmsnorm_fwd(xk, wk, EPS)
        q, k, v = K.rope_split(torch.cat([yq.view(M, nq), yk.view(M, nk), qkv[:, nq + nk:]], 1), cos_t, sin_t, None, *geo)
        return q, k, v, (xq, xk, rq, rk)

    q1, k1, v1, rstd = fused_fwd()
    q2, k2, v2, (xq, xk, rq, rk) = unfused_fwd()

    def fused_bwd():
        dqkv, part = K.qknorm_rope_merge(dq, dk, dv, qkv, rstd, wq, wk, cos_t, sin_t, None, *geo)
        return dqkv, K.colsum(part)

    def unfused_bwd():
        g = K.rope_merge(dq, dk, dv, cos_t, sin_t, None, *geo)
        gq, gk = g[:, :nq].contiguous().view(M * Hq, D), g[:, nq:nq + nk].contiguous().view(M * Hkv, D)
        dxq, dwq = K.rmsnorm_bwd(gq, xq, wq, rq)
        dxk, dwk = K.rmsnorm_bwd(gk, xk, wk, rk)
        return torch.cat([dxq.view(M, nq), dxk.view(M, nk), g[:, nq + nk:]], 1), torch.cat([dwq, dwk])

    lines = [__doc__.split("\n\n")[0], ""]
    d1, w1 = fused_bwd()
    d2, w2 = unfused_bwd()
    lines.append("outputs, max |fused - unfused|: " + "  ".join(
        f"{n} {(a.float() - b.float()).abs().max().item():.3e}" for n, a, b in
        (("q", q1, q2), ("k", k1, k2), ("v", v1, v2), ("dqkv", d1, d2), ("dw", w1, w2))) +
        f"   (|dw| max {w2.abs().max().item():.3e}; the unfused dqkv is rounded to bf16 once more, between the two kernels)")
    fns = dict(fused_fwd=fused_fwd, unfused_fwd=unfused_fwd, fused_bwd=fused_bwd, unfused_bwd=unfused_bwd)
    for f in fns.values():
        timed(f, 5)                                                    # warm up every shape
    t = {k: [] for k in fns}
    for _ in range(15):                                                # alternate the candidates round by round
        for k, f in fns.items():
            t[k].append(timed(f))
    byt = qkv.numel() * 2                                              # one pass over qkv in bf16
    need = dict(fused_fwd=2 * byt, unfused_fwd=2 * byt, fused_bwd=3 * byt, unfused_bwd=3 * byt)
    lines.append(f"B*S={B}x{S} Hq={Hq} Hkv={Hkv} D={D} bf16: us per call (device events, 20 calls per round, 15 alternating rounds)")
    for k, v in t.items():
        med = statistics.median(v)
        lines.append(f"  {k:12s} median {med:8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}   "
                     f"(bytes the operation needs: {need[k] / 1e6:.0f} MB -> {need[k] / med / 1e6:.2f} TB/s at the median)")
    for a, b in (("fused_fwd", "unfused_fwd"), ("fused_bwd", "unfused_bwd")):
        lines.append(f"  {b} / {a} at the medians: {statistics.median(t[b]) / statistics.median(t[a]):.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("qknorm_rope_bench: needs the GPU (no timing is taken on a CPU)")
    main()
