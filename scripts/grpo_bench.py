"""Time the GRPO policy head at the real width, forward + backward, in two formulations of the SAME loss:

  A  functional.BinPolicyLossFn: the last NB = num_bins - 1 rows of lm_head.weight as their own [NB, d] operand, dxa_bin_logprob_fwd /
     dxa_ppo_clip_fwd / dxa_bin_logprob_bwd; nothing V wide exists.
  B  what the package could do before: the full-vocabulary logits with K.mm_nt, the column slice, the loss in torch ops, and the
     head's backward as _lm_head_loss_bwd runs it (dW in row slabs with K.mm_tn, dH with K.mm_nn) on the [rows, V] gradient that
     autograd builds from the slice.

    python scripts/grpo_bench.py [--rows 448] [--reps 30] [--warmup 5]

d = 3584, V = 152064, NB = 255, 448 action rows (8 policy calls x 8 x 7 tokens), bf16 weights.  The two formulations alternate inside
one loop, each repetition timed with device events around forward + backward; the script prints the median, the quartiles and the
extremes of both, and the distance between their losses and input gradients (they must agree to bf16 rounding: faster and different
is not faster).  One JSON line at the end.  A FLOP ratio is not a speed-up: only what this prints on an MI355X is a measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dexbotic_amd import functional as Fn  # noqa: E402
from dexbotic_amd import kernels as K  # noqa: E402
from dexbotic_amd.engine import ParamStore  # noqa: E402

DEV = "cuda"
WN = "lm_head.weight"


class FullVocabHead(torch.autograd.Function):
    """logits over the whole vocabulary and the backward of functional._lm_head_loss_bwd for a given d logits"""

    @staticmethod
    def forward(ctx, rows, anchor, st):
        ctx.st = st
        ctx.save_for_backward(rows)
        return K.mm_nt(rows, st.w(WN))

    @staticmethod
    def backward(ctx, dz):
        st = ctx.st
        (rows,) = ctx.saved_tensors
        dz = dz.contiguous()
        g, acc = st.g(WN), st.accum_flag(WN)
        V, d = g.shape
        slab = max(256, min(V, Fn.LMHEAD_SLAB_BYTES // (4 * d) // 256 * 256))
        for lo in range(0, V, slab):
            hi = min(V, lo + slab)
            K.mm_tn(dz[:, lo:hi], rows, out=g[lo:hi], accumulate=acc)
        st.mark_written(WN)
        return K.mm_nn(dz, st.w(WN)), None, None


def loss_b(rows, st, NB, bins, old, adv, mask, temperature, lo, hi, denom):
    z = FullVocabHead.apply(rows, st.params[WN], st)
    zb = z[:, z.shape[1] - NB:].float() / temperature
    logp = torch.log_softmax(zb, dim=-1).gather(-1, bins.unsqueeze(-1)).squeeze(-1)
    ratio = torch.exp(logp - old)
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, lo, hi))
    return (pg * mask).sum() / denom


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=448)
    ap.add_argument("--d", type=int, default=3584)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--bins", type=int, default=255)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grpo_bench: needs the GPU (a timing taken anywhere else says nothing)")
    rows_n, d, V, NB = a.rows, a.d, a.vocab, a.bins
    st = ParamStore(DEV, torch.bfloat16)
    st.register([(WN, (V, d))])
    st.finalize(train=True)
    gen = torch.Generator(device=DEV).manual_seed(1)
    w = st.w32(WN)
    for lo in range(0, V, 8192):
        w[lo:lo + 8192].copy_(torch.randn((min(8192, V - lo), d), generator=gen, device=DEV) * 0.02)
    st.sync_shadow()
    rows = (torch.randn((rows_n, d), generator=gen, device=DEV) * 0.5).to(torch.bfloat16).requires_grad_(True)
    bins = torch.randint(0, NB, (rows_n,), generator=gen, device=DEV)
    old = -5.5 + 0.3 * torch.randn(rows_n, generator=gen, device=DEV)
    adv = torch.randn(rows_n, generator=gen, device=DEV)
    mask = (torch.rand(rows_n, generator=gen, device=DEV) > 0.2).float()
    temperature, clip_low, clip_high, denom = 1.6, 0.2, 0.28, float(rows_n)

    def run_a():
        st.begin_step()
        rows.grad = None
        loss, _, _, _ = Fn.BinPolicyLossFn.apply(rows, st.params[WN], st, WN, NB, bins, old, adv, mask, temperature, clip_low, clip_high, denom)
        loss.backward()
        return loss.detach(), rows.grad

    def run_b():
        st.begin_step()
        rows.grad = None
        loss = loss_b(rows, st, NB, bins, old, adv, mask, temperature, 1.0 - clip_low, 1.0 + clip_high, denom)
        loss.backward()
        return loss.detach(), rows.grad

    times = {"A": [], "B": []}
    outs = {}
    for i in range(a.warmup + a.reps):
        for name, fn in (("A", run_a), ("B", run_b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss, dh = fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
            outs[name] = (loss.float().item(), dh.float().clone(), st.g(WN)[V - NB:].clone())
    res = dict(rows=rows_n, d=d, vocab=V, bins=NB, reps=a.reps, warmup=a.warmup)
    for name, ts in times.items():
        t = torch.tensor(sorted(ts), dtype=torch.float64)
        q = torch.quantile(t, torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)).tolist()
        res[name] = dict(median_ms=q[1], q25_ms=q[0], q75_ms=q[2], min_ms=float(t[0]), max_ms=float(t[-1]))
        print(f"{name}: median {q[1]:.3f} ms, quartiles {q[0]:.3f} - {q[2]:.3f}, extremes {float(t[0]):.3f} - {float(t[-1]):.3f} ({len(ts)} repetitions)")
    (la, ha, wa), (lb, hb, wb) = outs["A"], outs["B"]
    res["loss_A"], res["loss_B"] = la, lb
    res["dh_rel_diff"] = float((ha - hb).abs().max() / hb.abs().max().clamp_min(1e-30))
    res["dw_bins_rel_diff"] = float((wa - wb).abs().max() / wb.abs().max().clamp_min(1e-30))
    print(f"loss A {la:.6f} B {lb:.6f}; largest difference of d rows {res['dh_rel_diff']:.3e}, of dW on the bin rows {res['dw_bins_rel_diff']:.3e} "
          "(relative to the largest entry)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
