#!/usr/bin/env python
"""OFT at full size: the head's fused LayerNorm and the in-place query insertion against the compositions they replace, one training
step and the action request.

Size: CLIP ViT-L/14 at 224 px and a 32-token prompt (S = 287 spliced rows) as bench.py, Qwen2.5-7B-class decoder (d 3584, 28 layers),
action_dim 7, chunk_size 16: Q = 112 query rows behind each sample, S + Q = 399, the head's rows 7 x 3584 = 25,088 columns wide, 256
of them at batch 16.  bf16 compute, synthetic data, random-init weights.

Measurements, written to the file given with --out (profiles/oft_head.txt); device events, the two sides of a pair alternated
in one process, medians and the spread (max - min over the rounds) of each side:
 1. ``action_layernorm`` forward and backward (with the dxa_colsum fold of dw | db) against (a) the composition of existing launches
    the issue names: ``gather_rows`` + ``layernorm_fwd`` / ``layernorm_bwd`` + ``scatter_rows``, and (b) the same with the scatter
    replaced by a zero fill and one ``copy2d`` per sample (``scatter_rows`` scans the whole index list per element: it was written
    for one row per sample);
 2. ``action_put`` against a copy-based insertion: a zero-filled [B, S + Q, d] buffer, the spliced [B, S, d] rows and the query rows
    copied in per sample (``insert_action_embedding`` as the reference writes it);
 3. one training step (NativeTrainer) of OFTForCausalLM, ms;
 4. ``inference_action`` p50 over varied requests.

    python scripts/oft_bench.py [--batch 16] [--reqs 10] [--steps 5] [--kernels-only] [--out profiles/oft_head.txt]
"""
import argparse
import gc
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EPS = 1e-5
D, A, T, S = 3584, 7, 16, 287


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def alternate(lines, name, sides, reps=10, rounds=9):
    """sides: [(label, fn, reps or None)]; every round times each side once, in order"""
    for _, f, _r in sides:
        timed(f, 2)
    t = {label: [] for label, _, _ in sides}
    for _ in range(rounds):
        for label, f, r in sides:
            t[label].append(timed(f, r or reps))
    base = statistics.median(t[sides[0][0]])
    lines.append(f"   {name}")
    for label, _, _ in sides:
        m = statistics.median(t[label])
        lines.append(f"      {label:58s} median {m:9.1f} us   spread {max(t[label]) - min(t[label]):8.1f} us   x{m / base:7.2f}")


def kernel_bench(lines, B):
    from dexbotic_amd import kernels as K
    dev, bf = "cuda", torch.bfloat16
    torch.manual_seed(0)
    Q = T * A
    Sq, cols = S + Q, A * D
    off_h = torch.full((B,), S, dtype=torch.int64)
    off_h[1::2] -= 5                                            # every other sample five rows shorter
    off = off_h.to(dev)
    h = torch.randn(B, Sq, D, device=dev).to(bf)
    w, b = (1 + 0.1 * torch.randn(cols, device=dev)).to(bf), (0.1 * torch.randn(cols, device=dev)).to(bf)
    dy = torch.randn(B * T, cols, device=dev).to(bf)
    idx = torch.cat([bb * Sq + off_h[bb] + torch.arange(Q) for bb in range(B)]).to(dev)
    h2 = h.view(B * Sq, D)
    y, mean, rstd = K.action_layernorm_fwd(h, off, w, b, T, A, False, EPS)
    rows = K.gather_rows(h2, idx, bf).view(B * T, cols)
    y0, mean0, rstd0 = K.layernorm_fwd(rows, w, b, EPS)
    lines.append(f"   (fused and composed forward agree: max |dy| {float((y.float() - y0.float()).abs().max()):.3e}, "
                 f"mean {float((mean - mean0).abs().max()):.3e})")

    def fused_fwd():
        return K.action_layernorm_fwd(h, off, w, b, T, A, False, EPS)

    def comp_fwd():
        return K.layernorm_fwd(K.gather_rows(h2, idx, bf).view(B * T, cols), w, b, EPS)

    def fused_bwd():
        dh, part = K.action_layernorm_bwd(dy, h, off, w, mean, rstd, T, A, False)
        return dh, K.colsum(part)

    def comp_bwd_core():
        dx, part = K.layernorm_bwd(dy, rows, w, mean0, rstd0, return_part=True)
        return dx, K.colsum(part)

    def comp_bwd_scatter():
        dx, s = comp_bwd_core()
        return K.scatter_rows(dx.view(B * Q, D), idx, B * Sq, bf), s

    def comp_bwd_copy():
        dx, s = comp_bwd_core()
        dh = torch.zeros(B * Sq, D, device=dev, dtype=bf)
        dxr = dx.view(B, Q, D)
        for bb in range(B):
            o = bb * Sq + int(off_h[bb])
            K.copy2d(dxr[bb], dh[o:o + Q], D, D)
        return dh, s

    a, _ = fused_bwd()
    c, _ = comp_bwd_copy()
    lines.append(f"   (fused and composed backward agree: max |d dh| {float((a.view(-1).float() - c.view(-1).float()).abs().max()):.3e})")
    lines.append(f"1. action_layernorm on h [{B}, {Sq}, {D}] bf16 -> [{B * T}, {cols}]: us per call")
    alternate(lines, "forward", [("action_layernorm_fwd", fused_fwd, None), ("gather_rows + layernorm_fwd", comp_fwd, None)])
    alternate(lines, "backward (dh complete, dw | db folded)",
              [("action_layernorm_bwd + colsum", fused_bwd, None),
               ("layernorm_bwd + colsum + zero fill + copy2d per sample", comp_bwd_copy, None),
               ("layernorm_bwd + colsum + scatter_rows", comp_bwd_scatter, 1)], rounds=5)

    # ---- action_put against a copy-based insertion
    query = (0.05 * torch.randn(Q, D, device=dev)).to(bf)
    spliced = torch.randn(B, S, D, device=dev).to(bf)
    x = torch.zeros(B, Sq, D, device=dev, dtype=bf)

    def put():
        return K.action_put_(x, query, off)

    def copy_insert():
        out = torch.zeros(B, Sq, D, device=dev, dtype=bf)
        for bb in range(B):
            n = int(off_h[bb])
            K.copy2d(spliced[bb, :n], out[bb, :n], D, D)
            K.copy2d(query, out[bb, n:n + Q], D, D)
        return out
    lines.append(f"2. action_put: {Q} query rows into x [{B}, {Sq}, {D}] bf16 in place, against a copy-based insertion: us per call")
    alternate(lines, "forward", [("action_put_fwd (rows reserved by the splice)", put, None),
                                 ("zero fill + copy of the spliced rows + copy of the query rows", copy_insert, None)])


def model_bench(a, lines):
    from dexbotic_amd.engine import OptimConfig
    from dexbotic_amd.model import OFTConfig, OFTForCausalLM
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    from dexbotic_amd.trainer import NativeTrainer
    dev = torch.device("cuda", 0)
    cfg = OFTConfig(llm_config=Qwen2Config(), mm_vision_tower=CLIPVisionConfig(), mm_projector_type="mlp2x_gelu",
                    action_model_type="Linear", action_dim=A, chunk_size=T, use_proprio=True, proprio_dim=8, compute_dtype="bfloat16")
    m = OFTForCausalLM(cfg, device=dev, train=True)
    m.init_random_(seed=0)
    g = torch.Generator().manual_seed(1)

    def request(B):
        ids = torch.randint(1000, 30000, (B, 32), generator=g)
        ids[:, 1] = -200
        return ids, torch.randn(B, 3, 224, 224, generator=g).clamp_(-2.5, 2.5).to(dev), torch.randn(B, 8, generator=g).to(dev)
    m.train()
    tr = NativeTrainer(m, OptimConfig(base_lr=2.5e-5, max_grad_norm=1.0), total_steps=1000)
    ids, images, states = request(a.batch)
    batch = dict(input_ids=ids, attention_mask=torch.ones(a.batch, 32, dtype=torch.bool), images=images, states=states,
                 actions=(torch.rand(a.batch, T * A, generator=g) * 2 - 1).to(dev))
    for _ in range(2):
        loss = tr.step(batch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        loss = tr.step(batch)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    lines.append(f"3. OFT training step, batch {a.batch}, S + Q = {S + T * A + 1}: median {statistics.median(ts):7.1f} ms  min {min(ts):7.1f}  "
                 f"max {max(ts):7.1f} over {a.steps} steps; loss {float(loss):.4f}; {m.store.total / 1e9:.3f} B parameters")
    m.eval()
    norms = {"min": [-1.0] * A, "max": [1.0] * A}
    lat = []
    for i in range(a.reqs + 2):
        ids, images, states = request(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.inference_action(ids, images, {"action_norms": norms, "states": states})
        lat.append(1e3 * (time.perf_counter() - t0))
    lat = lat[2:]
    lines.append(f"4. OFT inference_action, B=1, one decoder pass over {S + T * A + 1} rows, eager launches: p50 {np.median(lat):7.1f} ms  "
                 f"min {min(lat):7.1f}  max {max(lat):7.1f} over {len(lat)} varied requests")
    del tr, m
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reqs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [__doc__.split("\n\n")[0], __doc__.split("\n\n")[1], ""]
    kernel_bench(lines, a.batch)
    if not a.kernels_only:
        model_bench(a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("oft_bench: needs the GPU (no timing is taken on a CPU)")
    main()
