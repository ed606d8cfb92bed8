#!/usr/bin/env python
"""DM0 at an assumed DM0-base size: the sampler's suffix split at an offset against the sequence it replaces, the action request
with the graph on and off, and one training step.

ASSUMPTION, not read from a checkpoint (DM0-base is not available here): both experts take the attention geometry of HF's
Qwen3-1.7B config (28 layers, 16 query / 8 key-value heads x 128); the llm is Qwen3-1.7B (d 2048, F 6144), the action expert a
narrower decoder (d 1024, F 3072); CLIP ViT-L/14 at 224 px (256 tokens per camera).  Prefix = 3 cameras' tokens + 48 text tokens,
chunk 50, action_dim 32, bf16 compute.  Synthetic data, random-init weights.

Three measurements, written to the file given with --out (profiles/dm0_sampler.txt):
 1. one layer's suffix pass, us (device events, alternating rounds): ``qknorm_rope_split_into`` at kv0 = P into the layer's
    [B, Hkv, P + chunk, D] buffer, against ``qknorm_rope_split`` + the two ``torch.cat`` over the cached prefix K / V that a sampler
    built from the offset-free kernel needs per layer and per Euler step;
 2. ``inference_action`` p50 over varied requests (a different prompt, images and initial noise each), graph replay on and off;
 3. one training step (NativeTrainer), ms.

    python scripts/dm0_bench.py [--layers 28] [--batch 4] [--reqs 10] [--steps 3] [--out profiles/dm0_sampler.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EPS = 1e-6


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def split_bench(a, P, lines):
    from dexbotic_amd import kernels as K
    dev = "cuda"
    B, S, Hq, Hkv, D = 1, a.chunk, a.heads, a.kv_heads, a.head_dim
    torch.manual_seed(0)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=dev).bfloat16()
    wq = (0.5 + torch.rand(D, device=dev)).bfloat16()
    wk = (0.5 + torch.rand(D, device=dev)).bfloat16()
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    fr = torch.arange(P + S, dtype=torch.float32)[:, None] * inv[None]
    cos_t, sin_t = fr.cos().to(dev).contiguous(), fr.sin().to(dev).contiguous()
    pos = torch.arange(P, P + S, dtype=torch.int32, device=dev).repeat(B)
    kbuf = torch.randn(B, Hkv, P + S, D, device=dev).bfloat16()
    vbuf = torch.randn(B, Hkv, P + S, D, device=dev).bfloat16()
    kpre, vpre = kbuf[:, :, :P].contiguous(), vbuf[:, :, :P].contiguous()
    q = torch.empty(B, Hq, S, D, device=dev, dtype=torch.bfloat16)
    geo = (B, S, Hq, Hkv, D)

    def at_offset():
        K.qknorm_rope_split_into(qkv, q, kbuf, vbuf, 0, P, wq, wk, EPS, cos_t, sin_t, pos, *geo, want_rstd=False)

    def split_and_cat():
        q_, k_, v_, _ = K.qknorm_rope_split(qkv, wq, wk, EPS, cos_t, sin_t, pos, *geo, want_rstd=False)
        return q_, torch.cat([kpre, k_], dim=2), torch.cat([vpre, v_], dim=2)

    at_offset()
    q2, k2, v2 = split_and_cat()
    same = torch.equal(q, q2) and torch.equal(kbuf, k2) and torch.equal(vbuf, v2)
    fns = dict(at_offset=at_offset, split_and_cat=split_and_cat)
    for f in fns.values():
        timed(f, 5)
    t = {k: [] for k in fns}
    for _ in range(15):
        for k, f in fns.items():
            t[k].append(timed(f))
    lines.append(f"1. one layer's suffix pass, B={B} chunk={S} behind P={P} cached keys, Hq={Hq} Hkv={Hkv} D={D} bf16: us per call "
                 f"(device events, 20 calls per round, 15 alternating rounds); results identical: {same}")
    for k, v in t.items():
        lines.append(f"   {k:14s} median {statistics.median(v):7.1f} us  min {min(v):7.1f}  max {max(v):7.1f}")
    lines.append(f"   split_and_cat / at_offset at the medians: {statistics.median(t['split_and_cat']) / statistics.median(t['at_offset']):.2f}"
                 f"   (per action chunk this pass runs {a.layers} layers x 10 steps = {a.layers * 10} times)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--inter", type=int, default=6144)
    ap.add_argument("--action-hidden", type=int, default=1024)
    ap.add_argument("--action-inter", type=int, default=3072)
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--text", type=int, default=48)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reqs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dexbotic_amd.engine import OptimConfig
    from dexbotic_amd.model import DM0Config, DM0ForCausalLM
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    from dexbotic_amd.trainer import NativeTrainer
    dev = torch.device("cuda", 0)
    q3 = dict(model_type="qwen3", vocab_size=a.vocab, num_hidden_layers=a.layers, num_attention_heads=a.heads,
              num_key_value_heads=a.kv_heads, head_dim=a.head_dim, rms_norm_eps=1e-6, rope_theta=1e6, max_position_embeddings=40960)
    vis = CLIPVisionConfig()                                                   # ViT-L/14 at 224 px: 256 tokens per camera
    cfg = DM0Config(llm_config=dict(q3, hidden_size=a.hidden, intermediate_size=a.inter),
                    action_config=dict(q3, hidden_size=a.action_hidden, intermediate_size=a.action_inter), mm_vision_tower=vis,
                    action_dim=32, chunk_size=a.chunk, bf16=True)
    CAM = 3
    P = CAM * (vis.image_size // vis.patch_size) ** 2 + a.text
    lines = [__doc__.split("\n\n")[0], __doc__.split("\n\n")[1], ""]
    split_bench(a, P, lines)

    m = DM0ForCausalLM(cfg, device=dev, train=True)
    m.init_random_(seed=0)
    lines.append(f"model: {m.store.total / 1e9:.3f} B parameters, {a.layers} layers, prefix {P}, chunk {a.chunk}")
    g = torch.Generator().manual_seed(1)

    def request(B):
        return dict(input_ids=torch.randint(1000, 30000, (B, a.text), generator=g).to(dev),
                    attention_mask=torch.ones(B, a.text, dtype=torch.bool),
                    images=torch.randn(B, CAM, 3, 224, 224, generator=g).clamp_(-2.5, 2.5).to(dev),
                    image_masks=torch.ones(B, CAM, dtype=torch.bool), states=torch.randn(B, 32, generator=g).to(dev))
    # ---- 2. the action request
    m.eval()
    for use_graph in (False, True):
        lat = []
        for i in range(a.reqs + 3):                                            # (graph: eager, capture, first replay are warm-up)
            r = request(1)
            noise = torch.randn(1, a.chunk, 32, generator=g).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.inference_action(diffusion_steps=10, noise=noise, use_graph=use_graph, **r).cpu()
            lat.append(1e3 * (time.perf_counter() - t0))
        lat = lat[3:]
        lines.append(f"2. inference_action, B=1, 10 Euler steps, graph {'on ' if use_graph else 'off'}: p50 {np.median(lat):7.1f} ms  "
                     f"min {min(lat):7.1f}  max {max(lat):7.1f}  over {len(lat)} varied requests")
    # ---- 3. one training step
    m.train()
    tr = NativeTrainer(m, OptimConfig(base_lr=2.5e-5, weight_decay=1e-10, adam_beta2=0.95, max_grad_norm=1.0), total_steps=1000)
    batch = dict(request(a.batch), actions=torch.randn(a.batch, a.chunk, 32, generator=g).to(dev))
    for _ in range(2):
        loss = tr.step(batch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        loss = tr.step(batch)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    lines.append(f"3. training step, batch {a.batch}: median {statistics.median(ts):7.1f} ms  min {min(ts):7.1f}  max {max(ts):7.1f} "
                 f"over {a.steps} steps; loss {float(loss):.4f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("dm0_bench: needs the GPU (no timing is taken on a CPU)")
    main()
