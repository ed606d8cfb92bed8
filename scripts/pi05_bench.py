#!/usr/bin/env python
"""pi0.5 at full size beside pi0: the adaptive-norm kernels against the composition they replace, one training step and the action
request of both policies in one session.

Size: SigLIP-So400m/14 at 224 px and a 48-token prompt as scripts/pi0_bench.py (prefix = 3 cameras' tokens + 48), Gemma-2B llm,
18-layer action expert d 1024 / F 4096, 8 query / 1 key-value heads x 256, chunk 50, action_dim 32, 10 Euler steps, bf16 compute.
Synthetic data, random-init weights (the dense layers of the adaptive norms included: N(0, 0.02), so scale, shift and gate are live).

Measurements, written to the file given with --out (profiles/pi05_adarms.txt):
 1. each new kernel on [16 x 50, 1024] bf16 rows, us (device events, alternating rounds), against the same arithmetic from
    ``rmsnorm_fwd`` / ``rmsnorm_bwd`` plus aten element-wise ops;
 2. one training step (NativeTrainer) of Pi05ForCausalLM and of Pi0ForCausalLM at the same size, ms;
 3. ``inference_action`` p50 of both over varied requests, graph replay on.

    python scripts/pi05_bench.py [--batch 16] [--reqs 10] [--steps 3] [--out profiles/pi05_adarms.txt]
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
EPS = 1e-6


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def kernel_bench(lines, B=16, rps=50, d=1024):
    from dexbotic_amd import kernels as K
    dev, bf = "cuda", torch.bfloat16
    torch.manual_seed(0)
    rows = B * rps
    x, br, dy, res = (torch.randn(rows, d, device=dev).to(bf) for _ in range(4))
    mod, modp = (0.3 * torch.randn(B, 3 * d, device=dev)).to(bf), (0.3 * torch.randn(B, 3 * d, device=dev)).to(bf)
    gate = modp[:, 2 * d:]
    ones = torch.ones(d, device=dev, dtype=bf)
    exp = lambda t: t.repeat_interleave(rps, dim=0)
    _, rstd, r = K.adarms_fwd(x, mod, EPS, branch=br, gate_prev=gate)
    dmod, dmodp = torch.empty_like(mod), torch.empty_like(modp)

    def c_norm(x_):                                           # rmsnorm without gain, then the modulation
        h, rs = K.rmsnorm_fwd(x_, ones, EPS)
        return h * (1 + exp(mod[:, :d])) + exp(mod[:, d:2 * d]), rs

    def c_add():
        return x + br * exp(gate)

    def c_norm_bwd(r_, residual, gated):
        g = dy * (1 + exp(mod[:, :d]))
        dr, _ = K.rmsnorm_bwd(g, r_, None, rstd, residual=residual)
        xh = r_.float() * rstd[:, None]
        ds, db = (dy.float() * xh).view(B, rps, d).sum(1), dy.float().view(B, rps, d).sum(1)
        if gated:
            return dr, ds, db, dr * exp(gate), (dr.float() * br.float()).view(B, rps, d).sum(1)
        return dr, ds, db

    pairs = [
        ("adarms_fwd", lambda: K.adarms_fwd(x, mod, EPS), lambda: c_norm(x)),
        ("adarms_fwd + gated add (the mid-layer launch)", lambda: K.adarms_fwd(x, mod, EPS, branch=br, gate_prev=gate),
         lambda: c_norm(c_add())),
        ("gated_residual_fwd", lambda: K.gated_residual_fwd(x, br, gate), c_add),
        ("adarms_bwd (+ residual)", lambda: K.adarms_bwd(dy, x, mod, rstd, dmod, residual=res), lambda: c_norm_bwd(x, res, False)),
        ("adarms_bwd + gated add (+ residual)",
         lambda: K.adarms_bwd(dy, r, mod, rstd, dmod, residual=res, branch=br, gate_prev=gate, dgate_prev=dmodp[:, 2 * d:]),
         lambda: c_norm_bwd(r, res, True)),
        ("gated_residual_bwd", lambda: K.gated_residual_bwd(dy, br, gate, dmodp[:, 2 * d:]),
         lambda: (dy * exp(gate), (dy.float() * br.float()).view(B, rps, d).sum(1))),
    ]
    lines.append(f"1. the new kernels on [{B} x {rps}, {d}] bf16 rows against rmsnorm_fwd / rmsnorm_bwd + aten element-wise ops: us per "
                 "call (device events, 20 calls per round, 11 alternating rounds; medians)")
    for name, new, old in pairs:
        for f in (new, old):
            timed(f, 5)
        t = {"new": [], "old": []}
        for _ in range(11):
            t["new"].append(timed(new))
            t["old"].append(timed(old))
        a, b = statistics.median(t["new"]), statistics.median(t["old"])
        lines.append(f"   {name:48s} kernel {a:7.1f} us   composition {b:7.1f} us   ratio {b / a:5.2f}")


def model_bench(kind, a, lines):
    from dexbotic_amd.engine import OptimConfig
    from dexbotic_amd.trainer import NativeTrainer
    dev = torch.device("cuda", 0)
    vis = dict(model_type="siglip_vision_model")                                # SiglipVisionConfig defaults = So400m/14
    if kind == "pi05":
        from dexbotic_amd.model import Pi05Config, Pi05ForCausalLM
        cfg = Pi05Config(vision_config=vis, llm_config=dict(model_type="adarms_gemma"),
                         action_config=dict(model_type="adarms_gemma", hidden_size=1024, intermediate_size=4096, use_adarms=True),
                         mm_projector_type="linear", action_dim=32, chunk_size=a.chunk, compute_dtype="bfloat16")
        m = Pi05ForCausalLM(cfg, device=dev, train=True)
    else:
        from dexbotic_amd.model.pi0.pi0_arch import Pi0Config, Pi0ForCausalLM
        cfg = Pi0Config(vision_config=vis, llm_config=dict(model_type="gemma"),
                        action_config=dict(model_type="gemma", hidden_size=1024, intermediate_size=4096),
                        mm_projector_type="linear", action_dim=32, chunk_size=a.chunk, compute_dtype="bfloat16")
        m = Pi0ForCausalLM(cfg, device=dev, train=True)
    m.init_random_(seed=0)
    for n in m.store.slots:                                                     # GemmaRMSNorm scales by (1 + w)
        if n.startswith(("model.llm.", "model.action_expert.")) and n.endswith("norm.weight"):
            m.store.w32(n).zero_()
    m.post_load()
    g = torch.Generator().manual_seed(1)

    def request(B):
        return dict(input_ids=torch.randint(1000, 30000, (B, 48), generator=g).to(dev),
                    attention_mask=torch.ones(B, 48, dtype=torch.bool),
                    images=torch.randn(B, 3, 3, 224, 224, generator=g).clamp_(-2.5, 2.5).to(dev),
                    image_masks=torch.ones(B, 3, dtype=torch.bool), states=torch.randn(B, 32, generator=g).to(dev))
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
    lines.append(f"2. {kind:5s} training step, batch {a.batch}, chunk {a.chunk}: median {statistics.median(ts):7.1f} ms  min {min(ts):7.1f}  "
                 f"max {max(ts):7.1f} over {a.steps} steps; loss {float(loss):.4f}; {m.store.total / 1e9:.3f} B parameters")
    m.eval()
    lat = []
    for i in range(a.reqs + 3):                                                 # (eager, capture, first replay are warm-up)
        r = request(1)
        noise = torch.randn(1, a.chunk, 32, generator=g).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.inference_action(diffusion_steps=10, noise=noise, **r).cpu()
        lat.append(1e3 * (time.perf_counter() - t0))
    lat = lat[3:]
    lines.append(f"3. {kind:5s} inference_action, B=1, 10 Euler steps, graph on: p50 {np.median(lat):7.1f} ms  min {min(lat):7.1f}  "
                 f"max {max(lat):7.1f} over {len(lat)} varied requests")
    del tr, m
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reqs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [__doc__.split("\n\n")[0], __doc__.split("\n\n")[1], ""]
    kernel_bench(lines)
    if not a.kernels_only:
        for kind in ("pi0", "pi05"):
            model_bench(kind, a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("pi05_bench: needs the GPU (no timing is taken on a CPU)")
    main()
