#!/usr/bin/env python
"""OFT diffusion head at full size: the action request on the cached-prefix path against the reference's full pass per DDIM step, the
new kernels against the launches they replace, and one training step.

Size: CLIP ViT-L/14 at 224 px and a 32-token prompt (S = 287 spliced rows) as bench.py, Qwen2.5-7B-class decoder (d 3584, 28 layers),
action_dim 7, chunk_size 8: R = 56 noisy-action rows, a time row and a state row behind each sample, S + Q = 345; 10 DDIM steps.  bf16
compute, synthetic data, random-init weights.

Measurements, written to the file given with --out (profiles/oft_diffusion.txt); device events, the sides of a comparison alternated
in one process, 30 repetitions, medians and the spread (max - min) of each side:
 1. ``inference_action`` p50: ``cached`` True (one prefill of the prompt + state row into a KV cache, then 10 passes over the 57
    suffix rows) against False (the reference's algorithm: the whole model, vision tower included, once per step);
 2. each new kernel against the launches it replaces: dxa_noisy_embed_fwd against broadcast multiply + add + GELU; dxa_noisy_embed_bwd
    against act_bwd + a [d, R] x [R] product + colsum; dxa_diffusion_put_fwd against a copy-based insertion (zero fill, the spliced
    rows, the state / time / projected rows per sample); dxa_ddim_step_embed against the step as elementwise torch ops + the row copy
    + the embed;
 3. one training step (NativeTrainer) of OFTDiffusionForCausalLM at batch 16, ms (the Linear head: profiles/oft_head.txt).

    python scripts/oft_diffusion_bench.py [--batch 16] [--reps 30] [--steps 5] [--kernels-only] [--out profiles/oft_diffusion.txt]
"""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
D, A, T, S = 3584, 7, 8, 287
R = A * T


def alternate(lines, name, sides, reps, inner=1, unit="us"):
    """sides: [(label, fn)]; every repetition times each side once (``inner`` calls between two device events), in order"""
    scale = 1e3 if unit == "us" else 1.0
    for _, f in sides:
        f()
    torch.cuda.synchronize()
    t = {label: [] for label, _ in sides}
    for _ in range(reps):
        for label, f in sides:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(inner):
                f()
            e1.record()
            torch.cuda.synchronize()
            t[label].append(scale * e0.elapsed_time(e1) / inner)
    base = statistics.median(t[sides[0][0]])
    lines.append(f"   {name}")
    for label, _ in sides:
        m = statistics.median(t[label])
        lines.append(f"      {label:62s} median {m:9.1f} {unit}   spread {max(t[label]) - min(t[label]):8.1f} {unit}   x{m / base:7.2f}")
    return {label: statistics.median(v) for label, v in t.items()}


def kernel_bench(lines, B, reps):
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K
    dev, bf = "cuda", torch.bfloat16
    torch.manual_seed(0)
    rows = B * R
    a = torch.randn(rows, device=dev)
    w1, b1 = (0.05 * torch.randn(D, 1, device=dev)).to(bf), (0.05 * torch.randn(D, device=dev)).to(bf)
    dh = torch.randn(rows, D, device=dev).to(bf)

    def embed():
        return K.noisy_embed_fwd(a, w1, b1, bf)

    def embed_torch():
        return torch.nn.functional.gelu(a.to(bf)[:, None] * w1.view(1, D) + b1)

    lines.append(f"   (fused and composed embed agree: max |dh| {float((embed().float() - embed_torch().float()).abs().max()):.3e})")
    lines.append(f"2. the new kernels at d {D}, bf16: us per call")
    alternate(lines, f"noisy_embed forward, {rows} scalars -> [{rows}, {D}]",
              [("noisy_embed_fwd", embed), ("broadcast multiply + add + GELU (3 launches)", embed_torch)], reps, inner=10)
    pre = (a.to(bf)[:, None] * w1.view(1, D) + b1).contiguous()
    ab = a.to(bf).view(rows, 1).contiguous()

    def embed_bwd():
        return K.noisy_embed_bwd(dh, a, w1, b1)

    def embed_bwd_comp():
        dpre = K.act_bwd(pre, dh, L.ACT_GELU_ERF)
        return torch.mm(dpre.t(), ab), K.colsum(dpre)

    alternate(lines, f"noisy_embed backward, dh [{rows}, {D}] -> dw1 | db1",
              [("noisy_embed_bwd (pre-activation recomputed, 2 launches)", embed_bwd),
               ("act_bwd on a kept pre-activation + [d, R] x [R] product + colsum", embed_bwd_comp)], reps, inner=10)
    # ---- the reserved rows against a copy-based insertion
    Q = R + 2
    Sq = S + Q
    off_h = torch.full((B,), S, dtype=torch.int64)
    off_h[1::2] -= 5                                            # every other sample five rows shorter
    off = off_h.to(dev)
    proj, time_, state = (torch.randn(n, D, device=dev).to(bf) for n in (rows, B, B))
    spliced = torch.randn(B, S, D, device=dev).to(bf)
    x = torch.zeros(B, Sq, D, device=dev, dtype=bf)

    def put():
        return K.diffusion_put_(x, proj, time_, off, state)

    def copy_insert():
        out = torch.zeros(B, Sq, D, device=dev, dtype=bf)
        pr = proj.view(B, R, D)
        for bb in range(B):
            n = int(off_h[bb])
            K.copy2d(spliced[bb, :n], out[bb, :n], D, D)
            K.copy2d(state[bb:bb + 1], out[bb, n:n + 1], D, D)
            K.copy2d(time_[bb:bb + 1], out[bb, n + 1:n + 2], D, D)
            K.copy2d(pr[bb], out[bb, n + 2:n + Q], D, D)
        return out

    alternate(lines, f"diffusion_put: {Q} rows per sample into x [{B}, {Sq}, {D}] in place",
              [("diffusion_put_fwd (rows reserved by the splice)", put),
               ("zero fill + copies of the spliced, state, time and projected rows", copy_insert)], reps, inner=4)
    # ---- the two ends of a DDIM step
    x1 = torch.randn(R, device=dev)
    eps = torch.randn(R, device=dev).to(bf)
    trow = torch.randn(D, device=dev).to(bf)
    suffix = torch.empty(1 + R, D, device=dev, dtype=bf)
    h = torch.empty(R, D, device=dev, dtype=bf)
    c = (1.02, 0.2, 0.99, 0.14)

    def step():
        K.ddim_step_embed_(eps, x1, c, 1.0, trow, w1, b1, suffix, h)          # (in place: the clamp keeps x bounded over the repetitions)

    def step_torch():
        e = eps.float()
        x0 = (c[0] * x1 - c[1] * e).clamp(-1, 1)
        xn = c[2] * x0 + c[3] * e
        suffix[0].copy_(trow)
        return xn, torch.nn.functional.gelu(xn.to(bf)[:, None] * w1.view(1, D) + b1)

    alternate(lines, f"ddim_step_embed: the step on {R} values, the time row and the [{R}, {D}] operand",
              [("ddim_step_embed (1 launch)", step), ("elementwise torch ops + row copy + embed (11 launches)", step_torch)], reps, inner=10)


def model_bench(a, lines):
    """-> the training-step measurement, to be run after the kernel section"""
    from dexbotic_amd.model import OFTDiffusionConfig, OFTDiffusionForCausalLM
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    dev = torch.device("cuda", 0)
    cfg = OFTDiffusionConfig(llm_config=Qwen2Config(), mm_vision_tower=CLIPVisionConfig(), mm_projector_type="mlp2x_gelu",
                             action_model_type="DiT", action_dim=A, chunk_size=T, use_proprio=True, proprio_dim=8,
                             compute_dtype="bfloat16")
    m = OFTDiffusionForCausalLM(cfg, device=dev, train=True)
    m.init_random_(seed=0)
    g = torch.Generator().manual_seed(1)

    def request(B):
        ids = torch.randint(1000, 30000, (B, 32), generator=g)
        ids[:, 1] = -200
        return ids, torch.randn(B, 3, 224, 224, generator=g).clamp_(-2.5, 2.5).to(dev), torch.randn(B, 8, generator=g).to(dev)

    m.eval()
    norms = {"min": [-1.0] * A, "max": [1.0] * A}
    ids, images, states = request(1)
    noise = torch.randn(1, T, A, generator=g).to(dev)
    out = {}

    def run(cached):
        def f():
            out[cached] = m.inference_action(ids, images, {"action_norms": norms, "states": states, "noise": noise, "cached": cached})
        return f

    lines.append(f"1. inference_action, B = 1, 10 DDIM steps, eager launches (each call ends with the host copy of the chunk): ms per request")
    med = alternate(lines, f"prompt of {S} rows, suffix of {1 + R} rows",
                    [("cached: 1 prefill + 10 suffix passes", run(True)), ("full pass: the whole model per step", run(False))],
                    a.reps, unit="ms")
    # agreement of the two paths where it can be read: the first step's predicted noise.  With random weights the predicted noise is
    # several units large, every x0 sits on the clamp and a bf16 rounding flips its sign: the final chunks of the two paths are then
    # unrelated (tests/test_oft_diffusion_gpu.py compares the chunks on a model whose sampler is not saturated)
    tr = {}
    for cached in (True, False):
        tr[cached] = []
        m.sample_actions(ids, images, states=states, noise=noise, cached=cached, trajectory=tr[cached])
    e0, e1 = tr[True][0][0], tr[False][0][0]
    lines.append(f"   (first step's predicted noise, cached against full pass: max |d eps| {float((e0 - e1).abs().max()):.3e} at max |eps| "
                 f"{float(e1.abs().max()):.3e}, bf16; final chunks differ by {float((torch.tensor(out[True]) - torch.tensor(out[False])).abs().max()):.3e}"
                 f": random weights saturate the clamp)")
    lines.append(f"   cached path faster than the full pass in this run: {med['cached: 1 prefill + 10 suffix passes'] < med['full pass: the whole model per step']}")
    return lambda: train_bench(a, lines, m, request, g)


def train_bench(a, lines, m, request, g):
    from dexbotic_amd.engine import OptimConfig
    from dexbotic_amd.trainer import NativeTrainer
    dev = m.store.device
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
    lines.append(f"3. OFT diffusion training step (noise and timesteps drawn on the device), batch {a.batch}, S + Q = {S + R + 2}: median "
                 f"{statistics.median(ts):7.1f} ms  min {min(ts):7.1f}  max {max(ts):7.1f} over {a.steps} steps; loss {float(loss):.4f}; "
                 f"{m.store.total / 1e9:.3f} B parameters")
    del tr, m
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [__doc__.split("\n\n")[0], __doc__.split("\n\n")[1], ""]
    train = None if a.kernels_only else model_bench(a, lines)
    kernel_bench(lines, a.batch, a.reps)
    if train is not None:
        train()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("oft_diffusion_bench: needs the GPU (no timing is taken on a CPU)")
    main()
