#!/usr/bin/env python
"""OFT-discrete at full size: the one-launch inference head, the dense action rows and the shared-row fill against the compositions of
existing launches they replace, one training step and the action request.

Size as profiles/oft_head.txt: CLIP ViT-L/14 at 224 px and a 32-token prompt (S = 287 spliced rows), Qwen2.5-7B-class decoder (d 3584,
28 layers, vocabulary 152064), action_dim 7, chunk_size 16: R = 112 action rows behind each sample, S + R = 399, num_bins 256 (255 bin
columns).  bf16 compute, synthetic data, random-init weights.

Measurements, written to the file given with --out (profiles/oft_discrete.txt); device events after a warm-up, the sides of a
comparison alternated in one process, medians and the spread (max - min over the rounds) of each side; B = 1 and 16:
 (a) ``action_bins_fwd`` against ``gather_rows`` + ``mm_nt`` on the 255-row weight view + ``argmax_rows``, and against the
     full-vocabulary ``mm_nt`` + ``argmax_rows`` of the slice; the three results are compared first;
 (b) ``action_rows_bwd`` against a zero fill and one ``copy2d`` per sample;
 (c) ``splice_bwd`` + ``action_fill_bwd`` against the alternative of putting token 1 into the plan's reserved rows and letting
     ``splice_bwd`` add the B R duplicate rows;
 (d) one training step (NativeTrainer) of OFTDiscreteForCausalLM at batch 16, ms;
 (e) ``inference_action`` p50 over varied requests.

    python scripts/oft_discrete_bench.py [--batch 16] [--reqs 10] [--steps 5] [--kernels-only] [--out profiles/oft_discrete.txt]
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
D, V, A, T, S, NUM_BINS = 3584, 152064, 7, 16, 287, 256
R, NB = A * T, NUM_BINS - 1


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
        lines.append(f"      {label:62s} median {m:9.1f} us   spread {max(t[label]) - min(t[label]):8.1f} us   x{m / base:7.2f}")


def kernel_bench(lines, B, W):
    from dexbotic_amd import kernels as K
    from dexbotic_amd.splice import PLAN_PAD
    dev, bf = "cuda", torch.bfloat16
    torch.manual_seed(B)
    Sq = S + R
    off_h = torch.full((B,), S, dtype=torch.int64)
    off_h[1::2] -= 5                                            # every other sample five rows shorter
    off = off_h.to(dev)
    h = torch.randn(B, Sq, D, device=dev).to(bf)
    h2 = h.view(B * Sq, D)
    idx = torch.cat([bb * Sq + off_h[bb] + torch.arange(R) for bb in range(B)]).to(dev)
    w_bins = W[V - NB:]
    lines.append(f"B = {B}: h [{B}, {Sq}, {D}] bf16, {B * R} action rows")

    def fused():
        return K.action_bins_fwd(h, off, w_bins, R, False)

    def comp255():
        lg = K.mm_nt(K.gather_rows(h2, idx, bf), w_bins)
        return lg, K.argmax_rows(lg)

    def comp_full():
        lg = K.mm_nt(K.gather_rows(h2, idx, bf), W)
        return lg, K.argmax_rows(lg[:, V - NB:])

    lf, bf_, _ = fused()
    l1, b1 = comp255()
    l2, b2 = comp_full()
    own = torch.equal(bf_, lf.float().argmax(-1))
    lines.append(f"   (bins: fused = argmax of its own logits: {own}; logits fused vs 255-column product max |d| "
                 f"{float((lf.float() - l1.float()).abs().max()):.3e}, vs full-vocabulary slice {float((lf.float() - l2[:, V - NB:].float()).abs().max()):.3e} "
                 f"at max |logit| {float(lf.float().abs().max()):.2f}; bins equal {int((bf_ == b1).sum())}/{B * R} and {int((bf_ == b2).sum())}/{B * R}, "
                 f"255-column vs full {int((b1 == b2).sum())}/{B * R})")
    alternate(lines, f"(a) inference head over {B * R} rows x {NB} bins x {D}: us per call",
              [("action_bins_fwd (one launch, rows in place)", fused, None),
               ("gather_rows + mm_nt [255 columns] + argmax_rows", comp255, None),
               ("gather_rows + mm_nt [152064 columns] + argmax_rows of the slice", comp_full, 3)])

    dy = torch.randn(B * R, D, device=dev).to(bf)

    def rows_bwd():
        return K.action_rows_bwd(dy, off, B, Sq, R, False)

    def rows_bwd_copy():
        dh = torch.zeros(B * Sq, D, device=dev, dtype=bf)
        dyr = dy.view(B, R, D)
        for bb in range(B):
            o = bb * Sq + int(off_h[bb])
            K.copy2d(dyr[bb], dh[o:o + R], D, D)
        return dh
    same = torch.equal(rows_bwd().view(-1), rows_bwd_copy().view(-1))
    lines.append(f"   (action_rows_bwd equals the copies: {same})")
    alternate(lines, f"(b) gradient of the action rows into dh [{B}, {Sq}, {D}]: us per call",
              [("action_rows_bwd (dh complete)", rows_bwd, None), ("zero fill + copy2d per sample", rows_bwd_copy, None)])

    # (c) the plan of the batch: 31 text tokens, 256 image rows, then the reserved rows (PLAN_PAD) or token 1 in them
    g = torch.Generator().manual_seed(3)
    plan_h = torch.full((B, Sq), PLAN_PAD, dtype=torch.int64)
    for bb in range(B):
        n = int(off_h[bb])
        row = torch.randint(1000, 30000, (n,), generator=g)
        row[1:257] = -1 - (bb * 256 + torch.arange(256))
        plan_h[bb, :n] = row
    plan_tok = plan_h.clone()
    for bb in range(B):
        n = int(off_h[bb])
        plan_tok[bb, n:n + R] = 1
    plan, plan_tok = plan_h.to(dev).view(-1), plan_tok.to(dev).view(-1)
    dout = torch.randn(B * Sq, D, device=dev).to(bf)
    d_embed = torch.zeros(V, D, device=dev, dtype=torch.float32)

    def fill_path():
        K.splice_bwd(plan, dout, d_embed, None)
        K.action_fill_bwd(dout.view(B, Sq, D), off, R, False, drow=d_embed[1], accumulate=True)

    def plan_path():
        K.splice_bwd(plan_tok, dout, d_embed, None)
    d_embed.zero_()
    fill_path()
    r1 = d_embed[1].clone()
    d_embed.zero_()
    plan_path()
    r2 = d_embed[1].clone()
    lines.append(f"   (row 1 of the embedding gradient, fill path vs token-in-plan: max |d| {float((r1 - r2).abs().max()):.3e} at max "
                 f"{float(r2.abs().max()):.2f})")
    alternate(lines, f"(c) embedding gradient of the {B * R} query rows (token 1): us per call",
              [("splice_bwd + action_fill_bwd (fixed-order two-stage sum)", fill_path, None),
               ("splice_bwd with token 1 in the plan's reserved rows", plan_path, 3)], rounds=5)
    del d_embed
    torch.cuda.empty_cache()


def model_bench(a, lines):
    from dexbotic_amd.engine import OptimConfig
    from dexbotic_amd.model import OFTDiscreteConfig, OFTDiscreteForCausalLM
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    from dexbotic_amd.trainer import NativeTrainer
    dev = torch.device("cuda", 0)
    cfg = OFTDiscreteConfig(llm_config=Qwen2Config(), mm_vision_tower=CLIPVisionConfig(), mm_projector_type="mlp2x_gelu",
                            action_model_type="Discrete", action_dim=A, chunk_size=T, use_proprio=True, proprio_dim=8,
                            num_bins=NUM_BINS, compute_dtype="bfloat16")
    m = OFTDiscreteForCausalLM(cfg, device=dev, train=True)
    m.init_random_(seed=0)
    g = torch.Generator().manual_seed(1)

    def request(B):
        ids = torch.randint(1000, 30000, (B, 32), generator=g)
        ids[:, 1] = -200
        return ids, torch.randn(B, 3, 224, 224, generator=g).clamp_(-2.5, 2.5).to(dev), torch.randn(B, 8, generator=g).to(dev)
    m.train()
    tr = NativeTrainer(m, OptimConfig(base_lr=2.5e-5, max_grad_norm=1.0), total_steps=1000)
    B = a.batch
    ids, images, states = request(B)
    bins = torch.randint(0, NB, (B, R), generator=g)
    full = torch.cat([ids[:, :31], bins + cfg.vocab_size - NUM_BINS + 1, ids[:, 31:]], dim=1)        # [prefix][R action tokens][suffix]
    labels = torch.full_like(full, -100)
    labels[:, 31:31 + R] = full[:, 31:31 + R]
    batch = dict(input_ids=full, attention_mask=torch.ones(B, full.shape[1], dtype=torch.bool), labels=labels, images=images,
                 states=states, actions=(bins.float() / NB * 2 - 1).to(dev))
    for _ in range(2):
        loss = tr.step(batch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        loss = tr.step(batch)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    lines.append(f"(d) OFT-discrete training step, batch {B}, S + R = {S + R + 1}: median {statistics.median(ts):7.1f} ms  min {min(ts):7.1f}  "
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
    lines.append(f"(e) OFT-discrete inference_action, B=1, one decoder pass over {S + R + 1} rows, eager launches: p50 {np.median(lat):7.1f} ms  "
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
    torch.manual_seed(0)
    W = (0.02 * torch.randn(V, D, device="cuda")).to(torch.bfloat16)
    for B in (1, a.batch):
        kernel_bench(lines, B, W)
    del W
    torch.cuda.empty_cache()
    if not a.kernels_only:
        model_bench(a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("oft_discrete_bench: needs the GPU (no timing is taken on a CPU)")
    main()
