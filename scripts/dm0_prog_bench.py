#!/usr/bin/env python
"""DM0-prog at the size profiles/dm0_sampler.txt assumes: the two one-launch ends of an Euler step against the composed sequences they
replace, and the action request beside DM0's own.

ASSUMPTION, not read from a checkpoint (as scripts/dm0_bench.py): both experts take the attention geometry of HF's Qwen3-1.7B config
(28 layers, 16 query / 8 key-value heads x 128); llm d 2048 / F 6144, action expert d 1024 / F 3072; CLIP ViT-L/14 at 224 px; prefix =
3 cameras' tokens + 48 text tokens = 816, chunk 50, action_dim 32, B = 1, bf16 compute.  Synthetic data, random-init weights.

Two measurements, written to the file given with --out (profiles/dm0_prog.txt):
 1. us per call (device events, alternating rounds): ``flow_suffix_in`` / ``flow_euler_tail_`` with the progress row against the
    sequence of existing wrappers each replaces, written out below and nowhere else; their results are checked to agree;
 2. ``inference_action`` p50 / min / max over varied requests in alternating rounds: DM0-prog with and without ``progress`` and
    ``DM0ForCausalLM``, graph replay on and off.

    python scripts/dm0_prog_bench.py [--layers 28] [--reqs 10] [--out profiles/dm0_prog.txt]
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


def alternate(fns, lines, rounds=15):
    for f in fns.values():
        timed(f, 5)
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(timed(f))
    for k, v in t.items():
        lines.append(f"   {k:10s} median {statistics.median(v):7.1f} us  min {min(v):7.1f}  max {max(v):7.1f}")
    return {k: statistics.median(v) for k, v in t.items()}


def kernel_bench(a, lines):
    from dexbotic_amd import kernels as K
    dev, bf = "cuda", torch.bfloat16
    B, n, A, da = 1, a.chunk, 32, a.action_hidden
    dt = -0.1
    torch.manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev)
    x0, progress, te = r(B, n * A), torch.rand(B, 1, device=dev), r(B, da).to(bf)
    w_in, b_in = (r(da, A) / A ** 0.5).to(bf), (0.1 * r(da)).to(bf)
    w_p, b_p = r(da, 1).to(bf), (0.1 * r(da)).to(bf)
    h, g = r(B * (1 + n), da).to(bf), (1 + 0.1 * r(da)).to(bf)
    w_out, b_out = (r(A, da) / da ** 0.5).to(bf), (0.1 * r(A)).to(bf)
    w_q, b_q = (r(1, da) / da ** 0.5).to(bf), (0.1 * r(1)).to(bf)
    state = torch.empty(B, n * A + 1, device=dev)
    x, pm = state[:, :n * A], state[:, n * A:]

    # ---- the head: what DM0's get_suffix_hidden_states runs up to action_time_mlp_in, plus the progress token's launches
    def head_fused():
        return K.flow_suffix_in(x0, te, w_in, b_in, n, A, progress, w_p, b_p)

    def head_composed():
        act = K.mm_nt(x0.to(bf).reshape(B * n, A), w_in, bias=b_in).view(B, n, da)
        prog = K.mm_nt(progress.to(bf), w_p, bias=b_p).view(B, 1, da)               # the K = 1 product
        tok = torch.cat([prog, act], dim=1)
        return torch.cat([tok, te[:, None, :].expand(B, 1 + n, da)], dim=-1).reshape(B * (1 + n), 2 * da).contiguous()

    # ---- the tail: final norm, slicing copy, action_out_proj, .float(), scale, add, plus the progress head, the stack and the min
    def tail_fused():
        return K.flow_euler_tail_(h, g, w_out, b_out, x, n, EPS, dt, pm, w_q, b_q)

    cstate = dict(x=x0.clone(), pm=torch.full((B, 1), float("inf"), device=dev))

    def tail_composed():
        y = K.rmsnorm_fwd(h, g, EPS)[0].view(B, 1 + n, da)
        v = K.mm_nt(y[:, 1:].reshape(B * n, da).contiguous(), w_out, bias=b_out).float()
        cstate["x"] = K.add(cstate["x"], K.scale_(v.reshape(B, n * A).contiguous(), dt))
        e = K.mm_nt(y[:, :1].reshape(B, da).contiguous(), w_q, bias=b_q).float()  # the N = 1 product
        cstate["pm"] = torch.min(torch.stack([cstate["pm"], e]), dim=0)[0]
        return cstate["x"]

    lines.append(f"1. the two ends of one Euler step with the progress row, B={B} chunk={n} A={A} da={da} bf16: us per call (device events, "
                 "20 calls per round, 15 alternating rounds)")
    d_head = (head_fused().float() - head_composed().float()).abs().max().item()
    x.copy_(x0)
    pm.fill_(float("inf"))
    tail_fused()
    tail_composed()
    d_x = (x - cstate["x"]).abs().max().item()
    d_e = (pm - cstate["pm"]).abs().max().item()
    ok = d_head <= 1.0 / 64 * 8 and d_x <= 1e-2 and d_e <= 2e-2          # bf16 roundings of the composed path (y, v, e): a few ulp of O(1) values
    lines.append(f"   results agree: {ok} (max |difference| head {d_head:.2e} of bf16 outputs, x after one step {d_x:.2e}, progress "
                 f"prediction {d_e:.2e}; the composed tail rounds y, v and e to bf16, the kernel does not)")
    lines.append("   head: flow_suffix_in against cast, action_in_proj, progress_in_proj (K = 1), row cat, expand, column cat, contiguous")
    th = alternate(dict(fused=head_fused, composed=head_composed), lines)
    lines.append(f"   composed / fused at the medians: {th['composed'] / th['fused']:.2f}")
    lines.append("   tail: flow_euler_tail_ against rmsnorm, slicing copy, action_out_proj, .float(), scale, add, slice, progress_out_proj "
                 "(N = 1), .float(), stack, min")
    tt = alternate(dict(fused=tail_fused, composed=tail_composed), lines)
    lines.append(f"   composed / fused at the medians: {tt['composed'] / tt['fused']:.2f}   (each end runs 10 times per action chunk)")
    return th["fused"] + tt["fused"], th["composed"] + tt["composed"]


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
    ap.add_argument("--reqs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dexbotic_amd.model import DM0Config, DM0ForCausalLM, DM0ProgConfig, DM0ProgForCausalLM
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    dev = torch.device("cuda", 0)
    q3 = dict(model_type="qwen3", vocab_size=a.vocab, num_hidden_layers=a.layers, num_attention_heads=a.heads,
              num_key_value_heads=a.kv_heads, head_dim=a.head_dim, rms_norm_eps=1e-6, rope_theta=1e6, max_position_embeddings=40960)
    vis = CLIPVisionConfig()                                                   # ViT-L/14 at 224 px: 256 tokens per camera
    kw = dict(llm_config=dict(q3, hidden_size=a.hidden, intermediate_size=a.inter),
              action_config=dict(q3, hidden_size=a.action_hidden, intermediate_size=a.action_inter), mm_vision_tower=vis,
              action_dim=32, chunk_size=a.chunk, bf16=True)
    CAM = 3
    P = CAM * (vis.image_size // vis.patch_size) ** 2 + a.text
    lines = [__doc__.split("\n\n")[0], __doc__.split("\n\n")[1], ""]
    us_fused, us_composed = kernel_bench(a, lines)

    models = {}
    for name, ccls, mcls in (("dm0", DM0Config, DM0ForCausalLM), ("dm0_prog", DM0ProgConfig, DM0ProgForCausalLM)):
        m = mcls(ccls(**kw), device=dev, train=False)
        m.init_random_(seed=0)
        m.eval()
        models[name] = m
    lines.append(f"model: {models['dm0_prog'].store.total / 1e9:.3f} B parameters, {a.layers} layers, prefix {P}, chunk {a.chunk}")
    g = torch.Generator().manual_seed(1)

    def request():
        return dict(input_ids=torch.randint(1000, 30000, (1, a.text), generator=g).to(dev),
                    attention_mask=torch.ones(1, a.text, dtype=torch.bool),
                    images=torch.randn(1, CAM, 3, 224, 224, generator=g).clamp_(-2.5, 2.5).to(dev),
                    image_masks=torch.ones(1, CAM, dtype=torch.bool), states=torch.randn(1, 32, generator=g).to(dev),
                    noise=torch.randn(1, a.chunk, 32, generator=g).to(dev))
    # ---- 2. the action request: every configuration serves the same request of a round, one after the other
    configs = {}
    for use_graph in (False, True):
        tag = "on " if use_graph else "off"
        configs[f"DM0                       graph {tag}"] = ("dm0", False, use_graph)
        configs[f"DM0-prog without progress graph {tag}"] = ("dm0_prog", False, use_graph)
        configs[f"DM0-prog with progress    graph {tag}"] = ("dm0_prog", True, use_graph)
    lat = {k: [] for k in configs}
    for i in range(a.reqs + 3):                                                # (graph: eager, capture, first replay are warm-up)
        r = request()
        prog = torch.rand(1, 1, generator=g).to(dev)
        for k, (name, with_prog, use_graph) in configs.items():
            extra = dict(progress=prog) if with_prog else {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = models[name].inference_action(diffusion_steps=10, use_graph=use_graph, **extra, **r)
            (out[0] if with_prog else out).cpu()
            lat[k].append(1e3 * (time.perf_counter() - t0))
    lines.append(f"2. inference_action, B=1, 10 Euler steps, ms over {a.reqs} varied requests (host clock around the request, ended by "
                 "the copy of the chunk to the host; the configurations alternate within every round)")
    for k, v in lat.items():
        v = v[3:]
        lines.append(f"   {k}: p50 {np.median(v):7.1f} ms  min {min(v):7.1f}  max {max(v):7.1f}")
    for tag in ("off", "on "):
        base, prog = (lat[f"{n} graph {tag}"][3:] for n in ("DM0                      ", "DM0-prog with progress   "))
        lines.append(f"   graph {tag}: DM0-prog with progress - DM0 at p50 {np.median(prog) - np.median(base):+.2f} ms; DM0's own min - max "
                     f"spread in this run {max(base) - min(base):.2f} ms")
    p50 = np.median(lat["DM0                       graph on "][3:])
    lines.append(f"   reading: per step the two ends are {us_fused:.0f} us against {us_composed:.0f} us composed (1.), over ten steps "
                 f"{(us_composed - us_fused) / 100:.2f} ms of a {p50:.0f} ms request that the vision tower, the prefix pass and the "
                 f"{a.layers} mixture layers of every step dominate; the extra suffix row is one row more among {a.chunk}")
    text ="\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("dm0_prog_bench: needs the GPU (no timing is taken on a CPU)")
    main()
