#!/usr/bin/env python
"""Single-token decode of a Qwen3-8B-width decoder (36 layers, 4096 / 12288, 32 heads over 8 of 128, bf16, random weights): ms per
token of the decoder pass behind a 300-token prompt, the per-op cached path (DXA_DECODE_FUSED=0) against the persistent one-launch
step (csrc/decode_fused.hip, QKN instantiation), alternating in one process.

    python scripts/qwen3_decode_bench.py [tokens per walk, default 32] [repetitions, default 7]

A walk = a fresh cache, the prefill, then the timed single-token passes: one HIP event in front of the first pass and one behind the
last, on the stream itself.  The decoder alone is timed (no lm_head, no argmax): 13.9 GB of bf16 weights per token."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT = 300


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    from dexbotic_amd import kernels as K
    from dexbotic_amd.engine import ParamStore, attach_parameters
    from dexbotic_amd.model.llm.qwen3 import Qwen3Backbone, Qwen3Config
    n_tok = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = torch.device("cuda", 0)
    cfg = Qwen3Config(vocab_size=64)                         # (the embedding table is not part of the step)
    st = ParamStore(dev, torch.bfloat16)
    llm = Qwen3Backbone(st, "model.llm.", cfg)
    st.finalize(train=False)
    attach_parameters(llm, st)
    g = torch.Generator(device=dev).manual_seed(0)
    st.master.normal_(0.0, 0.02, generator=g)
    for name in st.slots:
        t = st.w32(name)
        if t.dim() == 1:
            t.fill_(1.0)
    st.sync_shadow()
    d = cfg.hidden_size
    c = cfg
    layer_bytes = 2 * ((c.num_attention_heads + 2 * c.num_key_value_heads) * c.head_dim * d + d * c.num_attention_heads * c.head_dim +
                       3 * c.intermediate_size * d)
    wbytes = layer_bytes * c.num_hidden_layers
    prompt = (torch.randn(1, PROMPT, d, generator=g, device=dev) * 0.5).bfloat16()
    steps = (torch.randn(n_tok, 1, 1, d, generator=g, device=dev) * 0.5).bfloat16()

    def walk(mode):
        os.environ["DXA_DECODE_FUSED"] = mode
        cache = llm.new_cache(1, PROMPT + n_tok, dev, torch.bfloat16)
        llm.forward_cached(prompt, cache)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(n_tok):
            out = llm.forward_cached(steps[t], cache)
        b.record()
        torch.cuda.synchronize()
        assert cache.fused_steps == (n_tok if mode == "1" else 0), (mode, cache.fused_steps)
        assert not K.decode_timed_out() and bool(torch.isfinite(out.float()).all())
        return a.elapsed_time(b) / n_tok

    for mode in ("0", "1"):                                  # untimed warm-up of both paths
        walk(mode)
    ms = {"0": [], "1": []}
    for rep in range(reps):
        for mode in ("0", "1"):                              # alternating: both paths see the same machine state
            ms[mode].append(walk(mode))
        print(f"rep {rep}: per-op {ms['0'][-1]:.3f} ms/token | persistent {ms['1'][-1]:.3f} ms/token", flush=True)
    for mode, name in (("0", "per-op cached path (DXA_DECODE_FUSED=0)"), ("1", "persistent one-launch step")):
        v = ms[mode]
        print(f"{name}: median {med(v):.3f} ms/token, min {min(v):.3f}, max {max(v):.3f} over {reps} walks of {n_tok} tokens behind "
              f"{PROMPT} cached positions ({wbytes * 1e-9:.2f} GB of decoder weights per token: {wbytes * 1e-9 / med(v):.2f} TB/s)",
              flush=True)
    print(f"persistent / per-op: {med(ms['1']) / med(ms['0']):.3f}", flush=True)


if __name__ == "__main__":
    main()
