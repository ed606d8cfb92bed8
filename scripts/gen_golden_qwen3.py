"""Generate tests/golden/qwen3_t1.npz by running the installed ``transformers.Qwen3Model`` on the CPU.

TEST INFRASTRUCTURE, CPU only; needs nothing but ``transformers``.  The fixture it writes is committed; tests/test_qwen3_golden.py
re-runs ``compute()`` and compares, so a drift of the installed library shows.

    python scripts/gen_golden_qwen3.py            # from the repository root

Pinned: a tiny Qwen3 decoder — vocab 64, hidden 64, intermediate 128, 2 layers, 4 heads, 2 kv heads, head_dim 32, so
Hq * head_dim = 128 != hidden_size (what code that derives head_dim from hidden_size gets wrong) — in fp32 on B = 2, S = 9 input
embeddings: ``last_hidden_state``, layer 0's q and k after q_norm / k_norm + RoPE (forward hooks on the two norms and HF's own
``apply_rotary_pos_emb`` on what they return), the gradients of every parameter and of the input embeddings under the scalar loss
sum(last_hidden_state * r) for a fixed random r, and the cached path: prefill of 6 tokens then 3 single-token steps with
``use_cache=True`` (hidden states of each).  Weights and inputs are rounded to bf16-representable fp32 values (a bf16 model starts
from exactly the same numbers); q_norm / k_norm weights are drawn from U(0.5, 1.5) so that a missing or swapped weight shows.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")

SEED = 31
VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS, HEAD_DIM = 64, 64, 128, 2, 4, 2, 32
THETA, EPS = 1e6, 1e-6
B, S, PREFILL = 2, 9, 6


def bf16_grid(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def hf_config():
    from transformers import Qwen3Config
    return Qwen3Config(vocab_size=VOCAB, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=LAYERS,
                       num_attention_heads=HEADS, num_key_value_heads=KV_HEADS, head_dim=HEAD_DIM, max_position_embeddings=4096,
                       rope_parameters={"rope_type": "default", "rope_theta": THETA}, rms_norm_eps=EPS, attention_bias=False,
                       tie_word_embeddings=False, use_sliding_window=False, attn_implementation="eager")


def compute() -> dict:
    from transformers import Qwen3Model
    from transformers.models.qwen3 import modeling_qwen3

    torch.manual_seed(SEED)
    cfg = hf_config()
    assert float(cfg.rope_parameters["rope_theta"]) == THETA
    m = Qwen3Model(cfg).float().eval()
    rs = np.random.RandomState(SEED)
    w = {}
    for k, v in m.state_dict().items():
        shape = tuple(v.shape)
        if k.endswith("q_norm.weight") or k.endswith("k_norm.weight"):
            a = rs.uniform(0.5, 1.5, size=shape)
        elif len(shape) == 1:
            a = 1.0 + 0.1 * rs.standard_normal(shape)
        else:
            a = 0.08 * rs.standard_normal(shape)
        w[k] = bf16_grid(a)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    x = bf16_grid(0.5 * rs.standard_normal((B, S, HIDDEN)))
    r = rs.standard_normal((B, S, HIDDEN)).astype(np.float32)

    # ---- full forward + backward, layer 0's q / k captured behind the norms
    got = {}
    attn0 = m.layers[0].self_attn
    hooks = [attn0.q_norm.register_forward_hook(lambda mod, a, out: got.__setitem__("qn", out.detach())),
             attn0.k_norm.register_forward_hook(lambda mod, a, out: got.__setitem__("kn", out.detach())),
             attn0.register_forward_pre_hook(lambda mod, a, kw: got.__setitem__("pe", kw["position_embeddings"]), with_kwargs=True)]
    xt = torch.from_numpy(x).requires_grad_(True)
    out = m(inputs_embeds=xt, use_cache=False).last_hidden_state
    for h in hooks:
        h.remove()
    (out * torch.from_numpy(r)).sum().backward()
    cos, sin = (t.detach() for t in got["pe"])
    q0, k0 = modeling_qwen3.apply_rotary_pos_emb(got["qn"].transpose(1, 2), got["kn"].transpose(1, 2), cos, sin)
    res = {"w/" + k: v for k, v in w.items()}
    res.update(seed=np.int64(SEED), cfg=np.array([VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS, HEAD_DIM], dtype=np.int64),
               rope_theta=np.float64(THETA), rms_norm_eps=np.float64(EPS), names=np.array(list(w)),
               inputs_embeds=x, loss_weight=r, last_hidden_state=out.detach().numpy().astype(np.float32),
               q0=q0.contiguous().numpy().astype(np.float32), k0=k0.contiguous().numpy().astype(np.float32),
               grad_inputs_embeds=xt.grad.numpy().astype(np.float32))
    for n, p_ in m.named_parameters():
        # (embed_tokens is not reached from inputs_embeds: HF leaves its gradient None, stored as zeros)
        res["grad/" + n] = (p_.grad if p_.grad is not None else torch.zeros_like(p_)).numpy().astype(np.float32)

    # ---- cached path: prefill PREFILL tokens, then one token at a time
    steps = []
    with torch.no_grad():
        o = m(inputs_embeds=torch.from_numpy(x[:, :PREFILL]), use_cache=True)
        steps.append(o.last_hidden_state.numpy().astype(np.float32))
        for s in range(PREFILL, S):
            o = m(inputs_embeds=torch.from_numpy(x[:, s:s + 1]), past_key_values=o.past_key_values, use_cache=True)
            steps.append(o.last_hidden_state.numpy().astype(np.float32))
    res["cached_prefill"] = steps[0]
    res["cached_steps"] = np.concatenate(steps[1:], axis=1)
    return res


def main():
    res = compute()
    path = os.path.join(GOLD, "qwen3_t1.npz")
    np.savez_compressed(path, **res)
    full, cached = res["last_hidden_state"], np.concatenate([res["cached_prefill"], res["cached_steps"]], axis=1)
    print(f"[gen_golden_qwen3] |h| {np.abs(full).max():.4f} cached-vs-full {np.abs(full - cached).max():.2e} "
          f"|q0| {np.abs(res['q0']).max():.4f} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.exit(main())
