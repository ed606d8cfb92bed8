"""Generate tests/golden/qwen3_d64.npz by running the installed ``transformers.Qwen3Model`` on the CPU.

TEST INFRASTRUCTURE, CPU only; needs nothing but ``transformers``.  The fixture it writes is committed;
tests/test_qwen3_decode_golden.py re-runs ``compute()`` and compares, so a drift of the installed library shows.

    python scripts/gen_golden_qwen3_decode.py     # from the repository root

The fixture of the persistent decode step on a Qwen3 decoder (csrc/decode_fused.hip, tests/test_qwen3_decode_fused_gpu.py).
Pinned: vocab 64, hidden 128, intermediate 256, 2 layers, 4 heads over 2 kv heads, head_dim 64 — the smallest head_dim the
persistent step takes, and Hq * head_dim = 256 != hidden_size — on B = 1: a prefill of 11 tokens, then 6 single-token steps with
``use_cache=True`` in fp32 (``cached_prefill``, ``cached_steps``), the same steps of the same HF model in bf16
(``cached_steps_bf16``: what bf16 arithmetic costs on these numbers, the yardstick of the GPU test) and the uncached fp32
forward over all 17 tokens (``last_hidden_state``).  Weights and inputs are rounded to bf16-representable fp32 values (a bf16
model starts from exactly the same numbers); q_norm / k_norm weights are drawn from U(0.5, 1.5) so that a missing or swapped
weight shows.  No gradients.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")

SEED = 37
VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS, HEAD_DIM = 64, 128, 256, 2, 4, 2, 64
THETA, EPS = 1e6, 1e-6
B, PREFILL, STEPS = 1, 11, 6
S = PREFILL + STEPS


def bf16_grid(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def hf_config():
    from transformers import Qwen3Config
    return Qwen3Config(vocab_size=VOCAB, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=LAYERS,
                       num_attention_heads=HEADS, num_key_value_heads=KV_HEADS, head_dim=HEAD_DIM, max_position_embeddings=4096,
                       rope_parameters={"rope_type": "default", "rope_theta": THETA}, rms_norm_eps=EPS, attention_bias=False,
                       tie_word_embeddings=False, use_sliding_window=False, attn_implementation="eager")


def _cached_walk(m, x: torch.Tensor):
    """prefill of PREFILL tokens, then one token at a time; (prefill hidden state, hidden states of the steps) as fp32 arrays"""
    steps = []
    with torch.no_grad():
        o = m(inputs_embeds=x[:, :PREFILL], use_cache=True)
        steps.append(o.last_hidden_state.float().numpy().astype(np.float32))
        for s in range(PREFILL, S):
            o = m(inputs_embeds=x[:, s:s + 1], past_key_values=o.past_key_values, use_cache=True)
            steps.append(o.last_hidden_state.float().numpy().astype(np.float32))
    return steps[0], np.concatenate(steps[1:], axis=1)


def compute() -> dict:
    from transformers import Qwen3Model

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
    xt = torch.from_numpy(x)
    with torch.no_grad():
        full = m(inputs_embeds=xt, use_cache=False).last_hidden_state.numpy().astype(np.float32)
    res = {"w/" + k: v for k, v in w.items()}
    res.update(seed=np.int64(SEED), cfg=np.array([VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS, HEAD_DIM], dtype=np.int64),
               rope_theta=np.float64(THETA), rms_norm_eps=np.float64(EPS), names=np.array(list(w)),
               inputs_embeds=x, last_hidden_state=full)
    res["cached_prefill"], res["cached_steps"] = _cached_walk(m, xt)
    # the same model in bf16 (weights and inputs are on the bf16 grid already): HF's own bf16-vs-fp32 distance on these steps
    m16 = Qwen3Model(cfg).eval()
    m16.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m16 = m16.bfloat16()
    _, res["cached_steps_bf16"] = _cached_walk(m16, xt.bfloat16())
    return res


def rel(a: np.ndarray, b: np.ndarray) -> float:
    """the suite's distance (tests/helpers.py rel_err): max |a - b| / max |b|"""
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())


def main():
    res = compute()
    path = os.path.join(GOLD, "qwen3_d64.npz")
    np.savez_compressed(path, **res)
    full, cached = res["last_hidden_state"], np.concatenate([res["cached_prefill"], res["cached_steps"]], axis=1)
    d16 = [rel(res["cached_steps_bf16"][:, t], res["cached_steps"][:, t]) for t in range(STEPS)]
    print(f"[gen_golden_qwen3_decode] |h| {np.abs(full).max():.4f} cached-vs-full {np.abs(full - cached).max():.2e} "
          f"bf16-vs-fp32 per step {' '.join(f'{e:.2e}' for e in d16)} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.exit(main())
