"""Qwen3 decoder backbone on libdexbotic_amd kernels.

Stands in for the HF ``Qwen3Model`` that ``AutoModel.from_config(llm_config)`` gives the reference for a Qwen3 ``llm_config``
(dexbotic/model/dexbotic_arch.py:52-62).  Arithmetic per HF:qwen3/modeling_qwen3.py; against Qwen2 only the attention block differs:

* ``head_dim`` is a config field of its own (Qwen3-0.6B: 1024 wide, 16 heads of 128), so ``Hq * head_dim != hidden_size`` is allowed;
* q / k / v projections have no bias;
* a per-head ``RMSNorm(head_dim)`` on q (``self_attn.q_norm.weight``) and on k (``self_attn.k_norm.weight``) sits between the
  projection and RoPE.  It runs inside the RoPE / split pass (``dxa_qknorm_rope_split`` forward, ``dxa_qknorm_rope_merge`` backward).

Everything else is shared: registration and the two forward drivers are ``Qwen2Backbone``'s, switched by two class attributes, and the
layer itself — with or without a key/value cache — is the one launch sequence of ``functional.Qwen2LayerFn._run``.
Parameter names are HF's.

Single-token decode (B = 1, bf16) is the persistent one-launch step of ``Qwen2Backbone.forward_cached`` (csrc/decode_fused.hip): its
QKN instantiation normalises q and the new key per head in front of RoPE, the layer table's bias pointer is NULL and the ``[L][2]``
table of q_norm / k_norm weights rides beside it (``dxa_decode_desc.qk_norm``).  It takes head_dim 64, 128 or 256; any other
head_dim, ``DXA_DECODE_FUSED=0``, fp32 or a batch run the per-op cached path (``cache.fused_steps`` stays 0).
"""
from __future__ import annotations

from dataclasses import dataclass

from ... import kernels as K
from .qwen2 import Qwen2Backbone, Qwen2Config


@dataclass
class Qwen3Config(Qwen2Config):
    """subset of HF Qwen3Config that defines the arithmetic (defaults = Qwen3-8B)"""
    vocab_size: int = 151936
    hidden_size: int = 4096
    intermediate_size: int = 12288
    num_hidden_layers: int = 36
    num_attention_heads: int = 32
    num_key_value_heads: int = 8
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1e6
    max_position_embeddings: int = 40960
    model_type: str = "qwen3"
    head_dim: int = 128            # a field here (Qwen2Config derives it from hidden_size / num_attention_heads)

    @classmethod
    def _check_supported(cls, d: dict) -> None:
        if d.get("attention_bias"):
            raise NotImplementedError("Qwen3 llm_config with attention_bias=True: the native Qwen3 layer has no projection bias")
        if d.get("use_sliding_window") or any(t != "full_attention" for t in (d.get("layer_types") or ())):
            raise NotImplementedError("Qwen3 llm_config with sliding-window attention layers (use_sliding_window / layer_types): "
                                      "only full attention is implemented natively")
        if d.get("tie_word_embeddings"):
            raise NotImplementedError("Qwen3 llm_config with tie_word_embeddings=True: lm_head and embed_tokens are separate "
                                      "parameters here")


class Qwen3Backbone(Qwen2Backbone):
    attention_bias = False
    qk_norm = True

    def __init__(self, store, prefix: str, config: Qwen3Config):
        if config.head_dim not in K.QKNORM_HEAD_DIMS:
            raise NotImplementedError(f"Qwen3 head_dim {config.head_dim}: the fused q/k-norm + RoPE kernels take {K.QKNORM_HEAD_DIMS}")
        super().__init__(store, prefix, config)


class Qwen3Expert(Qwen3Backbone):
    """``Qwen3ForCausalLM(config).model`` with ``embed_tokens = None`` (dm0_arch.py:79-80): the action expert of DM0's mixture, which
    is only ever fed embeddings.  The layers run through ``functional.MotLayerFn`` together with the llm's."""
    has_embed_tokens = False


def llm_config_from_any(obj) -> Qwen2Config:
    """``llm_config`` (a native config, a dict, an HF config object) -> Qwen3Config for ``model_type == "qwen3"``, Qwen2Config
    otherwise (which refuses every other type)"""
    if isinstance(obj, Qwen2Config):
        return obj
    d = obj if isinstance(obj, dict) else (obj.to_dict() if hasattr(obj, "to_dict") else vars(obj))
    return (Qwen3Config if d.get("model_type") == "qwen3" else Qwen2Config).from_any(obj)


def build_llm_backbone(store, prefix: str, config: Qwen2Config) -> Qwen2Backbone:
    """the decoder the reference gets from ``AutoModel.from_config(llm_config)``"""
    return (Qwen3Backbone if config.model_type == "qwen3" else Qwen2Backbone)(store, prefix, config)
