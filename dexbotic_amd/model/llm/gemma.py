"""Gemma decoder expert on libdexbotic_amd kernels (the two backbones of the pi0 mixture of transformers).

Stands in for the HF ``GemmaModel`` objects the reference builds through ``AutoModel.from_config`` (pi0_arch.py:
86-91) and walks layer by layer in ``_inner_forward_mot`` (:116-216).  Arithmetic per HF gemma/modeling_gemma.py:
GemmaRMSNorm (fp32 normalise, scale by 1 + weight), bias-free q/k/v/o, rotate-half RoPE, GeGLU MLP
(gelu_pytorch_tanh(gate) * up), final norm.  Parameter names are HF's.  This module registers the parameters and
names them per layer (``layer_specs``); the layer's launches are the two halves the mixture needs,
``functional.gemma_pre_attention`` (norm + fused QKV) and ``functional.gemma_post_attention`` (o_proj + residual +
norm + MLP + residual), around ONE attention over BOTH experts' tokens (pi0_arch.py:161-191): the Gemma kind of
``functional.MotLayerFn``, which a ``GemmaLayerSpec`` with norm gains selects.
"""
from __future__ import annotations

from dataclasses import asdict, dataclass
from typing import Dict, Tuple

import torch
import torch.nn as nn

from ... import functional as Fn
from ...engine import ParamStore


@dataclass
class GemmaConfig:
    """subset of HF GemmaConfig that defines the arithmetic (defaults = the 2 B backbone of pi0)"""
    vocab_size: int = 257152
    hidden_size: int = 2048
    intermediate_size: int = 16384
    num_hidden_layers: int = 18
    num_attention_heads: int = 8
    num_key_value_heads: int = 1
    head_dim: int = 256
    rms_norm_eps: float = 1e-6
    rope_theta: float = 10000.0
    max_position_embeddings: int = 8192
    model_type: str = "gemma"

    def to_dict(self):
        return asdict(self)

    @classmethod
    def from_any(cls, obj) -> "GemmaConfig":
        if isinstance(obj, cls):
            return obj
        d = obj if isinstance(obj, dict) else (obj.to_dict() if hasattr(obj, "to_dict") else vars(obj))
        rp = d.get("rope_parameters") or {}
        keys = {f for f in cls.__dataclass_fields__}
        kw = {k: v for k, v in d.items() if k in keys and v is not None}
        kw["rope_theta"] = d.get("rope_theta", rp.get("rope_theta", 10000.0))
        if kw.get("model_type", "gemma") != "gemma":
            raise NotImplementedError(f"pi0 experts are Gemma models, got model_type={kw['model_type']!r}")
        return cls(**kw)


class GemmaExpert(nn.Module):
    def __init__(self, store: ParamStore, prefix: str, config: GemmaConfig):
        super().__init__()
        self.store, self.p, self.config = store, prefix, config
        c = config
        d, f, hd, Hq, Hkv = c.hidden_size, c.intermediate_size, c.head_dim, c.num_attention_heads, c.num_key_value_heads
        store.new_bucket()
        store.register([(prefix + "embed_tokens.weight", (c.vocab_size, d))])
        self.layer_specs = []
        for i in range(c.num_hidden_layers):
            lp = f"{prefix}layers.{i}."
            store.new_bucket()
            qkv = tuple(lp + f"self_attn.{n}_proj.weight" for n in "qkv")
            gu = (lp + "mlp.gate_proj.weight", lp + "mlp.up_proj.weight")
            store.register([(lp + "input_layernorm.weight", (d,))])
            store.register([(qkv[0], (Hq * hd, d)), (qkv[1], (Hkv * hd, d)), (qkv[2], (Hkv * hd, d))])
            store.register([(lp + "self_attn.o_proj.weight", (d, Hq * hd))])
            store.register([(lp + "post_attention_layernorm.weight", (d,))])
            store.register([(gu[0], (f, d)), (gu[1], (f, d))])
            store.register([(lp + "mlp.down_proj.weight", (d, f))])
            self.layer_specs.append(Fn.GemmaLayerSpec(
                ln1=lp + "input_layernorm.weight", qkv=qkv, o=lp + "self_attn.o_proj.weight",
                ln2=lp + "post_attention_layernorm.weight", gu=gu, down=lp + "mlp.down_proj.weight", d=d, F=f, eps=c.rms_norm_eps))
        store.new_bucket()
        store.register([(prefix + "norm.weight", (d,))])
        self._rope: Dict = {}

    @property
    def embed_name(self) -> str:
        return self.p + "embed_tokens.weight"

    def rope_tables(self, n_pos: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """cos/sin [n_pos, head_dim/2] fp32 (GemmaRotaryEmbedding: inv_freq = theta^(-2i/hd), angles in fp32)"""
        key = str(device)
        cur = self._rope.get(key)
        if cur is None or cur[0].shape[0] < n_pos:
            hd = self.config.head_dim
            n = max(n_pos, 1024)
            inv = 1.0 / (self.config.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
            fr = torch.arange(n, dtype=torch.float32)[:, None] * inv[None, :]
            self._rope[key] = (fr.cos().contiguous().to(device), fr.sin().contiguous().to(device))
        return self._rope[key]

    def embed(self, input_ids: torch.Tensor) -> torch.Tensor:
        """embed_tokens(ids) * sqrt(hidden) (pi0_arch.py:247-250; the 4.51 GemmaModel embedding is unscaled).
        Differentiable: the gather is the splice kernel with a tokens-only plan (its backward adds rows into the
        fp32 embedding gradient), the scale is applied in the tensor's dtype."""
        st = self.store
        d = self.config.hidden_size
        dummy = torch.zeros((1, d), device=st.device, dtype=st.compute_dtype)
        rows = Fn.SpliceFn.apply(dummy, st.params[self.embed_name], st, self.embed_name,
                                 input_ids.reshape(-1).to(device=st.device, dtype=torch.int64).contiguous())
        return Fn.ScaleFn.apply(rows, float(d) ** 0.5).view(*input_ids.shape, d)
