"""The adaptive-RMSNorm Gemma decoder of pi0.5 (dexbotic/model/pi05/transformers_pi05/gemma: ``model_type: "adarms_gemma"``).

With ``use_adarms=False`` it is a Gemma decoder (``GemmaExpert`` serves it).  With ``use_adarms=True`` no norm has a gain: every
``GemmaRMSNorm`` owns ``dense = nn.Linear(adarms_cond_dim, 3 * hidden)`` whose output, per sample, is [scale | shift | gate]
(modeling_gemma.py:38-89) — ``AdaRMSGemmaExpert`` registers those parameters and names the layers; the arithmetic is
``functional.MotLayerFn``'s adaptive-norm kind, chosen by ``ln1 is None`` (kernels dxa_adarms_* / dxa_gated_residual_*).

Arena order: the 2 L + 1 ``dense`` weights lie back to back, and so do their biases, so that ONE product evaluates every norm's
modulation (``functional.FusedLinearFn`` over ``dense_w`` / ``dense_b``).  The state-dict order is the reference's all the same
(Pi05ForCausalLM.state_dict)."""
from __future__ import annotations

from dataclasses import asdict, dataclass
from typing import Optional, Tuple

import torch.nn as nn

from ... import functional as Fn
from ...engine import ParamStore
from .gemma import GemmaConfig


@dataclass
class AdaRMSGemmaConfig(GemmaConfig):
    """GemmaConfig + the reference's two switches and ``width`` (pi05_arch.py:94-99 sizes the time MLP by it)"""
    model_type: str = "adarms_gemma"
    use_adarms: bool = False
    adarms_cond_dim: Optional[int] = None
    width: Optional[int] = None

    def to_dict(self):
        return asdict(self)

    @classmethod
    def from_any(cls, obj, which: str = "config") -> "AdaRMSGemmaConfig":
        if isinstance(obj, cls):
            return obj
        d = obj if isinstance(obj, dict) else (obj.to_dict() if hasattr(obj, "to_dict") else vars(obj))
        mt = d.get("model_type", "adarms_gemma")
        if mt not in ("adarms_gemma", "gemma"):
            raise ValueError(f"pi0.5 {which}.model_type={mt!r}: the experts of the pi0.5 mixture are 'adarms_gemma' decoders "
                             "(the llm may also be a plain 'gemma'); no other type is supported")
        rp = d.get("rope_parameters") or {}
        kw = {k: v for k, v in d.items() if k in cls.__dataclass_fields__ and v is not None}
        kw["rope_theta"] = d.get("rope_theta") or rp.get("rope_theta", 10000.0)
        kw["model_type"] = mt
        c = cls(**kw)
        if c.use_adarms and c.adarms_cond_dim is None:
            c.adarms_cond_dim = c.hidden_size                 # configuration_gemma.py:141-142
        return c

    def plain(self) -> GemmaConfig:
        """the Gemma arithmetic of this config, for GemmaExpert"""
        return GemmaConfig(**{k: getattr(self, k) for k in GemmaConfig.__dataclass_fields__ if k != "model_type"})


class AdaRMSGemmaExpert(nn.Module):
    """parameters of AdaRMSGemmaModel(use_adarms=True) under HF's names; ``layer_specs[i]`` names a layer's matrices (its norms have
    no parameter of their own: ln1 / ln2 are None), ``dense_w`` / ``dense_b`` the norms' dense layers in evaluation order:
    layer 0 input, layer 0 post-attention, layer 1 input, ..., the final norm"""

    def __init__(self, store: ParamStore, prefix: str, config: AdaRMSGemmaConfig):
        super().__init__()
        self.store, self.p, self.config = store, prefix, config
        c = config
        d, f, hd, Hq, Hkv = c.hidden_size, c.intermediate_size, c.head_dim, c.num_attention_heads, c.num_key_value_heads
        store.new_bucket()
        store.register([(prefix + "embed_tokens.weight", (c.vocab_size, d))])
        self.layer_specs = []
        norms = []
        for i in range(c.num_hidden_layers):
            lp = f"{prefix}layers.{i}."
            store.new_bucket()
            qkv = tuple(lp + f"self_attn.{n}_proj.weight" for n in "qkv")
            gu = (lp + "mlp.gate_proj.weight", lp + "mlp.up_proj.weight")
            store.register([(qkv[0], (Hq * hd, d)), (qkv[1], (Hkv * hd, d)), (qkv[2], (Hkv * hd, d))])
            store.register([(lp + "self_attn.o_proj.weight", (d, Hq * hd))])
            store.register([(gu[0], (f, d)), (gu[1], (f, d))])
            store.register([(lp + "mlp.down_proj.weight", (d, f))])
            self.layer_specs.append(Fn.GemmaLayerSpec(ln1=None, qkv=qkv, o=lp + "self_attn.o_proj.weight", ln2=None, gu=gu,
                                                      down=lp + "mlp.down_proj.weight", d=d, F=f, eps=c.rms_norm_eps))
            norms += [lp + "input_layernorm.dense", lp + "post_attention_layernorm.dense"]
        norms.append(prefix + "norm.dense")
        store.new_bucket()
        self.dense_w: Tuple[str, ...] = tuple(n + ".weight" for n in norms)
        self.dense_b: Tuple[str, ...] = tuple(n + ".bias" for n in norms)
        store.register([(n, (3 * d, c.adarms_cond_dim)) for n in self.dense_w])
        store.register([(n, (3 * d,)) for n in self.dense_b])

    @property
    def n_norms(self) -> int:
        return len(self.dense_w)
