"""OFT policy: host-side mirror of dexbotic/model/oft/oft_arch.py on libdexbotic_amd kernels.

No sampler and no token-by-token decode: ``chunk_size x action_dim`` learned query rows (``action_head.action_query``) are placed
behind every sample's un-padded prompt rows — preceded by ONE projected proprio row with ``use_proprio`` — ONE causal decoder pass
runs, and the MLP-ResNet head reads the ``action_dim`` hidden rows of each time step as one row of ``action_dim x hidden`` columns
(oft_arch.py:104-147, oft/action_model/model.py:129-160).  Trained with an L1 loss.

Sequence layout (``insert_action_embedding``, :169-201): sample b has len_b spliced rows; its Q = T A (+ 1) rows go to positions
len_b ... len_b + Q - 1, padding follows; the mask is true on [0, len_b + Q); position ids are arange(S + Q).  Here the splice plan
reserves those rows (splice.build_oft_splice_plan), dxa_splice_fwd zero-fills them and dxa_action_put_fwd writes them in place
(functional.OftSpliceFn); the head's first LayerNorm reads its rows out of the decoder output at the same offsets
(functional.ActionNormFn).  Left padding is refused.  This class runs the ``Linear`` head; the ``Discrete`` head belongs to
oft_discrete_arch.py, the ``DiT`` (diffusion) head to oft_diffusion_arch.py (action_model/builder.py).
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from ... import functional as Fn
from ... import hostcpu
from ...engine import building
from ...splice import SplicePlan
from ..dexbotic_arch import (ActionOutputForCausalLM, CausalLMOutputDexbotic, DexboticConfig, DexboticForCausalLM,
                             DexboticVLMModel, register_model_with_hf, register_with_hf)
from .action_model.builder import build_action_model


class OFTConfig(DexboticConfig):
    model_type = "dexbotic_oft"

    def __init__(self, action_model_type: Optional[str] = None, action_dim: Optional[int] = None,
                 chunk_size: Optional[int] = None, use_proprio: Optional[bool] = False, proprio_dim: Optional[int] = None,
                 **kwargs):
        super().__init__(**kwargs)
        self.action_model_type = action_model_type
        self.action_dim = action_dim
        self.chunk_size = chunk_size
        self.use_proprio = use_proprio
        self.proprio_dim = proprio_dim


register_with_hf(OFTConfig)


class OFTModel(DexboticVLMModel):
    def __init__(self, config: OFTConfig, store):
        super().__init__(config, store)
        self.action_head = None
        if config.action_model_type is not None:
            self.action_head = self._build_action_head_module(config)

    def _build_action_head_module(self, config: OFTConfig):
        if getattr(self, "action_head", None) is not None:
            return self.action_head
        with building(self.store):
            self.action_head = build_action_model(config)
        return self.action_head

    @property
    def action_head_module(self) -> nn.Module:
        return self.action_head

    @property
    def action_head_prefix(self) -> str:
        return "action_head"

    def num_inserted_rows(self) -> int:
        """Q: the query rows, plus the proprio row in front of them"""
        return self.action_head.num_query_rows + (1 if self.config.use_proprio else 0)

    def oft_plan(self, input_ids, attention_mask, labels, images) -> SplicePlan:
        """the (cached) plan of the spliced prompt WITH the Q reserved rows behind each sample's rows"""
        return self._plans.get(input_ids, attention_mask, labels, self.num_image_tokens(images),
                               getattr(self.config, "tokenizer_model_max_length", None),
                               getattr(self.config, "tokenizer_padding_side", "right"), rule="oft",
                               n_query_rows=self.num_inserted_rows())

    @staticmethod
    def plan_offsets(plan: SplicePlan, device) -> torch.Tensor:
        """``non_padding_lengths`` (oft_arch.py:175) on the device: the first row of each sample's reserved block; uploaded once
        per plan"""
        cache = plan.__dict__.setdefault("_off", {})
        key = str(device)
        if key not in cache:
            cache[key] = hostcpu.upload(np.ascontiguousarray(plan.lengths, dtype=np.int64), device)
        return cache[key]


class OFTForCausalLM(DexboticForCausalLM, ActionOutputForCausalLM):
    config_class = OFTConfig

    def _real_init(self, config: OFTConfig):
        if getattr(config, "tokenizer_padding_side", "right") == "left":
            raise ValueError("OFT: tokenizer_padding_side='left' is not supported (the reference's insert_action_embedding counts the "
                             "action rows from the left edge and is wrong there); use right padding")
        self.model = OFTModel(config, self.store)
        self.store.new_bucket()
        self.store.register([("lm_head.weight", (config.vocab_size, config.hidden_size))])

    def unused_parameter_names(self) -> List[str]:
        """parameters that never get a gradient in OFT training (lm_head: the head reads the hidden states directly; the CLIP layer
        after hidden_states[-2] and post_layernorm): skipped by an external loop's bookkeeping and by the DP reducer"""
        return ["lm_head.weight"] + self.model.mm_vision_tower.unused_parameter_names()

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, images=None,
                return_dict=None, cache_position=None, actions=None, states=None, noisy_dict=None,
                **kwargs) -> CausalLMOutputDexbotic:
        model, cfg, st = self.model, self.config, self.store
        head = model.action_head
        if head is None:
            raise ValueError("OFT: config.action_model_type is not set: there is no action head to run")
        if model.mm_vision_module is None or images is None:
            raise NotImplementedError("text-only forward is outside the VLA path")
        A, T = cfg.action_dim, cfg.chunk_size
        # the integer plan first (host arithmetic on a few KB), then the device work is enqueued
        plan = model.oft_plan(input_ids, attention_mask, labels, images)
        model._last_plan = plan
        dev = st.device
        image_features = model._extract_vision_features(images.to(device=dev, dtype=st.compute_dtype))
        state_embeds = None
        if cfg.use_proprio:
            assert states is not None, "states is required when use_proprio is True"
            state_embeds = head.proprio_projector(states)                                # [B, d]: one row per sample
        pd = plan.dev(dev)
        off = model.plan_offsets(plan, dev)
        B, Sq = plan.plan.shape
        embed_n = model.llm.embed_name
        embeds = Fn.OftSpliceFn.apply(image_features, state_embeds, st.params[embed_n], st, embed_n, head.query_name, pd["plan"],
                                      off, B, Sq).view(B, Sq, -1)
        # causal attention, key range [0, len_b + Q) per sample (all of it when nothing is padded), positions arange(S + Q)
        mask = plan.attention_mask if attention_mask is not None else None
        hidden = model.run_llm(embeds, mask)
        predicted_actions = head.predict_action(hidden, off, bool(cfg.use_proprio))      # [B, T, A]
        loss = None
        if actions is not None:
            target = actions.to(device=dev, dtype=torch.float32).reshape(actions.size(0), -1, A)[:, :T, :].contiguous()
            loss = Fn.L1LossFn.apply(predicted_actions, target)
        return CausalLMOutputDexbotic(loss=loss, logits=predicted_actions, past_key_values=None, hidden_states=(hidden,),
                                      attentions=None)

    __call__ = nn.Module.__call__

    @torch.no_grad()
    def inference_action(self, input_ids, image_tensor, inference_args={}, **kwargs):
        """Reference contract (oft_arch.py:212-254, ``Linear`` branch): one full pass, the first sample's [T][A] actions
        de-normalised with ``inference_args["action_norms"]``; ``inference_args["states"]`` feeds the proprio row."""
        action_norms = inference_args.get("action_norms")
        states = inference_args.get("states", None)
        out = self(input_ids, images=image_tensor, use_cache=True, states=states)
        actions = out.logits[0]
        return self._denorm(actions.float().cpu().numpy(), action_norms).tolist()


register_model_with_hf(OFTForCausalLM)
