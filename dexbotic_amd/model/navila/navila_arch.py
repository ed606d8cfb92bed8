"""NaVILA policy: host-side mirror of dexbotic/model/navila/navila_arch.py on libdexbotic_amd kernels.

Several frames per sample go through the SigLIP tower (``hidden_states[-2]``: the last layer and post_layernorm never run,
mm_vision/siglip/siglip_encoder.py:13,61-65), the `mlp_downsample` projector merges 2x2 neighbouring tokens
(mm_projector/builder.py:9-33,62-69), and the frames of a sample are spliced into ITS prompt: a sample's placeholders share the
sample's own feature rows (navila_arch.py:156-214), not one block per placeholder counted across the batch.  The Qwen2 decoder
is trained with the causal-LM loss whose "time" tokens get Gaussian soft targets (navila/loss.py) when ``time_token_ids`` is
configured and the model is in training mode; otherwise with the standard loss.  Sequence repacking
(``repack_multimodal_data``) never runs with the HF Qwen2 backbone in the reference and is not mirrored.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from ... import functional as Fn
from ... import hostcpu
from ... import kernels as K
from ...constants import IGNORE_INDEX
from ...engine import building
from ...splice import SplicePlan, build_navila_splice_plan
from ..dexbotic_arch import (CausalLMOutputDexbotic, DexboticConfig, DexboticForCausalLM, DexboticVLMModel,
                             register_model_with_hf, register_with_hf)
from ..modules.mm_projector.builder import DownsampleProjector
from ..modules.mm_vision.builder import build_vision_tower


class NaVILAConfig(DexboticConfig):
    model_type = "dexbotic_navila"

    def __init__(self, mm_projector_type: Optional[str] = "mlp_downsample", chat_template: Optional[str] = "llama_3",
                 time_token_ids: Optional[List[int]] = None, soft_ce_std: float = 1.0, **kwargs):
        super().__init__(mm_projector_type=mm_projector_type, chat_template=chat_template, **kwargs)
        self.time_token_ids = None if time_token_ids is None else [int(i) for i in time_token_ids]
        self.soft_ce_std = float(soft_ce_std)
        self.tie_word_embeddings = False               # lm_head is never tied (navila_arch.py:219,239-252)


register_with_hf(NaVILAConfig)


class NaVILAModel(DexboticVLMModel):
    def _build_mm_vision_module(self, config):
        if getattr(self, "mm_vision_tower", None) is not None:
            return self.mm_vision_tower
        with building(self.store):
            self.mm_vision_tower = build_vision_tower(config, select_layer=-2)
        self.config.mm_hidden_size = self.mm_vision_tower.hidden_size
        return self.mm_vision_tower

    def encode_images(self, images: torch.Tensor) -> torch.Tensor:
        return self.mm_projector_module(self.mm_vision_module(images))

    def num_image_tokens(self, images: torch.Tensor) -> int:
        """feature rows one SAMPLE owns: frames x tokens per frame after the projector's 2x2 merge"""
        frames = images.shape[1] if images.ndim == 5 else 1
        per = self.mm_vision_module.num_patches
        if isinstance(self.mm_projector_module, DownsampleProjector):
            per = DownsampleProjector.num_tokens(per)
        return frames * per

    def _splice_plan(self, input_ids, attention_mask, labels, images) -> SplicePlan:
        return self._plans.get(input_ids, attention_mask, labels, self.num_image_tokens(images),
                               getattr(self.config, "tokenizer_model_max_length", None),
                               getattr(self.config, "tokenizer_padding_side", "right"), rule="navila",
                               n_feature_samples=int(images.shape[0]))


class NaVILAForCausalLM(DexboticForCausalLM):
    config_class = NaVILAConfig
    _tied_weights_keys: list = []

    def _real_init(self, config):
        self.model = NaVILAModel(config, self.store)
        self.store.new_bucket()
        self.store.register([("lm_head.weight", (config.vocab_size, config.hidden_size))])
        self._soft_tokens = None

    @property
    def mm_projector_prefix(self) -> str:
        return "model.mm_projector"

    @property
    def mm_vision_prefix(self) -> str:
        return "model.mm_vision_tower"

    def _soft(self) -> Optional["K.SoftTokens"]:
        """the configured time tokens on the device (built once per (ids, std)); None when the standard loss applies"""
        ids = getattr(self.config, "time_token_ids", None)
        if not (self.training and ids):
            return None
        key = (tuple(int(i) for i in ids), float(getattr(self.config, "soft_ce_std", 1.0)))
        if self._soft_tokens is None or self._soft_tokens[0] != key:
            if max(key[0]) >= self.config.vocab_size or min(key[0]) < 0:
                raise ValueError(f"time_token_ids {list(key[0])} outside the vocabulary of {self.config.vocab_size}")
            self._soft_tokens = (key, K.SoftTokens(key[0], key[1], self.store.device))
        return self._soft_tokens[1]

    def forward(self, input_ids=None, images=None, attention_mask=None, position_ids=None, past_key_values=None,
                seqlens_in_batch=None, inputs_embeds=None, labels=None, use_cache=None, output_attentions=None,
                output_hidden_states=None, return_dict=None, cache_position=None, image_masks=None) -> CausalLMOutputDexbotic:
        soft = self._soft() if labels is not None else None
        if soft is None:
            return super().forward(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                                   past_key_values=past_key_values, labels=labels, images=images, cache_position=cache_position)
        (_, position_ids, attention_mask, past_key_values, inputs_embeds, labels, cache_position
         ) = self.model._prepare_inputs_labels_for_multimodal(input_ids, position_ids, attention_mask, past_key_values,
                                                               labels, cache_position, images)
        hidden = self.model.run_llm(inputs_embeds, attention_mask)
        lab = self.model._last_plan.labels
        shifted = np.full_like(lab, IGNORE_INDEX)
        shifted[:, :-1] = lab[:, 1:]
        n_valid = int((shifted != IGNORE_INDEX).sum())
        loss, logits = Fn.LmHeadSoftLossFn.apply(hidden, self.store.params["lm_head.weight"], self.store, "lm_head.weight",
                                                 hostcpu.upload(shifted.reshape(-1), hidden.device), n_valid, soft)
        return CausalLMOutputDexbotic(loss=loss, logits=logits, hidden_states=(hidden,))

    def _generation_plan(self, input_ids: np.ndarray, attention_mask: Optional[np.ndarray], feats: torch.Tensor) -> SplicePlan:
        return build_navila_splice_plan(input_ids, attention_mask, None, feats.shape[1], feats.shape[0],
                                        getattr(self.config, "tokenizer_model_max_length", None),
                                        getattr(self.config, "tokenizer_padding_side", "right"))


register_model_with_hf(NaVILAForCausalLM)
