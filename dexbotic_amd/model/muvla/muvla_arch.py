"""MuVLA policy: host-side mirror of dexbotic/model/muvla/muvla_arch.py on libdexbotic_amd kernels.

``images`` is [B, V, 3, H, W]: image 0 is the map, image 1 the current observation, images 2.. the history.  The observation
frames go through the obs CLIP tower (``hidden_states[-2]`` without the class token), the history through ``SimpleQFormer`` (192
learned queries, one 8-head nn.MultiheadAttention over input_proj(history), LayerNorm, no residual), and
``cat([qformer, current])`` is fused against the map tower's tokens by ``CrossFuseReduce``: LN(MHA(obs, map, map) + obs) with 16
heads (muvla_arch.py:28-64,224-247).  The `mlp2x_gelu` projector turns the fused rows into ONE block of 192 + N (or N, without
history) rows per sample, spliced at that sample's placeholder by the base planner; the Qwen2 decoder follows.  The loss
(muvla_arch.py:559-592) is the per-sample normalised cross-entropy weighted by 1 + sigmoid(reward), plus an expectile regression
(0.9) of ``reward_head(hidden)[:, -1]`` — the last position of the PADDED sequence, as in the reference — weighted 0.5 beside the
language loss and 0.2 on its own.  4-D ``images`` take the base class's path.

Left out on purpose: the reference's ``_assert_finite`` checks of inputs_embeds, attention_mask, hidden_states and logits: each is
a device-wide synchronisation in the middle of the step.  The ``nn.MSELoss`` value the reference computes and overwrites
(muvla_arch.py:582-583) is not computed.  ``fuser.reduce_proj`` / ``fuser.back_proj`` exist in the checkpoint and are never used.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from ... import _lib as L
from ... import functional as Fn
from ... import hostcpu
from ... import kernels as K
from ...constants import IGNORE_INDEX
from ...engine import Fp32View, ParamStore
from ...splice import PlanCache
from ..dexbotic_arch import (CausalLMOutputDexbotic, DexboticConfig, DexboticForCausalLM, DexboticVLMModel,
                             register_model_with_hf, register_with_hf)
from ..llm.qwen3 import build_llm_backbone
from ..modules.mm_projector.builder import build_vision_projector
from ..modules.mm_vision.builder import build_vision_tower

FUSE_DIM = 1024          # widths fixed by the checkpoint format (muvla_arch.py:143,149)
NUM_QUERIES = 192
QFORMER_HEADS = 8
EXPECTILE = 0.9


class MUVLAConfig(DexboticConfig):
    model_type = "dexbotic"                    # the reference shares the base class's registry string (muvla_arch.py:18)

    def __init__(self, obs_vision_tower=None, mm_projector_type: Optional[str] = "mlp2x_gelu",
                 chat_template: Optional[str] = "dexbotic", action_model_type: Optional[str] = None,
                 action_dim: Optional[int] = None, chunk_size: Optional[int] = None, **kwargs):
        super().__init__(mm_projector_type=mm_projector_type, chat_template=chat_template, **kwargs)
        self.obs_vision_tower = obs_vision_tower
        self.action_model_type, self.action_dim, self.chunk_size = action_model_type, action_dim, chunk_size


register_with_hf(MUVLAConfig)


def _mha_names(p: str):
    return p + "in_proj_weight", p + "in_proj_bias", p + "out_proj.weight", p + "out_proj.bias"


def _register_mha(store: ParamStore, p: str, E: int) -> None:
    store.register([(p + "in_proj_weight", (3 * E, E)), (p + "in_proj_bias", (3 * E,))])
    store.register([(p + "out_proj.weight", (E, E)), (p + "out_proj.bias", (E,))])


class SimpleQFormer(nn.Module):
    """LN(MHA(query = query_embeddings, key = value = input_proj(x))): muvla_arch.py:50-64.  The queries are the same for every
    sample, so their in-projection runs once per forward on [192, E] rows and is broadcast; the backward sums dq over the batch
    before the projection's weight gradient."""

    def __init__(self, store: ParamStore, prefix: str, E: int = FUSE_DIM, num_queries: int = NUM_QUERIES, heads: int = QFORMER_HEADS):
        super().__init__()
        self.store, self.p, self.E, self.nq, self.H = store, prefix, E, num_queries, heads
        store.new_bucket()
        store.register([(prefix + "query_embeddings", (num_queries, E))])
        store.register([(prefix + "input_proj.weight", (E, E)), (prefix + "input_proj.bias", (E,))])
        _register_mha(store, prefix + "attn.", E)
        store.register([(prefix + "norm.weight", (E,)), (prefix + "norm.bias", (E,))], layernorm=True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, T, E] -> [B, 192, E]"""
        st, p, E, H = self.store, self.p, self.E, self.H
        B, T, _ = x.shape
        anchor = st.params[p + "input_proj.weight"]
        mem = Fn.LinearFn.apply(x.reshape(B * T, E), anchor, st, p + "input_proj.weight", p + "input_proj.bias", L.ACT_NONE, None)
        wn, bn, ow, ob = _mha_names(p + "attn.")
        queries = Fn.ParamFn.apply(st.params[p + "query_embeddings"], st, p + "query_embeddings")
        q, kv = Fn.PackedInProjFn.apply(queries, mem, anchor, st, wn, bn, E)              # q [192, E] once, [k | v] [B*T, 2E]
        qb = Fn.BroadcastBatchFn.apply(q.view(self.nq, H, E // H), B)
        o = Fn.AttnPackedFn.apply(qb, kv.view(B, T, 2, H, E // H)).reshape(B * self.nq, E)
        o = Fn.LinearFn.apply(o, anchor, st, ow, ob, L.ACT_NONE, None)
        return Fn.NormFn.apply(o, anchor, st, "ln", p + "norm.weight", p + "norm.bias", 1e-5).view(B, self.nq, E)


class CrossFuseReduce(nn.Module):
    """LN(MHA(query = obs, key = value = map) + obs) with E / 64 heads: muvla_arch.py:28-48.  ``reduce_proj`` and ``back_proj``
    are registered for the checkpoint's sake and never applied."""

    def __init__(self, store: ParamStore, prefix: str, E: int = FUSE_DIM):
        super().__init__()
        self.store, self.p, self.E, self.H = store, prefix, E, E // 64
        store.new_bucket()
        store.register([(prefix + "reduce_proj.weight", (E, 4096)), (prefix + "reduce_proj.bias", (E,))])
        _register_mha(store, prefix + "cross_attn.", E)
        store.register([(prefix + "ln.weight", (E,)), (prefix + "ln.bias", (E,))], layernorm=True)
        store.register([(prefix + "back_proj.weight", (4096, E)), (prefix + "back_proj.bias", (4096,))])

    def unused_parameter_names(self) -> List[str]:
        return [n for n in self.store.slots if n.startswith(self.p + "reduce_proj.") or n.startswith(self.p + "back_proj.")]

    def forward(self, map_tk: torch.Tensor, obs_tk: torch.Tensor) -> torch.Tensor:
        """map [B, N, E], obs [B, M, E] -> [B, M, E]"""
        st, p, E, H = self.store, self.p, self.E, self.H
        B, M, _ = obs_tk.shape
        N = map_tk.shape[1]
        wn, bn, ow, ob = _mha_names(p + "cross_attn.")
        anchor = st.params[wn]
        obs_q, obs_r = Fn.ForkFn.apply(obs_tk.reshape(B * M, E))
        q, kv = Fn.PackedInProjFn.apply(obs_q, map_tk.reshape(B * N, E), anchor, st, wn, bn, E)
        o = Fn.AttnPackedFn.apply(q.view(B, M, H, E // H), kv.view(B, N, 2, H, E // H)).reshape(B * M, E)
        a = Fn.LinearFn.apply(o, anchor, st, ow, ob, L.ACT_NONE, None)
        return Fn.AddNormFn.apply(a, obs_r, anchor, st, p + "ln.weight", p + "ln.bias", 1e-5).view(B, M, E)


class MUVLAModel(DexboticVLMModel):
    def __init__(self, config: MUVLAConfig, store: ParamStore):
        nn.Module.__init__(self)
        self.config, self.store = config, store
        if getattr(config, "mm_vision_tower", None) is None or getattr(config, "obs_vision_tower", None) is None:
            raise ValueError("MUVLA needs both config.mm_vision_tower (map) and config.obs_vision_tower (observations)")
        # registration order = forward order = arena order (the DP reducer walks it backwards)
        self.mm_vision_tower = self.mm_projector = self.obs_vision_tower = None
        self.obs_vision_tower = self._build_obs_vision_module(config.obs_vision_tower)
        self.history_qformer = SimpleQFormer(store, "model.history_qformer.")
        self.mm_vision_tower = self._build_mm_vision_module(config.mm_vision_tower)
        self.fuser = CrossFuseReduce(store, "model.fuser.")
        self.mm_projector = self._build_mm_projector_module(config)
        self.llm = build_llm_backbone(store, "model.llm.", config.llm_config)
        self._last_plan = None
        self._plans = PlanCache()

    @staticmethod
    def _check_width(tower, which: str):
        if tower.hidden_size != FUSE_DIM:
            raise ValueError(f"MUVLA: the {which} tower is {tower.hidden_size} wide; the fuser and the Q-former of the checkpoint "
                             f"format are fixed at {FUSE_DIM}")
        return tower

    def _build_mm_vision_module(self, config):
        if getattr(self, "mm_vision_tower", None) is not None:
            return self.mm_vision_tower
        self.mm_vision_tower = self._check_width(build_vision_tower(config, self.store, "model.mm_vision_tower."), "map (mm_vision_tower)")
        self.config.mm_hidden_size = self.mm_vision_tower.hidden_size
        return self.mm_vision_tower

    def _build_obs_vision_module(self, config):
        if getattr(self, "obs_vision_tower", None) is not None:
            return self.obs_vision_tower
        self.obs_vision_tower = self._check_width(build_vision_tower(config, self.store, "model.obs_vision_tower."), "observation (obs_vision_tower)")
        self.config.obs_hidden_size = self.obs_vision_tower.hidden_size
        return self.obs_vision_tower

    def _build_mm_projector_module(self, config):
        if getattr(self, "mm_projector", None) is not None:
            return self.mm_projector
        self.mm_projector = build_vision_projector(config, self.store, "model.mm_projector.")
        return self.mm_projector

    def fuse_obs_with_history_and_project(self, map_img: torch.Tensor, obs_imgs: torch.Tensor) -> torch.Tensor:
        """map [B, 3, H, W], observations [B, 1 + T, 3, H, W] (current first) -> [B, 192 + N or N, d] (muvla_arch.py:224-247).
        Current and history frames go through the obs tower in one call, the current frames first."""
        B, V1 = obs_imgs.shape[:2]
        T = V1 - 1
        if T == 0:
            obs = self.obs_vision_tower(obs_imgs[:, 0].contiguous())
        else:
            frames = torch.cat([obs_imgs[:, 0], obs_imgs[:, 1:].flatten(0, 1)], dim=0)
            cur, hist = Fn.SplitRowsFn.apply(self.obs_vision_tower(frames), B)                    # [B, N, E], [B*T, N, E]
            N, E = cur.shape[1], cur.shape[2]
            qf = self.history_qformer(hist.reshape(B, T * N, E))
            obs = Fn.CatLastFn.apply(qf.reshape(B, NUM_QUERIES * E), cur.reshape(B, N * E)).view(B, NUM_QUERIES + N, E)
        fused = self.fuser(self.mm_vision_tower(map_img.contiguous()), obs)
        return self.mm_projector_module(fused)

    def _extract_vision_features(self, images: torch.Tensor) -> torch.Tensor:
        if images.ndim == 5:
            if images.shape[1] < 2:
                raise ValueError("MUVLA: 5-D images hold the map and at least the current observation (V >= 2)")
            return self.fuse_obs_with_history_and_project(images[:, 0], images[:, 1:])
        return super()._extract_vision_features(images)

    def num_image_tokens(self, images: torch.Tensor) -> int:
        """rows one placeholder expands to: 192 query rows (with history) + the obs tower's patches; 4-D images: the base rule"""
        if images.ndim == 5:
            return (NUM_QUERIES if images.shape[1] > 2 else 0) + self.obs_vision_tower.num_patches
        return super().num_image_tokens(images)


class MUVLAForCausalLM(DexboticForCausalLM):
    config_class = MUVLAConfig
    _tied_weights_keys: list = []

    def _real_init(self, config):
        self.model = MUVLAModel(config, self.store)
        self.store.new_bucket()
        self.store.register([("lm_head.weight", (config.vocab_size, config.hidden_size))])
        self.store.new_bucket()
        self.store.register([("reward_head.weight", (1, config.hidden_size))])

    @property
    def mm_projector_prefix(self) -> str:
        return "model.mm_projector"

    @property
    def mm_vision_prefix(self) -> str:
        return "model.mm_vision_tower"

    def unused_parameter_names(self) -> List[str]:
        """parameters no loss reaches: ``reduce_proj`` / ``back_proj`` and each tower's last layer and post_layernorm.  (A batch
        without history frames or without rewards simply does not announce the Q-former / ``reward_head``.)"""
        m = self.model
        return m.fuser.unused_parameter_names() + m.obs_vision_tower.unused_parameter_names() + m.mm_vision_tower.unused_parameter_names()

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, images=None,
                return_dict=None, cache_position=None, actions=None, states=None, repeated_diffusion_steps: int = 4,
                reward=None, **kwargs) -> CausalLMOutputDexbotic:
        (_, position_ids, attention_mask, past_key_values, inputs_embeds, labels, cache_position
         ) = self.model._prepare_inputs_labels_for_multimodal(input_ids, position_ids, attention_mask, past_key_values,
                                                               labels, cache_position, images)
        hidden = self.model.run_llm(inputs_embeds, attention_mask)
        B, S, d = hidden.shape
        st = self.store
        if reward is not None:
            reward = reward.to(device=hidden.device, dtype=torch.float32).reshape(B).contiguous()
            h_lm, h_rw = Fn.ForkFn.apply(hidden)
        else:
            h_lm = hidden
        loss = None
        if labels is None:
            with torch.no_grad():
                logits = K.mm_nt(h_lm.reshape(B * S, d).contiguous(), st.w("lm_head.weight")).view(B, S, -1)
        else:
            lab = self.model._last_plan.labels
            shifted = np.full_like(lab, IGNORE_INDEX)
            shifted[:, :-1] = lab[:, 1:]
            loss, logits = Fn.LmHeadSampleLossFn.apply(h_lm, st.params["lm_head.weight"], st, "lm_head.weight",
                                                       hostcpu.upload(shifted.reshape(-1), hidden.device), B, reward)
        if reward is not None:
            # reward_head(hidden)[:, -1]: only the last position of the padded sequence is scored, so only its B rows are projected
            last = torch.arange(1, B + 1, dtype=torch.int64) * S - 1
            h_last = Fn.GatherRowsFn.apply(h_rw.reshape(B * S, d), hostcpu.upload(last, hidden.device))     # fp32 [B, d]
            pred = Fn.LinearFn.apply(h_last, st.params["reward_head.weight"], Fp32View(st), "reward_head.weight", None,
                                     L.ACT_NONE, None).reshape(B)
            reward_loss = Fn.ExpectileLossFn.apply(pred, reward, EXPECTILE)
            loss = loss + 0.5 * reward_loss if loss is not None else 0.2 * reward_loss
        return CausalLMOutputDexbotic(loss=loss, logits=logits, hidden_states=(hidden,))


register_model_with_hf(MUVLAForCausalLM)
