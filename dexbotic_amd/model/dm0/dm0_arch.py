"""DM0 policy (vision tower + dual-expert Qwen3 mixture of transformers + flow-matching action head): host-side mirror of
dexbotic/model/dm0/dm0_arch.py on libdexbotic_amd kernels.

``DM0Config`` (:35-60), ``DM0Model`` (:63-125: the base VLM's tower / projector / llm + ``action_expert``, a Qwen3 decoder without
``embed_tokens``, + the four small linears), ``DM0ForCausalLM``: ``get_prefix_hidden_states`` (:307-353),
``get_suffix_hidden_states`` (:355-404), ``_merged_attention_forward`` (:145-298) and ``inference_action`` (:513-641).  It is the
pi0 recipe on Qwen3 experts, and what differs from model/pi0/pi0_arch.py follows the reference:

* every prefix token opens a block of its own (``attn_mask`` = 1), so the prefix is CAUSAL; the suffix is [1, 0, 0, ...], one
  bidirectional block that sees every valid prefix key.  cumsum is still non-decreasing, so the mask is pi0's per-query key
  count + per-key validity, computed by the same ``mot.mask_tensors``;
* the suffix is the ``chunk_size`` action tokens alone: no state token, no ``state_proj`` (``states`` only gives the batch size);
* each expert's layer is HF Qwen3DecoderLayer arithmetic (plain RMSNorm gains, no projection bias, per-head q/k RMSNorm before RoPE,
  SwiGLU), the rotary tables are the llm's.

Every layer is ``functional.MotLayerFn`` with two experts of its Qwen3 kind: both experts' q/k-norm + RoPE launches write into ONE
q / k / v (``dxa_qknorm_rope_split_at``), one attention, two GEMM halves per expert; model/mot.py holds what pi0, pi0.5 and DM0 share.  The sampler keeps ONE key / value buffer
[B, Hkv, P + chunk, D] per layer: the prefix pass writes its keys at [0, P), every Euler step the suffix keys at [P, P + chunk) —
no concatenation and no copy for any batch size and any number of key / value heads — and the loop is replayed as one HIP graph.

bf16: the reference's ``bf16: bool`` (llm, expert, tower and projector in bf16, norm gains fp32) maps to the compute dtype of the
arena; as everywhere here the fp32 masters stay and the kernels read bf16 shadows.
"""
from __future__ import annotations

from itertools import takewhile
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from ... import _lib as L
from ... import functional as Fn
from ... import hostcpu
from ... import kernels as K
from ...engine import ParamStore
from ..dexbotic_arch import (ActionOutputForCausalLM, CausalLMOutputDexbotic, DexboticConfig, DexboticForCausalLM, DexboticVLMModel,
                             register_model_with_hf, register_with_hf)
from ..llm.qwen3 import Qwen3Expert, llm_config_from_any
from ..mot import MotPolicy, flow_times, mask_tensors
from ..pi0.pi0_arch import posemb_sincos

_GEOMETRY = ("num_hidden_layers", "num_attention_heads", "num_key_value_heads", "head_dim")


def _qwen3_config(obj, which: str):
    """``llm_config`` / ``action_config`` (a native config, a dict, an HF config object, a directory with config.json) -> Qwen3Config;
    any other model_type is refused here, by name"""
    if isinstance(obj, str):
        import json
        import os
        with open(os.path.join(obj, "config.json")) as f:
            obj = json.load(f)
    if obj is None:
        obj = {"model_type": "qwen3"}
    d = obj if isinstance(obj, dict) else (obj.to_dict() if hasattr(obj, "to_dict") else vars(obj))
    mt = d.get("model_type")
    if mt != "qwen3":
        raise ValueError(f"DM0 {which}.model_type={mt!r}: both experts of the DM0 mixture are 'qwen3' decoders (per-head q/k norm, no "
                         "projection bias); no other type is supported")
    return llm_config_from_any(obj)


class DM0Config(DexboticConfig):
    """dm0_arch.py:35-60, registered with ``AutoConfig`` under the reference's ``model_type``.  ``bf16`` is the reference's switch;
    it and ``compute_dtype`` say the same thing here (an explicit ``compute_dtype`` wins)."""
    model_type = "dexbotic_dm0"

    def __init__(self, llm_config=None, action_config=None, processor_config=None, action_dim: int = 32, chunk_size: int = 50,
                 bf16: bool = True, compute_dtype=None, **kwargs):
        llm = _qwen3_config(llm_config, "llm_config")
        act = _qwen3_config(action_config if action_config is not None else llm, "action_config")
        if compute_dtype is None:
            compute_dtype = "bfloat16" if bf16 else "float32"
        super().__init__(llm_config=llm, compute_dtype=compute_dtype, **kwargs)
        self.action_config = act
        self.processor_config = processor_config
        self.action_dim, self.chunk_size = int(action_dim), int(chunk_size)
        self.bf16 = "bfloat16" in self.compute_dtype
        bad = [k for k in _GEOMETRY if getattr(act, k) != getattr(llm, k)]
        if bad:
            raise ValueError("DM0: the two experts share one attention per layer, so depth, heads, key / value heads and head_dim must "
                             "match; llm_config and action_config differ in " +
                             ", ".join(f"{k} ({getattr(llm, k)} / {getattr(act, k)})" for k in bad))


register_with_hf(DM0Config)


class DM0Model(DexboticVLMModel):
    """registration order = forward order: vision tower, projector, llm, action expert, the four small linears"""

    def __init__(self, config: DM0Config, store: ParamStore):
        super().__init__(config, store)
        if self.mm_vision_tower is None:
            raise ValueError("DM0 needs config.mm_vision_tower")
        # Qwen3ForCausalLM(action_config) with model.embed_tokens = None: "model.action_expert.model." + its own lm_head
        self.action_expert = Qwen3Expert(store, "model.action_expert.model.", config.action_config)
        ac = config.action_config
        store.new_bucket()
        store.register([("model.action_expert.lm_head.weight", (ac.vocab_size, ac.hidden_size))])
        da, A = ac.hidden_size, config.action_dim
        store.new_bucket()
        for name, shape in (("action_in_proj", (da, A)), ("action_out_proj", (A, da)), ("action_time_mlp_in", (da, 2 * da)),
                            ("action_time_mlp_out", (da, da))):
            store.register([(f"model.{name}.weight", shape), (f"model.{name}.bias", (shape[0],))])


class DM0ForCausalLM(DexboticForCausalLM, ActionOutputForCausalLM, MotPolicy):
    config_class = DM0Config
    _tied_weights_keys: list = []
    gradient_side_stream = True          # as Pi0ForCausalLM: the small column sums beside the dX chain

    def _real_init(self, config):
        self.model = DM0Model(config, self.store)
        self.store.new_bucket()
        self.store.register([("lm_head.weight", (config.llm_config.vocab_size, config.llm_config.hidden_size))])

    @property
    def mm_projector_prefix(self) -> str:
        return "model.mm_projector"

    @property
    def mm_vision_prefix(self) -> str:
        return "model.mm_vision_tower"

    def unused_parameter_names(self) -> List[str]:
        """no gradient on the flow-matching loss: what only feeds prefix_out (the last llm layer after its q/k/v projections, the
        llm's final norm), the tower's layer after ``hidden_states[-2]`` and its post_layernorm, and the two lm_heads.  The last llm
        layer's q_proj / q_norm are NOT here: their gradient is written, and is zero (nothing reads the prefix queries' outputs)."""
        st, c = self.store, self.config
        last = f"model.llm.layers.{c.llm_config.num_hidden_layers - 1}."
        names = list(self.model.mm_vision_tower.unused_parameter_names())
        names += ["model.llm.norm.weight", "model.action_expert.lm_head.weight", "lm_head.weight"]
        names += [n for n in st.slots if n.startswith(last) and
                  (".o_proj." in n or ".mlp." in n or "post_attention_layernorm" in n)]
        return names

    # ------------------------------------------------------------------------------------ embeddings
    def encode_images(self, images: torch.Tensor) -> torch.Tensor:
        return self.model.mm_projector(self.model.mm_vision_tower(images))

    def prefix_mask(self, attention_mask, image_masks) -> np.ndarray:
        """prefix padding mask np.bool [B, CAM * T + L] from the two host-side masks alone (T = tokens per camera): the per-camera
        ``image_masks`` repeated per image token, then the text mask — a masked camera is a hole in the middle of the prefix"""
        T = self.model.mm_vision_tower.num_patches
        im = np.asarray(image_masks.cpu() if torch.is_tensor(image_masks) else image_masks, dtype=bool)
        am = np.asarray(attention_mask.cpu() if torch.is_tensor(attention_mask) else attention_mask, dtype=bool)
        return np.concatenate([np.repeat(im, T, axis=1), am], axis=1)

    def get_prefix_hidden_states(self, input_ids, images) -> torch.Tensor:
        """-> prefix tokens [B, CAM * T + L, d] (compute dtype): all cameras in one tower pass, camera-major like the reference's
        per-camera loop, then the text embeddings (the gather is the splice kernel with a tokens-only plan)"""
        B, CAM = images.shape[:2]
        st = self.store
        dev, cdt = st.device, st.compute_dtype
        feats = self.encode_images(images.to(device=dev).transpose(0, 1).reshape(B * CAM, *images.shape[2:]))
        T = feats.shape[1]
        img_tok = feats.view(CAM, B, T, -1).permute(1, 0, 2, 3).reshape(B, CAM * T, -1)
        llm = self.model.llm
        dummy = torch.zeros((1, llm.config.hidden_size), device=dev, dtype=cdt)
        txt = Fn.SpliceFn.apply(dummy, st.params[llm.embed_name], st, llm.embed_name,
                                input_ids.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()).view(*input_ids.shape, -1)
        return torch.cat([img_tok.to(cdt), txt.to(cdt)], dim=1)

    def get_suffix_hidden_states(self, noisy_actions: torch.Tensor, time: Optional[np.ndarray], te: Optional[torch.Tensor] = None):
        """-> suffix tokens [B, chunk, d_a]: action_time_mlp_out(silu(action_time_mlp_in(cat(action_in_proj(x_t), time_emb)))).
        ``te``: the sin/cos time embedding [B, d_a] already on the device (the sampler precomputes its schedule)."""
        st, c = self.store, self.config
        cdt = st.compute_dtype
        B, n, da = noisy_actions.shape[0], c.chunk_size, c.action_config.hidden_size
        if te is None:
            te = hostcpu.upload(posemb_sincos(time, da), st.device).to(cdt)                       # [B, da]
        act_tok = self._lin(noisy_actions.to(cdt).reshape(B * n, -1), "action_in_proj").view(B, n, da)
        h = torch.cat([act_tok, te[:, None, :].expand(B, n, da)], dim=-1).reshape(B * n, 2 * da)
        h = self._lin(h.contiguous(), "action_time_mlp_in", L.ACT_SILU)
        return self._lin(h, "action_time_mlp_out").view(B, n, da)

    # ------------------------------------------------------------------------------ mixture forward
    def _final_norm(self, x: torch.Tensor) -> torch.Tensor:
        exp = self.model.action_expert
        return Fn.NormFn.apply(x, self.store.params[exp.p + "norm.weight"], self.store, "rms", exp.p + "norm.weight", None,
                               exp.config.rms_norm_eps)

    def _mot(self, ptok, stok, positions: np.ndarray, q_limit, key_valid) -> torch.Tensor:
        """_merged_attention_forward over both experts (dm0_arch.py:270-298): one MotLayerFn per layer (mot.MotPolicy._mot_layers);
        only the action expert's final norm is evaluated (prefix_out is never read).  -> suffix_out [B, chunk, d_a]"""
        return self._final_norm(self._mot_rows(ptok, stok, positions, q_limit, key_valid)).view(*stok.shape[:2], -1)

    # ------------------------------------------------------------------------------------- training
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None, actions=None,
                states=None, images=None, cache_position=None, image_masks=None, **kwargs) -> CausalLMOutputDexbotic:
        """flow-matching step (dm0_arch.py:406-511).  kwargs ``noise`` [B, chunk, A] and ``time`` [B] inject the draws (reference:
        N(0, 1) and Beta(1.5, 1) * 0.999 + 0.001)."""
        c, dev = self.config, self.store.device
        B = actions.shape[0]
        acts = actions.to(dev).float().reshape(B, c.chunk_size, c.action_dim)
        noise = kwargs.get("noise")
        noise = torch.randn_like(acts) if noise is None else noise.to(dev).float()
        time = kwargs.get("time")
        time = (np.random.beta(1.5, 1.0, size=B) * 0.999 + 0.001).astype(np.float32) if time is None else \
            np.asarray(time.cpu() if torch.is_tensor(time) else time, dtype=np.float32)
        # every mask and position of the mixture first, on the host: they depend on the two input masks only (the suffix is all
        # valid); uploaded through pinned memory before the tower is launched
        pmask = self.prefix_mask(attention_mask, image_masks)
        P, n = pmask.shape[1], c.chunk_size
        input_mask = np.concatenate([pmask, np.ones((B, n), dtype=bool)], axis=1)
        # cumsum of attn_mask = [1] * P + [1, 0, 0, ...]: 1 .. P over the (causal) prefix, P + 1 over the whole suffix block
        cum = np.broadcast_to(np.concatenate([np.arange(1, P + 1), np.full(n, P + 1)]).astype(np.int64), input_mask.shape)
        q_limit, key_valid = mask_tensors(cum, input_mask, cum, input_mask, dev)
        positions = np.maximum(np.cumsum(input_mask, axis=1) - 1, 0)       # (a padded first token would read row -1; it is never a key)
        te = hostcpu.upload(time, dev)[:, None, None]
        x_t = te * noise + (1 - te) * acts
        u_t = noise - acts
        ptok = self.get_prefix_hidden_states(input_ids, images)
        assert ptok.shape[1] == P, (ptok.shape, pmask.shape)
        stok = self.get_suffix_hidden_states(x_t, time)
        v_t = self._v_t(self._mot(ptok, stok, positions, q_limit, key_valid))
        loss = Fn.MseLossFn.apply(v_t.contiguous(), u_t.contiguous())
        return CausalLMOutputDexbotic(loss=loss, logits=v_t)

    # ------------------------------------------------------------------------------------ inference
    def _sampler_plan(self, attention_mask, image_masks, B: int, S: int, diffusion_steps: int) -> SimpleNamespace:
        """the host side of a sampling request whose suffix is ONE bidirectional block of ``S`` rows behind the causal prefix (masks,
        positions, rotary tables, the schedule's time embeddings), uploaded through pinned memory, and the per-layer key / value
        buffers [B, Hkv, P + S, D]"""
        c, st = self.config, self.store
        dev = st.device
        dt = -1.0 / diffusion_steps
        pmask = self.prefix_mask(attention_mask, image_masks)
        P = pmask.shape[1]
        pcum = np.broadcast_to(np.arange(1, P + 1, dtype=np.int64), pmask.shape)
        p_limit, p_valid = mask_tensors(pcum, pmask, pcum, pmask, dev)
        ppos = np.maximum(np.cumsum(pmask, axis=1) - 1, 0)
        smask = np.ones((B, S), dtype=bool)
        scum = np.full((B, S), P + 1, dtype=np.int64)
        q_limit, key_valid = mask_tensors(scum, smask, np.concatenate([pcum, scum], axis=1),
                                          np.concatenate([pmask, smask], axis=1), dev)
        fpos = pmask.sum(-1)[:, None] + np.cumsum(smask, axis=-1) - 1
        n_pos = int(max(fpos.max(), ppos.max())) + 1
        cos_t, sin_t = self.model.llm.rope_tables(n_pos, dev)
        ppos_d = hostcpu.upload(ppos.astype(np.int32), dev).reshape(-1)
        pos = hostcpu.upload(fpos.astype(np.int32), dev).reshape(-1)
        times = list(takewhile(lambda t: t >= -dt / 2, flow_times(dt)))   # the reference's float32 schedule (dm0_arch.py:571)
        da = c.action_config.hidden_size
        te_table = hostcpu.upload(np.stack([posemb_sincos(np.full(B, t, dtype=np.float32), da) for t in times]), dev
                                  ).to(st.compute_dtype)                                            # [steps, B, da]
        return SimpleNamespace(B=B, P=P, S=S, dt=dt, steps=len(times), p_limit=p_limit, p_valid=p_valid, ppos_d=ppos_d, q_limit=q_limit,
                               key_valid=key_valid, pos=pos, cos_t=cos_t, sin_t=sin_t, te_table=te_table,
                               kv=self.sampler_kv_buffers(B, P + S), geom_s=self._geom(B, 0, S))

    def _prefix_pass(self, plan: SimpleNamespace, input_ids, images) -> None:
        """the llm alone over the prefix, each layer's keys / values written straight into [0, P) of its buffer"""
        B, P = plan.B, plan.P
        ptok = self.get_prefix_hidden_states(input_ids, images)
        self._mot_layers(self._geom(B, P, 0), ptok.reshape(B * P, -1).contiguous(), None, None, plan.cos_t, plan.sin_t, plan.ppos_d,
                         None, plan.p_limit, plan.p_valid, kv=plan.kv, kv0=0)

    @torch.no_grad()
    def inference_action(self, input_ids=None, attention_mask=None, states=None, images=None, image_masks=None,
                         diffusion_steps: int = 10, **kwargs):
        """dm0_arch.py:513-641.  kwarg ``noise`` [B, chunk, A] injects the initial sample, ``use_graph`` overrides the graph switch.
        Returns the [B, chunk, A] tensor."""
        c, dev = self.config, self.store.device
        B, n = states.shape[0], c.chunk_size
        noise = kwargs.get("noise")
        x = (torch.randn(B, n, c.action_dim, device=dev) if noise is None else noise.to(dev)).float().contiguous()
        pl = self._sampler_plan(attention_mask, image_masks, B, n, diffusion_steps)
        self._prefix_pass(pl, input_ids, images)
        P, dt, kv, cos_t, sin_t = pl.P, pl.dt, pl.kv, pl.cos_t, pl.sin_t

        # ---- the Euler loop: tensors in / tensors out; every step writes the suffix keys / values at [P, P + chunk) of the buffers
        def euler(x, te_table, q_limit, key_valid, pos):
            for s in range(pl.steps):
                h = self.get_suffix_hidden_states(x, None, te=te_table[s]).reshape(B * n, -1).contiguous()
                _, h = self._mot_layers(pl.geom_s, None, h, None, cos_t, sin_t, None, pos, q_limit, key_valid, kv=kv, kv0=P)
                v_t = self._v_t(self._final_norm(h).view(B, n, -1))
                x = K.add(x, K.scale_(v_t.contiguous(), dt))             # Euler step x += v dt
            return x
        inputs = dict(x=x, te_table=pl.te_table, q_limit=pl.q_limit, key_valid=pl.key_valid, pos=pl.pos)
        key = ("euler", int(diffusion_steps), P, cos_t.data_ptr(), kv[0][0].data_ptr())
        return self._run_sampler(euler, inputs, key, kwargs.get("use_graph"))


register_model_with_hf(DM0ForCausalLM)
