"""pi0.5 policy (SigLIP + dual-expert Gemma mixture of transformers + flow-matching action head, the flow time applied through
adaptive RMSNorms): host-side mirror of dexbotic/model/pi05/pi05_arch.py on libdexbotic_amd kernels.

``Pi05Config`` (:54-84), ``Pi05Model`` (:87-108: tower / projector / llm + ``action_expert``, an ``adarms_gemma`` decoder with
``use_adarms=True``, + ``time_mlp_in`` / ``time_mlp_out`` / ``action_in_proj`` / ``action_out_proj``), ``Pi05ForCausalLM``:
``embed_prefix`` (:257-291), ``embed_suffix`` (:293-332), ``_inner_forward_mot`` (:118-250), ``inference_action`` (:423-515).  It is
pi0 (model/pi0/pi0_arch.py) with one difference: the time embedding is not concatenated into the action tokens.
``adarms_cond = silu(time_mlp_out(silu(time_mlp_in(sincos(t)))))`` [B, width] goes into EVERY norm of the action expert instead:
each norm's ``dense(cond)`` is, per sample, [scale | shift | gate]; the norm's output is x_hat (1 + scale) + shift and both residual
adds of the layer are x + y gate.  So: no state token and no ``state_proj`` (``states`` only gives the batch size), the suffix is the
``chunk_size`` action tokens ([True, False, ...]: one bidirectional block behind the bidirectional prefix), the final norm is adaptive
too (its gate is unused).

Every layer is ``functional.MotLayerFn`` — through autograd when gradients are on, its ``_run`` alone otherwise and in the
sampler (the llm is its Gemma kind, the action expert its adaptive-norm kind; model/mot.py holds what pi0, pi0.5 and DM0 share).  The 2 L + 1 dense layers are ONE product (``functional.FusedLinearFn``: their weights lie back to back in the arena); the
sampler evaluates it once for the whole Euler schedule, before the loop (the condition depends on the time alone).  The sampler
keeps ONE key / value buffer [B, Hkv, P + chunk, D] per layer as DM0's does, and replays the loop as one HIP graph.
"""
from __future__ import annotations

from collections import OrderedDict
from itertools import takewhile
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from ... import _lib as L
from ... import functional as Fn
from ... import hostcpu
from ... import kernels as K
from ...engine import ParamStore
from ..dexbotic_arch import CausalLMOutputDexbotic, register_model_with_hf, register_with_hf
from ..llm.adarms_gemma import AdaRMSGemmaConfig, AdaRMSGemmaExpert
from ..llm.gemma import GemmaExpert
from ..modules.mm_projector.builder import build_vision_projector
from ..modules.mm_vision.builder import build_vision_tower
from ..modules.mm_vision.siglip.siglip_encoder import SiglipVisionConfig
from ..mot import flow_times, mask_tensors
from ..pi0.pi0_arch import Pi0Config, Pi0ForCausalLM, posemb_sincos

_GEOMETRY = ("num_hidden_layers", "num_attention_heads", "num_key_value_heads", "head_dim")


class Pi05Config(Pi0Config):
    """pi05_arch.py:54-84, registered with ``AutoConfig`` under the reference's ``model_type``.  ``action_config`` must be an
    ``adarms_gemma`` config with ``use_adarms=True`` (``adarms_cond_dim`` defaults to its ``hidden_size``; ``width``, which sizes the
    time MLP, is read as ``action_config.width`` and defaults to ``hidden_size`` too); ``llm_config`` an ``adarms_gemma`` config with
    ``use_adarms=False`` or a plain ``gemma`` one."""
    model_type = "dexbotic_pi05"

    def __init__(self, vision_config=None, processor_config=None, action_config=None, llm_config=None,
                 mm_projector_type: str = "linear", action_dim: int = 32, chunk_size: int = 50, compute_dtype="float32", **kwargs):
        self.vision_config = SiglipVisionConfig.from_any(vision_config if vision_config is not None else {})
        self.processor_config = processor_config
        act = AdaRMSGemmaConfig.from_any(action_config if action_config is not None else
                                         {"model_type": "adarms_gemma", "use_adarms": True, "hidden_size": 1024,
                                          "intermediate_size": 4096}, "action_config")
        llm = AdaRMSGemmaConfig.from_any(llm_config if llm_config is not None else {"model_type": "adarms_gemma"}, "llm_config")
        if act.model_type != "adarms_gemma" or not act.use_adarms:
            raise ValueError(f"pi0.5 action_config must be model_type 'adarms_gemma' with use_adarms=True (got {act.model_type!r}, "
                             f"use_adarms={act.use_adarms}): the action expert takes the flow time through its adaptive norms")
        if llm.use_adarms:
            raise ValueError("pi0.5 llm_config.use_adarms=True: the llm's norms are plain GemmaRMSNorms (nothing conditions the prefix)")
        if act.width is None:
            act.width = act.hidden_size
        if not (act.width == act.hidden_size == act.adarms_cond_dim):
            raise ValueError(f"pi0.5 action_config: width ({act.width}), hidden_size ({act.hidden_size}) and adarms_cond_dim "
                             f"({act.adarms_cond_dim}) must be equal: the time MLP maps sincos(t) [hidden_size] to the condition "
                             "of every adaptive norm")
        bad = [k for k in _GEOMETRY if getattr(act, k) != getattr(llm, k)]
        if bad:
            raise ValueError("pi0.5: the two experts share one attention per layer, so depth, heads, key / value heads and head_dim "
                             "must match; llm_config and action_config differ in " +
                             ", ".join(f"{k} ({getattr(llm, k)} / {getattr(act, k)})" for k in bad))
        self.action_config, self.llm_config = act, llm
        self.mm_projector_type = mm_projector_type
        self.action_dim, self.chunk_size = int(action_dim), int(chunk_size)
        self.compute_dtype = compute_dtype if isinstance(compute_dtype, str) else str(compute_dtype).replace("torch.", "")
        for k in ("model_type", "architectures", "transformers_version"):
            kwargs.pop(k, None)
        hidden, vocab = kwargs.pop("hidden_size", None), kwargs.pop("vocab_size", None)
        super(Pi0Config, self).__init__(**kwargs)
        self.hidden_size = llm.hidden_size if hidden is None else hidden
        self.vocab_size = llm.vocab_size if vocab is None else vocab


register_with_hf(Pi05Config)


class Pi05Model(nn.Module):
    """registration order = forward order: vision tower, projector, llm expert, action expert, the four small linears"""

    def __init__(self, config: Pi05Config, store: ParamStore):
        super().__init__()
        self.config, self.store = config, store
        self.mm_vision_tower = build_vision_tower(config.vision_config, store, "model.mm_vision_tower.",
                                                  processor_config=config.processor_config, select_layer=None)
        config.mm_hidden_size = self.mm_vision_tower.hidden_size
        self.mm_projector = build_vision_projector(config, store, "model.mm_projector.")
        self.llm = GemmaExpert(store, "model.llm.", config.llm_config.plain())
        self.action_expert = AdaRMSGemmaExpert(store, "model.action_expert.", config.action_config)
        ac = config.action_config
        da, A, wd = ac.hidden_size, config.action_dim, ac.width
        store.new_bucket()
        for name, shape in (("time_mlp_in", (wd, wd)), ("time_mlp_out", (wd, wd)), ("action_in_proj", (da, A)),
                            ("action_out_proj", (A, da))):
            store.register([(f"model.{name}.weight", shape), (f"model.{name}.bias", (shape[0],))])

    @property
    def backbone(self):
        return self.llm

    @property
    def mm_vision_module(self):
        return self.mm_vision_tower

    @property
    def mm_projector_module(self):
        return self.mm_projector


_TOP = ("model.llm.", "model.mm_vision_tower.", "model.mm_projector.", "model.action_expert.", "model.time_mlp_in.",
        "model.time_mlp_out.", "model.action_in_proj.", "model.action_out_proj.")
_GEMMA_LAYER = ("self_attn.q_proj.", "self_attn.k_proj.", "self_attn.v_proj.", "self_attn.o_proj.", "mlp.gate_proj.", "mlp.up_proj.",
                "mlp.down_proj.", "input_layernorm.", "post_attention_layernorm.")
_SIGLIP_LAYER = ("layer_norm1.", "self_attn.k_proj.", "self_attn.v_proj.", "self_attn.q_proj.", "self_attn.out_proj.", "layer_norm2.",
                 "mlp.fc1.", "mlp.fc2.")


def _reference_key_order(keys) -> List[str]:
    """state-dict keys in the order the reference's module tree yields them: DexboticVLMModel builds llm, tower, projector, then
    Pi05Model its own modules; an HF Gemma layer lists self_attn (q, k, v, o), mlp, then its two norms; a SigLIP layer layer_norm1,
    self_attn (k, v, q, out), layer_norm2, mlp.  Inside one module, and among what follows a stack of layers (final norm,
    post_layernorm, the pooling head), the order the keys come in stands."""
    pos = {k: i for i, k in enumerate(keys)}

    def rank(k: str):
        t = next(i for i, p in enumerate(_TOP) if k.startswith(p))
        rest = k[len(_TOP[t]):]
        if "layers." in rest:
            layer = int(rest.split("layers.")[1].split(".")[0])
            order = _SIGLIP_LAYER if t == 1 else _GEMMA_LAYER
            return (t, 1, layer, next(i for i, p in enumerate(order) if p in rest), pos[k])
        before = rest.startswith(("embed_tokens.", "vision_tower.embeddings."))
        return (t, 0 if before else 2, 0, 0, pos[k])
    return sorted(keys, key=rank)


class Pi05ForCausalLM(Pi0ForCausalLM):
    config_class = Pi05Config

    def __init__(self, config: Pi05Config, device=None, train: bool = True):
        nn.Module.__init__(self)
        self.config = config
        device = device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
        from ..dexbotic_arch import _DTYPES
        self.store = ParamStore(device, _DTYPES[config.compute_dtype])
        self.model = Pi05Model(config, self.store)
        self._finish_init(train)

    def state_dict(self, *args, **kwargs):
        """the reference's keys in the reference's ORDER (the arena, hence the module tree, is in forward order and keeps the dense
        layers of the adaptive norms together)"""
        sd = super().state_dict(*args, **kwargs)
        prefix = kwargs.get("prefix", "")
        keys = [k[len(prefix):] for k in sd]
        out = OrderedDict((prefix + k, sd[prefix + k]) for k in _reference_key_order(keys))
        if hasattr(sd, "_metadata"):
            out._metadata = sd._metadata
        return out

    # unused_parameter_names(): Pi0ForCausalLM's — the SigLIP head, the action expert's token embedding, the last llm layer after its
    # k / v projections and the llm's final norm get no gradient here either

    # ------------------------------------------------------------------------------------ embeddings
    def modulations(self, te: torch.Tensor) -> torch.Tensor:
        """sin/cos time embeddings te [R, d_a] (one row per sample, or per (step, sample) of a schedule) -> the modulation of every
        adaptive norm [2 L + 1, R, 3 d_a]: adarms_cond = silu(time_mlp_out(silu(time_mlp_in(te)))) (pi05_arch.py:310-317), then all
        the dense layers as ONE product"""
        st, exp = self.store, self.model.action_expert
        d, cd, J = exp.config.hidden_size, exp.config.adarms_cond_dim, exp.n_norms
        cond = self._lin(self._lin(te, "time_mlp_in", L.ACT_SILU), "time_mlp_out", L.ACT_SILU)
        mod = Fn.FusedLinearFn.apply(cond, st.params[exp.dense_w[0]], st, exp.dense_w, exp.dense_b, (J * 3 * d, cd))
        return mod.view(te.shape[0], J, 3 * d).transpose(0, 1).contiguous()

    def embed_suffix(self, noisy_actions: torch.Tensor, time: Optional[np.ndarray]):
        """-> (action tokens [B, chunk, d_a], modulations [2 L + 1, B, 3 d_a])"""
        st, c = self.store, self.config
        cdt = st.compute_dtype
        B, n, da = noisy_actions.shape[0], c.chunk_size, c.action_config.hidden_size
        te = hostcpu.upload(posemb_sincos(time, da), st.device).to(cdt)                            # [B, da]
        tok = self._lin(noisy_actions.to(cdt).reshape(B * n, -1), "action_in_proj").view(B, n, da)
        return tok, self.modulations(te)

    # ------------------------------------------------------------------------------ mixture forward
    def _mot(self, ptok, stok, mods, positions: np.ndarray, q_limit, key_valid) -> torch.Tensor:
        """_inner_forward_mot over both experts: one MotLayerFn per layer (mot.MotPolicy._mot_layers) with the layer's two modulations;
        only the action expert's final norm is evaluated.  -> suffix_out [B, chunk, d_a]"""
        n, eps = self.model.llm.config.num_hidden_layers, self.model.action_expert.config.rms_norm_eps
        grad = torch.is_grad_enabled()
        if grad:
            mods = mods.unbind(0)                 # (one autograd node for all 2 L + 1 modulations)
        x1 = self._mot_rows(ptok, stok, positions, q_limit, key_valid, mods)
        y = Fn.AdaRMSNormFn.apply(x1, mods[2 * n], eps) if grad else K.adarms_fwd(x1, mods[2 * n], eps)[0]
        return y.view(*stok.shape[:2], -1)

    # ------------------------------------------------------------------------------------- training
    def forward(self, input_ids=None, attention_mask=None, actions=None, states=None, images=None, image_masks=None,
                **kwargs) -> CausalLMOutputDexbotic:
        """flow-matching step (pi05_arch.py:334-421).  kwargs ``noise`` [B, chunk, A] and ``time`` [B] inject the draws (reference:
        N(0, 1) and Beta(1.5, 1) * 0.999 + 0.001)."""
        c, dev = self.config, self.store.device
        B = actions.shape[0]
        acts = actions.to(dev).float().reshape(B, c.chunk_size, c.action_dim)
        noise = kwargs.get("noise")
        noise = torch.randn_like(acts) if noise is None else noise.to(dev).float()
        time = kwargs.get("time")
        time = (np.random.beta(1.5, 1.0, size=B) * 0.999 + 0.001).astype(np.float32) if time is None else \
            np.asarray(time.cpu() if torch.is_tensor(time) else time, dtype=np.float32)
        # every mask and position of the mixture first, on the host: they depend on the two input masks only (the suffix is all valid)
        pmask = self.prefix_mask(attention_mask, image_masks)
        P, n = pmask.shape[1], c.chunk_size
        input_mask = np.concatenate([pmask, np.ones((B, n), dtype=bool)], axis=1)
        # cumsum of ar_mask = [False] * P + [True, False, ...]: 0 over the (bidirectional) prefix, 1 over the whole suffix block
        cum = np.broadcast_to(np.concatenate([np.zeros(P), np.ones(n)]).astype(np.int64), input_mask.shape)
        q_limit, key_valid = mask_tensors(cum, input_mask, cum, input_mask, dev)
        positions = np.maximum(np.cumsum(input_mask, axis=1) - 1, 0)       # (a padded first token would read row -1; it is never a key)
        te = hostcpu.upload(time, dev)[:, None, None]
        x_t = te * noise + (1 - te) * acts
        u_t = noise - acts
        ptok, _, par = self.embed_prefix(input_ids, attention_mask, images, image_masks, input_mask=pmask)
        assert ptok.shape[1] == P and not par.any()
        stok, mods = self.embed_suffix(x_t, time)
        v_t = self._v_t(self._mot(ptok, stok, mods, positions, q_limit, key_valid))
        loss = Fn.MseLossFn.apply(v_t.contiguous(), u_t.contiguous())
        return CausalLMOutputDexbotic(loss=loss, logits=v_t)

    # ------------------------------------------------------------------------------------ inference
    @torch.no_grad()
    def inference_action(self, input_ids=None, attention_mask=None, states=None, images=None, image_masks=None,
                         diffusion_steps: int = 10, **kwargs):
        """pi05_arch.py:423-515.  kwarg ``noise`` [B, chunk, A] injects the initial sample, ``use_graph`` overrides the graph switch.
        Returns the [B, chunk, A] tensor."""
        c, st = self.config, self.store
        dev = st.device
        llm, exp = self.model.llm, self.model.action_expert
        B, n = states.shape[0], c.chunk_size
        dt = -1.0 / diffusion_steps
        noise = kwargs.get("noise")
        x = (torch.randn(B, n, c.action_dim, device=dev) if noise is None else noise.to(dev)).float().contiguous()
        # host side first (masks, positions, the schedule's time embeddings), uploaded through pinned memory
        pmask = self.prefix_mask(attention_mask, image_masks)
        P = pmask.shape[1]
        pcum = np.zeros(pmask.shape, dtype=np.int64)
        p_limit, p_valid = mask_tensors(pcum, pmask, pcum, pmask, dev)
        ppos = np.maximum(np.cumsum(pmask, axis=1) - 1, 0)
        smask = np.ones((B, n), dtype=bool)
        scum = np.ones((B, n), dtype=np.int64)
        q_limit, key_valid = mask_tensors(scum, smask, np.concatenate([pcum, scum], axis=1),
                                                np.concatenate([pmask, smask], axis=1), dev)
        fpos = pmask.sum(-1)[:, None] + np.cumsum(smask, axis=-1) - 1
        n_pos = int(max(fpos.max(), ppos.max())) + 1
        cos_t, sin_t = llm.rope_tables(n_pos, dev)
        ppos_d = hostcpu.upload(ppos.astype(np.int32), dev).reshape(-1)
        pos = hostcpu.upload(fpos.astype(np.int32), dev).reshape(-1)
        times = list(takewhile(lambda t: t > -dt / 2, flow_times(dt)))    # the reference's float32 schedule (pi05_arch.py:512)
        da = c.action_config.hidden_size
        te = hostcpu.upload(np.concatenate([posemb_sincos(np.full(B, t, dtype=np.float32), da) for t in times]), dev
                            ).to(st.compute_dtype)                                                  # [steps * B, da]
        # the condition depends on the time alone: every norm's modulation for the WHOLE schedule, one product, before the loop
        J = exp.n_norms
        mods = self.modulations(te).view(J, len(times), B, -1).transpose(0, 1).contiguous()        # [steps, 2 L + 1, B, 3 da]
        n_layers = llm.config.num_hidden_layers
        kv = self.sampler_kv_buffers(B, P + n)
        # ---- prefix pass: the llm alone, each layer's keys / values written straight into [0, P) of its buffer
        ptok, _, par = self.embed_prefix(input_ids, attention_mask, images, image_masks, input_mask=pmask)
        assert not par.any()
        self._mot_layers(self._geom(B, P, 0), ptok.reshape(B * P, -1).contiguous(), None, None, cos_t, sin_t, ppos_d, None,
                         p_limit, p_valid, kv=kv, kv0=0)
        geom_s = self._geom(B, 0, n)
        eps = exp.config.rms_norm_eps

        # ---- the Euler loop: tensors in / tensors out; every step writes the suffix keys / values at [P, P + chunk) of the buffers
        def euler(x, mods, q_limit, key_valid, pos):
            for s in range(len(times)):
                h = self._lin(x.to(st.compute_dtype).reshape(B * n, -1), "action_in_proj")
                _, h = self._mot_layers(geom_s, None, h, mods[s], cos_t, sin_t, None, pos, q_limit, key_valid, kv=kv, kv0=P)
                v_t = self._v_t(K.adarms_fwd(h, mods[s, 2 * n_layers], eps)[0].view(B, n, -1))
                x = K.add(x, K.scale_(v_t.contiguous(), dt))             # Euler step x += v dt
            return x
        inputs = dict(x=x, mods=mods, q_limit=q_limit, key_valid=key_valid, pos=pos)
        # (a weight change needs no new capture: the modulations are inputs formed above)
        key = ("euler", int(diffusion_steps), P, cos_t.data_ptr(), kv[0][0].data_ptr())
        return self._run_sampler(euler, inputs, key, kwargs.get("use_graph"))


register_model_with_hf(Pi05ForCausalLM)
