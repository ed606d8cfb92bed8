"""pi0 policy (SigLIP + dual-expert Gemma mixture of transformers + flow-matching action head): host-side mirror of
dexbotic/model/pi0/pi0_arch.py on libdexbotic_amd kernels.

``Pi0Config`` (:53-83), ``Pi0Model`` (:86-106: llm + action_expert + the five small linears), ``Pi0ForCausalLM``:
``embed_prefix`` (:223-259), ``embed_suffix`` (:261-315), ``_inner_forward_mot`` (:116-216) and
``inference_action`` (:402-491: prefix pass fills a K/V cache, 10 Euler steps x += v dt re-encode the suffix against
it).  What differs is underneath: parameters live in the flat arenas of engine.ParamStore; every layer is two GEMM
halves per expert around ONE attention call over both experts' tokens, with the reference's block mask expressed as
per-query key counts + per-key validity (cumsum(ar_mask) is non-decreasing, so "cumsum[j] <= cumsum[i]" is a prefix).

Every layer is ``functional.MotLayerFn`` (one autograd node per layer over both experts, gradients written straight into the
arena; its ``_run`` alone when gradients are off and in the sampler), driven by what model/mot.py shares with pi0.5 and DM0.  The
sampler keeps ONE key / value buffer [B, Hkv, P + 1 + chunk, D] per layer: the prefix pass writes [0, P), every Euler step the
suffix slots behind it, and the loop is replayed as one HIP graph.
"""
from __future__ import annotations

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
from ..dexbotic_arch import (ActionOutputForCausalLM, CausalLMOutputDexbotic, NativePreTrainedMixin, _DTYPES, _hf_config_base,
                             register_with_hf)
from ..llm.gemma import GemmaConfig, GemmaExpert
from ..modules.mm_projector.builder import build_vision_projector
from ..modules.mm_vision.builder import build_vision_tower
from ..modules.mm_vision.siglip.siglip_encoder import SiglipVisionConfig
from ..mot import MotPolicy, flow_times, mask_tensors


class Pi0Config(_hf_config_base()):
    """``transformers.PretrainedConfig`` subclass registered with ``AutoConfig`` under the reference's ``model_type``
    (pi0_arch.py:54-110): ``AutoConfig.from_pretrained`` on a reference pi0 checkpoint directory resolves to it, the nested
    vision / llm / action-expert configs round-trip through ``config.json``."""
    model_type = "dexbotic_pi0"

    def __init__(self, vision_config=None, processor_config=None, action_config=None, llm_config=None,
                 mm_projector_type: str = "linear", action_dim: int = 32, chunk_size: int = 50,
                 compute_dtype="float32", **kwargs):
        self.vision_config = SiglipVisionConfig.from_any(vision_config if vision_config is not None else {})
        self.processor_config = processor_config
        self.action_config = GemmaConfig.from_any(action_config if action_config is not None else {})
        self.llm_config = GemmaConfig.from_any(llm_config if llm_config is not None else {})
        self.mm_projector_type = mm_projector_type
        self.action_dim, self.chunk_size = action_dim, chunk_size
        self.compute_dtype = compute_dtype if isinstance(compute_dtype, str) else str(compute_dtype).replace("torch.", "")
        a, l_ = self.action_config, self.llm_config
        if (a.num_hidden_layers, a.num_attention_heads, a.num_key_value_heads, a.head_dim) != (
                l_.num_hidden_layers, l_.num_attention_heads, l_.num_key_value_heads, l_.head_dim):
            raise ValueError("the two experts share one attention: depth, heads and head_dim must match")
        for k in ("model_type", "architectures", "transformers_version"):
            kwargs.pop(k, None)
        hidden, vocab = kwargs.pop("hidden_size", None), kwargs.pop("vocab_size", None)
        super().__init__(**kwargs)
        self.hidden_size = self.llm_config.hidden_size if hidden is None else hidden
        self.vocab_size = self.llm_config.vocab_size if vocab is None else vocab

    def to_dict(self):
        out = {}
        for k, v in super().to_dict().items():
            if hasattr(v, "to_dict"):
                v = v.to_dict()
            elif isinstance(v, torch.dtype):
                v = str(v).replace("torch.", "")
            out[k] = v
        out["model_type"] = self.model_type
        return out

    def to_diff_dict(self):
        return self.to_dict()

    @classmethod
    def from_dict(cls, d, **kwargs):
        d = dict(d)
        for k in ("model_type", "architectures", "transformers_version"):
            d.pop(k, None)
        config = cls(**d)
        if kwargs.pop("return_unused_kwargs", False):
            unused = {k: v for k, v in kwargs.items() if not k.startswith("_") and k not in ("name_or_path", "trust_remote_code")}
            return config, unused
        return config

    @classmethod
    def from_pretrained(cls, path: str, **kwargs):
        import json
        import os
        with open(os.path.join(path, "config.json")) as f:
            return cls.from_dict(json.load(f), **kwargs)

    def save_pretrained(self, path: str, **kwargs) -> None:
        import json
        import os
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.to_dict(), f, indent=2, default=str)


register_with_hf(Pi0Config)


class Pi0Model(nn.Module):
    """registration order = forward order: vision tower, projector, llm expert, action expert, suffix/head linears"""

    def __init__(self, config: Pi0Config, store: ParamStore):
        super().__init__()
        self.config, self.store = config, store
        self.mm_vision_tower = build_vision_tower(config.vision_config, store, "model.mm_vision_tower.",
                                                  processor_config=config.processor_config, select_layer=None)
        config.mm_hidden_size = self.mm_vision_tower.hidden_size
        self.mm_projector = build_vision_projector(config, store, "model.mm_projector.")
        self.llm = GemmaExpert(store, "model.llm.", config.llm_config)
        self.action_expert = GemmaExpert(store, "model.action_expert.", config.action_config)
        da, A = config.action_config.hidden_size, config.action_dim
        store.new_bucket()
        for name, shape in (("state_proj", (da, A)), ("action_in_proj", (da, A)), ("action_time_mlp_in", (da, 2 * da)),
                            ("action_time_mlp_out", (da, da)), ("action_out_proj", (A, da))):
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


def posemb_sincos(time: np.ndarray, dim: int, min_period: float = 4e-3, max_period: float = 4.0) -> np.ndarray:
    """pi0_arch.py:36-51 on the host (the schedule is known before any device work): float64 periods, the time in
    float32, sin/cos of the float64 quotient — returned float64 like the reference tensor"""
    frac = np.linspace(0.0, 1.0, dim // 2, dtype=np.float64)
    period = min_period * (max_period / min_period) ** frac
    x = time.astype(np.float32)[:, None].astype(np.float64) / period[None, :] * 2 * np.pi
    return np.concatenate([np.sin(x), np.cos(x)], axis=-1)


class Pi0ForCausalLM(NativePreTrainedMixin, nn.Module, ActionOutputForCausalLM, MotPolicy):
    config_class = Pi0Config
    # trainer.NativeTrainer: the bias gradients' column sums (and any fp32 dW product) beside the dX chain on a side stream:
    # 250.0 -> 245.3 ms per step, two alternating runs each in one box (profiles/r06_memvla_hostbound.txt)
    gradient_side_stream = True

    def __init__(self, config: Pi0Config, device=None, train: bool = True):
        super().__init__()
        self.config = config
        device = device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
        self.store = ParamStore(device, _DTYPES[config.compute_dtype])
        self.model = Pi0Model(config, self.store)
        self._finish_init(train)

    @property
    def device(self):
        return self.store.device

    @property
    def dtype(self):
        return self.store.compute_dtype

    def unused_parameter_names(self) -> List[str]:
        """no gradient on the pi0 loss: SigLIP pooling head, the action expert's token embedding, and what only
        feeds prefix_out (last llm layer after its K/V projections, llm final norm)"""
        st, c = self.store, self.config
        last = f"model.llm.layers.{c.llm_config.num_hidden_layers - 1}."
        names = self.model.mm_vision_tower.unused_parameter_names()
        names += ["model.action_expert.embed_tokens.weight", "model.llm.norm.weight"]
        names += [n for n in st.slots if n.startswith(last) and
                  (".o_proj." in n or ".mlp." in n or "post_attention_layernorm" in n)]
        return names

    # ------------------------------------------------------------------------------------ embeddings
    def encode_images(self, images: torch.Tensor) -> torch.Tensor:
        return self.model.mm_projector(self.model.mm_vision_tower(images))

    def process_images(self, images):
        """pi0_arch.py:493-511 on the device, the contract of DexboticForCausalLM.process_images: PIL / numpy / torch uint8 frames
        [h, w, 3] -> [n, 3, H, W] float32 on the device.  The frames are padded to a square with BLACK (the reference's own
        expand2square colour here, not the processor's mean), resized with the Pillow-exact bicubic of the tower's
        SiglipImageProcessor and normalised with its mean / std (data/dataset/rgb_preprocess.py: two launches).  Frames of equal size
        share one launch pair; the result is stacked when all outputs have one shape, as in the reference."""
        from ...data.dataset.rgb_preprocess import PreprocessRGB
        if getattr(self.config, "image_aspect_ratio", "pad") != "pad":
            raise NotImplementedError("process_images: without image_aspect_ratio='pad' the reference hands the frames to the SigLIP "
                                      "processor, which stretches them to the tower's size; the device path pads to a square first")
        return PreprocessRGB(self.model.mm_vision_module.image_processor, image_aspect_ratio="pad", image_pad_mode="zero",
                             device=self.device).process(images)

    @staticmethod
    def _to_dev(a: np.ndarray, device) -> torch.Tensor:
        """small host array -> device through pinned memory, non-blocking (hostcpu.upload: a pageable source would make the copy wait
        for the stream to drain)"""
        return hostcpu.upload(a, device)

    def prefix_mask(self, attention_mask, image_masks) -> np.ndarray:
        """input_mask np.bool [B, CAM * T + L] of embed_prefix from the two host-side masks alone (T = tokens per camera): the
        training step computes every mask and position of the mixture BEFORE it launches the vision tower — fetching a device
        mask with .cpu() afterwards waits for the tower, and the 7 ms of numpy that follow run with the GPU idle"""
        T = self.model.mm_vision_tower.num_patches
        im = np.asarray(image_masks.cpu() if torch.is_tensor(image_masks) else image_masks, dtype=bool)
        am = np.asarray(attention_mask.cpu() if torch.is_tensor(attention_mask) else attention_mask, dtype=bool)
        return np.concatenate([np.repeat(im, T, axis=1), am], axis=1)

    def embed_prefix(self, input_ids, attention_mask, images, image_masks, input_mask: Optional[np.ndarray] = None):
        """-> tokens [B, P, d] (compute dtype), input_mask np.bool [B, P], ar_mask np.bool [P] (all False).
        ``input_mask``: prefix_mask(...) computed by the caller beforehand."""
        B, CAM = images.shape[:2]
        dev, cdt = self.store.device, self.store.compute_dtype
        # all cameras in one tower pass: [B, CAM, ...] -> camera-major tokens like the reference's per-camera loop
        feats = self.encode_images(images.to(device=dev).transpose(0, 1).reshape(B * CAM, *images.shape[2:]))
        T = feats.shape[1]
        img_tok = feats.view(CAM, B, T, -1).permute(1, 0, 2, 3).reshape(B, CAM * T, -1)
        txt = self.model.llm.embed(input_ids.to(dev))
        tokens = torch.cat([img_tok.to(cdt), txt.to(cdt)], dim=1)
        if input_mask is None:
            im = np.asarray(image_masks.cpu() if torch.is_tensor(image_masks) else image_masks, dtype=bool)
            am = np.asarray(attention_mask.cpu() if torch.is_tensor(attention_mask) else attention_mask, dtype=bool)
            input_mask = np.concatenate([np.repeat(im, T, axis=1), am], axis=1)
        assert input_mask.shape[1] == tokens.shape[1], (input_mask.shape, tokens.shape)
        return tokens, input_mask, np.zeros(tokens.shape[1], dtype=bool)

    def embed_suffix(self, states: torch.Tensor, noisy_actions: torch.Tensor, time: Optional[np.ndarray], te: Optional[torch.Tensor] = None):
        """-> tokens [B, 1 + chunk, d_a] fp32->compute dtype, input_mask (all True), ar_mask [True, True, False...].
        ``te``: the sin/cos time embedding [B, d_a] already on the device (the sampler precomputes its schedule)."""
        st, c = self.store, self.config
        cdt = st.compute_dtype
        B, da = states.shape[0], c.action_config.hidden_size
        state_tok = self._lin(states.to(cdt), "state_proj").view(B, 1, da)
        if te is None:
            te = self._to_dev(posemb_sincos(time, da), st.device).to(cdt)                       # [B, da]
        act_tok = self._lin(noisy_actions.to(cdt).reshape(B * c.chunk_size, -1), "action_in_proj").view(B, c.chunk_size, da)
        h = torch.cat([act_tok, te[:, None, :].expand(B, c.chunk_size, da)], dim=-1).reshape(B * c.chunk_size, 2 * da)
        h = self._lin(h.contiguous(), "action_time_mlp_in", L.ACT_SILU)
        h = self._lin(h, "action_time_mlp_out").view(B, c.chunk_size, da)
        tokens = torch.cat([state_tok, h], dim=1)
        mask = np.ones((B, 1 + c.chunk_size), dtype=bool)
        ar = np.array([True, True] + [False] * (c.chunk_size - 1))
        return tokens, mask, ar

    # ------------------------------------------------------------------------------ mixture forward
    def _final_norm(self, x: torch.Tensor) -> torch.Tensor:
        exp = self.model.action_expert
        return Fn.NormFn.apply(x, self.store.params[exp.p + "norm.weight"], self.store, "rms1p", exp.p + "norm.weight", None,
                               exp.config.rms_norm_eps)

    def _mot(self, ptok, stok, positions: np.ndarray, q_limit, key_valid) -> torch.Tensor:
        """_inner_forward_mot over both experts (pi0_arch.py:116-216): one MotLayerFn per layer (mot.MotPolicy._mot_layers); only the
        action expert's final norm is evaluated (prefix_out is never read by the loss, pi0_arch.py:372-388)
        -> suffix_out [B, 1 + chunk, d_a]"""
        return self._final_norm(self._mot_rows(ptok, stok, positions, q_limit, key_valid)).view(*stok.shape[:2], -1)

    # ------------------------------------------------------------------------------------- training
    def forward(self, input_ids=None, attention_mask=None, actions=None, states=None, images=None, image_masks=None,
                **kwargs) -> CausalLMOutputDexbotic:
        """flow-matching step (pi0_arch.py:317-400).  kwargs ``noise`` [B,chunk,A] and ``time`` [B] inject the draws
        (reference: N(0,1) and Beta(1.5,1)*0.999+0.001)."""
        c, dev = self.config, self.store.device
        B = actions.shape[0]
        acts = actions.to(dev).float().reshape(B, c.chunk_size, c.action_dim)
        noise = kwargs.get("noise")
        noise = torch.randn_like(acts) if noise is None else noise.to(dev).float()
        time = kwargs.get("time")
        time = (np.random.beta(1.5, 1.0, size=B) * 0.999 + 0.001).astype(np.float32) if time is None else \
            np.asarray(time.cpu() if torch.is_tensor(time) else time, dtype=np.float32)
        # every mask and position of the mixture first: they depend on the two input masks only (the suffix is all valid), the
        # device masks are fetched while the stream still holds the previous step's tail, and the numpy below runs under it
        pmask = self.prefix_mask(attention_mask, image_masks)
        smask = np.ones((B, 1 + c.chunk_size), dtype=bool)
        sar = np.array([True, True] + [False] * (c.chunk_size - 1))
        input_mask = np.concatenate([pmask, smask], axis=1)
        cum = np.broadcast_to(np.cumsum(np.concatenate([np.zeros(pmask.shape[1], dtype=bool), sar]).astype(np.int64)), input_mask.shape)
        q_limit, key_valid = mask_tensors(cum, input_mask, cum, input_mask, dev)
        positions = np.maximum(np.cumsum(input_mask, axis=1) - 1, 0)       # (a padded first token would read row -1; it is never a key)
        te = self._to_dev(time, dev)[:, None, None]
        x_t = te * noise + (1 - te) * acts
        u_t = noise - acts
        ptok, pmask2, par = self.embed_prefix(input_ids, attention_mask, images, image_masks, input_mask=pmask)
        stok, smask2, sar2 = self.embed_suffix(states.to(dev).float(), x_t, time)
        assert smask2.shape == smask.shape and np.array_equal(sar2, sar) and not par.any()
        v_t = self._v_t(self._mot(ptok, stok, positions, q_limit, key_valid))
        loss = Fn.MseLossFn.apply(v_t.contiguous(), u_t.contiguous())
        return CausalLMOutputDexbotic(loss=loss, logits=v_t)

    # ------------------------------------------------------------------------------------ inference
    @torch.no_grad()
    def inference_action(self, input_ids=None, attention_mask=None, states=None, images=None, image_masks=None,
                         diffusion_steps: int = 10, **kwargs):
        """pi0_arch.py:402-491.  kwarg ``noise`` [B,chunk,A] injects the initial sample, ``use_graph`` overrides the graph switch.
        Returns the [B,chunk,A] tensor (the exp layer de-normalises and slices, pi0_exp.py:484-514)."""
        c, dev, st = self.config, self.store.device, self.store
        B, n = states.shape[0], c.chunk_size
        dt = -1.0 / diffusion_steps
        noise = kwargs.get("noise")
        x = (torch.randn(B, n, c.action_dim, device=dev) if noise is None else noise.to(dev)).float().contiguous()
        # host side first (masks, positions, the schedule's time embeddings: they depend on the input masks only), uploaded through
        # pinned memory — then the device work of the request is enqueued without a single wait on the stream
        pmask = self.prefix_mask(attention_mask, image_masks)
        P, Sx = pmask.shape[1], 1 + n
        pcum = np.zeros(pmask.shape, dtype=np.int64)
        p_limit, p_valid = mask_tensors(pcum, pmask, pcum, pmask, dev)
        ppos = np.maximum(np.cumsum(pmask, axis=1) - 1, 0)
        smask = np.ones((B, Sx), dtype=bool)
        sar = np.array([True, True] + [False] * (n - 1))
        scum = np.broadcast_to(np.cumsum(sar.astype(np.int64)), smask.shape)
        # keys = [cached prefix (all visible where valid: cumsum 0) ; suffix]; queries = suffix (cumsum >= 1)
        q_limit, key_valid = mask_tensors(scum, smask, np.concatenate([pcum, scum], axis=1),
                                          np.concatenate([pmask, smask], axis=1), dev)
        fpos = pmask.sum(-1)[:, None] + np.cumsum(smask, axis=-1) - 1
        cos_t, sin_t = self.model.llm.rope_tables(int(max(fpos.max(), ppos.max())) + 1, dev)
        ppos_d = self._to_dev(ppos.astype(np.int32), dev).reshape(-1)
        pos = self._to_dev(fpos.astype(np.int32), dev).reshape(-1)
        times = list(takewhile(lambda t: t > -dt / 2, flow_times(dt)))    # the reference's float32 schedule (pi0_arch.py:470-489)
        da = c.action_config.hidden_size
        te_table = self._to_dev(np.stack([posemb_sincos(np.full(B, t, dtype=np.float32), da) for t in times]), dev
                                ).to(st.compute_dtype)                                            # [steps, B, da]
        kv = self.sampler_kv_buffers(B, P + Sx)
        # ---- prefix pass: the llm alone, each layer's keys / values written straight into [0, P) of its buffer
        ptok, _, par = self.embed_prefix(input_ids, attention_mask, images, image_masks, input_mask=pmask)
        assert not par.any()
        self._mot_layers(self._geom(B, P, 0), ptok.reshape(B * P, -1).contiguous(), None, None, cos_t, sin_t, ppos_d, None,
                         p_limit, p_valid, kv=kv, kv0=0)
        states_d = states.to(dev).float().contiguous()
        geom_s = self._geom(B, 0, Sx)

        # ---- the Euler loop: everything that does not depend on x is prepared above, the loop itself is tensors in / tensors out
        #      (10 steps x 18 layers x ~14 tiny launches are host-bound when issued from Python); every step's RoPE launch writes the
        #      suffix keys / values behind the prefix, at [P, P + 1 + chunk) of the layer's buffer
        def euler(x, states_d, te_table, q_limit, key_valid, pos):
            for s in range(len(times)):
                stok, _, _ = self.embed_suffix(states_d, x, None, te=te_table[s])
                _, h = self._mot_layers(geom_s, None, stok.reshape(B * Sx, -1).contiguous(), None, cos_t, sin_t, None, pos,
                                        q_limit, key_valid, kv=kv, kv0=P)
                v_t = self._v_t(self._final_norm(h).view(B, Sx, -1))
                x = K.add(x, K.scale_(v_t.contiguous(), dt))             # Euler step x += v dt
            return x
        inputs = dict(x=x, states_d=states_d, te_table=te_table, q_limit=q_limit, key_valid=key_valid, pos=pos)
        key = ("euler", int(diffusion_steps), P, cos_t.data_ptr(), kv[0][0].data_ptr())
        return self._run_sampler(euler, inputs, key, kwargs.get("use_graph"))



from ..dexbotic_arch import register_model_with_hf  # noqa: E402

register_model_with_hf(Pi0ForCausalLM)
