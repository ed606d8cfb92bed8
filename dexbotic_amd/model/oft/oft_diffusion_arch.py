"""OFT with the diffusion (``DiT``) head: host-side mirror of the ``else`` branches of dexbotic/model/oft/oft_arch.py on libdexbotic_amd
kernels.

The OFT sequence (oft_arch.py) with noisy actions in place of the learned queries: behind every sample's un-padded prompt rows stand
``[state row, with use_proprio] [time row] [T A noisy-action rows]``.  Every noisy action COMPONENT is one row
(``noisy_action_projector``: Linear(1, d) -> GELU(erf) -> Linear(d, d)), the time row is the sinusoidal encoding of the diffusion
timestep, one causal decoder pass runs and the MLP-ResNet (``noise_predictor.mlp_resnet``) reads the T A hidden rows behind the time
row as T rows of A d columns: the predicted noise.  Trained with an MSE against the noise that was added.

What runs where:
* ``functional.NoisyEmbedFn`` (dxa_noisy_embed_fwd/bwd): fc1 and the GELU in one pass, the [B T A, d] operand of fc2; fc2 is a product
  with a bias epilogue; ``functional.DiffusionSpliceFn`` (dxa_diffusion_put_fwd/bwd) writes the rows into the block the ``rule="oft"``
  plan reserves; the head's first LayerNorm reads its rows out of the decoder output (``functional.ActionNormFn``);
  ``functional.MseLossFn`` in fp32;
* ``inference_action``: the reference runs the WHOLE model once per DDIM step (oft_arch.py:232-249).  Attention is causal and the
  time and action rows stand behind the prompt, so the prompt's keys and values do not depend on the step: here the prompt (and the
  state row) is prefilled ONCE into a ``KVCache`` and every step runs the decoder on the 1 + T A suffix rows alone, with
  dxa_ddim_step_embed as the two ends of a step in one launch.  ``inference_args["cached"] = False`` runs the reference's algorithm,
  one full ``forward`` per step.

Deviations from the reference, all deliberate: a config class of its own (``OFTDiffusionConfig``, same model_type string; see
action_model/builder.py); ``inference_action`` refuses a batch (the reference dies in ``torch.cat`` there); the sampler's state is fp32
in every compute dtype (the reference keeps it in the images' dtype); the schedule is ``action_model/ddim.py``, pinned to the DDIM
formulas and not checked against the ``diffusers`` package; ``inference_args`` takes ``noise`` / ``generator`` / ``cached``; ``forward``
returns a loss whenever it knows the noise (the reference: only with ``actions``); with neither ``actions`` nor ``noisy_dict`` it raises
ValueError (the reference dies in ``sample_noisy_actions(None)``).
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from ... import functional as Fn
from ... import hostcpu
from ... import kernels as K
from ...splice import SplicePlan
from ..dexbotic_arch import CausalLMOutputDexbotic
from .action_model.ddim import CLIP_SAMPLE_RANGE
from .oft_arch import OFTConfig, OFTForCausalLM, OFTModel


class OFTDiffusionConfig(OFTConfig):
    """``OFTConfig`` for ``action_model_type="DiT"``.  The model_type string stays the reference's ``dexbotic_oft`` (a saved
    config.json is the reference's), so the class is NOT registered with AutoConfig: the string belongs to ``OFTConfig``;
    ``dexbotic_amd.from_pretrained`` tells the two apart by ``action_model_type``."""
    model_type = "dexbotic_oft"

    def __init__(self, num_diffusion_steps: Optional[int] = 100, **kwargs):
        super().__init__(**kwargs)
        self.num_diffusion_steps = num_diffusion_steps


class OFTDiffusionModel(OFTModel):
    @staticmethod
    def time_offsets(plan: SplicePlan, skip: int, device) -> torch.Tensor:
        """the TIME row of each sample's reserved block on the device (``non_padding_lengths`` + 1 with a state row): what the head's
        LayerNorm takes as its offset with one row to skip; uploaded once per plan"""
        if not skip:
            return OFTModel.plan_offsets(plan, device)
        cache = plan.__dict__.setdefault("_toff", {})
        key = str(device)
        if key not in cache:
            cache[key] = hostcpu.upload(np.ascontiguousarray(plan.lengths, dtype=np.int64) + 1, device)
        return cache[key]


class OFTDiffusionForCausalLM(OFTForCausalLM):
    config_class = OFTDiffusionConfig

    def _real_init(self, config: OFTDiffusionConfig):
        if getattr(config, "tokenizer_padding_side", "right") == "left":
            raise ValueError("OFT: tokenizer_padding_side='left' is not supported (the reference's insert_action_embedding counts the "
                             "action rows from the left edge and is wrong there); use right padding")
        self.model = OFTDiffusionModel(config, self.store)
        self.store.new_bucket()
        self.store.register([("lm_head.weight", (config.vocab_size, config.hidden_size))])

    def _head(self):
        head, cfg = self.model.action_head, self.config
        if head is None:
            raise ValueError("OFT: config.action_model_type is not set: there is no action head to run")
        assert "DiT" in cfg.action_model_type, "This forward method is only for the OFT diffusion head."
        return head

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, images=None,
                return_dict=None, cache_position=None, actions=None, states=None, noisy_dict=None,
                **kwargs) -> CausalLMOutputDexbotic:
        """``logits``: the predicted noise [B, T, A].  ``noisy_dict`` (``noisy_actions`` [B, T, A], ``diffusion_timestep_embeddings``
        [B, 1, d], ``noise`` [B, T, A] or absent) makes the pass deterministic; without it ``sample_noisy_actions(actions)`` draws."""
        model, cfg, st = self.model, self.config, self.store
        head = self._head()
        if model.mm_vision_module is None or images is None:
            raise NotImplementedError("text-only forward is outside the VLA path")
        if actions is None and noisy_dict is None:
            raise ValueError("OFT diffusion: forward needs `actions` (noise and timesteps are then drawn) or a `noisy_dict`")
        A, T = cfg.action_dim, cfg.chunk_size
        dev = st.device
        if actions is not None:
            actions = actions.to(device=dev, dtype=torch.float32).reshape(actions.size(0), -1, A)[:, :T, :]
        if noisy_dict is None:
            noisy_dict = head.sample_noisy_actions(actions)
        noise, noisy = noisy_dict.get("noise"), noisy_dict["noisy_actions"]
        # the integer plan first (host arithmetic on a few KB), then the device work is enqueued
        plan = model.oft_plan(input_ids, attention_mask, labels, images)
        model._last_plan = plan
        image_features = model._extract_vision_features(images.to(device=dev, dtype=st.compute_dtype))
        skip = 1 if cfg.use_proprio else 0
        state_embeds = None
        if skip:
            assert states is not None, "states is required when use_proprio is True"
            state_embeds = head.proprio_projector(states)                                # [B, d]: one row per sample
        pd = plan.dev(dev)
        off = model.plan_offsets(plan, dev)
        B, Sq = plan.plan.shape
        if noisy.numel() != B * T * A:
            raise ValueError(f"OFT diffusion: noisy_actions holds {noisy.numel()} values for {B} x {T} x {A}")
        proj = head.project_noisy_actions(noisy)                                         # [B T A, d]
        time = noisy_dict["diffusion_timestep_embeddings"].to(device=dev, dtype=st.compute_dtype).reshape(B, -1).contiguous()
        embed_n = model.llm.embed_name
        embeds = Fn.DiffusionSpliceFn.apply(image_features, proj, time, state_embeds, st.params[embed_n], st, embed_n, pd["plan"], off,
                                            B, Sq).view(B, Sq, -1)
        # causal attention, key range [0, len_b + Q) per sample (all of it when nothing is padded), positions arange(S + Q)
        mask = plan.attention_mask if attention_mask is not None else None
        hidden = model.run_llm(embeds, mask)
        predicted_noise = head.predict_noise(hidden, model.time_offsets(plan, skip, dev), 1)      # [B, T, A]
        loss = None
        if noise is not None:
            target = noise.to(device=dev, dtype=torch.float32).reshape(B, T, A).contiguous()
            loss = Fn.MseLossFn.apply(predicted_noise, target)
        return CausalLMOutputDexbotic(loss=loss, logits=predicted_noise, past_key_values=None, hidden_states=(hidden,),
                                      attentions=None)

    __call__ = nn.Module.__call__

    # ------------------------------------------------------------------------------------------------ the sampler
    @torch.no_grad()
    def sample_actions(self, input_ids, image_tensor, states=None, noise: Optional[torch.Tensor] = None,
                       generator: Optional[torch.Generator] = None, num_ddim_steps: int = 10, cached: bool = True,
                       trajectory: Optional[List] = None) -> torch.Tensor:
        """The DDIM loop for ONE sample -> the normalised action chunk [T, A] fp32 on the device.  ``noise`` [1, T, A] is the start;
        without it ``torch.randn`` (``generator``) draws it.  ``trajectory``: a list that receives (eps_k, x_k) fp32 clones per step."""
        cfg, st = self.config, self.store
        head = self._head()
        dev = st.device
        A, T = cfg.action_dim, cfg.chunk_size
        R = T * A
        if int(input_ids.shape[0]) != 1:
            raise ValueError(f"OFT diffusion: inference_action takes one sample, got a batch of {int(input_ids.shape[0])} (the "
                             "reference cannot run a batch either: its time row is [1, 1, d])")
        if noise is None:
            gdev = generator.device if generator is not None else dev
            noise = torch.randn((1, T, A), generator=generator, device=gdev, dtype=torch.float32)
        if noise.numel() != R:
            raise ValueError(f"OFT diffusion: the start noise holds {noise.numel()} values for 1 x {T} x {A}")
        x = noise.to(device=dev, dtype=torch.float32).reshape(R).contiguous().clone()
        sched = head.noise_scheduler
        ts = sched.set_timesteps(int(num_ddim_steps))
        n = len(ts)
        trows = head.time_table(dev)[ts].to(st.compute_dtype).contiguous()              # [n, d]: the time rows, computed once
        step = self._cached_steps if cached else self._full_pass_steps
        return step(input_ids, image_tensor, states, x, trows, n, trajectory).view(T, A)

    def _full_pass_steps(self, input_ids, image_tensor, states, x, trows, n, trajectory):
        """the reference's algorithm (oft_arch.py:232-249): the whole model per step, the scheduler's step on the host's formulas"""
        cfg, sched = self.config, self.model.action_head.noise_scheduler
        for k in range(n):
            nd = dict(noisy_actions=x.view(1, cfg.chunk_size, cfg.action_dim), diffusion_timestep_embeddings=trows[k].view(1, 1, -1))
            eps = self(input_ids, images=image_tensor, use_cache=True, noisy_dict=nd, states=states).logits.reshape(-1).float()
            x = sched.step(eps, k, x)
            if trajectory is not None:
                trajectory.append((eps.clone(), x.clone()))
        return x

    def _cached_steps(self, input_ids, image_tensor, states, x, trows, n, trajectory):
        model, cfg, st = self.model, self.config, self.store
        head = model.action_head
        sched = head.noise_scheduler
        dev, cd = st.device, st.compute_dtype
        R = x.numel()
        if model.mm_vision_module is None or image_tensor is None:
            raise NotImplementedError("text-only forward is outside the VLA path")
        # the prompt through the vision tower and the splice ONCE; with proprio its state row follows
        plan = model._splice_plan(input_ids, None, None, image_tensor)
        image_features = model._extract_vision_features(image_tensor.to(device=dev, dtype=cd))
        embed_n = model.llm.embed_name
        d = image_features.shape[-1]
        prefix = Fn.SpliceFn.apply(image_features, st.params[embed_n], st, embed_n, plan.dev(dev)["plan"]).view(1, -1, d)
        if cfg.use_proprio:
            assert states is not None, "states is required when use_proprio is True"
            prefix = torch.cat([prefix, head.proprio_projector(states).view(1, 1, d)], dim=1)
        P = prefix.shape[1]
        cache = model.llm.new_cache(1, P + 1 + R, dev, cd)
        model.llm.forward_cached(prefix, cache)
        pp = head.p + "noisy_action_projector."
        w1, b1, W2, b2 = (st.w(pp + n_) for n_ in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"))
        suffix = torch.empty((1, 1 + R, d), device=dev, dtype=cd)
        h = torch.empty((R, d), device=dev, dtype=cd)
        off0 = torch.zeros(1, device=dev, dtype=torch.int64)
        eps, coef = None, (0.0, 0.0, 0.0, 0.0)
        for k in range(n):
            # the end of step k - 1 (x updated in place) and the start of step k: time row k and the fc2 operand of the new x
            K.ddim_step_embed_(eps, x, coef, CLIP_SAMPLE_RANGE, trows[k], w1, b1, suffix[0], h)
            if trajectory is not None and eps is not None:
                trajectory.append((eps.float().clone(), x.clone()))
            K.mm_nt(h, W2, bias=b2, out=suffix[0, 1:])                                   # the rows behind the time row, in place
            cache.length = P                                                             # the suffix of the last step is overwritten
            hidden = model.llm.forward_cached(suffix, cache)
            eps = head.predict_noise(hidden, off0, 1).reshape(R).contiguous()
            coef = sched.step_coefficients(k)
        K.ddim_step_embed_(eps, x, coef, CLIP_SAMPLE_RANGE, trows[n - 1], w1, b1, suffix[0], h)      # the last step's end: x is the chunk
        if trajectory is not None:
            trajectory.append((eps.float().clone(), x.clone()))
        return x

    @torch.no_grad()
    def inference_action(self, input_ids, image_tensor, inference_args={}, **kwargs):
        """Reference contract (oft_arch.py:212-254, the diffusion branch): ``num_ddim_steps`` (10) DDIM steps from Gaussian noise,
        the sample's [T][A] actions de-normalised with ``inference_args["action_norms"]``; ``states`` feeds the proprio row.  Here
        also ``noise`` ([1, T, A]) / ``generator`` for the start and ``cached`` (True: one prefill + suffix passes; False: the
        reference's full pass per step)."""
        x = self.sample_actions(input_ids, image_tensor, states=inference_args.get("states", None),
                                noise=inference_args.get("noise", None), generator=inference_args.get("generator", None),
                                num_ddim_steps=inference_args.get("num_ddim_steps", 10), cached=inference_args.get("cached", True))
        return self._denorm(x.float().cpu().numpy(), inference_args.get("action_norms")).tolist()
