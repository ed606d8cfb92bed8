"""OFT-discrete policy: host-side mirror of dexbotic/model/oft/oft_discrete_arch.py on libdexbotic_amd kernels.

The OFT sequence (oft_arch.py) with the LLM's own vocabulary as the action head: the R = ``chunk_size x action_dim`` query rows of every
sample are the embedding row of token 1 (``action_query`` is ``torch.ones(1, R)`` used as token ids, not a parameter), one causal
decoder pass runs, and ``lm_head`` reads the R action rows.  Training scores them with a cross-entropy against the R action tokens cut
out of the prompt; an action request needs only the last ``num_bins - 1`` vocabulary logits of those rows.

What runs where:
* the label surgery (oft_discrete_arch.py:66-106: ``[prefix][R action tokens][1 suffix token][padding]`` -> ``[prefix][suffix]
  [padding]``, the R labels become the targets) is host integer work on the ids, done before the splice plan is built;
* ``functional.OftDiscreteSpliceFn`` writes the token's embedding row (and the projected proprio row) into the rows the
  ``rule="oft"`` plan reserves; ``functional.ActionRowsFn`` hands the R rows of every sample to ``functional.LmHeadLossFn`` as one
  dense [B R, d] operand, on the UN-shifted targets (``F.cross_entropy`` over the rows, ignore_index -100, mean);
* ``inference_action`` / ``generate_action`` run the decoder pass and then dxa_action_bins_fwd on the decoder output in place: the
  ``num_bins - 1`` logits, their first-index argmax and the action value, in one launch.  The vocabulary logits are never formed;
* the GRPO policy update (dexbotic/exp/rl/rl_trainer.py): ``action_log_probs`` scores taken bins with dxa_bin_logprob_fwd on those
  bin logits, and ``forward`` with ``old_log_probs`` returns the clipped policy loss through ``functional.BinPolicyLossFn`` (the bin
  rows of ``lm_head.weight`` as their own operand); the loop around them is ``exp/rl.py``.

Quirks kept from the reference: the loss is computed only when ``actions`` is given (and needs the targets cut from ``labels``:
``actions`` without ``labels`` raises ValueError here, where the reference dies with an unbound name); ``get_output_embeddings()`` is
None; ``lm_head.weight`` receives a gradient.  Left padding is refused, as in OFT.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from ... import functional as Fn
from ... import hostcpu
from ... import kernels as K
from ...constants import IGNORE_INDEX
from ..dexbotic_arch import CausalLMOutputDexbotic, register_model_with_hf, register_with_hf
from .oft_arch import OFTConfig, OFTForCausalLM, OFTModel


class OFTDiscreteConfig(OFTConfig):
    model_type = "dexbotic_oft_discrete"

    def __init__(self, num_bins: Optional[int] = 256, **kwargs):
        super().__init__(**kwargs)
        self.num_bins = num_bins


register_with_hf(OFTDiscreteConfig)


class OFTDiscreteModel(OFTModel):
    pass


def cut_action_tokens(input_ids, attention_mask, labels, n_action: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The reference's label surgery (oft_discrete_arch.py:66-106) on host integers.  Sample i has n_i = attention_mask[i].sum()
    un-padded tokens ``[prefix (n_i - n_action - 1)][n_action action tokens][1 suffix token]``; the action tokens are removed:
    ids -> ``ids[:prefix] + ids[n_i - 1:]`` (the suffix token and the padding behind it), mask -> ones on ``[0, prefix]``, targets ->
    ``labels[prefix : prefix + n_action]``.  Returns (ids [B, L - n_action], mask, targets [B, n_action])."""
    ids = np.asarray(input_ids, dtype=np.int64)
    mask = np.asarray(attention_mask)
    lab = np.asarray(labels, dtype=np.int64)
    B, L = ids.shape
    new_ids = np.empty((B, L - n_action), dtype=np.int64)
    new_mask = np.zeros((B, L - n_action), dtype=mask.dtype)
    targets = np.empty((B, n_action), dtype=np.int64)
    for i in range(B):
        n = int(mask[i].sum())
        prefix = n - n_action - 1
        if prefix < 0:
            raise ValueError(f"OFT-discrete: sample {i} has {n} un-padded tokens, fewer than the {n_action} action tokens plus the "
                             "suffix token that the labelled layout holds")
        new_ids[i] = np.concatenate([ids[i, :prefix], ids[i, n - 1:]])
        targets[i] = lab[i, prefix:prefix + n_action]
        new_mask[i, :prefix + 1] = 1
    return new_ids, new_mask, targets


class OFTDiscreteForCausalLM(OFTForCausalLM):
    config_class = OFTDiscreteConfig

    def _real_init(self, config: OFTDiscreteConfig):
        if getattr(config, "tokenizer_padding_side", "right") == "left":
            raise ValueError("OFT: tokenizer_padding_side='left' is not supported (the reference's insert_action_embedding counts the "
                             "action rows from the left edge and is wrong there); use right padding")
        self.model = OFTDiscreteModel(config, self.store)
        self.store.new_bucket()
        self.store.register([("lm_head.weight", (config.vocab_size, config.hidden_size))])

    def get_output_embeddings(self):
        return None

    def unused_parameter_names(self) -> List[str]:
        """parameters that never get a gradient (the CLIP layer after hidden_states[-2] and post_layernorm); lm_head.weight is
        trained here"""
        return self.model.mm_vision_tower.unused_parameter_names()

    # ------------------------------------------------------------------------------------------------ the shared decoder pass
    def _token_rows(self, device) -> torch.Tensor:
        """the query token as a one-entry list of embedding rows on the device (functional.OftDiscreteSpliceFn), uploaded once"""
        cache = self.__dict__.setdefault("_token_rows_cache", {})
        key = str(device)
        if key not in cache:
            cache[key] = hostcpu.upload(np.array([self.model.action_head.QUERY_TOKEN], dtype=np.int64), device)
        return cache[key]

    def _decode(self, input_ids, attention_mask, images, states):
        """splice + fill + ONE decoder pass -> (hidden [B, Sq, d], off [B] int64 on the device)"""
        model, cfg, st = self.model, self.config, self.store
        head = model.action_head
        if head is None:
            raise ValueError("OFT: config.action_model_type is not set: there is no action head to run")
        assert "Discrete" in cfg.action_model_type, "This forward method is only for OFT-discrete model."
        if model.mm_vision_module is None or images is None:
            raise NotImplementedError("text-only forward is outside the VLA path")
        plan = model.oft_plan(input_ids, attention_mask, None, images)
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
        embeds = Fn.OftDiscreteSpliceFn.apply(image_features, state_embeds, st.params[embed_n], st, embed_n, head.QUERY_TOKEN,
                                              self._token_rows(dev), pd["plan"], off, B, Sq, head.num_query_rows).view(B, Sq, -1)
        mask = plan.attention_mask if attention_mask is not None else None
        return model.run_llm(embeds, mask), off

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, images=None,
                return_dict=None, cache_position=None, actions=None, states=None, noisy_dict=None,
                responses=None, old_log_probs=None, advantages=None, response_mask=None, temperature: float = 1.0,
                clip_ratio_low: float = 0.2, clip_ratio_high: float = 0.28, loss_denominator: Optional[float] = None,
                token_offset: Optional[int] = None, **kwargs) -> CausalLMOutputDexbotic:
        """``logits`` [B, R, V] as in the reference.  With ``labels`` and ``actions``: the loss; with ``labels`` alone: no loss (the
        action tokens are still cut out of the prompt); with ``actions`` alone: ValueError.  With ``old_log_probs``: the GRPO policy
        update (``_policy_forward``)."""
        cfg, st = self.config, self.store
        R = cfg.chunk_size * cfg.action_dim
        if old_log_probs is not None:
            return self._policy_forward(input_ids, attention_mask, images, states, responses, old_log_probs, advantages,
                                        response_mask, temperature, clip_ratio_low, clip_ratio_high, loss_denominator, token_offset)
        targets = None
        if labels is not None:
            if attention_mask is None:
                raise ValueError("OFT-discrete: labels need the attention_mask (the action tokens are found from the un-padded length)")
            plans = self.model._plans
            input_ids, attention_mask, targets = cut_action_tokens(plans.host(input_ids), plans.host(attention_mask),
                                                                   plans.host(labels), R)
        elif actions is not None:
            raise ValueError("OFT-discrete: actions without labels: the cross-entropy targets are the action tokens' labels, cut from "
                             "`labels`")
        hidden, off = self._decode(input_ids, attention_mask, images, states)
        B = hidden.shape[0]
        rows = Fn.ActionRowsFn.apply(hidden, off, R, bool(cfg.use_proprio))               # [B R, d]
        loss = None
        if actions is not None:
            flat = np.ascontiguousarray(targets.reshape(-1))
            loss, logits = Fn.LmHeadLossFn.apply(rows, st.params["lm_head.weight"], st, "lm_head.weight",
                                                 hostcpu.upload(flat, hidden.device), int((flat != IGNORE_INDEX).sum()))
        else:
            logits = K.mm_nt(rows, st.w("lm_head.weight"))
        return CausalLMOutputDexbotic(loss=loss, logits=logits.view(B, R, -1), past_key_values=None, hidden_states=(hidden,),
                                      attentions=None)

    __call__ = nn.Module.__call__

    # ------------------------------------------------------------------------------------------------ GRPO policy update
    def _response_bins(self, responses, rows: int, token_offset: Optional[int]) -> torch.Tensor:
        """token ids [N, R] -> bin indices [N R] int64 on the device: ``responses - (len(tokenizer) - num_bins + 1)``
        (rl_trainer.py:355); ``token_offset`` defaults to what ``generate_action`` adds"""
        cfg = self.config
        off = cfg.vocab_size - cfg.num_bins + 1 if token_offset is None else int(token_offset)
        r = torch.as_tensor(responses).to(device=self.store.device, dtype=torch.int64).reshape(-1)
        if r.numel() != rows:
            raise ValueError(f"OFT-discrete: {r.numel()} response tokens for {rows} action rows")
        return (r - off).contiguous()

    def _policy_forward(self, input_ids, attention_mask, images, states, responses, old_log_probs, advantages, response_mask,
                        temperature, clip_low, clip_high, denom, token_offset) -> CausalLMOutputDexbotic:
        """One update chunk of the reference's ``update_policy`` (rl_trainer.py:591-634): the log-probabilities of the taken bins
        under the current weights and the clipped policy loss against ``old_log_probs`` / ``advantages`` over ``response_mask``
        (each N R values, any shape), through functional.BinPolicyLossFn.  ``loss`` = sum / ``loss_denominator`` (None: the mask's
        own count, the reference's masked_mean; an empty mask gives 0 and zero gradients).  The output also carries ``sums`` [4]
        (sum of max(pg1, pg2), clipped count, sum of old - new log-prob, valid count), ``log_probs`` and ``entropy`` [N, R] fp32.
        No labels and no actions: a rollout prompt holds no action tokens.  ``logits`` is None: not even the bin logits outlive
        the backward."""
        cfg, st = self.config, self.store
        if responses is None or advantages is None or response_mask is None:
            raise ValueError("OFT-discrete: old_log_probs needs responses, advantages and response_mask")
        R = cfg.chunk_size * cfg.action_dim
        hidden, off = self._decode(input_ids, attention_mask, images, states)
        N = hidden.shape[0]
        rows = Fn.ActionRowsFn.apply(hidden, off, R, bool(cfg.use_proprio))               # [N R, d]
        dev = hidden.device

        def f32(t, what):
            t = torch.as_tensor(t).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if t.numel() != N * R:
                raise ValueError(f"OFT-discrete: {what} holds {t.numel()} values for {N * R} action rows")
            return t

        loss, logp, entropy, sums = Fn.BinPolicyLossFn.apply(
            rows, st.params["lm_head.weight"], st, "lm_head.weight", cfg.num_bins - 1, self._response_bins(responses, N * R, token_offset),
            f32(old_log_probs, "old_log_probs"), f32(advantages, "advantages"), f32(response_mask, "response_mask"),
            float(temperature), float(clip_low), float(clip_high), None if denom is None else float(denom))
        out = CausalLMOutputDexbotic(loss=loss, logits=None, past_key_values=None, hidden_states=(hidden,), attentions=None)
        out.sums, out.log_probs, out.entropy = sums, logp.view(N, R), entropy.view(N, R)
        return out

    @torch.no_grad()
    def action_log_probs(self, input_ids, attention_mask, images, responses, temperature, states=None,
                         token_offset: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(entropy, log_probs), each [N, R] fp32, of the taken bins ``responses`` (token ids [N, R]) under softmax(bin logits /
        temperature): the reference's ``_forward_micro_batch`` without its masking (rl_trainer.py:343-359).  One decoder pass,
        dxa_action_bins_fwd on the decoder output in place, dxa_bin_logprob_fwd; the vocabulary logits are never formed."""
        bin_logits, _, _ = self._bins(input_ids, attention_mask, images, states)
        rows = bin_logits.shape[0]
        logp, entropy, _ = K.bin_logprob_fwd(bin_logits, self._response_bins(responses, rows, token_offset), float(temperature))
        R = self.config.chunk_size * self.config.action_dim
        return entropy.view(-1, R), logp.view(-1, R)

    # ------------------------------------------------------------------------------------------------ action requests
    def _bins(self, input_ids, attention_mask, images, states):
        """decoder pass + dxa_action_bins_fwd -> (bin_logits [B R, NB], bin [B R] int64, action [B R] fp32)"""
        cfg = self.config
        hidden, off = self._decode(input_ids, attention_mask, images, states)
        W = self.store.w("lm_head.weight")
        NB = cfg.num_bins - 1
        return K.action_bins_fwd(hidden.contiguous(), off, W[W.shape[0] - NB:], cfg.chunk_size * cfg.action_dim, bool(cfg.use_proprio))

    @torch.no_grad()
    def inference_action(self, input_ids, image_tensor, inference_args={}, **kwargs):
        """Reference contract (oft_discrete_arch.py:206-235): one pass, the argmax over the last ``num_bins - 1`` vocabulary logits
        of every action row, bin / (num_bins - 1) * 2 - 1, the first sample's [T][A] de-normalised with
        ``inference_args["action_norms"]``."""
        cfg = self.config
        _, _, action = self._bins(input_ids, None, image_tensor, inference_args.get("states", None))
        actions = action.view(-1, cfg.chunk_size, cfg.action_dim)[0]
        return self._denorm(actions.float().cpu().numpy(), inference_args.get("action_norms")).tolist()

    @torch.no_grad()
    def generate_action(self, input_ids, pixel_values, attention_masks, temperature, inference_args={},
                        generator: Optional[torch.Generator] = None, return_logits: bool = False, **kwargs):
        """Reference contract (oft_discrete_arch.py:237-282): one draw per action row from softmax(bin logits / temperature);
        returns (actions of the WHOLE batch, de-normalised; response_ids = bin + vocab_size - num_bins + 1).

        The draw is dxa_sample_rows on the bin logits (temperature, top_k = 0, top_p = 1) with the uniforms
        ``torch.rand(B R, dtype=float32, generator=generator, device=<the generator's, or the model's when it is None>)``: the same
        generator state gives the same ids.  ``torch.multinomial``'s random stream cannot be matched: the reference's draws for a
        given seed differ, their distribution does not.  ``return_logits``: the bin logits [B R, NB] as a third result."""
        cfg = self.config
        dev = self.store.device
        bin_logits, _, _ = self._bins(input_ids, attention_masks, pixel_values, inference_args.get("states", None))
        rows = bin_logits.shape[0]
        u = torch.rand(rows, dtype=torch.float32, generator=generator,
                       device=generator.device if generator is not None else dev).to(dev)
        bins = K.sample_rows(bin_logits, u, float(temperature), 0, 1.0).view(-1, cfg.chunk_size * cfg.action_dim)
        response_ids = bins + cfg.vocab_size - cfg.num_bins + 1
        predicted = self.model.action_head.discrete_tokens_to_continuous(bins.cpu())
        actions = self._denorm(predicted.float().cpu().numpy(), inference_args.get("action_norms")).tolist()
        return (actions, response_ids, bin_logits) if return_logits else (actions, response_ids)


register_model_with_hf(OFTDiscreteForCausalLM)
