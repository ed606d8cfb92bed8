"""Host side of the reference's SimpleVLA-RL post-training of OFT-discrete (dexbotic/exp/rl/rl_trainer.py): outcome rewards, KL
penalty, group-normalised advantages, the trajectory mask, and the GRPO policy update driven through ``NativeTrainer``.

The functions keep the reference's names, arithmetic and quirks (cited per function); they are small torch expressions over a
rollout batch and run wherever their inputs live.  The device work of the update is the model's: ``action_log_probs`` and the
``forward`` with ``old_log_probs`` (model/oft/oft_discrete_arch.py, functional.BinPolicyLossFn).

A rollout batch is a dict of tensors with a leading [B, traj] (B trajectories of ``traj`` policy calls, each predicting R =
chunk_size x action_dim tokens): ``input_ids`` / ``attention_mask`` [B, traj, L], ``pixel_values`` [B, traj, ...], ``responses``
[B, traj, R] token ids, ``finish_step`` [B] (environment steps until the episode ended), optionally ``proprio`` [B, traj, P]; the
update also reads ``old_log_probs`` and ``advantages`` [B, traj R].

Out of scope: rollout collection, environments, the Redis re-balancer and the torch.distributed glue of simplevla_rl_exp.py; a critic;
running a frozen reference policy (``ref_log_prob`` is an input of ``apply_kl_penalty``).
"""
from __future__ import annotations

from collections import defaultdict
from dataclasses import dataclass
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch


def response_mask(finish_step: torch.Tensor, response_length: int, action_dim: int) -> torch.Tensor:
    """[B, response_length] bool: token t of trajectory b is valid iff t < finish_step[b] * action_dim (rl_trainer.py:93-97,
    156-158, 562-566)"""
    finish = finish_step * action_dim
    steps = torch.arange(response_length, device=finish.device)
    return steps.unsqueeze(0).expand(finish.size(0), -1) < finish.unsqueeze(1)


def masked_mean(values, mask, axis=None):
    """rl_trainer.py:124-129: sum(values * mask) / sum(mask), and 0 where the mask is empty"""
    mask_sum = mask.sum(axis=axis)
    masked_sum = (values * mask).sum(axis=axis)
    result = masked_sum / torch.clamp(mask_sum, min=1e-8)
    return torch.where(mask_sum > 0, result, masked_sum * 0.0)


def _key(x):
    """a group id as a dict key.  The reference keys its dict with ``index[i]`` itself (rl_trainer.py:74): strings out of a numpy
    array there.  Tensor and numpy scalars are unwrapped here, so equal ids share a group also when ``uid`` is a tensor (which the
    reference, hashing tensors by identity, would put into groups of one)."""
    return x.item() if hasattr(x, "item") else x


def grpo_outcome_advantage(token_level_rewards: torch.Tensor, mask: torch.Tensor, uid, epsilon: float = 1e-6):
    """compute_grpo_outcome_advantage (rl_trainer.py:58-88): a trajectory's score is the sum of its token rewards; scores are
    normalised within their ``uid`` group by the group's mean and UNBIASED standard deviation (``torch.std``), a group of one by
    mean 0 and std 1; the result is tiled over the response and masked.  Returns (advantages, returns), the same tensor twice."""
    response_length = token_level_rewards.shape[-1]
    scores = token_level_rewards.sum(dim=-1)
    id2score = defaultdict(list)
    id2mean, id2std = {}, {}
    with torch.no_grad():
        bsz = scores.shape[0]
        for i in range(bsz):
            id2score[_key(uid[i])].append(scores[i])
        for idx in id2score:
            if len(id2score[idx]) == 1:
                id2mean[idx] = torch.tensor(0.0)
                id2std[idx] = torch.tensor(1.0)
            else:
                id2mean[idx] = torch.mean(torch.tensor(id2score[idx]))
                id2std[idx] = torch.std(torch.tensor([id2score[idx]]))
        for i in range(bsz):
            k = _key(uid[i])
            scores[i] = (scores[i] - id2mean[k]) / (id2std[k] + epsilon)
        scores = scores.unsqueeze(-1).tile([1, response_length]) * mask
    return scores, scores


def kl_penalty(logprob: torch.Tensor, ref_logprob: torch.Tensor, kl_penalty: str) -> torch.Tensor:
    """rl_trainer.py:132-143"""
    if kl_penalty == "kl":
        return logprob - ref_logprob
    if kl_penalty == "abs":
        return (logprob - ref_logprob).abs()
    if kl_penalty == "mse":
        return 0.5 * (logprob - ref_logprob).square()
    raise NotImplementedError(kl_penalty)


class FixedKLController:
    """rl_trainer.py:179-184"""

    def __init__(self, kl_coef):
        self.value = kl_coef

    def update(self, current_kl, n_steps):
        pass


def apply_kl_penalty(batch: Dict[str, Any], kl_ctrl, kl_penalty: str = "kl", action_token_len: int = 7, action_chunks_len: int = 8):
    """rl_trainer.py:146-176: ``token_level_rewards = token_level_scores - beta * kl(old_log_probs, ref_log_prob)`` over the valid
    tokens; without ``ref_log_prob`` in the batch beta is 0.  Returns (batch, {"critic/kl", "critic/kl_coeff"}).  The keyword
    ``kl_penalty`` shadows the function of that name, as in the reference, which then calls the string and raises TypeError whenever
    a ``ref_log_prob`` is present; here the module-level function is looked up explicitly, so that branch computes what it says."""
    responses = batch["responses"]
    traj_length = responses.size(1) * action_chunks_len
    mask = response_mask(batch["finish_step"], traj_length * action_token_len, action_token_len)
    if "ref_log_prob" in batch.keys():
        kld = globals()["kl_penalty"](batch["old_log_probs"], batch["ref_log_prob"], kl_penalty) * mask
        beta = kl_ctrl.value
    else:
        beta = 0
        kld = torch.zeros_like(mask, dtype=torch.float32)
    batch["token_level_rewards"] = batch["token_level_scores"] - beta * kld
    current_kl = torch.mean(masked_mean(kld, mask=mask, axis=-1), dim=0).item()
    kl_ctrl.update(current_kl=current_kl, n_steps=responses.shape[0])
    return batch, {"critic/kl": current_kl, "critic/kl_coeff": beta}


def outcome_rewards(batch: Dict[str, Any], action_dim: int, reward_coef: float = 5.0) -> Tuple[Dict[str, torch.Tensor], Dict[str, float]]:
    """RobRewardManager.__call__ (rl_trainer.py:214-247): ``reward_coef x complete[b]`` on token ``finish_step[b] * action_dim - 1``
    of the flattened response (index -1, the last token, for finish_step 0), zero elsewhere.  ``acc`` in the batch takes the place
    of ``complete``.  Returns ({"gt_scores", "all"} each [B, traj R] fp32, metrics)."""
    responses = batch["responses"]
    B = responses.shape[0]
    verifier = torch.zeros((B, responses[0].numel()), dtype=torch.float32, device=responses.device)
    valid = batch["finish_step"] * action_dim
    metrics = {}
    if "acc" in batch:
        score = batch["acc"].cpu().numpy().tolist()
    else:
        score = [float(c) for c in batch["complete"].tolist()]
        assert len(score) == B
        metrics["all"] = float(np.mean(score)) if B else 0.0
    for i in range(B):
        verifier[i, int(valid[i]) - 1] += score[i]
    reward = torch.zeros_like(verifier)
    if reward_coef != 0:
        metrics["verifier"] = verifier.sum(dim=1).mean().item()
        reward = reward + reward_coef * verifier
    metrics["reward_all"] = reward.sum(dim=-1).mean(dim=0).item()
    return {"gt_scores": verifier, "all": reward}, metrics


@dataclass
class GRPOUpdateConfig:
    """what ``update_policy`` / ``compute_log_prob`` read from the reference's exp config (model_config.rollout.temperature,
    model_config.actor.*; rl_trainer.py:545-587)"""
    temperature: float = 1.6
    clip_ratio_low: float = 0.2
    clip_ratio_high: float = 0.28
    traj_mini_batch_size: int = 8
    update_iters: int = 3                   # the reference's fixed three passes over the batch
    token_offset: Optional[int] = None      # len(tokenizer) - num_bins + 1 when the tokenizer length differs from vocab_size


class GRPOPolicyUpdater:
    """``compute_log_prob`` and ``update_policy`` of DexboticRLTrainer (rl_trainer.py:401-418, 537-669) on a ``NativeTrainer``
    whose model is an ``OFTDiscreteForCausalLM``."""

    METRICS = ("actor/pg_loss", "actor/pg_clipfrac", "actor/ppo_kl")

    def __init__(self, trainer, cfg: Optional[GRPOUpdateConfig] = None):
        self.trainer, self.model, self.cfg = trainer, trainer.model, cfg or GRPOUpdateConfig()
        mc = self.model.config
        self.action_dim, self.chunk_size, self.use_proprio = int(mc.action_dim), int(mc.chunk_size), bool(mc.use_proprio)
        # every update chunk carries its own loss denominator and reports its own sums: chunks are never merged into one pass
        trainer.coalesce = False

    @staticmethod
    def _flat(t, lo: int = 0, hi: Optional[int] = None):
        """[B, traj, ...] -> [B traj, ...]; with B = 1, the calls lo .. hi of the trajectory"""
        t = t.reshape((t.shape[0] * t.shape[1],) + tuple(t.shape[2:]))
        return t if hi is None else t[lo:hi]

    def compute_log_prob(self, batch: Dict[str, Any], masked: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """(entropy, log_probs) under the current weights, no gradient.  ``masked``: the chunks from ``finish_step`` on are zeroed
        and both results are [B, traj R]; otherwise [B, traj chunk_size, action_dim], as in the reference (rl_trainer.py:361-376)."""
        self.model.eval()
        B, traj = batch["responses"].shape[:2]
        R = batch["responses"].shape[-1]
        entropy, log_probs = self.model.action_log_probs(
            self._flat(batch["input_ids"]), self._flat(batch["attention_mask"]), self._flat(batch["pixel_values"]),
            self._flat(batch["responses"]), self.cfg.temperature, states=self._flat(batch["proprio"]) if self.use_proprio else None,
            token_offset=self.cfg.token_offset)
        log_probs = log_probs.reshape(B, traj * self.chunk_size, self.action_dim)
        entropy = entropy.reshape(B, traj * self.chunk_size, self.action_dim)
        if masked:
            steps = torch.arange(traj * self.chunk_size, device=log_probs.device)
            keep = (steps.unsqueeze(0) < batch["finish_step"].to(log_probs.device).unsqueeze(1)).unsqueeze(-1)
            log_probs = torch.where(keep, log_probs, torch.zeros_like(log_probs)).reshape(B, traj * R)
            entropy = torch.where(keep, entropy, torch.zeros_like(entropy)).reshape(B, traj * R)
        return entropy, log_probs

    def _chunks(self, batch: Dict[str, Any]):
        """the (trajectory, first call, end call, chunk mask [1, n], trajectory mask count) of one pass, in the reference's order;
        trajectories and chunks with an empty mask are left out (the reference runs such a chunk's forward and drops it)"""
        B, traj = batch["responses"].shape[:2]
        R = batch["responses"].shape[-1]
        finish = torch.as_tensor(batch["finish_step"]).cpu()
        split = max(1, int(traj / self.cfg.traj_mini_batch_size))
        step = int(traj / split)
        out = []
        for b in range(B):
            mask = response_mask(finish[b:b + 1], traj * R, self.action_dim)
            total = int(mask.sum())
            if total == 0:
                continue
            for i in range(0, traj, step):
                end = min(i + step, traj)
                cm = mask[:, i * R:end * R]
                if int(cm.sum()) > 0:
                    out.append((b, i, end, cm, total))
        return out

    def chunk_batch(self, batch: Dict[str, Any], b: int, i: int, end: int, chunk_mask: torch.Tensor, total: int) -> Dict[str, Any]:
        """the keyword arguments of the model's forward for calls i .. end of trajectory b: the loss is the chunk's sum over the
        trajectory's valid-token count and the batch size (rl_trainer.py:630-633)"""
        B = batch["responses"].shape[0]
        R = batch["responses"].shape[-1]
        one = slice(b, b + 1)
        kw = dict(input_ids=self._flat(batch["input_ids"][one], i, end), attention_mask=self._flat(batch["attention_mask"][one], i, end),
                  images=self._flat(batch["pixel_values"][one], i, end), responses=self._flat(batch["responses"][one], i, end),
                  old_log_probs=batch["old_log_probs"][one, i * R:end * R], advantages=batch["advantages"][one, i * R:end * R],
                  response_mask=chunk_mask, temperature=self.cfg.temperature, clip_ratio_low=self.cfg.clip_ratio_low,
                  clip_ratio_high=self.cfg.clip_ratio_high, loss_denominator=float(total) * B, token_offset=self.cfg.token_offset)
        if self.use_proprio:
            kw["states"] = self._flat(batch["proprio"][one], i, end)
        return kw

    def update_policy(self, batch: Dict[str, Any]) -> Dict[str, float]:
        """``update_iters`` passes over the batch, trajectory by trajectory in chunks of ``traj_mini_batch_size`` policy calls, one
        clipped optimizer step per pass.  The metrics add up over ALL passes, as the reference's ``loss_info`` does, and are kept
        on the device until the one read-back at the end (the reference reads three scalars back per chunk)."""
        tr = self.trainer
        self.model.train()
        B = batch["responses"].shape[0]
        acc = None
        step0, lr_scale = tr.global_step, tr.lr_scale()     # the reference's scheduler steps once per call, after the passes
        for _ in range(self.cfg.update_iters):
            chunks = self._chunks(batch)
            if not chunks:                    # nothing valid anywhere: the reference steps its optimizer on zero gradients
                continue
            tr.set_grad_accum(len(chunks))
            for b, i, end, cm, total in chunks:
                tr.micro_step(self.chunk_batch(batch, b, i, end, cm, total), loss_scale=1.0)
                part = tr.last_output.sums[:3] / (float(total) * B)
                acc = part if acc is None else acc + part
            tr.apply_update(lr_scale=lr_scale)
        tr.global_step = step0 + 1
        info = {k: 0.0 for k in self.METRICS}
        info["actor/grad_norm"] = 0.0
        if acc is not None:
            opt = tr.opt
            if tr.cfg.max_grad_norm is None:
                raise NotImplementedError("actor/grad_norm is the clip's norm: OptimConfig.max_grad_norm must be set")
            host = torch.cat([acc, opt.norm.reshape(1).float()]).cpu().tolist()
            info.update(dict(zip(self.METRICS + ("actor/grad_norm",), host)))
        return info
