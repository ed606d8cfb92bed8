"""The host side of the GRPO policy update (dexbotic_amd/exp/rl.py) without a GPU, against what the reference's own functions
produced (tests/golden/grpo_t1.npz, written by scripts/gen_golden_grpo.py): trajectory mask, outcome rewards, the three KL penalties,
``apply_kl_penalty``, the group-normalised advantages (with a group of one), ``masked_mean``, the chunk schedule of
``update_policy`` and the closed form of d loss / d log_prob that dxa_ppo_clip_fwd writes, against torch autograd.

Bounds.  Masks, rewards and the KL penalties are integer work or the same torch expression on the same fp32 inputs: compared
exactly.  The normalised advantages are an fp32 mean and unbiased standard deviation over a handful of values: 1e-6 relative."""
import os
import types

import numpy as np
import pytest
import torch

_G = {}
TAGS = ("np", "pp")
ADIM, CHUNK, R, TRAJ = 3, 2, 6, 2


def load(golden_dir):
    if not _G:
        _G["g"] = np.load(os.path.join(golden_dir, "grpo_t1.npz"), allow_pickle=False)
    return _G["g"]


def T(a):
    return torch.from_numpy(np.asarray(a))


def valid_mask(g):
    return np.arange(TRAJ * R)[None, :] < (g["finish_step"] * ADIM)[:, None]


def test_response_mask_is_exact(golden_dir):
    from dexbotic_amd.exp import rl
    g = load(golden_dir)
    m = rl.response_mask(T(g["finish_step"]), TRAJ * R, ADIM)
    assert m.dtype == torch.bool and np.array_equal(m.numpy(), valid_mask(g)) and np.array_equal(m.numpy(), g["np/adv3/mask"][:2])
    assert m.sum(1).tolist() == [12, 9]                                    # trajectory 1 ends inside its second call
    assert not rl.response_mask(torch.tensor([0]), 12, ADIM).any()


@pytest.mark.parametrize("tag", TAGS)
def test_outcome_rewards_match_the_reward_manager(golden_dir, tag):
    from dexbotic_amd.exp import rl
    g = load(golden_dir)
    P = tag + "/"
    batch = dict(responses=T(g[P + "responses"]), finish_step=T(g["finish_step"]), complete=T(g["complete"]))
    out, metrics = rl.outcome_rewards(batch, ADIM)
    assert np.array_equal(out["gt_scores"].numpy(), g[P + "gt_scores"]) and np.array_equal(out["all"].numpy(), g[P + "token_level_scores"])
    assert out["all"][0, 4 * ADIM - 1] == 5.0 and float(out["all"].sum()) == 5.0
    assert [metrics["all"], metrics["verifier"], metrics["reward_all"]] == g[P + "reward_metrics"].tolist()
    # ``acc`` takes the place of ``complete``; finish_step 0 lands on the last token (index -1), as in the reference
    out2, _ = rl.outcome_rewards(dict(responses=batch["responses"], finish_step=torch.tensor([0, 3]), acc=torch.tensor([1.0, 0.5])), ADIM)
    assert out2["all"][0, -1] == 5.0 and out2["all"][1, 8] == 2.5 and float(out2["all"].sum()) == 7.5


@pytest.mark.parametrize("tag", TAGS)
def test_kl_penalties_and_apply_kl_penalty(golden_dir, tag):
    from dexbotic_amd.exp import rl
    g = load(golden_dir)
    P = tag + "/"
    old, ref = T(g[P + "old_log_probs"]), T(g[P + "ref_log_prob"])
    for kind in ("kl", "abs", "mse"):
        assert np.array_equal(rl.kl_penalty(old, ref, kind).numpy(), g[P + "kl/" + kind])
    with pytest.raises(NotImplementedError):
        rl.kl_penalty(old, ref, "full")
    ctrl = rl.FixedKLController(float(g["kl_coef"]))
    ctrl.update(current_kl=1.0, n_steps=2)
    assert ctrl.value == float(g["kl_coef"])
    base = dict(responses=T(g[P + "responses"]), finish_step=T(g["finish_step"]), token_level_scores=T(g[P + "token_level_scores"]),
                old_log_probs=old)
    # without a reference policy: beta 0, as recorded from the reference's own call
    b1, m1 = rl.apply_kl_penalty(dict(base), ctrl, "kl", action_token_len=ADIM, action_chunks_len=CHUNK)
    assert np.array_equal(b1["token_level_rewards"].numpy(), g[P + "token_level_rewards"])
    assert [m1["critic/kl"], m1["critic/kl_coeff"]] == g[P + "kl_metrics"].tolist() == [0.0, 0.0]
    # with one (the reference raises TypeError there): scores - beta * penalty on the valid tokens, the penalties being the
    # reference's own
    mask = valid_mask(g)
    for kind in ("kl", "abs", "mse"):
        b2, m2 = rl.apply_kl_penalty(dict(base, ref_log_prob=ref), ctrl, kind, action_token_len=ADIM, action_chunks_len=CHUNK)
        kld = g[P + "kl/" + kind] * mask
        want = g[P + "token_level_scores"] - np.float32(g["kl_coef"]) * kld.astype(np.float32)
        assert np.abs(b2["token_level_rewards"].numpy() - want).max() <= 1e-6 * np.abs(want).max()
        assert m2["critic/kl_coeff"] == float(g["kl_coef"])
        assert abs(m2["critic/kl"] - float((kld.sum(1) / mask.sum(1)).mean())) <= 1e-6 * np.abs(kld).max()


@pytest.mark.parametrize("tag", TAGS)
def test_grpo_advantages_match_the_reference(golden_dir, tag):
    from dexbotic_amd.exp import rl
    g = load(golden_dir)
    P = tag + "/"
    mask = T(valid_mask(g))
    for uid in (g["uid"], T(g["uid"]), np.array(["a", "a"]), ["a", "a"]):
        adv, ret = rl.grpo_outcome_advantage(T(g[P + "token_level_rewards"]), mask, uid)
        assert ret is adv and np.abs(adv.numpy() - g[P + "advantages"]).max() <= 1e-6 * np.abs(g[P + "advantages"]).max()
    assert adv[0, 0] > 0 and adv[1, 0] < 0 and float(adv[1, 9:].abs().max()) == 0        # masked tokens: exactly 0
    # two members and a group of one (mean 0, std 1: the score itself over 1 + epsilon)
    a3, _ = rl.grpo_outcome_advantage(T(g[P + "adv3/token_level_rewards"]), T(g[P + "adv3/mask"]), T(g[P + "adv3/uid"]))
    assert np.abs(a3.numpy() - g[P + "adv3/advantages"]).max() <= 1e-6 * np.abs(g[P + "adv3/advantages"]).max()
    score = float(g[P + "adv3/token_level_rewards"][2].sum())
    assert abs(float(a3[2, 0]) - score / (1 + 1e-6)) <= 1e-6 * score
    # the unbiased deviation: two scores s0, s1 give +- (s0 - s1) / 2 / (|s0 - s1| / sqrt(2) + epsilon)
    assert abs(float(a3[0, 0]) - 0.5 ** 0.5) < 1e-5


def test_masked_mean():
    from dexbotic_amd.exp import rl
    v = torch.tensor([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]])
    m = torch.tensor([[True, True, False], [False, False, False]])
    assert rl.masked_mean(v, m).item() == 1.5
    assert rl.masked_mean(v, m, axis=-1).tolist() == [1.5, 0.0]             # an empty mask: 0, not NaN
    assert rl.masked_mean(v, torch.zeros_like(m)).item() == 0.0


def reference_loss(logp, old, adv, mask, lo, hi, inv):
    """_compute_policy_loss (rl_trainer.py:488-506) with the clamp bounds as given numbers; inv * masked sum"""
    ratio = torch.exp(logp - old)
    pg1 = -adv * ratio
    pg2 = -adv * torch.clamp(ratio, lo, hi)
    return (torch.max(pg1, pg2) * mask).sum() * inv, pg1, pg2


def test_closed_form_of_the_loss_gradient_matches_autograd_ties_included():
    """what dxa_ppo_clip_fwd writes as ``coef``: mask * inv * (pg1 >= pg2 ? -adv * ratio : 0).  torch.maximum hands half of the
    gradient to each side at a tie: inside the range and ON a bound (clamp passes the gradient there) both sides are -adv * ratio, so
    the halves add up to the whole; outside the range a tie needs adv = 0, where the gradient is 0 either way."""
    gen = torch.Generator().manual_seed(3)
    n = 64
    old = torch.randn(n, generator=gen, dtype=torch.float64)
    delta = torch.randn(n, generator=gen, dtype=torch.float64) * 0.4
    adv = torch.randn(n, generator=gen, dtype=torch.float64)
    adv[::7] = 0.0                                                         # ties outside (and inside) the range
    mask = (torch.rand(n, generator=gen) > 0.25).double()
    logp = (old + delta).requires_grad_(True)
    ratio = torch.exp(logp.detach() - old)
    above, below = int((ratio > 1.4).nonzero()[0]), int((ratio < 0.7).nonzero()[0])
    for lo, hi in ((0.8, 1.28), (0.8, float(ratio[above])), (float(ratio[below]), 1.28)):       # the last two: a ratio exactly on a bound
        loss, pg1, pg2 = reference_loss(logp, old, adv, mask, lo, hi, 0.125)
        (grad,) = torch.autograd.grad(loss, logp)
        coef = mask * 0.125 * torch.where(pg1 >= pg2, pg1, torch.zeros_like(pg1)).detach()
        assert torch.allclose(grad, coef, rtol=1e-14, atol=0)
        assert bool((pg1 == pg2).any()) and bool((pg2 > pg1).any()) and bool((pg1 > pg2).any())
    mask[above] = 1.0
    adv[above] = -1.0                                                      # on the upper bound, a term that counts
    loss, pg1, pg2 = reference_loss(logp, old, adv, mask, 0.8, float(ratio[above]), 1.0)
    (grad,) = torch.autograd.grad(loss, logp)
    assert pg1[above] == pg2[above] and grad[above] == pg1[above].detach() != 0


def fake_updater(use_proprio=False, mini=1):
    from dexbotic_amd.exp import rl
    model = types.SimpleNamespace(config=types.SimpleNamespace(action_dim=ADIM, chunk_size=CHUNK, use_proprio=use_proprio))
    trainer = types.SimpleNamespace(model=model, coalesce=True)
    return rl.GRPOPolicyUpdater(trainer, rl.GRPOUpdateConfig(traj_mini_batch_size=mini)), trainer


def test_update_chunks_follow_the_reference_schedule(golden_dir):
    g = load(golden_dir)
    up, trainer = fake_updater()
    assert trainer.coalesce is False                                       # chunks carry their own denominators: never merged
    batch = dict(responses=T(g["np/responses"]), finish_step=T(g["finish_step"]), input_ids=T(g["np/input_ids"]),
                 attention_mask=T(g["np/attention_mask"]), pixel_values=torch.zeros(2, TRAJ, 3, 4, 4),
                 old_log_probs=T(g["np/old_log_probs"]), advantages=T(g["np/advantages"]))
    ch = up._chunks(batch)
    assert [(b, i, e, int(cm.sum()), tot) for b, i, e, cm, tot in ch] == [(0, 0, 1, 6, 12), (0, 1, 2, 6, 12), (1, 0, 1, 6, 9), (1, 1, 2, 3, 9)]
    assert [int(cm.sum()) for *_, cm, _ in ch] == g["np/chunk_mask_sum"].tolist()
    kw = up.chunk_batch(batch, *ch[3])
    assert kw["loss_denominator"] == 9.0 * 2 and kw["input_ids"].shape == (1, 10) and kw["responses"].shape == (1, R)
    assert torch.equal(kw["old_log_probs"], batch["old_log_probs"][1:2, R:]) and torch.equal(kw["advantages"], batch["advantages"][1:2, R:])
    assert kw["response_mask"].tolist() == [[True] * 3 + [False] * 3] and "states" not in kw
    assert (kw["temperature"], kw["clip_ratio_low"], kw["clip_ratio_high"]) == (1.6, 0.2, 0.28)
    # a trajectory that never started and a chunk behind the end of one are left out; a whole trajectory per chunk
    batch["finish_step"] = torch.tensor([1, 0])
    assert [(b, i, e, int(cm.sum()), tot) for b, i, e, cm, tot in up._chunks(batch)] == [(0, 0, 1, 3, 3)]
    up2, _ = fake_updater(mini=2)
    batch["finish_step"] = T(g["finish_step"])
    assert [(b, i, e, int(cm.sum()), tot) for b, i, e, cm, tot in up2._chunks(batch)] == [(0, 0, 2, 12, 12), (1, 0, 2, 9, 9)]
    up3, _ = fake_updater(use_proprio=True)
    batch["proprio"] = T(g["proprio"])
    assert torch.equal(up3.chunk_batch(batch, *ch[1])["states"], batch["proprio"][0, 1:2])
