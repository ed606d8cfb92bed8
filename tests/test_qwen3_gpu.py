"""Qwen3Backbone (model/llm/qwen3.py) on the GPU against tests/golden/qwen3_t1.npz, the installed transformers.Qwen3Model's numbers
(scripts/gen_golden_qwen3.py): hidden states, layer 0's q / k behind q_norm / k_norm + RoPE, every gradient, the KV-cached path, and
the decoder inside DexboticForCausalLM (training step, greedy generate, HF's key names)."""
import os

import numpy as np
import pytest
import torch

from .helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_TOL = 1e-3      # the standing fp32 bound against reference fixtures
P = "model.llm."


def T(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "qwen3_t1.npz"), allow_pickle=False)


def _llm_config(g):
    from dexbotic_amd.model.llm.qwen3 import Qwen3Config
    V, H, I, NL, NH, NKV, D = (int(v) for v in g["cfg"])
    return Qwen3Config(vocab_size=V, hidden_size=H, intermediate_size=I, num_hidden_layers=NL, num_attention_heads=NH,
                       num_key_value_heads=NKV, head_dim=D, rope_theta=float(g["rope_theta"]), rms_norm_eps=float(g["rms_norm_eps"]))


def _backbone(g, dtype=torch.float32, train=True):
    from dexbotic_amd.engine import ParamStore, attach_parameters
    from dexbotic_amd.model.llm.qwen3 import Qwen3Backbone
    st = ParamStore(DEV, dtype)
    llm = Qwen3Backbone(st, P, _llm_config(g))
    st.finalize(train=train)
    attach_parameters(llm, st)
    assert sorted(st.slots) == sorted(P + str(n) for n in g["names"])
    for n in g["names"]:
        st.w32(P + str(n)).copy_(T(g["w/" + str(n)]))
    st.sync_shadow()
    return st, llm


@pytest.mark.parametrize("recompute", [False, True])
def test_fp32_forward_and_gradients_match_the_hf_fixture(gold, recompute, monkeypatch):
    from dexbotic_amd import kernels as K
    g = gold
    st, llm = _backbone(g)
    st.recompute = recompute
    st.begin_step()
    seen = []
    split = K.qknorm_rope_split
    monkeypatch.setattr(K, "qknorm_rope_split", lambda *a, **kw: (seen.append(split(*a, **kw)), seen[-1])[1])
    x = T(g["inputs_embeds"]).requires_grad_(True)
    y = llm(x)
    q0, k0 = seen[0][0], seen[0][1]
    assert rel_err(y.detach().cpu().numpy(), g["last_hidden_state"]) < FP32_TOL
    assert rel_err(q0.cpu().numpy(), g["q0"]) < FP32_TOL and rel_err(k0.cpu().numpy(), g["k0"]) < FP32_TOL
    (y * T(g["loss_weight"])).sum().backward()
    assert len(seen) == int(g["cfg"][3]) * (2 if recompute else 1)          # recompute re-runs every layer's forward launches
    assert rel_err(x.grad.cpu().numpy(), g["grad_inputs_embeds"]) < FP32_TOL
    for n in g["names"]:
        assert rel_err(st.g(P + str(n)).cpu().numpy(), g["grad/" + str(n)]) < FP32_TOL, n
    assert float(np.abs(g["grad/layers.0.self_attn.k_norm.weight"]).max()) > 0


def test_cached_prefill_and_single_token_steps_match_the_hf_fixture(gold):
    g = gold
    st, llm = _backbone(g, train=False)
    x = T(g["inputs_embeds"])
    B, S, _ = x.shape
    n0 = g["cached_prefill"].shape[1]
    cache = llm.new_cache(B, S, DEV, torch.float32)
    with torch.no_grad():
        h = llm.forward_cached(x[:, :n0].contiguous(), cache)
        assert rel_err(h.cpu().numpy(), g["cached_prefill"]) < FP32_TOL
        for s in range(n0, S):
            h = llm.forward_cached(x[:, s:s + 1].contiguous(), cache)
            assert rel_err(h.cpu().numpy(), g["cached_steps"][:, s - n0:s - n0 + 1]) < FP32_TOL, s
    assert cache.length == S and cache.fused_steps == 0


def test_bf16_single_token_steps_stay_on_the_per_op_path(gold):
    """B = 1, bf16, one new token: where Qwen2Backbone takes the persistent decode launch; Qwen3Backbone must not (known gap)"""
    g = gold
    st, llm = _backbone(g, dtype=torch.bfloat16, train=False)
    x = T(g["inputs_embeds"])[:1].to(torch.bfloat16)
    cache = llm.new_cache(1, x.shape[1], DEV, torch.bfloat16)
    with torch.no_grad():
        llm.forward_cached(x[:, :6].contiguous(), cache)
        h = llm.forward_cached(x[:, 6:7].contiguous(), cache)
    assert cache.fused_steps == 0 and llm._decode_state(cache) is None
    # bf16 against the fp32 fixture: 2^-8 per rounding, about a dozen roundings along the residual path of two layers
    assert rel_err(h.float().cpu().numpy(), g["cached_steps"][:1, :1]) < 5e-2


@pytest.fixture(scope="module")
def lm(gold):
    """DexboticForCausalLM over the fixture's decoder and the suite's toy CLIP tower; the decoder holds the fixture's weights"""
    from dexbotic_amd.model.dexbotic_arch import DexboticConfig, DexboticForCausalLM
    from dexbotic_amd.model.llm.qwen3 import Qwen3Backbone
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    vis = CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, image_size=56,
                           patch_size=14, layer_norm_eps=1e-5)
    cfg = DexboticConfig(llm_config=_llm_config(gold).to_dict(), mm_vision_tower=vis, mm_projector_type="mlp2x_gelu",
                         compute_dtype="float32")
    m = DexboticForCausalLM(cfg, device=DEV, train=True)
    assert isinstance(m.model.llm, Qwen3Backbone)
    m.init_random_(seed=3, std=0.05)
    return m


def test_state_dict_keys_and_round_trip_are_hfs(gold, lm):
    g = gold
    keys = {k[len(P):] for k in lm.state_dict() if k.startswith(P)}
    assert keys == {str(n) for n in g["names"]}
    sd = {k: v.detach().clone() for k, v in lm.state_dict().items()}
    sd.update({P + str(n): torch.from_numpy(g["w/" + str(n)]) for n in g["names"]})
    lm.load_state_dict(sd, strict=True)
    after = lm.state_dict()
    for n in g["names"]:
        assert np.array_equal(after[P + str(n)].cpu().numpy(), g["w/" + str(n)]), n


def test_causal_lm_training_step_and_greedy_generate(gold, lm):
    m = lm
    rs = np.random.RandomState(5)
    B, Lp = 2, 10
    ids = rs.randint(3, 60, size=(B, Lp)).astype(np.int64)
    ids[:, 1] = -200
    mask = np.ones((B, Lp), dtype=bool)
    mask[1, Lp - 2:] = False
    labels = ids.copy()
    labels[:, :4] = -100
    labels[~mask] = -100
    images = np.clip(rs.standard_normal((B, 3, 56, 56)), -2.5, 2.5).astype(np.float32)
    m.train()
    m.store.begin_step()
    out = m(input_ids=T(ids), attention_mask=T(mask), labels=T(labels), images=T(images))
    out.loss.backward()
    assert np.isfinite(out.loss.item())
    gq = m.store.g(P + "layers.1.self_attn.q_norm.weight")
    assert bool(torch.isfinite(m.store.grad).all()) and gq.abs().max().item() > 0
    # greedy: KV-cached generate against an uncached re-forward of the growing sequence
    m.eval()
    n_new = 4
    seq = m.generate(T(ids[:1]), images=T(images[:1]), max_new_tokens=n_new, do_sample=False)
    assert seq.shape == (1, Lp + n_new)
    cur = T(ids[:1])
    with torch.no_grad():
        for t in range(n_new):
            nxt = int(torch.argmax(m(input_ids=cur, images=T(images[:1])).logits[0, -1].float()))
            assert int(seq[0, Lp + t]) == nxt, (t, seq[0, Lp:].tolist())
            cur = torch.cat([cur, torch.tensor([[nxt]], device=DEV, dtype=cur.dtype)], dim=1)
