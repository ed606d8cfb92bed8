"""NaVILA on the GPU against golden vectors from the reference's NaVILAForCausalLM (tests/golden/navila_t1.npz, written by
scripts/gen_golden_navila.py): three frames per sample through SigLIP (hidden_states[-2]) and the mlp_downsample projector,
spliced per sample (three placeholders / one placeholder), soft-target loss in training mode, standard loss in eval mode,
KV-cached greedy decode."""
import os

import numpy as np
import pytest
import torch

from .helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_TOL = 1e-3


def T(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


_GOLDEN = {}


def load(golden_dir):
    if not _GOLDEN:
        g = np.load(os.path.join(golden_dir, "navila_t1.npz"), allow_pickle=False)
        _GOLDEN["g"] = g
        _GOLDEN["w"] = {k[2:]: g[k] for k in g.files if k.startswith("w/")}
    return _GOLDEN["g"], _GOLDEN["w"]


def config(g, dtype):
    from dexbotic_amd.model import NaVILAConfig
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config
    from dexbotic_amd.model.modules.mm_vision.siglip.siglip_encoder import SiglipVisionConfig
    V, H, I, NL, NH, NKV, vh, vi, vl, vhd, vimg, vp = (int(v) for v in g["cfg"])
    llm = Qwen2Config(vocab_size=V, hidden_size=H, intermediate_size=I, num_hidden_layers=NL, num_attention_heads=NH,
                      num_key_value_heads=NKV, rms_norm_eps=1e-6, rope_theta=1e6)
    vis = SiglipVisionConfig(hidden_size=vh, intermediate_size=vi, num_hidden_layers=vl, num_attention_heads=vhd,
                             image_size=vimg, patch_size=vp, layer_norm_eps=1e-6)
    return NaVILAConfig(llm_config=llm, mm_vision_tower=vis, time_token_ids=[int(i) for i in g["time_token_ids"]],
                        soft_ce_std=float(g["soft_ce_std"]), compute_dtype=dtype)


def build(g, w, dtype, train=True):
    from dexbotic_amd.model import NaVILAForCausalLM
    m = NaVILAForCausalLM(config(g, dtype), device=DEV, train=train)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return m


def batch(g):
    return dict(input_ids=T(g["input_ids"]), attention_mask=T(g["attention_mask"]), labels=T(g["labels"]), images=T(g["images"]))


def test_config_defaults_and_state_dict_keys(golden_dir):
    g, w = load(golden_dir)
    c = config(g, "float32")
    assert c.model_type == "dexbotic_navila" and c.mm_projector_type == "mlp_downsample" and c.chat_template == "llama_3"
    m = build(g, w, "float32", train=False)
    assert set(m.state_dict().keys()) == set(w)
    assert {k for k in w if k.startswith("model.mm_projector.")} == {
        f"model.mm_projector.{i}.{n}" for i in (1, 2, 4) for n in ("weight", "bias")}
    assert sorted(m.unused_parameter_names()) == sorted(str(n) for n in g["no_grad"])


def test_fp32_losses_logits_and_grads_match_reference(golden_dir):
    g, w = load(golden_dir)
    m = build(g, w, "float32")
    m.train()
    st = m.store
    st.set_expected(m.unused_parameter_names())
    st.begin_step()
    out = m(**batch(g))
    assert rel_err(out.logits.detach().cpu().numpy(), g["logits"]) < FP32_TOL
    assert abs(out.loss.item() - float(g["loss"])) < FP32_TOL * abs(float(g["loss"]))
    out.loss.backward()
    seen = 0
    for key in g.files:
        if key.startswith("grad/"):
            assert rel_err(st.g(key[5:]).cpu().numpy(), g[key]) < FP32_TOL, key
            seen += 1
        elif key.startswith("gradN/") and key[6:] in st.slots and st.grad_written.get(key[6:], False):
            gn = float(g[key])
            # (k_proj biases have a mathematically zero gradient — softmax shift invariance — hence the floor)
            assert abs(st.g(key[6:]).double().norm().item() - gn) < FP32_TOL * gn + 1e-6 * float(g["grad_norm"]), key
            seen += 1
    assert seen == 6 + sum(k.startswith("gradN/") for k in g.files)          # every pinned gradient was written and compared
    # eval mode: the standard causal-LM loss on the same batch
    m.eval()
    with torch.no_grad():
        ev = m(**batch(g))
    assert abs(ev.loss.item() - float(g["eval_loss"])) < FP32_TOL * abs(float(g["eval_loss"]))
    assert abs(float(g["eval_loss"]) - float(g["loss"])) > 10 * FP32_TOL * float(g["loss"])   # the two losses are told apart


def test_soft_loss_of_a_batch_without_targets_is_zero(golden_dir):
    g, w = load(golden_dir)
    m = build(g, w, "float32")
    m.train()
    m.store.begin_step()
    b = batch(g)
    b["labels"] = torch.full_like(b["labels"], -100)
    assert m(**b).loss.item() == 0.0


def test_bf16_loss_tracks_reference(golden_dir):
    g, w = load(golden_dir)
    m = build(g, w, "bfloat16")
    m.train()
    m.store.begin_step()
    out = m(**batch(g))
    assert abs(out.loss.item() - float(g["loss"])) < 2e-2 * abs(float(g["loss"]))
    out.loss.backward()
    gn = float(g["gradN/lm_head.weight"])
    assert abs(m.store.g("lm_head.weight").double().norm().item() - gn) < 6e-2 * gn


def test_fp32_greedy_decode_token_ids_exact(golden_dir):
    """three frames, three placeholders: the KV-cached decode picks what the reference's full-prefix loop picked"""
    g, w = load(golden_dir)
    m = build(g, w, "float32", train=False)
    m.eval()
    n_new = len(g["decode_new_ids"])
    seq = m.generate(T(g["decode_prompt"]), images=T(g["images"][:1]), max_new_tokens=n_new, do_sample=False)
    L0 = g["decode_prompt"].shape[1]
    assert np.array_equal(seq[0, :L0].cpu().numpy(), g["decode_prompt"][0])
    assert np.array_equal(seq[0, L0:].cpu().numpy(), g["decode_new_ids"])


def test_save_and_load_reproduce_the_loss(golden_dir, tmp_path):
    from dexbotic_amd.model import NaVILAForCausalLM
    g, w = load(golden_dir)
    m = build(g, w, "float32")
    m.train()
    m.store.begin_step()
    loss = m(**batch(g)).loss.item()
    m.save_pretrained(str(tmp_path))
    m2 = NaVILAForCausalLM.from_pretrained(str(tmp_path), device=DEV, train=True)
    assert m2.config.time_token_ids == m.config.time_token_ids and m2.model.mm_vision_tower.select_layer == -2
    m2.train()
    m2.store.begin_step()
    assert m2(**batch(g)).loss.item() == loss


def test_gradient_checkpointing_step_is_bit_identical(golden_dir):
    g, w = load(golden_dir)
    res = []
    for ckpt in (False, True):
        m = build(g, w, "float32")
        if ckpt:
            m.gradient_checkpointing_enable()
        m.train()
        m.store.begin_step()
        out = m(**batch(g))
        out.loss.backward()
        torch.cuda.synchronize()
        res.append((out.loss.item(), m.store.g("lm_head.weight").clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
