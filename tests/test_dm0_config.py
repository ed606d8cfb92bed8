"""DM0 without a GPU: the registry entry, the config's round trip and refusals, the state-dict keys and shapes of the native class
against the list the reference's class produced (tests/golden/dm0_t1.npz), and the weight recipe against the stored checksums."""
import json
import os

import numpy as np
import pytest
import torch

from . import muvla_weights as MW

_G = {}


def load(golden_dir):
    if not _G:
        _G["g"] = np.load(os.path.join(golden_dir, "dm0_t1.npz"), allow_pickle=False)
    return _G["g"]


def q3(hidden, inter, layers=3, heads=4, kv=2, head_dim=32, vocab=264, model_type="qwen3"):
    return dict(model_type=model_type, vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers,
                num_attention_heads=heads, num_key_value_heads=kv, head_dim=head_dim, rms_norm_eps=1e-6, rope_theta=1e6,
                max_position_embeddings=4096)


def config(g, dtype="float32", **over):
    from dexbotic_amd.model import DM0Config
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    V, H, I, NL, NH, NKV, HD, AH, AI, vh, vi, vl, vhd, vimg, vp, chunk, adim, _ = (int(v) for v in g["cfg"])
    vis = CLIPVisionConfig(hidden_size=vh, intermediate_size=vi, num_hidden_layers=vl, num_attention_heads=vhd, image_size=vimg,
                           patch_size=vp)
    kw = dict(llm_config=q3(H, I, NL, NH, NKV, HD, V), action_config=q3(AH, AI, NL, NH, NKV, HD, V), mm_vision_tower=vis,
              action_dim=adim, chunk_size=chunk, compute_dtype=dtype)
    kw.update(over)
    return DM0Config(**kw)


def test_registry_and_autoconfig_resolve_dexbotic_dm0(golden_dir, tmp_path):
    import dexbotic_amd
    from transformers import AutoConfig
    from dexbotic_amd.model import DM0Config, DM0ForCausalLM
    assert dexbotic_amd.model_registry()["dexbotic_dm0"] == (DM0Config, DM0ForCausalLM)
    c = config(load(golden_dir))
    c.save_pretrained(str(tmp_path))
    with open(os.path.join(str(tmp_path), "config.json")) as f:
        assert json.load(f)["model_type"] == "dexbotic_dm0"
    assert isinstance(AutoConfig.from_pretrained(str(tmp_path)), DM0Config)


def test_config_round_trip_with_nested_qwen3_configs(golden_dir, tmp_path):
    from dexbotic_amd.model import DM0Config
    from dexbotic_amd.model.llm.qwen3 import Qwen3Config
    c = DM0Config()
    assert c.model_type == "dexbotic_dm0" and c.action_dim == 32 and c.chunk_size == 50 and c.bf16 is True
    assert c.compute_dtype == "bfloat16" and isinstance(c.llm_config, Qwen3Config) and isinstance(c.action_config, Qwen3Config)
    assert DM0Config(bf16=False).compute_dtype == "float32"
    c = config(load(golden_dir))
    assert c.bf16 is False and c.hidden_size == 96 and c.vocab_size == 264
    c.save_pretrained(str(tmp_path))
    c2 = DM0Config.from_pretrained(str(tmp_path))
    assert c2.to_dict() == c.to_dict()
    assert isinstance(c2.action_config, Qwen3Config) and isinstance(c2.llm_config, Qwen3Config)
    assert (c2.action_config.hidden_size, c2.action_config.intermediate_size, c2.action_config.head_dim) == (64, 80, 32)
    assert (c2.llm_config.hidden_size, c2.chunk_size, c2.action_dim, c2.compute_dtype) == (96, 6, 8, "float32")
    # the reference's own switch alone (its config.json has no compute_dtype)
    d = c.to_dict()
    d.pop("compute_dtype")
    d["bf16"] = True
    assert DM0Config.from_dict(d).compute_dtype == "bfloat16"


@pytest.mark.parametrize("model_type", ["qwen2", "gemma"])
def test_an_action_config_that_is_not_qwen3_is_refused_by_name(golden_dir, model_type):
    with pytest.raises(ValueError, match="qwen3"):
        config(load(golden_dir), action_config=q3(64, 80, model_type=model_type))
    with pytest.raises(ValueError, match="qwen3"):
        config(load(golden_dir), llm_config=q3(96, 128, model_type=model_type))


@pytest.mark.parametrize("over", [dict(heads=8), dict(kv=1), dict(head_dim=64), dict(layers=2)])
def test_experts_of_different_attention_geometry_are_refused(golden_dir, over):
    with pytest.raises(ValueError, match="share one attention"):
        config(load(golden_dir), action_config=q3(64, 80, **over))


def test_state_dict_keys_and_shapes_equal_the_references(golden_dir, tmp_path):
    import dexbotic_amd
    from dexbotic_amd.model import DM0ForCausalLM
    g = load(golden_dir)
    m = DM0ForCausalLM(config(g), device="cpu", train=False)
    want = dict(zip((str(k) for k in g["w_keys"]), MW.unpack_shapes(g["w_shapes"])))
    have = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert have == want
    assert "model.action_expert.lm_head.weight" in have and "lm_head.weight" in have
    assert not any("action_expert.model.embed_tokens" in k for k in have)
    assert have["model.action_expert.model.layers.0.self_attn.q_norm.weight"] == (32,)
    assert sorted(m.unused_parameter_names()) == sorted(str(n) for n in g["no_grad"])
    zero = [str(n) for n in g["zero_grad"]]
    assert zero == ["model.llm.layers.2.self_attn.q_norm.weight", "model.llm.layers.2.self_attn.q_proj.weight"]
    assert not set(zero) & set(m.unused_parameter_names())
    # registration order follows forward order
    order = list(m.store.slots)
    first = lambda p: next(i for i, n in enumerate(order) if n.startswith(p))
    marks = [first(p) for p in ("model.mm_vision_tower.", "model.mm_projector.", "model.llm.", "model.action_expert.model.",
                                "model.action_expert.lm_head.", "model.action_in_proj.", "lm_head.")]
    assert marks == sorted(marks)
    # a directory whose config.json says dexbotic_dm0 resolves to the class
    m.save_pretrained(str(tmp_path))
    m2 = dexbotic_amd.from_pretrained(str(tmp_path), device="cpu")
    assert type(m2) is DM0ForCausalLM
    assert torch.equal(m2.state_dict()["model.action_time_mlp_in.weight"], m.state_dict()["model.action_time_mlp_in.weight"])


def test_weight_recipe_reproduces_the_stored_checksums(golden_dir):
    g = load(golden_dir)
    w, images = MW.from_fixture(g)
    keys = [str(k) for k in g["w_keys"]]
    np.testing.assert_allclose(MW.checksums(keys, w), g["w_checksums"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(MW.checksums(["images"], {"images": images}), g["image_checksum"], rtol=1e-12, atol=1e-9)
