"""MuVLA without a GPU: config defaults and round trip, the state-dict keys and shapes of the native class against the list the
reference's class produced (tests/golden/muvla_t1.npz), the weight recipe against the stored checksums, and the width check."""
import os

import numpy as np
import pytest
import torch

from . import muvla_weights as MW

_G = {}


def load(golden_dir):
    if not _G:
        _G["g"] = np.load(os.path.join(golden_dir, "muvla_t1.npz"), allow_pickle=False)
    return _G["g"]


def config(g, dtype="float32", v_hidden=None):
    from dexbotic_amd.model import MUVLAConfig
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    V, H, I, NL, NH, NKV, vh, vi, vl, vhd, vimg, vp = (int(v) for v in g["cfg"])
    vh = v_hidden or vh
    llm = Qwen2Config(vocab_size=V, hidden_size=H, intermediate_size=I, num_hidden_layers=NL, num_attention_heads=NH,
                      num_key_value_heads=NKV, rms_norm_eps=1e-6, rope_theta=1e6)
    vis = lambda: CLIPVisionConfig(hidden_size=vh, intermediate_size=vi, num_hidden_layers=vl, num_attention_heads=vhd,
                                   image_size=vimg, patch_size=vp)
    return MUVLAConfig(llm_config=llm, mm_vision_tower=vis(), obs_vision_tower=vis(), compute_dtype=dtype)


def test_config_defaults_and_round_trip(golden_dir, tmp_path):
    from dexbotic_amd.model import MUVLAConfig
    c = MUVLAConfig()
    assert c.model_type == "dexbotic" and c.mm_projector_type == "mlp2x_gelu" and c.chat_template == "dexbotic"
    assert c.mm_vision_tower is None and c.obs_vision_tower is None and c.init_llm_weights is False
    assert c.action_model_type is None and c.action_dim is None and c.chunk_size is None
    c = config(load(golden_dir))
    c.save_pretrained(str(tmp_path))
    c2 = MUVLAConfig.from_pretrained(str(tmp_path))
    assert c2.to_dict() == c.to_dict()
    assert c2.obs_vision_tower["hidden_size"] == 1024 and c2.mm_vision_tower["patch_size"] == 2 and c2.vocab_size == 264


def test_state_dict_keys_and_shapes_equal_the_references(golden_dir):
    from dexbotic_amd.model import MUVLAForCausalLM
    import dexbotic_amd
    assert dexbotic_amd.muvla() is MUVLAForCausalLM
    g = load(golden_dir)
    m = MUVLAForCausalLM(config(g), device="cpu", train=False)
    want = dict(zip((str(k) for k in g["w_keys"]), MW.unpack_shapes(g["w_shapes"])))
    have = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert have == want
    for k in ("model.obs_vision_tower.vision_tower.embeddings.class_embedding", "model.fuser.reduce_proj.weight",
              "model.fuser.cross_attn.in_proj_weight", "model.fuser.cross_attn.out_proj.bias", "model.fuser.ln.bias",
              "model.fuser.back_proj.bias", "model.history_qformer.query_embeddings", "model.history_qformer.input_proj.weight",
              "model.history_qformer.attn.in_proj_bias", "model.history_qformer.norm.weight", "model.mm_projector.2.weight",
              "lm_head.weight", "reward_head.weight"):
        assert k in have, k
    assert have["model.history_qformer.query_embeddings"] == (192, 1024) and have["reward_head.weight"] == (1, 96)
    assert sorted(m.unused_parameter_names()) == sorted(str(n) for n in g["no_grad"])
    # registration order follows forward order: obs tower, Q-former, map tower, fuser, projector, decoder, heads
    order = list(m.store.slots)
    first = lambda p: next(i for i, n in enumerate(order) if n.startswith(p))
    marks = [first(p) for p in ("model.obs_vision_tower.", "model.history_qformer.", "model.mm_vision_tower.", "model.fuser.",
                                "model.mm_projector.", "model.llm.", "lm_head.", "reward_head.")]
    assert marks == sorted(marks)


def test_weight_recipe_reproduces_the_stored_checksums(golden_dir):
    g = load(golden_dir)
    w, images = MW.from_fixture(g)
    keys = [str(k) for k in g["w_keys"]]
    assert sum(v.size for v in w.values()) == 36878144
    np.testing.assert_allclose(MW.checksums(keys, w), g["w_checksums"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(MW.checksums(["images"], {"images": images}), g["image_checksum"], rtol=1e-12, atol=1e-9)
    some = torch.from_numpy(w["model.fuser.cross_attn.in_proj_weight"])
    assert torch.equal(some.bfloat16().float(), some)                    # on the bf16 grid


def test_a_768_wide_tower_is_refused(golden_dir):
    from dexbotic_amd.model import MUVLAForCausalLM
    with pytest.raises(ValueError, match="1024"):
        MUVLAForCausalLM(config(load(golden_dir), v_hidden=768), device="cpu", train=False)
