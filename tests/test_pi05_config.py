"""pi0.5 without a GPU: the registry entry, the config's round trip and refusals, the state-dict keys and shapes of the native class
against the ORDERED list the reference's class produced (tests/golden/pi05_t1.npz), the weight recipe against the stored checksums,
and the argument checks of the adaptive-norm entry points (they return before any launch)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from . import muvla_weights as MW

_G = {}


def load(golden_dir):
    if not _G:
        _G["g"] = np.load(os.path.join(golden_dir, "pi05_t1.npz"), allow_pickle=False)
    return _G["g"]


def gemma(hidden, inter, layers=3, heads=4, kv=1, head_dim=32, vocab=264, model_type="adarms_gemma", **over):
    d = dict(model_type=model_type, vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers,
             num_attention_heads=heads, num_key_value_heads=kv, head_dim=head_dim, rms_norm_eps=1e-6, rope_theta=10000.0,
             max_position_embeddings=512)
    d.update(over)
    return d


def config(g, dtype="float32", **over):
    from dexbotic_amd.model import Pi05Config
    V, H, I, NL, NH, NKV, HD, AH, AI, vh, vi, vl, vhd, vimg, vp, chunk, adim, _ = (int(v) for v in g["cfg"])
    vis = dict(model_type="siglip_vision_model", hidden_size=vh, intermediate_size=vi, num_hidden_layers=vl, num_attention_heads=vhd,
               image_size=vimg, patch_size=vp, layer_norm_eps=1e-6)
    kw = dict(vision_config=vis, llm_config=gemma(H, I, NL, NH, NKV, HD, V, use_adarms=False),
              action_config=gemma(AH, AI, NL, NH, NKV, HD, V, use_adarms=True, adarms_cond_dim=AH, width=AH),
              mm_projector_type="linear", action_dim=adim, chunk_size=chunk, compute_dtype=dtype)
    kw.update(over)
    return Pi05Config(**kw)


def test_registry_and_autoconfig_resolve_dexbotic_pi05(golden_dir, tmp_path):
    import dexbotic_amd
    from transformers import AutoConfig
    from dexbotic_amd.model import Pi05Config, Pi05ForCausalLM, Pi05Model  # noqa: F401
    assert dexbotic_amd.model_registry()["dexbotic_pi05"] == (Pi05Config, Pi05ForCausalLM)
    assert dexbotic_amd.Pi05ForCausalLM is Pi05ForCausalLM and dexbotic_amd.Pi05Config is Pi05Config
    c = config(load(golden_dir))
    c.save_pretrained(str(tmp_path))
    with open(os.path.join(str(tmp_path), "config.json")) as f:
        assert json.load(f)["model_type"] == "dexbotic_pi05"
    assert isinstance(AutoConfig.from_pretrained(str(tmp_path)), Pi05Config)


def test_config_round_trip_with_nested_adarms_configs(golden_dir, tmp_path):
    from dexbotic_amd.model import Pi05Config
    from dexbotic_amd.model.llm.adarms_gemma import AdaRMSGemmaConfig
    c = Pi05Config()
    assert c.model_type == "dexbotic_pi05" and c.action_dim == 32 and c.chunk_size == 50
    assert c.action_config.use_adarms and c.action_config.adarms_cond_dim == c.action_config.hidden_size == c.action_config.width
    c = config(load(golden_dir))
    assert c.hidden_size == 96 and c.vocab_size == 264
    c.save_pretrained(str(tmp_path))
    c2 = Pi05Config.from_pretrained(str(tmp_path))
    assert c2.to_dict() == c.to_dict()
    assert isinstance(c2.action_config, AdaRMSGemmaConfig) and isinstance(c2.llm_config, AdaRMSGemmaConfig)
    a = c2.action_config
    assert (a.model_type, a.use_adarms, a.adarms_cond_dim, a.width, a.hidden_size, a.intermediate_size) == \
        ("adarms_gemma", True, 64, 64, 64, 80)
    assert (c2.llm_config.use_adarms, c2.llm_config.hidden_size, c2.chunk_size, c2.action_dim, c2.compute_dtype) == \
        (False, 96, 6, 8, "float32")
    # adarms_cond_dim and width default to hidden_size; a plain gemma llm is accepted
    c3 = config(load(golden_dir), action_config=gemma(64, 80, use_adarms=True), llm_config=gemma(96, 128, model_type="gemma"))
    assert c3.action_config.adarms_cond_dim == 64 and c3.action_config.width == 64 and c3.llm_config.model_type == "gemma"


def test_configs_the_mixture_cannot_run_are_refused_by_name(golden_dir):
    g = load(golden_dir)
    for mt in ("gemma", "qwen3"):
        with pytest.raises(ValueError, match="adarms_gemma"):
            config(g, action_config=gemma(64, 80, model_type=mt, use_adarms=True))
    with pytest.raises(ValueError, match="use_adarms=True"):
        config(g, action_config=gemma(64, 80, use_adarms=False))
    with pytest.raises(ValueError, match="adarms_gemma"):
        config(g, llm_config=gemma(96, 128, model_type="qwen2"))
    with pytest.raises(ValueError, match="llm_config.use_adarms"):
        config(g, llm_config=gemma(96, 128, use_adarms=True))
    with pytest.raises(ValueError, match="width"):
        config(g, action_config=gemma(64, 80, use_adarms=True, width=32))
    with pytest.raises(ValueError, match="adarms_cond_dim"):
        config(g, action_config=gemma(64, 80, use_adarms=True, adarms_cond_dim=48))


@pytest.mark.parametrize("over", [dict(heads=8), dict(kv=2), dict(head_dim=64), dict(layers=2)])
def test_experts_of_different_attention_geometry_are_refused(golden_dir, over):
    with pytest.raises(ValueError, match="share one attention"):
        config(load(golden_dir), action_config=gemma(64, 80, use_adarms=True, **over))


def test_state_dict_keys_and_shapes_equal_the_references_in_order(golden_dir, tmp_path):
    import dexbotic_amd
    from dexbotic_amd.model import Pi05ForCausalLM
    g = load(golden_dir)
    m = Pi05ForCausalLM(config(g), device="cpu", train=False)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["w_keys"]]
    assert [tuple(v.shape) for v in sd.values()] == MW.unpack_shapes(g["w_shapes"])
    assert sd["model.action_expert.layers.0.input_layernorm.dense.weight"].shape == (192, 64)
    assert sd["model.action_expert.norm.dense.bias"].shape == (192,) and sd["model.time_mlp_in.weight"].shape == (64, 64)
    assert not any("state_proj" in k or "action_time_mlp" in k or "action_expert.norm.weight" in k for k in sd)
    assert sorted(m.unused_parameter_names()) == sorted(str(n) for n in g["no_grad"])
    # the dense layers of the 2 L + 1 adaptive norms lie back to back in the arena, in evaluation order: one product serves them all
    exp = m.model.action_expert
    assert exp.n_norms == 7 and exp.dense_w[0].endswith("layers.0.input_layernorm.dense.weight") and \
        exp.dense_w[-1] == "model.action_expert.norm.dense.weight"
    assert m.store.w(*exp.dense_w, shape=(7 * 192, 64)).shape == (7 * 192, 64) and m.store.w(*exp.dense_b).shape == (7 * 192,)
    # a directory whose config.json says dexbotic_pi05 resolves to the class
    m.save_pretrained(str(tmp_path))
    m2 = dexbotic_amd.from_pretrained(str(tmp_path), device="cpu")
    assert type(m2) is Pi05ForCausalLM
    assert torch.equal(m2.state_dict()["model.time_mlp_in.weight"], sd["model.time_mlp_in.weight"])


def test_weight_recipe_reproduces_the_stored_checksums(golden_dir):
    g = load(golden_dir)
    w, images = MW.from_fixture(g)
    keys = [str(k) for k in g["w_keys"]]
    np.testing.assert_allclose(MW.checksums(keys, w), g["w_checksums"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(MW.checksums(["images"], {"images": images}), g["image_checksum"], rtol=1e-12, atol=1e-9)
    assert len([k for k in g.files if k.startswith("grad/")]) == 8 and "bf16/v_t" in g.files and "bf16/loss" in g.files


def test_adarms_entry_points_refuse_bad_arguments_with_a_message():
    """a null pointer, rows that are no whole number of samples, cols <= 0: -1 and a message, before any launch (so no GPU is needed;
    the pointers handed in are never read)"""
    from dexbotic_amd import _lib as L
    lib = L.lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    f32 = L.F32

    def msg():
        return lib.dxa_last_error().decode()
    fwd = lambda x, mod, y, rows, rps, cols, branch=None, gate=None, r=None: lib.dxa_adarms_fwd(
        x, branch, gate, 3 * max(cols, 1), mod, r, y, None, rows, rps, cols, 1e-6, f32, None)
    assert fwd(None, p, p, 4, 2, 4) == -1 and "dxa_adarms_fwd" in msg()
    assert fwd(p, None, p, 4, 2, 4) == -1 and "null" in msg()
    assert fwd(p, p, p, 5, 2, 4) == -1 and "whole number of samples" in msg()
    assert fwd(p, p, p, 4, 2, 0) == -1 and "cols 0" in msg()
    assert fwd(p, p, p, 4, 2, 4, branch=p) == -1 and "branch" in msg()          # a branch without gate_prev / r_out
    gr = lambda x, b, g_, y, rows, rps, cols: lib.dxa_gated_residual_fwd(x, b, g_, cols, y, rows, rps, cols, f32, None)
    assert gr(p, None, p, p, 4, 2, 4) == -1 and "dxa_gated_residual_fwd" in msg()
    assert gr(p, p, p, p, 3, 2, 4) == -1 and "whole number of samples" in msg()
    assert gr(p, p, p, p, 4, 2, -1) == -1
    bwd = lambda dy, rows, rps, cols, nbytes: lib.dxa_adarms_bwd(dy, p, p, p, None, p, p, None, None, 0, None, None, 0, p, nbytes,
                                                                 rows, rps, cols, f32, None)
    assert bwd(None, 4, 2, 4, 1 << 20) == -1 and "dxa_adarms_bwd" in msg()
    assert bwd(p, 7, 2, 4, 1 << 20) == -1 and "whole number of samples" in msg()
    assert bwd(p, 4, 2, 0, 1 << 20) == -1
    assert bwd(p, 4, 2, 4, 8) == -1 and "partial too small" in msg()
    gb = lambda dy, rows, rps, cols: lib.dxa_gated_residual_bwd(dy, p, p, cols, p, p, cols, p, 1 << 20, rows, rps, cols, f32, None)
    assert gb(None, 4, 2, 4) == -1 and "dxa_gated_residual_bwd" in msg()
    assert gb(p, 5, 2, 4) == -1 and gb(p, 4, 2, 0) == -1
    assert lib.dxa_adarms_bwd_groups(50) == 13 and lib.dxa_adarms_bwd_groups(1) == 1 and lib.dxa_adarms_bwd_groups(10 ** 6) == 128
