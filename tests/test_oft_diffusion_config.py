"""The OFT diffusion head without a GPU: the registry entry stays OFT's, ``OFTDiffusionConfig`` round-trips, the builder builds the head
only for that config, the state-dict keys / shapes and the parameters without a gradient against the lists the reference's class
produced (tests/golden/oft_dit_t1.npz, scripts/gen_golden_oft_dit.py), ``from_pretrained`` dispatch, the refusals, and
``DDIMSchedule`` against the fixture's tables (both written from the same formulas: consistency) and against the closed form of the
cosine schedule (independent)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from . import muvla_weights as MW

_G = {}
TAGS = ("np", "pp")                         # use_proprio False / True


def load(golden_dir):
    if not _G:
        _G["g"] = np.load(os.path.join(golden_dir, "oft_dit_t1.npz"), allow_pickle=False)
    return _G["g"]


def config(g, tag="np", dtype="float32", cls=None, **over):
    from dexbotic_amd.model import OFTDiffusionConfig
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    V, H, I, NL, NH, NKV, vh, vi, vl, vhd, vimg, vp, adim, chunk, pdim = (int(v) for v in g["cfg"])
    llm = Qwen2Config(vocab_size=V, hidden_size=H, intermediate_size=I, num_hidden_layers=NL, num_attention_heads=NH,
                      num_key_value_heads=NKV, rms_norm_eps=1e-6, rope_theta=1e6)
    vis = CLIPVisionConfig(hidden_size=vh, intermediate_size=vi, num_hidden_layers=vl, num_attention_heads=vhd, image_size=vimg,
                           patch_size=vp, layer_norm_eps=1e-5)
    kw = dict(llm_config=llm, mm_vision_tower=vis, mm_projector_type="mlp2x_gelu", action_model_type="DiT", action_dim=adim,
              chunk_size=chunk, use_proprio=(tag == "pp"), proprio_dim=pdim, compute_dtype=dtype)
    kw.update(over)
    return (cls or OFTDiffusionConfig)(**kw)


def weights(g, tag):
    keys = [str(k) for k in g[tag + "/w_keys"]]
    return keys, MW.make_weights(keys, MW.unpack_shapes(g[tag + "/w_shapes"]), int(g["seed"]))


def test_registry_is_unchanged_and_the_config_round_trips(golden_dir, tmp_path):
    import dexbotic_amd
    from transformers import AutoConfig
    from dexbotic_amd.model import OFTConfig, OFTDiffusionConfig, OFTDiffusionForCausalLM, OFTDiffusionModel, OFTForCausalLM  # noqa: F401
    assert dexbotic_amd.model_registry()["dexbotic_oft"] == (OFTConfig, OFTForCausalLM)
    assert dexbotic_amd.OFTDiffusionForCausalLM is OFTDiffusionForCausalLM and dexbotic_amd.OFTDiffusionConfig is OFTDiffusionConfig
    c = OFTDiffusionConfig()
    assert c.model_type == "dexbotic_oft" and c.num_diffusion_steps == 100 and issubclass(OFTDiffusionConfig, OFTConfig)
    c = config(load(golden_dir), "pp", num_diffusion_steps=50)
    c.save_pretrained(str(tmp_path))
    with open(os.path.join(str(tmp_path), "config.json")) as f:
        d = json.load(f)
    assert d["model_type"] == "dexbotic_oft" and d["action_model_type"] == "DiT" and d["num_diffusion_steps"] == 50
    c2 = OFTDiffusionConfig.from_pretrained(str(tmp_path))
    assert (c2.action_model_type, c2.action_dim, c2.chunk_size, c2.use_proprio, c2.proprio_dim, c2.num_diffusion_steps) == \
        ("DiT", 3, 2, True, 5, 50)
    # the string still belongs to OFTConfig in the AutoConfig registry
    assert type(AutoConfig.from_pretrained(str(tmp_path))) is OFTConfig


def test_builder_builds_the_head_only_for_the_diffusion_config(golden_dir):
    from dexbotic_amd.engine import ParamStore, building
    from dexbotic_amd.model import OFTConfig, OFTDiscreteConfig
    from dexbotic_amd.model.oft.action_model.builder import build_action_model
    from dexbotic_amd.model.oft.action_model.model import DiffusionActionHead, L1RegressionActionHead
    g = load(golden_dir)
    with building(ParamStore("cpu")):
        for cls in (OFTConfig, OFTDiscreteConfig):
            with pytest.raises(NotImplementedError, match="DiT.*OFTDiffusionConfig"):
                build_action_model(config(g, cls=cls))
        head = build_action_model(config(g, "pp"))
        assert isinstance(head, DiffusionActionHead) and head.num_query_rows == 7 and head.proprio_projector is not None
        assert head.num_diffusion_steps == 100
        assert isinstance(build_action_model(config(g, action_model_type="Linear")), L1RegressionActionHead)
        with pytest.raises(ValueError, match="multiple of 8"):
            DiffusionActionHead(ParamStore("cpu"), "h.", 100, 100, 3, 2)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_keys_shapes_and_unused_parameters_equal_the_references(golden_dir, tmp_path, tag):
    import dexbotic_amd
    from dexbotic_amd.model import OFTDiffusionForCausalLM
    g = load(golden_dir)
    m = OFTDiffusionForCausalLM(config(g, tag), device="cpu", train=False)
    sd = m.state_dict()
    keys, w = weights(g, tag)
    ref_shapes = dict(zip(keys, MW.unpack_shapes(g[tag + "/w_shapes"])))
    assert sorted(sd.keys()) == sorted(keys)
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref_shapes
    # inside the action head also the reference's order: trunk, projector, proprio projector last; no action_query
    H = "model.action_head."
    assert [k for k in sd if k.startswith(H)] == [k for k in keys if k.startswith(H)]
    assert not any("action_query" in k for k in sd)
    assert sd[H + "noisy_action_projector.fc1.weight"].shape == (96, 1) and sd[H + "noisy_action_projector.fc2.weight"].shape == (96, 96)
    assert sd[H + "noise_predictor.mlp_resnet.fc1.weight"].shape == (96, 288)
    assert ((H + "proprio_projector.fc1.weight") in sd) == (tag == "pp")
    np.testing.assert_allclose(MW.checksums(keys, w), g[tag + "/w_checksums"], rtol=1e-12, atol=1e-9)
    # the parameters the reference leaves without a gradient are the Linear head's list: lm_head, the last CLIP layer, post_layernorm
    no_grad = sorted(str(n) for n in g[tag + "/no_grad"])
    assert sorted(m.unused_parameter_names()) == no_grad and "lm_head.weight" in no_grad
    assert set(no_grad) == set(keys) - {k[len(tag) + 7:] for k in g.files if k.startswith(tag + "/gradN/")}
    assert isinstance(m.model.action_head.noise_predictor.mlp_resnet.layer_norm1, torch.nn.LayerNorm)
    # a directory whose config.json says dexbotic_oft + DiT resolves to the class; one with Linear still to OFTForCausalLM
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m.save_pretrained(str(tmp_path))
    m2 = dexbotic_amd.from_pretrained(str(tmp_path), device="cpu")
    assert type(m2) is OFTDiffusionForCausalLM and m2.config.use_proprio == (tag == "pp") and m2.config.num_diffusion_steps == 100
    k = H + "noisy_action_projector.fc1.weight"
    assert torch.equal(m2.state_dict()[k], torch.from_numpy(w[k]))


def test_linear_directory_still_resolves_to_oft(golden_dir, tmp_path):
    import dexbotic_amd
    from dexbotic_amd.model import OFTConfig, OFTForCausalLM
    m = OFTForCausalLM(config(load(golden_dir), cls=OFTConfig, action_model_type="Linear"), device="cpu", train=False)
    m.save_pretrained(str(tmp_path))
    assert type(dexbotic_amd.from_pretrained(str(tmp_path), device="cpu")) is OFTForCausalLM


def test_refusals(golden_dir):
    """neither actions nor noisy_dict; a batch in inference_action; left padding: all before any device work"""
    from dexbotic_amd.model import OFTDiffusionForCausalLM
    g = load(golden_dir)
    m = OFTDiffusionForCausalLM(config(g), device="cpu", train=False)
    ids, images = torch.from_numpy(g["input_ids"]), torch.zeros(tuple(g["image_shape"]))
    with pytest.raises(ValueError, match="actions.*noisy_dict"):
        m(input_ids=ids, images=images)
    with pytest.raises(ValueError, match="one sample.*reference"):
        m.inference_action(ids, images, {})
    with pytest.raises(ValueError, match="left"):
        OFTDiffusionForCausalLM(config(g, tokenizer_padding_side="left"), device="cpu", train=False)


def test_ddim_schedule_is_consistent_with_the_fixture(golden_dir):
    """both were written from the same formulas: a check of consistency, not of the formulas"""
    from dexbotic_amd.model.oft.action_model.ddim import DDIMSchedule
    g = load(golden_dir)
    s = DDIMSchedule(100)
    assert np.array_equal(s.alphas_cumprod.numpy(), g["alphas_cumprod"]) and s.alphas_cumprod.dtype == torch.float32
    assert s.set_timesteps(10) == g["ddim_timesteps"].tolist() == [90, 80, 70, 60, 50, 40, 30, 20, 10, 0]
    assert s.set_timesteps(100) == list(range(99, -1, -1)) and s.set_timesteps(3) == [66, 33, 0]
    with pytest.raises(ValueError):
        s.set_timesteps(101)
    # add_noise reproduces the fixture's noisy actions at both ends of the schedule
    t = torch.from_numpy
    noisy = s.add_noise(t(g["actions"]), t(g["np/noise"]), t(g["train_timesteps"]))
    np.testing.assert_allclose(noisy.numpy(), g["np/noisy_actions"], rtol=1e-6, atol=1e-7)
    # one step on the recorded eps reproduces the recorded x, every step of the trajectory
    s.set_timesteps(10)
    x = t(g["sampler_start"][0])
    for k in range(10):
        x = s.step(t(g["np/sampler/eps"][k]), k, x)
        np.testing.assert_allclose(x.numpy(), g["np/sampler/x"][k], rtol=0, atol=2e-6)
    c0, c1, c2, c3 = s.step_coefficients(9)
    assert (c2, c3) == (1.0, 0.0)                        # the last step lands on final_alpha_cumprod = 1


def test_ddim_schedule_against_the_closed_form():
    """independent of the fixture: the cumulative product telescopes to ab((t + 1) / N) / ab(0) while the 0.999 cap is inactive
    (t <= 98), within the fp32 rounding of a 99-term product (1e-5 relative); the capped last beta multiplies by 0.001"""
    from dexbotic_amd.model.oft.action_model.ddim import DDIMSchedule
    N = 100
    a = DDIMSchedule(N).alphas_cumprod.double().numpy()

    def ab(s):
        return math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2

    for t_ in range(N - 1):
        want = ab((t_ + 1) / N) / ab(0.0)
        assert abs(a[t_] - want) <= 1e-5 * want, (t_, a[t_], want)
    # the last beta is stored as fp32(0.999), at most half an ulp (2^-25 in [0.5, 1)) from 0.999: the factor 1 - beta is exact in fp32
    # and so within 2^-25 / 0.001 = 3.0e-5 relative of 0.001; the product rounds once more (2^-24)
    assert abs(a[99] - a[98] * 0.001) <= (2.0 ** -25 / 0.001 + 2.0 ** -24) * a[98] * 0.001
    assert (np.diff(a) < 0).all() and 0.999 < a[0] < 1.0


def test_time_encoder_and_sample_noisy_actions_on_the_host(golden_dir):
    """the time rows equal the reference's (same torch ops on the host); the draw has the reference's keys and shapes and is
    reproducible from a generator"""
    from dexbotic_amd.model import OFTDiffusionForCausalLM
    g = load(golden_dir)
    m = OFTDiffusionForCausalLM(config(g), device="cpu", train=False)
    head = m.model.action_head
    assert torch.equal(head.time_encoder(g["train_timesteps"]), torch.from_numpy(g["np/time_embeddings"][:, 0]))
    acts = torch.from_numpy(g["actions"])
    a = head.sample_noisy_actions(acts, generator=torch.Generator().manual_seed(5))
    b = head.sample_noisy_actions(acts, generator=torch.Generator().manual_seed(5))
    assert sorted(a) == ["diffusion_timestep_embeddings", "noise", "noisy_actions"]
    assert a["noise"].shape == a["noisy_actions"].shape == (2, 2, 3) and a["diffusion_timestep_embeddings"].shape == (2, 1, 96)
    assert all(torch.equal(a[k], b[k]) for k in a) and a["noise"].dtype == torch.float32


def test_fixture_holds_what_the_gpu_tests_read(golden_dir):
    g = load(golden_dir)
    H = "model.action_head."
    for tag in TAGS:
        full = {k[len(tag) + 6:] for k in g.files if k.startswith(tag + "/grad/")}
        assert {H + "noisy_action_projector.fc1.weight", H + "noisy_action_projector.fc1.bias", H + "noisy_action_projector.fc2.weight",
                H + "noise_predictor.mlp_resnet.layer_norm1.weight", "model.llm.layers.0.self_attn.q_proj.weight"} <= full
        assert ((H + "proprio_projector.fc1.weight") in full) == (tag == "pp")
        for k in ("noise", "noisy_actions", "time_embeddings", "pred", "loss", "bf16/loss", "bf16/pred", "bf16_gap_loss", "bf16_gap_pred",
                  "sampler/eps", "sampler/x", "sampler/actions", "sampler/bf16/x", "sampler/bf16/actions", "bf16_gap_x",
                  "bf16_gap_actions"):
            assert tag + "/" + k in g.files
        # a final element the clamp saturated says nothing: at most one in four
        assert 4 * int((np.abs(g[tag + "/sampler/x"][-1]) >= 1.0).sum()) <= 6
    assert g["train_timesteps"].tolist() == [7, 93]
    assert os.path.getsize(os.path.join(golden_dir, "oft_dit_t1.npz")) < 1 << 20
