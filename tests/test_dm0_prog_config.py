"""DM0-prog without a GPU: the registry entry, the config's round trip, the state-dict keys and shapes of the native class against the
list the reference's class produced (tests/golden/dm0_prog_t1.npz), the weight recipe against the stored checksums, the refusals of
``forward`` and of a malformed ``progress``, and the condition that makes the fixture's ``end_progress`` tell a wrong reduction apart."""
import json
import os

import numpy as np
import pytest
import torch

from . import muvla_weights as MW
from .test_dm0_config import q3

FP32_TOL = 1e-3                      # the bound of tests/test_dm0_prog_gpu.py
_G = {}


def load(golden_dir):
    if not _G:
        _G["g"] = np.load(os.path.join(golden_dir, "dm0_prog_t1.npz"), allow_pickle=False)
    return _G["g"]


def config(g, dtype="float32", **over):
    from dexbotic_amd.model import DM0ProgConfig
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    V, H, I, NL, NH, NKV, HD, AH, AI, vh, vi, vl, vhd, vimg, vp, chunk, adim, _ = (int(v) for v in g["cfg"])
    vis = CLIPVisionConfig(hidden_size=vh, intermediate_size=vi, num_hidden_layers=vl, num_attention_heads=vhd, image_size=vimg,
                           patch_size=vp)
    kw = dict(llm_config=q3(H, I, NL, NH, NKV, HD, V), action_config=q3(AH, AI, NL, NH, NKV, HD, V), mm_vision_tower=vis,
              action_dim=adim, chunk_size=chunk, compute_dtype=dtype)
    kw.update(over)
    return DM0ProgConfig(**kw)


def test_registry_and_autoconfig_resolve_dexbotic_dm0_prog(golden_dir, tmp_path):
    import dexbotic_amd
    from transformers import AutoConfig
    from dexbotic_amd.model import DM0Config, DM0ForCausalLM, DM0ProgConfig, DM0ProgForCausalLM, DM0ProgModel
    from dexbotic_amd.model.dm0 import DM0Model
    assert dexbotic_amd.model_registry()["dexbotic_dm0_prog"] == (DM0ProgConfig, DM0ProgForCausalLM)
    assert dexbotic_amd.model_registry()["dexbotic_dm0"] == (DM0Config, DM0ForCausalLM)
    assert issubclass(DM0ProgConfig, DM0Config) and issubclass(DM0ProgModel, DM0Model) and issubclass(DM0ProgForCausalLM, DM0ForCausalLM)
    c = config(load(golden_dir))
    c.save_pretrained(str(tmp_path))
    with open(os.path.join(str(tmp_path), "config.json")) as f:
        assert json.load(f)["model_type"] == "dexbotic_dm0_prog"
    assert type(AutoConfig.from_pretrained(str(tmp_path))) is DM0ProgConfig


def test_config_round_trip(golden_dir, tmp_path):
    from dexbotic_amd.model import DM0ProgConfig
    from dexbotic_amd.model.llm.qwen3 import Qwen3Config
    c = DM0ProgConfig()
    assert c.model_type == "dexbotic_dm0_prog" and c.action_dim == 32 and c.chunk_size == 50 and c.bf16 is True
    c = config(load(golden_dir))
    c.save_pretrained(str(tmp_path))
    c2 = DM0ProgConfig.from_pretrained(str(tmp_path))
    assert c2.to_dict() == c.to_dict()
    assert isinstance(c2.action_config, Qwen3Config) and isinstance(c2.llm_config, Qwen3Config)
    assert (c2.action_config.hidden_size, c2.llm_config.hidden_size, c2.chunk_size, c2.action_dim, c2.compute_dtype) == \
        (64, 96, 6, 8, "float32")


def test_state_dict_keys_and_shapes_equal_the_references(golden_dir, tmp_path):
    import dexbotic_amd
    from dexbotic_amd.model import DM0ProgForCausalLM
    g = load(golden_dir)
    m = DM0ProgForCausalLM(config(g), device="cpu", train=False)
    want = dict(zip((str(k) for k in g["w_keys"]), MW.unpack_shapes(g["w_shapes"])))
    have = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert have == want
    assert have["model.progress_in_proj.weight"] == (64, 1) and have["model.progress_in_proj.bias"] == (64,)
    assert have["model.progress_out_proj.weight"] == (1, 64) and have["model.progress_out_proj.bias"] == (1,)
    # the reference's order: the four DM0 linears, then the progress projections, then lm_head
    order = list(m.store.slots)
    first = lambda p: next(i for i, n in enumerate(order) if n.startswith(p))
    marks = [first(p) for p in ("model.action_in_proj.", "model.action_time_mlp_out.", "model.progress_in_proj.",
                                "model.progress_out_proj.", "lm_head.")]
    assert marks == sorted(marks)
    m.save_pretrained(str(tmp_path))
    m2 = dexbotic_amd.from_pretrained(str(tmp_path), device="cpu")
    assert type(m2) is DM0ProgForCausalLM
    assert torch.equal(m2.state_dict()["model.progress_out_proj.weight"], m.state_dict()["model.progress_out_proj.weight"])


def test_weight_recipe_reproduces_the_stored_checksums(golden_dir):
    g = load(golden_dir)
    w, images = MW.from_fixture(g)
    keys = [str(k) for k in g["w_keys"]]
    np.testing.assert_allclose(MW.checksums(keys, w), g["w_checksums"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(MW.checksums(["images"], {"images": images}), g["image_checksum"], rtol=1e-12, atol=1e-9)


def test_forward_is_refused_and_a_malformed_progress_raises_before_the_device(golden_dir):
    from dexbotic_amd.model import DM0ProgForCausalLM
    g = load(golden_dir)
    m = DM0ProgForCausalLM(config(g), device="cpu", train=False)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m(input_ids=torch.from_numpy(g["input_ids"]))
    B = g["input_ids"].shape[0]
    kw = dict(input_ids=torch.from_numpy(g["input_ids"]), attention_mask=torch.from_numpy(g["attention_mask"]), images=None,
              image_masks=torch.from_numpy(g["image_masks"]), states=torch.from_numpy(g["states"]))
    for bad in (torch.zeros(B), torch.zeros(B, 1, 1, 1)):
        with pytest.raises(ValueError, match="progress"):
            m.inference_action(progress=bad, **kw)


def test_the_fixture_tells_a_wrong_minimum_apart(golden_dir):
    """per sample the minimum is attained at an inner step, at a different step for each sample, and lies more than 10 x FP32_TOL
    below the second-smallest step value: the last step, step 0 or one minimum for the whole batch all miss ``end_progress``"""
    g = load(golden_dir)
    steps, end = g["end_progress_steps"], g["end_progress"]
    assert steps.shape == (int(g["cfg"][-1]), g["input_ids"].shape[0]) and end.shape == (steps.shape[1], 1, 1)
    assert np.array_equal(steps.min(axis=0), end.reshape(-1))
    arg = steps.argmin(axis=0)
    assert np.all((arg > 0) & (arg < steps.shape[0] - 1)), arg
    assert len(set(arg.tolist())) == steps.shape[1], arg
    srt = np.sort(steps, axis=0)
    assert np.all(srt[1] - srt[0] > 10 * FP32_TOL), srt[1] - srt[0]
    assert g["progress"].shape == (steps.shape[1], 1) and len(set(g["progress"].reshape(-1).tolist())) == steps.shape[1]
    assert g["infer_actions"].shape == g["infer_actions_noprog"].shape == g["init_noise"].shape
    assert not np.array_equal(g["infer_actions"], g["infer_actions_noprog"])
