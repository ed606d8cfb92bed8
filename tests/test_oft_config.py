"""OFT without a GPU: the registry entry and the config's defaults, the action-model builder's refusals, the state-dict keys and the
parameters without a gradient against the lists the reference's class produced (tests/golden/oft_t1.npz, scripts/gen_golden_oft.py),
``build_oft_splice_plan`` against the reference's inserted mask / lengths, the plan cache's key, and the argument checks of the three
new entry points (they return before any launch)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from . import muvla_weights as MW

_G = {}
TAGS = ("np", "pp")                         # use_proprio False / True


def load(golden_dir):
    if not _G:
        _G["g"] = np.load(os.path.join(golden_dir, "oft_t1.npz"), allow_pickle=False)
    return _G["g"]


def config(g, tag="np", dtype="float32", **over):
    from dexbotic_amd.model import OFTConfig
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    V, H, I, NL, NH, NKV, vh, vi, vl, vhd, vimg, vp, adim, chunk, pdim = (int(v) for v in g["cfg"])
    llm = Qwen2Config(vocab_size=V, hidden_size=H, intermediate_size=I, num_hidden_layers=NL, num_attention_heads=NH,
                      num_key_value_heads=NKV, rms_norm_eps=1e-6, rope_theta=1e6)
    vis = CLIPVisionConfig(hidden_size=vh, intermediate_size=vi, num_hidden_layers=vl, num_attention_heads=vhd, image_size=vimg,
                           patch_size=vp, layer_norm_eps=1e-5)
    kw = dict(llm_config=llm, mm_vision_tower=vis, mm_projector_type="mlp2x_gelu", action_model_type="Linear", action_dim=adim,
              chunk_size=chunk, use_proprio=(tag == "pp"), proprio_dim=pdim, compute_dtype=dtype)
    kw.update(over)
    return OFTConfig(**kw)


def weights(g, tag):
    keys = [str(k) for k in g[tag + "/w_keys"]]
    return keys, MW.make_weights(keys, MW.unpack_shapes(g[tag + "/w_shapes"]), int(g["seed"]))


def test_registry_and_config_defaults(golden_dir, tmp_path):
    import dexbotic_amd
    from transformers import AutoConfig
    from dexbotic_amd.model import OFTConfig, OFTForCausalLM, OFTModel  # noqa: F401
    assert dexbotic_amd.model_registry()["dexbotic_oft"] == (OFTConfig, OFTForCausalLM)
    c = OFTConfig()
    assert c.model_type == "dexbotic_oft"
    assert (c.action_model_type, c.action_dim, c.chunk_size, c.use_proprio, c.proprio_dim) == (None, None, None, False, None)
    c = config(load(golden_dir), "pp")
    c.save_pretrained(str(tmp_path))
    with open(os.path.join(str(tmp_path), "config.json")) as f:
        assert json.load(f)["model_type"] == "dexbotic_oft"
    c2 = AutoConfig.from_pretrained(str(tmp_path))
    assert isinstance(c2, OFTConfig)
    assert (c2.action_model_type, c2.action_dim, c2.chunk_size, c2.use_proprio, c2.proprio_dim) == ("Linear", 3, 2, True, 5)


def test_builder_contract_and_heads_that_are_not_built(golden_dir):
    from dexbotic_amd.engine import ParamStore, building
    from dexbotic_amd.model.oft.action_model.builder import build_action_model
    g = load(golden_dir)
    with pytest.raises(RuntimeError):
        build_action_model(config(g))                     # one-argument reference signature: needs an open build context
    with building(ParamStore("cpu")):
        with pytest.raises(ValueError, match="Missing required config keys"):
            build_action_model(object())
        for mt in ("DiT", "Discrete"):
            with pytest.raises(NotImplementedError, match=mt):
                build_action_model(config(g, action_model_type=mt))
        with pytest.raises(AssertionError, match="Unsupported action model type"):
            build_action_model(config(g, action_model_type="Transformer"))
        head = build_action_model(config(g, "pp"))
    assert head.num_query_rows == 6 and head.proprio_projector is not None


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_keys_shapes_and_unused_parameters_equal_the_references(golden_dir, tmp_path, tag):
    import dexbotic_amd
    from dexbotic_amd.model import OFTForCausalLM
    g = load(golden_dir)
    m = OFTForCausalLM(config(g, tag), device="cpu", train=False)
    sd = m.state_dict()
    keys, w = weights(g, tag)
    ref_shapes = dict(zip(keys, MW.unpack_shapes(g[tag + "/w_shapes"])))
    assert sorted(sd.keys()) == sorted(keys)
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref_shapes
    for k in ("model.action_head.action_query", "model.action_head.model.layer_norm1.weight", "model.action_head.model.fc1.bias",
              "model.action_head.model.mlp_resnet_blocks.0.ffn.0.weight", "model.action_head.model.mlp_resnet_blocks.1.ffn.1.bias",
              "model.action_head.model.layer_norm2.bias", "model.action_head.model.fc2.weight", "lm_head.weight"):
        assert k in sd, k
    assert sd["model.action_head.action_query"].shape == (1, 6, 96) and sd["model.action_head.model.fc1.weight"].shape == (96, 288)
    assert ("model.action_head.proprio_projector.fc1.weight" in sd) == (tag == "pp")
    assert ("model.action_head.proprio_projector.fc2.bias" in sd) == (tag == "pp")
    np.testing.assert_allclose(MW.checksums(keys, w), g[tag + "/w_checksums"], rtol=1e-12, atol=1e-9)
    # the parameters the reference leaves without a gradient are the ones reported unused, lm_head among them
    no_grad = sorted(str(n) for n in g[tag + "/no_grad"])
    assert sorted(m.unused_parameter_names()) == no_grad and "lm_head.weight" in no_grad
    assert set(no_grad) == set(keys) - {k[len(tag) + 7:] for k in g.files if k.startswith(tag + "/gradN/")}
    # the LayerNorms of the head are nn.LayerNorm containers (the no-weight-decay rule selects by module type)
    assert isinstance(m.model.action_head.model.layer_norm1, torch.nn.LayerNorm)
    assert isinstance(m.get_submodule("model.action_head.model.mlp_resnet_blocks.1.ffn.0"), torch.nn.LayerNorm)
    assert not isinstance(m.get_submodule("model.action_head.model.mlp_resnet_blocks.1.ffn.1"), torch.nn.LayerNorm)
    # a directory whose config.json says dexbotic_oft resolves to the class
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m.save_pretrained(str(tmp_path))
    m2 = dexbotic_amd.from_pretrained(str(tmp_path), device="cpu")
    assert type(m2) is OFTForCausalLM
    assert torch.equal(m2.state_dict()["model.action_head.action_query"], torch.from_numpy(w["model.action_head.action_query"]))


def test_left_padding_is_refused(golden_dir):
    from dexbotic_amd.model import OFTForCausalLM
    from dexbotic_amd.splice import PlanCache, build_oft_splice_plan
    g = load(golden_dir)
    with pytest.raises(ValueError, match="left"):
        OFTForCausalLM(config(g, tokenizer_padding_side="left"), device="cpu", train=False)
    with pytest.raises(ValueError, match="left"):
        build_oft_splice_plan(g["input_ids"], g["attention_mask"], None, 4, 6, padding_side="left")
    with pytest.raises(ValueError, match="left"):
        PlanCache().get(g["input_ids"], g["attention_mask"], None, 4, None, "left", rule="oft", n_query_rows=6)


@pytest.mark.parametrize("tag", TAGS)
def test_oft_plan_reproduces_the_references_insertion(golden_dir, tag):
    """mask, lengths and key ranges of ``insert_action_embedding`` on the fixture's right-padded batch; the reserved rows are
    PLAN_PAD rows with IGNORE_INDEX labels; everything in front of them is the base plan"""
    from dexbotic_amd.constants import IGNORE_INDEX
    from dexbotic_amd.splice import PLAN_PAD, build_oft_splice_plan, build_splice_plan
    g = load(golden_dir)
    ids, mask = g["input_ids"], g["attention_mask"]
    n_img = (int(g["cfg"][10]) // int(g["cfg"][11])) ** 2
    Q = 6 + (tag == "pp")
    labels = np.where(mask, ids, IGNORE_INDEX)
    plan = build_oft_splice_plan(ids, mask, labels, n_img, Q)
    base = build_splice_plan(ids, mask, labels, n_img)
    B, S = base.plan.shape
    want_mask, lengths = g[tag + "/inserted_mask"], g[tag + "/non_padding_lengths"]
    assert plan.plan.shape == (B, S + Q) == want_mask.shape
    assert np.array_equal(plan.attention_mask, want_mask)
    assert np.array_equal(plan.lengths, lengths) and np.array_equal(plan.lengths, base.lengths) and lengths[1] == lengths[0] - 3
    assert np.array_equal(plan.kv_start, np.zeros(B)) and np.array_equal(plan.kv_end, lengths + Q)
    assert np.array_equal(plan.last_index, lengths + Q - 1)
    for b in range(B):
        n = int(lengths[b])
        assert np.array_equal(plan.plan[b, :n], base.plan[b, :n]) and np.array_equal(plan.labels[b, :n], base.labels[b, :n])
        assert (plan.plan[b, n:] == PLAN_PAD).all() and (plan.labels[b, n:] == IGNORE_INDEX).all()
        assert (plan.plan[b, :n] != PLAN_PAD).all()
    assert (plan.labels[0, :int(lengths[0])] != IGNORE_INDEX).any()


def test_oft_plan_without_a_mask(golden_dir):
    """no mask: every sample is as long as the spliced prompt, the Q rows are appended (oft_arch.py:170-173)"""
    from dexbotic_amd.splice import PLAN_PAD, build_oft_splice_plan
    g = load(golden_dir)
    plan = build_oft_splice_plan(g["input_ids"], None, None, 4, 7)
    B, Sq = plan.plan.shape
    S = g["input_ids"].shape[1] - 1 + 4
    assert Sq == S + 7 and plan.attention_mask.all() and (plan.lengths == S).all() and (plan.kv_end == Sq).all()
    assert (plan.plan[:, S:] == PLAN_PAD).all() and (plan.plan[:, :S] != PLAN_PAD).all()
    with pytest.raises(ValueError):
        build_oft_splice_plan(g["input_ids"], None, None, 4, 0)


def test_oft_rule_and_row_count_are_part_of_the_cache_key(golden_dir):
    from dexbotic_amd.splice import PlanCache
    g = load(golden_dir)
    ids, mask = g["input_ids"], g["attention_mask"]
    pc = PlanCache()
    base = pc.get(ids, mask, None, 4, None, "right")
    oft6 = pc.get(ids, mask, None, 4, None, "right", rule="oft", n_query_rows=6)
    oft7 = pc.get(ids, mask, None, 4, None, "right", rule="oft", n_query_rows=7)
    assert base.plan.shape[1] + 6 == oft6.plan.shape[1] == oft7.plan.shape[1] - 1
    assert pc.get(ids, mask, None, 4, None, "right", rule="oft", n_query_rows=6) is oft6
    assert pc.get(ids, mask, None, 4, None, "right") is base
    with pytest.raises(ValueError):
        pc.get(ids, mask, None, 4, None, "right", rule="oft")
    with pytest.raises(ValueError):
        pc.get(ids, mask, None, 4, None, "right", n_query_rows=6)


def test_fixture_holds_what_the_gpu_tests_read(golden_dir):
    g = load(golden_dir)
    for tag in TAGS:
        full = {k[len(tag) + 6:] for k in g.files if k.startswith(tag + "/grad/")}
        assert {"model.action_head.action_query", "model.action_head.model.layer_norm1.weight", "model.action_head.model.fc1.weight",
                "model.llm.layers.0.self_attn.q_proj.weight"} <= full
        assert ("model.action_head.proprio_projector.fc1.weight" in full) == (tag == "pp")
        for k in ("pred", "loss", "nomask_pred", "infer_actions", "bf16/loss", "bf16/pred", "bf16_gap_loss", "bf16_gap_actions"):
            assert tag + "/" + k in g.files
        # the L1 gradient is a sign: no element of either run sits near pred == target
        assert np.abs(g[tag + "/pred"] - g["actions"]).min() > 1e-2 and np.abs(g[tag + "/bf16/pred"] - g["actions"]).min() > 5e-2
    assert os.path.getsize(os.path.join(golden_dir, "oft_t1.npz")) < 1 << 20


def test_oft_entry_points_refuse_bad_arguments_with_a_message():
    """null pointers, a block that does not fit the sequence, a bad dtype pair, n <= 0: -1 (or unsupported) and a message, before any
    launch (so no GPU is needed; the pointers handed in are never read)"""
    from dexbotic_amd import _lib as L
    lib = L.lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value

    def msg():
        return lib.dxa_last_error().decode()
    put = lambda x, q, off, B=2, Sq=16, d=8, n=6, dtp=L.F32, qd=L.F32: lib.dxa_action_put_fwd(x, q, None, off, B, Sq, d, n, dtp, qd, None)
    assert put(None, p, p) == -1 and "dxa_action_put_fwd" in msg() and "null" in msg()
    assert put(p, p, None) == -1 and "null" in msg()
    assert put(p, p, p, Sq=5) == -1 and "fit into Sq" in msg()
    assert put(p, p, p, d=0) == -1 and "bad sizes" in msg()
    assert put(p, p, p, dtp=L.F32, qd=L.BF16) != 0 and "dxa_action_put_fwd" in msg()
    assert lib.dxa_action_put_bwd(None, p, p, None, 2, 16, 8, 6, 0, 0, L.F32, None) == -1 and "dxa_action_put_bwd" in msg()
    assert lib.dxa_action_put_bwd(p, p, p, p, 2, 16, 8, 6, 0, 0, L.F32, None) == -1 and "dstate" in msg()
    lnf = lambda h, off, y, B=2, Sq=16, d=8, T=2, A=3, skip=0, dtp=L.F32, wd=L.F32: lib.dxa_action_layernorm_fwd(
        h, off, None, None, y, None, None, B, Sq, d, T, A, skip, 1e-5, dtp, wd, None)
    assert lnf(None, p, p) == -1 and "dxa_action_layernorm_fwd" in msg()
    assert lnf(p, p, p, Sq=6, skip=1) == -1 and "fit into Sq" in msg()
    assert lnf(p, p, p, skip=2) == -1 and "bad sizes" in msg()
    assert lnf(p, p, p, dtp=L.F32, wd=L.BF16) != 0 and "unsupported dtype" in msg()
    lnb = lambda dy, w=None, part=None, T=2: lib.dxa_action_layernorm_bwd(dy, p, p, w, p, p, p, part, 2, 16, 8, T, 3, 0, L.F32, L.F32, None)
    assert lnb(None) == -1 and "dxa_action_layernorm_bwd" in msg()
    assert lnb(p, w=p) == -1 and "partial_dwdb" in msg()
    assert lnb(p, T=0) == -1 and "bad sizes" in msg()
    assert lib.dxa_action_layernorm_bwd_blocks(1) == 1 and lib.dxa_action_layernorm_bwd_blocks(16) == 16
    assert lib.dxa_action_layernorm_bwd_blocks(256) == 64
    assert lib.dxa_l1_loss(None, p, p, None, 4, 1.0, None) == -1 and "dxa_l1_loss" in msg()
    assert lib.dxa_l1_loss(p, p, p, None, 0, 1.0, None) == -1 and "dxa_l1_loss" in msg()
