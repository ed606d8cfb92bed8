"""OFT-discrete without a GPU: the registry entry and the config round trip, the builder's rule for the ``Discrete`` head, the
state-dict keys in the reference's order, the label surgery and the splice plan against what the reference's class produced
(tests/golden/oft_discrete_t1.npz, scripts/gen_golden_oft_discrete.py), the ValueError for ``actions`` without ``labels``, the bin
<-> continuous helpers against the reference's formulas, and the argument checks of the new entry points (they return before any
launch)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from . import muvla_weights as MW

_G = {}
TAGS = ("np", "pp")                         # no proprio, num_bins 256 / proprio, num_bins 32
R = 6


def load(golden_dir):
    if not _G:
        _G["g"] = np.load(os.path.join(golden_dir, "oft_discrete_t1.npz"), allow_pickle=False)
    return _G["g"]


def config(g, tag="np", dtype="float32", **over):
    from dexbotic_amd.model import OFTDiscreteConfig
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    V, H, I, NL, NH, NKV, vh, vi, vl, vhd, vimg, vp, adim, chunk, pdim = (int(v) for v in g["cfg"])
    llm = Qwen2Config(vocab_size=V, hidden_size=H, intermediate_size=I, num_hidden_layers=NL, num_attention_heads=NH,
                      num_key_value_heads=NKV, rms_norm_eps=1e-6, rope_theta=1e6)
    vis = CLIPVisionConfig(hidden_size=vh, intermediate_size=vi, num_hidden_layers=vl, num_attention_heads=vhd, image_size=vimg,
                           patch_size=vp, layer_norm_eps=1e-5)
    kw = dict(llm_config=llm, mm_vision_tower=vis, mm_projector_type="mlp2x_gelu", action_model_type="Discrete", action_dim=adim,
              chunk_size=chunk, use_proprio=(tag == "pp"), proprio_dim=pdim, compute_dtype=dtype, num_bins=int(g[tag + "/num_bins"]))
    kw.update(over)
    return OFTDiscreteConfig(**kw)


def weights(g, tag):
    keys = [str(k) for k in g[tag + "/w_keys"]]
    return keys, MW.make_weights(keys, MW.unpack_shapes(g[tag + "/w_shapes"]), int(g["seed"]))


def test_registry_and_config_round_trip(golden_dir, tmp_path):
    import dexbotic_amd
    from transformers import AutoConfig
    from dexbotic_amd.model import OFTConfig, OFTDiscreteConfig, OFTDiscreteForCausalLM, OFTDiscreteModel, OFTForCausalLM, OFTModel
    assert dexbotic_amd.model_registry()["dexbotic_oft_discrete"] == (OFTDiscreteConfig, OFTDiscreteForCausalLM)
    assert dexbotic_amd.OFTDiscreteForCausalLM is OFTDiscreteForCausalLM and dexbotic_amd.OFTDiscreteConfig is OFTDiscreteConfig
    assert issubclass(OFTDiscreteConfig, OFTConfig) and issubclass(OFTDiscreteForCausalLM, OFTForCausalLM)
    assert issubclass(OFTDiscreteModel, OFTModel)
    c = OFTDiscreteConfig()
    assert c.model_type == "dexbotic_oft_discrete" and c.num_bins == 256
    c = config(load(golden_dir), "pp")
    c.save_pretrained(str(tmp_path))
    with open(os.path.join(str(tmp_path), "config.json")) as f:
        assert json.load(f)["model_type"] == "dexbotic_oft_discrete"
    c2 = AutoConfig.from_pretrained(str(tmp_path))
    assert isinstance(c2, OFTDiscreteConfig)
    assert (c2.action_model_type, c2.action_dim, c2.chunk_size, c2.use_proprio, c2.proprio_dim, c2.num_bins) == ("Discrete", 3, 2, True, 5, 32)


def test_builder_builds_the_discrete_head_only_for_its_own_config(golden_dir):
    from dexbotic_amd.engine import ParamStore, building
    from dexbotic_amd.model import OFTConfig
    from dexbotic_amd.model.oft.action_model.builder import build_action_model
    from dexbotic_amd.model.oft.action_model.model import DiscreteActionHead
    g = load(golden_dir)
    cd = config(g, "pp")
    plain = OFTConfig(**{k: getattr(cd, k) for k in ("llm_config", "mm_vision_tower", "mm_projector_type", "action_model_type",
                                                      "action_dim", "chunk_size", "use_proprio", "proprio_dim")})
    with building(ParamStore("cpu")) as _:
        with pytest.raises(NotImplementedError, match="Discrete"):
            build_action_model(plain)
        with pytest.raises(NotImplementedError, match="DiT"):
            build_action_model(config(g, action_model_type="DiT"))
        head = build_action_model(cd)
        bare = build_action_model(config(g, "np"))
    assert isinstance(head, DiscreteActionHead) and head.num_query_rows == R and head.num_bins == 32
    assert head.proprio_projector is not None and bare.proprio_projector is None and bare.num_bins == 256
    assert torch.equal(head.action_query, torch.ones(1, R)) and not list(bare.parameters())


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_key_order_and_unused_parameters_equal_the_references(golden_dir, tmp_path, tag):
    import dexbotic_amd
    from dexbotic_amd.model import OFTDiscreteForCausalLM
    g = load(golden_dir)
    m = OFTDiscreteForCausalLM(config(g, tag), device="cpu", train=False)
    sd = m.state_dict()
    keys, w = weights(g, tag)
    # the same keys and shapes.  The ORDER of the whole dict is the arena's (vision tower first, in order of use), as for every
    # policy of this package, not the reference's module order; the weight recipe walks the FIXTURE's list, so nothing depends on it.
    # Within the action head, whose keys are new here, the order is the reference's.
    assert sorted(sd.keys()) == sorted(keys)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(zip(keys, MW.unpack_shapes(g[tag + "/w_shapes"])))
    assert [k for k in sd if k.startswith("model.action_head.")] == [k for k in keys if k.startswith("model.action_head.")]
    assert list(sd.keys())[-1] == keys[-1] == "lm_head.weight"
    assert not any("action_query" in k for k in keys)
    assert ("model.action_head.proprio_projector.fc1.weight" in sd) == (tag == "pp")
    np.testing.assert_allclose(MW.checksums(keys, w), g[tag + "/w_checksums"], rtol=1e-12, atol=1e-9)
    no_grad = sorted(str(n) for n in g[tag + "/no_grad"])
    assert sorted(m.unused_parameter_names()) == no_grad and "lm_head.weight" not in no_grad
    assert all("encoder.layers.2." in n or "post_layernorm" in n for n in no_grad)
    assert m.get_output_embeddings() is None
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m.save_pretrained(str(tmp_path))
    m2 = dexbotic_amd.from_pretrained(str(tmp_path), device="cpu")
    assert type(m2) is OFTDiscreteForCausalLM and m2.config.num_bins == int(g[tag + "/num_bins"])


def test_left_padding_is_refused(golden_dir):
    from dexbotic_amd.model import OFTDiscreteForCausalLM
    with pytest.raises(ValueError, match="left"):
        OFTDiscreteForCausalLM(config(load(golden_dir), tokenizer_padding_side="left"), device="cpu", train=False)


@pytest.mark.parametrize("tag", TAGS)
def test_label_surgery_and_plan_reproduce_the_references(golden_dir, tag):
    """the cut ids / mask / targets the reference hands on, then its inserted mask and lengths from the ``rule="oft"`` plan of the
    cut prompt"""
    from dexbotic_amd.model.oft.oft_discrete_arch import cut_action_tokens
    from dexbotic_amd.splice import PLAN_PAD, build_oft_splice_plan
    g = load(golden_dir)
    P = tag + "/"
    ids, mask, labels = g[P + "input_ids"], g[P + "attention_mask"], g[P + "labels"]
    cut_ids, cut_mask, targets = cut_action_tokens(ids, mask, labels, R)
    assert np.array_equal(cut_ids, g[P + "cut_ids"]) and cut_ids.shape == (2, ids.shape[1] - R)
    assert np.array_equal(cut_mask.astype(bool), g[P + "cut_mask"])
    assert np.array_equal(targets, g[P + "targets"]) and (targets == -100).sum() == 1
    lo = int(g["cfg"][0]) - int(g[P + "num_bins"]) + 1
    assert ((targets >= lo) | (targets == -100)).all() and (cut_ids < 60).all()
    n_img = (int(g["cfg"][10]) // int(g["cfg"][11])) ** 2
    Q = R + (tag == "pp")
    plan = build_oft_splice_plan(cut_ids, cut_mask, None, n_img, Q)
    assert np.array_equal(plan.attention_mask, g[P + "inserted_mask"])
    assert np.array_equal(plan.lengths, g[P + "non_padding_lengths"]) and plan.lengths[1] == plan.lengths[0] - 2
    for b in range(2):
        n = int(plan.lengths[b])
        assert (plan.plan[b, n:] == PLAN_PAD).all() and (plan.plan[b, :n] != PLAN_PAD).all()
    with pytest.raises(ValueError, match="fewer than"):
        cut_action_tokens(ids[:, :6], mask[:, :6], labels[:, :6], R)


def test_actions_without_labels_raise_value_error(golden_dir):
    from dexbotic_amd.model import OFTDiscreteForCausalLM
    g = load(golden_dir)
    m = OFTDiscreteForCausalLM(config(g, "np"), device="cpu", train=False)
    with pytest.raises(ValueError, match="actions without labels"):
        m(input_ids=torch.from_numpy(g["np/cut_ids"]), images=torch.zeros(2, 3, 28, 28), actions=torch.from_numpy(g["np/actions"]))
    with pytest.raises(ValueError, match="attention_mask"):
        m(input_ids=torch.from_numpy(g["np/input_ids"]), labels=torch.from_numpy(g["np/labels"]), images=torch.zeros(2, 3, 28, 28))


@pytest.mark.parametrize("num_bins", [256, 32])
def test_bin_helpers_follow_the_references_formulas(num_bins):
    from dexbotic_amd.engine import ParamStore
    from dexbotic_amd.model.oft.action_model.model import DiscreteActionHead
    head = DiscreteActionHead(ParamStore("cpu"), "model.action_head.", 96, 320, 3, 2, num_bins=num_bins)
    a = torch.tensor(np.random.RandomState(3).uniform(-1.3, 1.3, size=(4, 2, 3)).astype(np.float32))
    want = ((torch.clamp(a, -1, 1) + 1) / 2 * (num_bins - 1)).round().long()
    assert torch.equal(head.discretize_actions(a), want) and want.min() == 0 and want.max() == num_bins - 1
    tok = head.continuous_to_discrete_tokens(a)
    assert tok.shape == (4, 6) and torch.equal(tok, want.reshape(4, -1))
    back = head.discrete_tokens_to_continuous(tok)
    assert back.shape == (4, 2, 3) and torch.equal(back, (tok.reshape(4, 2, 3).float() / (num_bins - 1)) * 2 - 1)
    assert (back - torch.clamp(a, -1, 1)).abs().max() <= 1.0 / (num_bins - 1) + 1e-6
    text = "actions: 3 17 0 9 30 1 and 99 more"
    s = head.discrete_tokens_to_continuous(text)
    assert s.shape == (1, 2, 3)
    assert torch.equal(s, (torch.tensor([[[3., 17., 0.], [9., 30., 1.]]]) / (num_bins - 1)) * 2 - 1)


def test_fixture_holds_what_the_gpu_tests_read(golden_dir):
    g = load(golden_dir)
    tol = float(g["fp32_tol"])
    for tag in TAGS:
        P = tag + "/"
        full = {k[len(P) + 5:] for k in g.files if k.startswith(P + "grad/")}
        assert {"lm_head.weight", "model.llm.embed_tokens.weight", "model.llm.layers.0.self_attn.q_proj.weight"} <= full
        assert ("model.action_head.proprio_projector.fc1.weight" in full) == (tag == "pp")
        nb = int(g[P + "num_bins"]) - 1
        # the margins the bins are compared under: every fp32 row, and at least 3/4 of the bf16 rows
        for k in ("logits", "nomask_logits"):
            x = np.sort(g[P + k][..., -nb:].astype(np.float64), axis=-1)
            assert (x[..., -1] - x[..., -2]).min() > 4 * tol * np.abs(x).max()
        xb = np.sort(g[P + "bf16/logits"][..., -nb:].astype(np.float64), axis=-1)
        ok = (xb[..., -1] - xb[..., -2]) > 2 * float(g[P + "bf16_gap_logits"]) * float(g[P + "bin_logit_max"])
        assert np.array_equal(ok, g[P + "bf16_rows"]) and ok.mean() >= 0.75
        # the token-1 row of the embedding gradient is the query rows' gradient: it is there, and no prompt token is 1
        assert np.abs(g[P + "grad/model.llm.embed_tokens.weight"][1]).max() > 0 and (g[P + "cut_ids"] != 1).all()
    assert os.path.getsize(os.path.join(golden_dir, "oft_discrete_t1.npz")) < 1 << 20


def test_discrete_entry_points_refuse_bad_arguments_with_a_message():
    """null pointers, a block that does not fit the sequence, bad sizes, an unaligned width for the MFMA operands: an error code and a
    message, before any launch (so no GPU is needed; the pointers handed in are never read)"""
    from dexbotic_amd import _lib as L
    lib = L.lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    p = (p + 15) // 16 * 16

    def msg():
        return lib.dxa_last_error().decode()
    assert lib.dxa_action_rows_fwd(None, p, p, 2, 16, 8, 6, 0, L.F32, None) == -1 and "dxa_action_rows_fwd" in msg() and "null" in msg()
    assert lib.dxa_action_rows_fwd(p, p, p, 2, 5, 8, 6, 0, L.F32, None) == -1 and "fit into Sq" in msg()
    assert lib.dxa_action_rows_bwd(p, None, p, 2, 16, 8, 6, 0, L.F32, None) == -1 and "dxa_action_rows_bwd" in msg()
    assert lib.dxa_action_rows_bwd(p, p, p, 2, 16, 8, 6, 2, L.F32, None) == -1 and "bad sizes" in msg()
    assert lib.dxa_action_fill_fwd(p, None, None, p, 2, 16, 8, 6, L.F32, L.F32, None) == -1 and "dxa_action_fill_fwd" in msg()
    assert lib.dxa_action_fill_fwd(p, p, None, p, 2, 16, 8, 6, L.F32, L.BF16, None) != 0 and "dxa_action_fill_fwd" in msg()
    assert lib.dxa_action_fill_bwd(p, p, p, None, None, 2, 16, 8, 6, 0, 0, L.F32, None) == -1 and "partial" in msg()
    assert lib.dxa_action_fill_bwd(p, p, p, p, p, 2, 16, 8, 6, 0, 0, L.F32, None) == -1 and "dstate" in msg()
    assert lib.dxa_action_fill_bwd_blocks(1) == 1 and lib.dxa_action_fill_bwd_blocks(16) == 1 and lib.dxa_action_fill_bwd_blocks(224) == 14
    bins = lambda h=p, w=p, cnt=p, d=8, nb=31, dtp=L.F32: lib.dxa_action_bins_fwd(h, p, w, p, p, p, cnt, 2, 16, d, 6, 0, nb, dtp, None)
    assert bins(h=None) == -1 and "dxa_action_bins_fwd" in msg() and "null" in msg()
    assert bins(cnt=None) == -1 and "counters" in msg()
    assert bins(nb=0) == -1 and "n_bins" in msg()
    assert bins(d=6) == L.lib.dxa_action_bins_fwd(p, p, p, p, p, p, p, 2, 16, 6, 6, 0, 31, L.F32, None) != 0 and "multiple of 4" in msg()
    assert bins(d=12, dtp=L.BF16) not in (0, -1) and "multiple of 8" in msg()
    assert bins(w=p + 4) not in (0, -1) and "16-byte aligned" in msg()
    assert lib.dxa_action_bins_counters(1) == 4 and lib.dxa_action_bins_counters(112) == 8 and lib.dxa_action_bins_counters(1792) == 112
