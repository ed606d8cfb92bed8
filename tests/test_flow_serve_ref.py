"""The host side of the flow policies' serving route without a GPU: the request transforms and the prompt tokenisers against what the
reference's own classes gave on the same inputs (tests/golden/flow_serve_t1.npz, scripts/gen_golden_flow_serve.py; the cases are
stated once, in tests/flow_serve_cases.py) — values AND dtypes, the statistics mapping after two requests included — and
FlowInferenceServer's request parsing.  ``answer_formulas`` restates the answer side in plain numpy; it is pinned to the fixture here
and used by tests/test_flow_serve_gpu.py on the raw chunk of a served request."""
import json
import os
import types

import numpy as np
import pytest

from . import flow_serve_cases as C
from .flow_serve_tokenizers import pi0_tokenizer

_G = {}


def load(golden_dir):
    if not _G:
        _G["g"] = np.load(os.path.join(golden_dir, "flow_serve_t1.npz"), allow_pickle=False)
    return _G["g"]


def native_transforms():
    from dexbotic_amd.data.dataset.transform import action, common, output
    return types.SimpleNamespace(PadState=action.PadState, PadAction=action.PadAction, ActionNorm=action.ActionNorm,
                                 ActionDenorm=output.ActionDenorm, AbsoluteAction=output.AbsoluteAction, ToNumpy=common.ToNumpy,
                                 ToTensor=common.ToTensor, Pipeline=common.Pipeline)


def assert_same(got: dict, g, what: str):
    want = {k[4:] for k in g.files if k.startswith("ref/" + what)}
    assert want and {k for k in got if k.startswith(what)} == want
    for k in sorted(want):
        a, b = np.asarray(got[k]), g["ref/" + k]
        assert a.dtype == b.dtype, (k, a.dtype, b.dtype)
        assert a.shape == b.shape and np.array_equal(a, b), k


def answer_formulas(chunk, state, stats, quantiles, non_delta_mask=(6,)):
    """ToNumpy -> ActionDenorm(strict=False) -> AbsoluteAction in plain numpy: ``chunk`` float32 [B, n, A] as sampled, ``state``
    float32 [B, A] as the model saw it (normalised), ``stats`` {"state": ..., "action": ...} float64 (short ones padded here, on
    copies) -> float64 [B, n, A]"""
    def padded(v, fill, width):
        v = np.asarray(v, dtype=np.float64)
        return np.concatenate([v, np.full(width - v.shape[-1], fill)])

    def denorm(x, s):
        w = x.shape[-1]
        if quantiles:
            lo, hi = padded(s["min"], -1.0, w), padded(s["max"], 1.0, w)
            return (x + 1) / 2 * (hi - lo + 1e-6) + lo
        return x * (padded(s["std"], 1.0, w) + 1e-6) + padded(s["mean"], 0.0, w)
    action = denorm(chunk, stats["action"]) if "action" in stats else chunk
    st = denorm(state, stats["state"]) if "state" in stats else state
    out = st[:, None, :] + action
    out[..., list(non_delta_mask)] = action[..., list(non_delta_mask)]
    return out


def test_transforms_match_the_reference_in_value_and_dtype(golden_dir):
    g = load(golden_dir)
    inputs = {k[3:]: g[k] for k in g.files if k.startswith("in/")}
    got = C.run_transforms(native_transforms(), inputs)
    ref_names = {k[4:] for k in g.files if k.startswith("ref/") and not k.startswith("ref/tok/")}
    assert set(got) == ref_names
    for k in sorted(ref_names):
        a, b = np.asarray(got[k]), g["ref/" + k]
        assert a.dtype == b.dtype, (k, a.dtype, b.dtype)
        assert a.shape == b.shape and np.array_equal(a, b), k
    # what the issue names, by dtype: ActionNorm float32, ActionDenorm / AbsoluteAction float64
    assert got["ms/in_2d/state"].dtype == got["q/in_absent/state"].dtype == np.float32
    assert got["ms/out1/action"].dtype == got["q/out2/state"].dtype == got["q/out_same_rank/action"].dtype == np.float64


def test_statistics_mapping_is_padded_in_place_and_stays_padded(golden_dir):
    g = load(golden_dir)
    inputs = {k[3:]: g[k] for k in g.files if k.startswith("in/")}
    got = C.run_transforms(native_transforms(), inputs)
    for mode, (a, b) in C.STAT_KEYS.items():
        fill = {"mean": 0.0, "std": 1.0, "min": -1.0, "max": 1.0}
        for n in (a, b):
            after = got[f"{mode}/stats_after/action/{n}"]
            assert after.shape == (C.WIDTH,) and np.array_equal(after, g[f"ref/{mode}/stats_after/action/{n}"])
            assert np.array_equal(after[:C.ACTION_STATS], inputs[f"stats/{mode}/action/{n}"]) and (after[C.ACTION_STATS:] == fill[n]).all()
            assert np.array_equal(got[f"{mode}/stats_after/state/{n}"], inputs[f"stats/{mode}/state/{n}"])


def test_answer_formulas_restate_the_pinned_transforms(golden_dir):
    """the numpy restatement the GPU tests apply to a served request's raw chunk, against the reference's results"""
    g = load(golden_dir)
    inputs = {k[3:]: g[k] for k in g.files if k.startswith("in/")}
    for mode, uq in (("ms", False), ("q", True)):
        st = C.statistics(inputs, mode)
        normed = g[f"ref/{mode}/in_2d/state"]
        for i in (1, 2):
            out = answer_formulas(inputs[f"chunk{i}"], normed, st, uq)
            assert out.dtype == np.float64 and np.array_equal(out, g[f"ref/{mode}/out{i}/action"])


def test_strict_transforms_name_the_missing_key():
    T = native_transforms()
    st = {"default": {"min": -1, "max": 1}, "action": {"mean": np.zeros(2), "std": np.ones(2)}}
    with pytest.raises(KeyError, match="action"):
        T.ActionNorm(statistic_mapping=st)({"state": np.zeros(2)})
    with pytest.raises(KeyError, match="default"):
        T.ActionDenorm(statistic_mapping=st)({"action": np.zeros(2, dtype=np.float32)})
    with pytest.raises(ValueError, match="dim of action"):
        T.AbsoluteAction()({"state": np.zeros((2, 3, 4)), "action": np.zeros(4), "meta_data": {}})


def test_tokenisers_match_the_reference(golden_dir):
    from dexbotic_amd.tokenization import process as P
    g = load(golden_dir)
    assert [str(p) for p in g["prompts"]] == list(C.PROMPTS)
    got = C.run_tokenizers(P)
    assert_same(got, g, "tok/")
    ids = got["tok/pi0/0/input_ids"]
    assert ids.shape == (C.PI0_MAX_LEN,) and ids[0] == 1                                   # BOS first
    assert (got["tok/pi0/3/input_ids"][3:] == 0).all()                                      # "stack": BOS, word, newline, zeros
    assert (got["tok/pi0/2/input_ids"] != 0).all()                                          # longer than model_max_length: cut
    assert (got["tok/dm0/0/input_ids"][~got["tok/dm0/0/token_mask"]] == 2).all()            # padded with pad_token_id
    assert np.array_equal(got["tok/dm0/empty_gpt/input_ids"], got["tok/dm0/0/input_ids"])   # the empty assistant turn is dropped
    assert got["tok/dm0/answered/loss_mask"].any() and not got["tok/dm0/0/loss_mask"].any()


# ------------------------------------------------------------------------------------------------ request parsing (no device)
def server(**kw):
    from dexbotic_amd.serve import FlowInferenceServer
    model = types.SimpleNamespace(config=types.SimpleNamespace(action_dim=8))
    return FlowInferenceServer(model, pi0_tokenizer(), None, policy=kw.pop("policy", "pi0"), **kw)


def test_request_parsing_splits_and_refuses():
    s = server()
    with pytest.raises(ValueError, match="not divisible"):
        s.parse_request("go", 5, None, 2)
    with pytest.raises(ValueError, match="not divisible"):
        s.get_response("go", [None] * 3, batch_size="2")          # refused before a single frame is opened
    B, V, texts, states = s.parse_request("go", 6, None, "2")      # the form field is a string
    assert (B, V, texts) == (2, 3, ["go", "go"])
    assert states.shape == (2, 8) and states.dtype == np.float32 and not states.any()   # absent: zeros of the model's action_dim
    assert s.parse_request(["a", "b"], 4, None, 2)[2] == ["a", "b"]
    with pytest.raises(ValueError, match="texts"):
        s.parse_request(["a", "b", "c"], 4, None, 2)


def test_request_parsing_of_states():
    s = server()
    one = json.dumps([0.5] * 5)
    assert s.parse_request("go", 2, one, 1)[3].shape == (1, 5)                             # 1-D: one sample
    two = json.dumps([[0.5] * 5, [1.5] * 5])
    st = s.parse_request("go", 2, two, 2)[3]
    assert st.shape == (2, 5) and st.dtype == np.float64 and st[1, 0] == 1.5
    assert np.array_equal(s.parse_request("go", 2, [one, one], 2)[3], np.full((2, 5), 0.5))   # a list of JSON strings
    for bad, B in ((one, 2), (two, 1), ([one], 2), (json.dumps([[0.5] * 5] * 3), 2)):
        with pytest.raises(ValueError, match="states"):
            s.parse_request("go", 2 * B, bad, B)
    with pytest.raises(ValueError, match="states"):
        s.parse_request("go", 2, {"a": 1}, 1)


def test_server_policies_and_statistics_file(tmp_path):
    from dexbotic_amd.serve import FlowInferenceServer, read_normalization_stats
    from dexbotic_amd.tokenization.process import DM0Tokenization, Pi0Tokenization
    for policy, tok, uq, batch in (("pi0", Pi0Tokenization, False, False), ("pi05", Pi0Tokenization, True, False),
                                   ("dm0", DM0Tokenization, True, True)):
        s = server(policy=policy)
        assert type(s.tokenization_func) is tok and s.answer_batch is batch
        assert s.input_transform.transforms[1].use_quantiles is uq and s.output_transform.transforms[1].use_quantiles is uq
        assert s.input_transform.transforms[0].ndim == 8 and s.input_transform.transforms[1].strict is False
        assert s.input_transform.statistic_mapping is s.output_transform.statistic_mapping is s.norm_stats
        assert (s.num_images, s.non_delta_mask, s.action_dim, s.port, s.views) == (3, [6], 7, 7891, "pad")
    with pytest.raises(ValueError, match="policy"):
        server(policy="cogact")
    with pytest.raises(ValueError, match="views"):
        server(views="skip")
    assert read_normalization_stats(str(tmp_path / "norm_stats.json")) == {"min": -1, "max": 1}
    body = {"state": {"mean": [0.0, 1.0], "std": [1.0, 2.0]}, "action": {"mean": [0.5], "std": [2.0]}}
    for name, doc in (("a.json", body), ("b.json", {"norm_stats": body})):
        with open(tmp_path / name, "w") as f:
            json.dump(doc, f)
        st = read_normalization_stats(str(tmp_path / name))
        assert set(st) == {"state", "action"} and st["state"]["std"].dtype == np.float64
        assert np.array_equal(st["state"]["std"], [1.0, 2.0]) and np.array_equal(st["action"]["mean"], [0.5])


def test_from_pretrained_resolves_the_policy_and_reads_the_statistics(golden_dir, tmp_path):
    """a saved tiny checkpoint directory per policy (host tensors: nothing is launched): the policy from config.json's model_type,
    norm_stats.json unwrapped and turned into arrays, a missing file the reference's default, another model_type refused"""
    from dexbotic_amd.model import DM0ForCausalLM, Pi05ForCausalLM
    from dexbotic_amd.model.pi0.pi0_arch import Pi0Config, Pi0ForCausalLM
    from dexbotic_amd.serve import FlowInferenceServer
    from .test_dm0_config import config as dm0_config
    from .test_pi05_config import config as pi05_config, gemma
    g5 = np.load(os.path.join(golden_dir, "pi05_t1.npz"), allow_pickle=False)
    gd = np.load(os.path.join(golden_dir, "dm0_t1.npz"), allow_pickle=False)
    vis = dict(model_type="siglip_vision_model", hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
               image_size=28, patch_size=14, layer_norm_eps=1e-6)
    pi0_cfg = Pi0Config(vision_config=vis, llm_config=gemma(96, 128, model_type="gemma"), action_config=gemma(64, 80, model_type="gemma"),
                        action_dim=8, chunk_size=6)
    body = {"state": {"min": [-1.0] * 8, "max": [2.0] * 8}, "action": {"min": [-1.0] * 7, "max": [1.0] * 7}}
    for policy, cls, cfg in (("pi0", Pi0ForCausalLM, pi0_cfg), ("pi05", Pi05ForCausalLM, pi05_config(g5)), ("dm0", DM0ForCausalLM, dm0_config(gd))):
        d = tmp_path / policy
        cls(cfg, device="cpu", train=False).save_pretrained(str(d))
        s = FlowInferenceServer.from_pretrained(str(d), tokenizer=pi0_tokenizer(), device="cpu", views="present")
        assert (s.policy, type(s.model), s.views) == (policy, cls, "present") and s.norm_stats == {"min": -1, "max": 1}
        with open(d / "norm_stats.json", "w") as f:
            json.dump({"norm_stats": body}, f)
        s = FlowInferenceServer.from_pretrained(str(d), tokenizer=pi0_tokenizer(), device="cpu")
        assert np.array_equal(s.norm_stats["state"]["max"], [2.0] * 8) and s.norm_stats["action"]["min"].shape == (7,)
        assert s.input_transform.transforms[0].ndim == 8
    other = tmp_path / "other"
    other.mkdir()
    with open(other / "config.json", "w") as f:
        json.dump({"model_type": "dexbotic_cogact"}, f)
    with pytest.raises(ValueError, match="not a flow policy"):
        FlowInferenceServer.from_pretrained(str(other), tokenizer=pi0_tokenizer())


def test_tokenize_gives_ids_and_the_pad_mask():
    s = server()
    ids, mask = s.tokenize(["pick up", "stack the red_block now"])
    assert ids.shape == mask.shape == (2, 12) and ids.dtype == np.int64 and mask.dtype == bool
    assert mask.sum(1).tolist() == [4, 7] and (ids[~mask] == 0).all()                       # BOS + words + newline
