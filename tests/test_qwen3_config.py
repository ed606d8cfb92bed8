"""CPU checks of the decoder dispatch: Qwen3Config.from_any (head_dim, theta, what it refuses), llm_config_from_any, and that a Qwen2
llm_config still becomes the same Qwen2Config."""
import pytest

from dexbotic_amd.model.llm.qwen2 import Qwen2Config
from dexbotic_amd.model.llm.qwen3 import Qwen3Config, llm_config_from_any

TINY = dict(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
            head_dim=32)


def test_defaults_are_qwen3_8b():
    c = Qwen3Config()
    assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim,
            c.rms_norm_eps, c.rope_theta, c.vocab_size, c.model_type) == (4096, 12288, 36, 32, 8, 128, 1e-6, 1e6, 151936, "qwen3")
    assert c.to_dict()["head_dim"] == 128


def test_from_hf_config_object():
    import transformers
    hf = transformers.Qwen3Config(**TINY, rope_parameters={"rope_type": "default", "rope_theta": 5e5}, rms_norm_eps=1e-5)
    for c in (Qwen3Config.from_any(hf), llm_config_from_any(hf)):
        assert type(c) is Qwen3Config
        assert (c.head_dim, c.hidden_size, c.num_attention_heads, c.rope_theta, c.rms_norm_eps) == (32, 64, 4, 5e5, 1e-5)
        assert c.num_attention_heads * c.head_dim != c.hidden_size
    assert Qwen3Config.from_any(c) is c and llm_config_from_any(c) is c


def test_from_dict_and_rope_parameters():
    c = llm_config_from_any(dict(TINY, model_type="qwen3", rope_theta=2e5))
    assert type(c) is Qwen3Config and c.head_dim == 32 and c.rope_theta == 2e5
    c = llm_config_from_any(dict(TINY, model_type="qwen3", rope_parameters={"rope_theta": 3e5, "rope_type": "default"}))
    assert c.rope_theta == 3e5
    assert Qwen3Config.from_any(dict(TINY)).model_type == "qwen3"            # a dict without model_type, asked for as Qwen3
    assert llm_config_from_any(c.to_dict()) == c                            # what config.json holds


@pytest.mark.parametrize("bad", [dict(attention_bias=True), dict(tie_word_embeddings=True), dict(use_sliding_window=True),
                                 dict(layer_types=["full_attention", "sliding_attention"])])
def test_refuses_what_the_native_layer_does_not_compute(bad):
    with pytest.raises(NotImplementedError, match=next(iter(bad)).split("_")[0]):
        llm_config_from_any(dict(TINY, model_type="qwen3", **bad))
    llm_config_from_any(dict(TINY, model_type="qwen3", attention_bias=False, tie_word_embeddings=False, use_sliding_window=False,
                             layer_types=["full_attention"] * 2))


def test_unknown_model_type_names_both_supported_types():
    for from_any in (llm_config_from_any, Qwen2Config.from_any):
        with pytest.raises(NotImplementedError) as e:
            from_any(dict(TINY, model_type="llama"))
        assert "'llama'" in str(e.value) and "qwen2" in str(e.value) and "qwen3" in str(e.value)
    with pytest.raises(NotImplementedError):
        Qwen3Config.from_any(dict(TINY, model_type="qwen2"))


def test_qwen2_dicts_are_unchanged():
    d = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
             num_key_value_heads=1, rope_theta=1e4, model_type="qwen2", attention_bias=True, tie_word_embeddings=True, head_dim=999)
    for c in (Qwen2Config.from_any(d), llm_config_from_any(d), llm_config_from_any({k: v for k, v in d.items() if k != "model_type"})):
        assert type(c) is Qwen2Config
        assert c == Qwen2Config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                                num_key_value_heads=1, rope_theta=1e4)
        assert c.head_dim == 128 and "head_dim" not in c.to_dict()
    assert Qwen2Config.from_any({}) == Qwen2Config() and Qwen2Config().model_type == "qwen2"


def test_dexbotic_config_picks_the_decoder_by_model_type():
    from dexbotic_amd.model.dexbotic_arch import DexboticConfig
    c = DexboticConfig(llm_config=dict(TINY, model_type="qwen3"), mm_vision_tower=None)
    assert type(c.llm_config) is Qwen3Config and c.head_dim == 32 and c.hidden_size == 64
    again = DexboticConfig.from_dict(c.to_dict())
    assert type(again.llm_config) is Qwen3Config and again.llm_config == c.llm_config
    assert type(DexboticConfig(llm_config=None, mm_vision_tower=None).llm_config) is Qwen2Config
