"""The key/value-cached path runs the decoder layer's one launch sequence (functional.Qwen2LayerFn._run): a prefill into an empty
cache of exactly S positions hands every launch the operands, shapes and strides the uncached forward hands it, so the two outputs
are the same bits — Qwen2 and Qwen3 layers, fp32 and bf16, the two-launch and the fused SwiGLU product."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = "model.llm."


def _backbone(kind: str, dtype):
    from dexbotic_amd.engine import ParamStore, attach_parameters
    from dexbotic_amd.model.llm.qwen2 import Qwen2Backbone, Qwen2Config
    from dexbotic_amd.model.llm.qwen3 import Qwen3Backbone, Qwen3Config
    dims = dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                num_key_value_heads=2)
    st = ParamStore(DEV, dtype)
    llm = Qwen3Backbone(st, P, Qwen3Config(head_dim=32, **dims)) if kind == "qwen3" else Qwen2Backbone(st, P, Qwen2Config(**dims))
    assert llm.config.head_dim == 32
    st.finalize(train=False)
    attach_parameters(llm, st)
    gen = torch.Generator().manual_seed(7)
    for name, slot in st.slots.items():
        w = torch.randn(slot.shape, generator=gen)
        st.w32(name).copy_((1.0 + 0.1 * w if "norm" in name else 0.05 * w).to(DEV))
    st.sync_shadow()
    return llm


@pytest.mark.parametrize("B,S", [(2, 24), (1, 160)])      # 160 rows: bf16 takes the fused-SwiGLU product (M >= 129, K % 64 == 0)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["qwen2", "qwen3"])
def test_cached_prefill_into_an_empty_cache_is_the_uncached_forward(kind, dtype, B, S):
    from dexbotic_amd import kernels as K
    llm = _backbone(kind, dtype)
    x = torch.randn((B, S, 128), generator=torch.Generator().manual_seed(11)).to(device=DEV, dtype=dtype)
    sp = llm.layer_specs[0]
    fused = K.swiglu_gemm_supported(torch.empty((B * S, 128), device=DEV, dtype=dtype),
                                    llm.store.w(*sp.gu_w, shape=(2 * sp.F, sp.d)))
    assert fused == (dtype == torch.bfloat16 and B * S >= 129)        # the shapes cover both forms of the gated MLP
    cache = llm.new_cache(B, S, DEV, dtype)
    with torch.no_grad():
        want = llm(x)
        got = llm.forward_cached(x, cache)
    assert torch.isfinite(want.float()).all() and float(want.float().abs().max()) > 0
    assert torch.equal(got, want)
    assert cache.length == S and cache.fused_steps == 0
