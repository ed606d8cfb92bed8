"""The persistent one-launch decode step on a Qwen3 decoder (csrc/decode_fused.hip, the QKN instantiation: per-head RMSNorm of q and
of the new key in front of RoPE, no q / k / v bias) — against the installed transformers.Qwen3Model's numbers
(tests/golden/qwen3_d64.npz, scripts/gen_golden_qwen3_decode.py), against the per-op cached path it replaces and against the same
decoder computed in fp32, at toy and at real widths, and inside generate()."""
import os

import numpy as np
import pytest
import torch

from .helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = "model.llm."
FIXTURE_DIMS = dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                    num_key_value_heads=2, head_dim=64)


def T(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "qwen3_d64.npz"), allow_pickle=False)


def _config(**dims):
    from dexbotic_amd.model.llm.qwen3 import Qwen3Config
    return Qwen3Config(rope_theta=1e6, rms_norm_eps=1e-6, **dims)


def _backbone(cfg, dtype, weights=None, seed=7):
    """Qwen3Backbone holding `weights` ({HF name: fp32 array}) or seeded random weights on the bf16 grid — the same VALUES for every
    dtype: N(0, 0.6 / sqrt(fan_in)) matrices, 1 + 0.1 N(0, 1) layer norms, U(0.5, 1.5) q / k norms (a missing or swapped one shows)"""
    from dexbotic_amd.engine import ParamStore, attach_parameters
    from dexbotic_amd.model.llm.qwen3 import Qwen3Backbone
    st = ParamStore(DEV, dtype)
    llm = Qwen3Backbone(st, P, cfg)
    st.finalize(train=False)
    attach_parameters(llm, st)
    if weights is not None:
        assert sorted(st.slots) == sorted(P + n for n in weights)
        for n, v in weights.items():
            st.w32(P + n).copy_(T(v))
    else:
        gen = torch.Generator(device=DEV).manual_seed(seed)
        for name, slot in st.slots.items():                  # (slot order is registration order: the same draws for every dtype)
            shape = tuple(slot.shape)
            if name.endswith("q_norm.weight") or name.endswith("k_norm.weight"):
                w = 0.5 + torch.rand(shape, generator=gen, device=DEV)
            elif len(shape) == 1:
                w = 1.0 + 0.1 * torch.randn(shape, generator=gen, device=DEV)
            else:
                w = torch.randn(shape, generator=gen, device=DEV) * (0.6 / shape[1] ** 0.5)
            st.w32(name).copy_(w.bfloat16().float())
    st.sync_shadow()
    return llm


def _walk(llm, prompt, steps, pad, dtype):
    """prefill + one pass per new embedding; returns (hidden state per step [T, d], cache)"""
    cache = llm.new_cache(1, prompt.shape[1] + len(steps), DEV, dtype)
    with torch.no_grad():
        llm.forward_cached(prompt.to(dtype), cache, pad)
        out = [llm.forward_cached(e.to(dtype).view(1, 1, -1), cache, pad)[0, 0].float().cpu().numpy() for e in steps]
    torch.cuda.synchronize()
    return np.stack(out), cache


def _both_paths(llm16, prompt, steps, pad, monkeypatch):
    from dexbotic_amd import kernels as K
    monkeypatch.setenv("DXA_DECODE_FUSED", "0")
    per_op, c_u = _walk(llm16, prompt, steps, pad, torch.bfloat16)
    monkeypatch.setenv("DXA_DECODE_FUSED", "1")
    fused, c_f = _walk(llm16, prompt, steps, pad, torch.bfloat16)
    assert c_u.fused_steps == 0 and c_f.fused_steps == len(steps)
    assert not K.decode_timed_out()
    return per_op, c_u, fused, c_f


def _inputs(d, n_prompt, n_steps, seed):
    """prompt [1, n_prompt, d] and step embeddings on the bf16 grid: every path sees the same numbers"""
    g = torch.Generator().manual_seed(seed)
    prompt = (torch.randn(1, n_prompt, d, generator=g) * 0.5).bfloat16().float().to(DEV)
    steps = [(torch.randn(d, generator=g) * 0.5).bfloat16().float().to(DEV) for _ in range(n_steps)]
    return prompt, steps


def _assert_tracks(tag, fused, per_op, ref):
    """the bound of tests/test_decode_fused_gpu.py: the persistent step is as close to the fp32 model as the per-op step is"""
    for t in range(len(fused)):
        e_f, e_u, e_fu = rel_err(fused[t], ref[t]), rel_err(per_op[t], ref[t]), rel_err(fused[t], per_op[t])
        print(f"{tag} step {t}: fused vs fp32 {e_f:.2e} | per-op vs fp32 {e_u:.2e} | fused vs per-op {e_fu:.2e}")
        assert e_f < 3e-2 and e_f <= 1.5 * e_u + 3e-3, (tag, t, e_f, e_u)


def _assert_caches_agree(c_f, c_u, n0):
    for i in range(len(c_f.k)):                              # the appended keys / values: what later tokens attend to
        for a, b in ((c_f.k[i], c_u.k[i]), (c_f.v[i], c_u.v[i])):
            assert rel_err(a[:, :, n0:c_f.length].float().cpu().numpy(), b[:, :, n0:c_u.length].float().cpu().numpy()) < 3e-2, i


@pytest.mark.parametrize("pad", [None, [3]])
def test_fixture_walk_on_the_persistent_step_matches_hf(gold, pad, monkeypatch):
    """the fixture's decoder in bf16: prefill of 11 tokens, six single-token steps.  pad=None: every fused hidden state within 3 x
    HF's own bf16-vs-fp32 distance of that step from HF's fp32 step (the standing factor of tests/test_lm_real_gpu.py).  pad=[3]:
    three left-padding slots in front of the prompt, for which HF stored nothing: fused against per-op and this project's fp32
    decoder, the bound of tests/test_decode_fused_gpu.py."""
    g = gold
    w = {str(n): g["w/" + str(n)] for n in g["names"]}
    cfg = _config(**FIXTURE_DIMS)
    assert [int(v) for v in g["cfg"]] == [cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers,
                                          cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim]
    llm16 = _backbone(cfg, torch.bfloat16, w)
    x = T(g["inputs_embeds"])
    n0, n_steps = g["cached_prefill"].shape[1], g["cached_steps"].shape[1]
    prompt, steps = x[:, :n0].contiguous(), [x[0, n0 + t].contiguous() for t in range(n_steps)]
    if pad is not None:
        filler = (torch.randn(1, pad[0], x.shape[2], generator=torch.Generator().manual_seed(2)) * 0.5).bfloat16().float().to(DEV)
        prompt = torch.cat([filler, prompt], dim=1).contiguous()
    per_op, c_u, fused, c_f = _both_paths(llm16, prompt, steps, pad, monkeypatch)
    for t in range(n_steps):
        hf32, hf16 = g["cached_steps"][0, t], g["cached_steps_bf16"][0, t]
        gap, e = rel_err(hf16, hf32), rel_err(fused[t], hf32)
        print(f"pad {pad} step {t}: fused vs HF fp32 {e:.2e} | per-op vs HF fp32 {rel_err(per_op[t], hf32):.2e} | HF bf16 vs fp32 {gap:.2e}")
        if pad is None:
            assert e <= 3.0 * gap, (t, e, gap)
    if pad is not None:
        ref, _ = _walk(_backbone(cfg, torch.float32, w), prompt, steps, pad, torch.float32)
        _assert_tracks(f"fixture pad {pad}", fused, per_op, ref)
    _assert_caches_agree(c_f, c_u, prompt.shape[1])


TOY = {
    "d64": FIXTURE_DIMS,                                     # the fixture's shape: GQA group of 2, Hq D = 2 d
    "d128g4": dict(vocab_size=64, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                   num_key_value_heads=1, head_dim=128),     # GQA group of 4: four workgroups normalise and rotate the one new key
}


@pytest.mark.parametrize("tag", sorted(TOY))
def test_persistent_step_tracks_the_per_op_step_and_the_fp32_decoder(tag, monkeypatch):
    cfg = _config(**TOY[tag])
    llm16, llm32 = _backbone(cfg, torch.bfloat16), _backbone(cfg, torch.float32)      # the same weight VALUES, fp32 arithmetic
    prompt, steps = _inputs(cfg.hidden_size, 11, 6, seed=5)
    ref, _ = _walk(llm32, prompt, steps, None, torch.float32)
    per_op, c_u, fused, c_f = _both_paths(llm16, prompt, steps, None, monkeypatch)
    _assert_tracks(tag, fused, per_op, ref)
    _assert_caches_agree(c_f, c_u, prompt.shape[1])


REAL = {
    # Qwen3-0.6B: Hq D = 2048 = 2 d — 16 / 4 / 12 rows per workgroup on 256 CUs and only two K blocks of 512 in the qkv product
    "0.6b": dict(vocab_size=64, hidden_size=1024, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=16,
                 num_key_value_heads=8, head_dim=128),
    # Qwen3-8B
    "8b": dict(vocab_size=64, hidden_size=4096, intermediate_size=12288, num_hidden_layers=2, num_attention_heads=32,
               num_key_value_heads=8, head_dim=128),
}


@pytest.mark.parametrize("tag", ["0.6b", "8b"])
def test_persistent_step_at_real_qwen3_widths(tag, monkeypatch):
    """two decoder layers at real widths over a 300-token cache, three steps: the bound of the toy shapes, and run-to-run identical"""
    cfg = _config(**REAL[tag])
    llm16 = _backbone(cfg, torch.bfloat16, seed=3)
    prompt, steps = _inputs(cfg.hidden_size, 300, 3, seed=9)
    llm32 = _backbone(cfg, torch.float32, seed=3)
    ref, _ = _walk(llm32, prompt, steps, None, torch.float32)
    del llm32
    per_op, c_u, fused, c_f = _both_paths(llm16, prompt, steps, None, monkeypatch)
    _assert_tracks(f"Qwen3-{tag} widths", fused, per_op, ref)
    again, _ = _walk(llm16, prompt, steps, None, torch.bfloat16)
    assert np.array_equal(again, fused)                      # fixed summation order: run-to-run identical


@pytest.fixture(scope="module")
def lm():
    """DexboticForCausalLM in bf16 over the head_dim 64 decoder and the toy CLIP tower of tests/test_qwen3_gpu.py"""
    from dexbotic_amd.model.dexbotic_arch import DexboticConfig, DexboticForCausalLM
    from dexbotic_amd.model.llm.qwen3 import Qwen3Backbone
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    vis = CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, image_size=56,
                           patch_size=14, layer_norm_eps=1e-5)
    cfg = DexboticConfig(llm_config=_config(**FIXTURE_DIMS).to_dict(), mm_vision_tower=vis, mm_projector_type="mlp2x_gelu",
                         compute_dtype="bfloat16")
    m = DexboticForCausalLM(cfg, device=DEV, train=False)
    assert isinstance(m.model.llm, Qwen3Backbone)
    m.init_random_(seed=3, std=0.05)
    m.eval()
    return m


def _prompt():
    rs = np.random.RandomState(5)
    ids = rs.randint(3, 60, size=(1, 10)).astype(np.int64)
    ids[:, 1] = -200
    images = np.clip(rs.standard_normal((1, 3, 56, 56)), -2.5, 2.5).astype(np.float32)
    return T(ids), T(images)


def _caches_of(m, monkeypatch):
    """the caches generate() makes (they are local to the call)"""
    seen = []
    new_cache = m.model.llm.new_cache
    monkeypatch.setattr(m.model.llm, "new_cache", lambda *a, **kw: (seen.append(new_cache(*a, **kw)), seen[-1])[1])
    return seen


def test_bf16_generate_on_a_qwen3_decoder_uses_the_persistent_step(lm, monkeypatch):
    """greedy ids of the persistent path = ids of the per-op path wherever the per-op path's top-1 / top-2 logit margin exceeds
    twice the distance between the two paths' logits (the rule of tests/test_decode_fused_gpu.py)"""
    ids, img = _prompt()
    seen = _caches_of(lm, monkeypatch)
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DXA_DECODE_FUSED", mode)
        outs[mode] = lm.generate(ids, images=img, max_new_tokens=6, do_sample=False, return_dict_in_generate=True, output_logits=True)
    assert seen[0].fused_steps == 0 and seen[1].fused_steps == 5      # (the first token comes from the prefill)
    L0 = ids.shape[1]
    a, b = outs["0"].sequences[0, L0:].cpu().numpy(), outs["1"].sequences[0, L0:].cpu().numpy()
    for t in range(len(a)):
        la, lb = outs["0"].logits[t][0].float().cpu().numpy(), outs["1"].logits[t][0].float().cpu().numpy()
        top2 = np.sort(la)[-2:]
        margin, dist = float(top2[1] - top2[0]), float(np.abs(la - lb).max())
        print(f"token {t}: ids {a[t]} / {b[t]}  margin {margin:.3f}  logit distance {dist:.3f}")
        if margin > 2 * dist:
            assert a[t] == b[t], t
        if a[t] != b[t]:
            break                                           # the sequences part ways at a near-tie: later steps see different prefixes


def test_sampled_generate_on_a_qwen3_decoder_runs_on_the_persistent_step(lm, monkeypatch):
    ids, img = _prompt()
    seen = _caches_of(lm, monkeypatch)
    monkeypatch.setenv("DXA_DECODE_FUSED", "1")
    seqs = [lm.generate(ids, images=img, max_new_tokens=5, do_sample=True, temperature=0.8, top_k=20,
                        generator=torch.Generator().manual_seed(11)) for _ in range(2)]
    assert all(c.fused_steps > 0 for c in seen)
    assert seqs[0].shape == (1, ids.shape[1] + 5) and torch.equal(seqs[0], seqs[1])     # the same generator state: the same tokens
    assert int(seqs[0][0, ids.shape[1]:].min()) >= 0 and int(seqs[0][0, ids.shape[1]:].max()) < FIXTURE_DIMS["vocab_size"]
