"""Sampled decoding through DexboticForCausalLM.generate on the tiny model of tests/golden/lm_t1.npz (fp32): the documented draw
of the uniforms, HF's warpers as the truth for the kept set of every step, and the defaults DiscreteVLAForCausalLM hands down."""
import numpy as np
import pytest
import torch

from dexbotic_amd import kernels as K

from . import sample_ref as R
from .helpers import build_lm_product, load_lm_golden
from .test_lm_gpu import _FakeTokenizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_NEW = 6


def T(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


@pytest.fixture(scope="module")
def lm(golden_dir):
    g, cfg, w = load_lm_golden(golden_dir)
    m = build_lm_product(cfg, w, "float32", DEV, train=False)
    m.eval()
    return g, m


def gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def test_top_k_1_equals_greedy(lm):
    g, m = lm
    prompt, img = T(g["decode_prompt"]), T(g["images"][:1])
    greedy = m.generate(prompt, images=img, max_new_tokens=N_NEW)
    assert np.array_equal(greedy[0, prompt.shape[1]:].cpu().numpy(), g["decode_new_ids"][:N_NEW])
    for seed in (0, 1, 2):
        seq = m.generate(prompt, images=img, max_new_tokens=N_NEW, do_sample=True, top_k=1, temperature=0.7,
                         generator=gen(DEV, seed))
        assert torch.equal(seq, greedy), seed


@pytest.mark.parametrize("gen_device", ["cpu", DEV])
def test_seeded_draw_follows_the_documented_contract(lm, gen_device):
    g, m = lm
    prompt, img = T(g["decode_prompt"]), T(g["images"][:1])
    Tm, k, p = 0.7, 5, 0.9
    out = m.generate(prompt, images=img, max_new_tokens=N_NEW, do_sample=True, top_k=k, top_p=p, temperature=Tm,
                     return_dict_in_generate=True, output_logits=True, generator=gen(gen_device, 77))
    new = out.sequences[0, prompt.shape[1]:].cpu()
    assert len(new) == N_NEW == len(out.logits)
    u = torch.rand(N_NEW, 1, dtype=torch.float32, generator=gen(gen_device, 77), device=gen_device).cpu()
    for t in range(N_NEW):
        x32 = out.logits[t].float().cpu()                                   # [1, V]: what step t drew from
        keep = torch.isfinite(R.hf_warp(x32, Tm, k, p))
        assert 1 <= int(keep.sum()) <= k
        R.check_draw(new[t:t + 1], None, u[t], keep, *R.cdf64(x32, keep, Tm), what=f"step {t}")
    again = m.generate(prompt, images=img, max_new_tokens=N_NEW, do_sample=True, top_k=k, top_p=p, temperature=Tm,
                       generator=gen(gen_device, 77))
    assert torch.equal(again, out.sequences)


def test_discrete_vla_hands_hf_defaults_to_the_kernel(golden_dir, monkeypatch):
    from dexbotic_amd.model.discrete_vla.discrete_vla_arch import DiscreteVLAForCausalLM
    g, cfg, w = load_lm_golden(golden_dir)
    m = build_lm_product(cfg, w, "float32", DEV, train=False, cls=DiscreteVLAForCausalLM)
    m.eval()

    class Conv:
        sep, sep2 = "</s>", "</s>"
        sep_style = type("S", (), {"name": "TWO"})()

    calls = []
    real = K.sample_rows

    def spy(logits, u, temperature=1.0, top_k=0, top_p=1.0, return_info=False):
        calls.append((temperature, top_k, top_p))
        return real(logits, u, temperature, top_k, top_p, return_info)

    monkeypatch.setattr(K, "sample_rows", spy)
    norms = {"min": [-1.0] * 7, "max": [1.0] * 7}
    args = {"conv": Conv(), "tokenizer": _FakeTokenizer(), "vocab_size": 255, "action_norms": norms, "do_sample": True,
            "max_new_tokens": 8}
    acts = m.inference_action(T(g["decode_prompt"]), T(g["images"][:1]), args, generator=gen(DEV, 5))
    assert np.asarray(acts).shape == (1, 7)
    assert calls and all(c == (0.7, 50, 1.0) for c in calls), calls
    del calls[:]
    m.inference_action(T(g["decode_prompt"]), T(g["images"][:1]), dict(args, top_k=3), generator=gen(DEV, 5))
    assert calls and all(c == (0.7, 3, 1.0) for c in calls), calls


def test_no_aten_sampling_on_the_path(lm, monkeypatch):
    g, m = lm

    def refuse(*a, **k):
        raise AssertionError("ATen sampling arithmetic on the decode path")

    monkeypatch.setattr(torch, "softmax", refuse)
    monkeypatch.setattr(torch, "multinomial", refuse)
    prompt = T(g["decode_prompt"])
    seq = m.generate(prompt, images=T(g["images"][:1]), max_new_tokens=N_NEW, do_sample=True, temperature=0.7, top_k=50,
                     generator=gen(DEV, 3))
    assert seq.shape[1] == prompt.shape[1] + N_NEW
    seq = m.generate(prompt, images=T(g["images"][:1]), max_new_tokens=2, do_sample=True)          # no filter, no generator
    assert seq.shape[1] == prompt.shape[1] + 2
