"""The bf16 one-launch DiT sampler with several requests in the launch (csrc/dit_fused.hip, request groups; K.dit_sample_bf16_batched_fwd).

The main handle is exact: a group walks the instruction sequence of a single launch on its own arrays, so request g of a G-request
launch must have the BITS K.dit_sample_bf16_fwd gives on that request alone.  G = 2 catches a wrong group stride, odd G and G = 5 an
overlap of two groups' workspaces or split-K tile counters, T1 = 5 a row mask taken from G * M instead of M.  Inputs follow the recipe
of tests/test_kernels_gpu.py::test_dit_sample_bf16_operands, with x0, z_emb (and keys / values) different per request."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K

from tests.test_kernels_gpu import DEV, _dit_sampler_restated, _dit_weights, rnd

A = 7
GMAX = 5
SHAPES = [(128, 2, 512, 2, 3, True), (192, 3, 768, 3, 4, False), (768, 12, 3072, 2, 2, True)]
PER_SHAPES = [(128, 2, 512, 2, 3, True), (192, 3, 768, 3, 4, False)]


@functools.lru_cache(maxsize=None)
def _case(cfg, T1, P):
    """inputs of GMAX requests and the single-launch result of each (computed once, never modified)"""
    H, heads, I, depth, steps, use_cfg = cfg
    T, Ng = T1 - 1, (2 if use_cfg else 1)
    ws, table = _dit_weights(H, I, depth, seed0=350 if P else 150, per=P > 0)
    x0 = rnd(GMAX, T, A, seed=7)
    ze = rnd(GMAX, Ng, H, seed=8, scale=0.5)
    te, pos = rnd(steps, H, seed=9, scale=0.5), rnd(T1, H, seed=10, scale=0.1)
    xw, xb, fw, fb = rnd(H, A, seed=11, scale=0.3), rnd(H, seed=12, scale=0.1), rnd(A, H, seed=13, scale=H ** -0.5), rnd(A, seed=14, scale=0.1)
    kv = rnd(depth, GMAX, Ng, P, 2, H, seed=15, scale=1.0) if P else None
    ab = torch.linspace(0.05, 0.95, steps + 1, device=DEV, dtype=torch.float64)
    coef = torch.zeros(steps, 4, device=DEV)
    coef[:, 0] = (1.0 / ab[:-1]).sqrt().float(); coef[:, 1] = (1.0 / ab[:-1] - 1.0).sqrt().float(); coef[:, 2] = ab[1:].float()
    arena, ptab = K.dit_bf16_pack(table, depth, H, I, per=P > 0)
    shared = (te, pos, xw, xb, fw, fb, coef)
    tail = (ptab, depth, T1, H, heads, I, 1e-6)
    singles = []
    for g in range(GMAX):
        kw = {"per_kv": kv[:, g].contiguous()} if P else {}
        singles.append(K.dit_sample_bf16_fwd(x0[g:g + 1].clone(), ze[g].contiguous(), *shared, 1, use_cfg, 1.5, *tail, **kw))
        assert not K.dit_blocks_timed_out()
    return dict(ws=ws, keep=(table, arena), x0=x0, ze=ze, kv=kv, shared=shared, tail=tail, use_cfg=use_cfg, Ng=Ng, heads=heads,
                singles=torch.cat(singles, 0))


def _batched(c, G, x0=None):
    x = (c["x0"] if x0 is None else x0)[:G].clone()
    kw = {"per_kv": c["kv"][:, :G].contiguous()} if c["kv"] is not None else {}
    out = K.dit_sample_bf16_batched_fwd(x, c["ze"][:G].contiguous(), *c["shared"], c["use_cfg"], 1.5, *c["tail"], **kw)
    assert out is x
    assert not K.dit_blocks_timed_out()
    return out


def _check_groups_equal_singles(c, G, what):
    out = _batched(c, G)
    again = _batched(c, G)
    assert torch.isfinite(out).all()
    for g in range(G):
        assert torch.equal(out[g], c["singles"][g]), f"{what}: request {g} of {G} differs from its single launch by " \
            f"{float((out[g] - c['singles'][g]).abs().max()):.3e}"
    assert torch.equal(out, again), f"{what}: G={G} not run-to-run identical"


@pytest.mark.parametrize("G", [1, 2, 3, 5])
@pytest.mark.parametrize("T1", [17, 5])
@pytest.mark.parametrize("cfg", SHAPES)
def test_each_group_has_the_bits_of_its_single_launch(cfg, T1, G):
    H, heads, I = cfg[:3]
    assert K.dit_sample_bf16_groups_supported(G, 2 if cfg[5] else 1, T1, H, heads, I)
    _check_groups_equal_singles(_case(cfg, T1, 0), G, f"{cfg} T1={T1}")


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("P", [64, 128])
@pytest.mark.parametrize("cfg", PER_SHAPES)
def test_each_group_has_the_bits_of_its_single_launch_with_perceptual_attention(cfg, P, G):
    H, heads, I = cfg[:3]
    assert K.dit_sample_bf16_groups_supported(G, 2 if cfg[5] else 1, 17, H, heads, I, P)
    _check_groups_equal_singles(_case(cfg, 17, P), G, f"{cfg} P={P}")


@pytest.mark.parametrize("P", [0, 64])
def test_groups_are_independent(P):
    """another x0 for one request changes that request's sample and not one bit of the others'"""
    c = _case(SHAPES[0], 17, P)
    base = _batched(c, 3)
    x0 = c["x0"].clone()
    x0[1] += 0.25
    moved = _batched(c, 3, x0=x0)
    assert torch.equal(moved[0], base[0]) and torch.equal(moved[2], base[2])
    assert not torch.equal(moved[1], base[1])


@pytest.mark.parametrize("P", [0, 128])
def test_three_groups_against_the_fp64_restatement(P):
    """arithmetic that is not under test: the float64 restatement of the sampler, request by request, with the bounds the
    single-request tests hold the same kernel to (tests/test_kernels_gpu.py: 6e-3 to the restatement of its bf16-operand arithmetic
    and 8e-3 to the exact sampler; 8e-3 and 1.2e-2 with perceptual attention)"""
    cfg = SHAPES[0]
    c = _case(cfg, 17, P)
    out = _batched(c, 3)
    te, pos, xw, xb, fw, fb, coef = c["shared"]
    b_same, b_exact = (8e-3, 1.2e-2) if P else (6e-3, 8e-3)
    for g in range(3):
        kv = c["kv"][:, g] if P else None
        args = (c["x0"][g:g + 1], c["ze"][g], te, pos, xw, xb, fw, fb, coef, c["ws"], c["Ng"], c["heads"], 1.5 if c["use_cfg"] else None)
        want, exact = _dit_sampler_restated(*args, True, kv=kv), _dit_sampler_restated(*args, False, kv=kv)
        scale = float(exact.abs().max())
        d_same, d_exact = float((out[g:g + 1].double() - want).abs().max()) / scale, float((out[g:g + 1].double() - exact).abs().max()) / scale
        print(f"batched sampler P={P} request {g}: vs its restatement {d_same:.2e}, vs exact {d_exact:.2e}")
        assert d_same < b_same, (g, d_same)
        assert d_exact < b_exact, (g, d_exact)


def test_argument_refusals():
    c = _case(SHAPES[0], 17, 0)
    H, heads, I, depth = SHAPES[0][:4]
    with pytest.raises(L.DxaError):                       # x holds 3 requests, z_emb 2
        K.dit_sample_bf16_batched_fwd(c["x0"][:3].clone(), c["ze"][:2].contiguous(), *c["shared"], True, 1.5, *c["tail"])
    T1 = 25                                               # 50 rows a group
    assert not K.dit_sample_bf16_groups_supported(2, 2, T1, H, heads, I)
    te, _, xw, xb, fw, fb, coef = c["shared"]
    with pytest.raises(L.DxaError):
        K.dit_sample_bf16_batched_fwd(rnd(2, T1 - 1, A, seed=1), c["ze"][:2].contiguous(), te, rnd(T1, H, seed=2), xw, xb, fw, fb, coef,
                                      True, 1.5, c["tail"][0], depth, T1, H, heads, I, 1e-6)
    with pytest.raises(L.DxaError):                       # more groups than the launch takes
        G = K.DIT_SAMPLE_MAX_GROUPS + 1
        K.dit_sample_bf16_batched_fwd(rnd(G, 16, A, seed=1), rnd(G, 2, H, seed=2), *c["shared"], True, 1.5, *c["tail"])
    assert not K.dit_blocks_timed_out()
    _check_groups_equal_singles(c, 2, "after the refusals")
