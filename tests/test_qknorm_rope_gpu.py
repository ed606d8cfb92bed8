"""dxa_qknorm_rope_split / dxa_qknorm_rope_merge (Qwen3's per-head RMSNorm of q and k inside the RoPE / split pass) against a float64
torch restatement of HF:qwen3/modeling_qwen3.py: norm -> weight -> rotate-half, its backward through autograd.

Bounds.  fp32: the band of the existing RMSNorm kernel tests (tests/test_kernels_gpu.py: rtol 1e-5 + atol 1e-5 forward, 2 x that atol
for dx, atol * sqrt(number of summed terms) for dw) — tighter than a 1e-4 rtol, and the one those kernels already answer to.  rstd is
an fp32 quantity whatever the tensors' dtype, so it is held to the fp32 band in both.  bf16: the SAME formula evaluated by torch in
bf16 (HF's cast order: statistics in fp32, cast, times the weight; cos / sin cast to bf16; its autograd for the backward) is measured
against the float64 one as a max-norm ratio, and the kernel is allowed twice that distance (the rule of tests/test_lm_real_gpu.py).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K

DEV = "cuda"
EPS = 1e-6
HEADS = [(4, 2), (7, 1), (2, 2)]
ROWS = [(1, 1), (1, 3), (3, 11)]          # B x S = 1, 3, 33 tokens; 33 tokens are more than one 256-thread workgroup at every D
N_POS = 40


def _randn(shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def _tables(n, D, theta=1e6):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    fr = torch.arange(n, dtype=torch.float32)[:, None] * inv[None]
    return fr.cos().to(DEV).contiguous(), fr.sin().to(DEV).contiguous()


def _formula(qkv, wq, wk, cos_rows, sin_rows, eps, B, S, Hq, Hkv, D, stat_dtype):
    """q, k, v head-major and rstd [B*S, Hq+Hkv] in qkv's dtype, statistics in stat_dtype (HF Qwen3RMSNorm + apply_rotary_pos_emb)"""
    x = qkv.view(B, S, Hq + 2 * Hkv, D)
    cos = torch.cat([cos_rows, cos_rows], -1).to(qkv.dtype).view(B, S, 1, D)
    sin = torch.cat([sin_rows, sin_rows], -1).to(qkv.dtype).view(B, S, 1, D)

    def norm(t, w):
        tf = t.to(stat_dtype)
        rstd = torch.rsqrt(tf.pow(2).mean(-1, keepdim=True) + eps)
        return w * (tf * rstd).to(t.dtype), rstd.squeeze(-1)

    def rope(t):
        return t * cos + torch.cat([-t[..., D // 2:], t[..., :D // 2]], -1) * sin

    qn, rq = norm(x[:, :, :Hq], wq)
    kn, rk = norm(x[:, :, Hq:Hq + Hkv], wk)
    q, k, v = rope(qn).transpose(1, 2), rope(kn).transpose(1, 2), x[:, :, Hq + Hkv:].transpose(1, 2)
    return q, k, v, torch.cat([rq, rk], -1).reshape(B * S, Hq + Hkv)


def _with_grads(qkv, wq, wk, gq, gk, gv, *args):
    qkv, wq, wk = (t.detach().clone().requires_grad_(True) for t in (qkv, wq, wk))
    q, k, v, rstd = _formula(qkv, wq, wk, *args)
    ((q * gq).sum() + (k * gk).sum() + (v * gv).sum()).backward()
    return dict(q=q.detach(), k=k.detach(), v=v.detach(), rstd=rstd.detach(), dqkv=qkv.grad, dwq=wq.grad, dwk=wk.grad)


def _dist(a, b):
    """max-norm ratio (tests/helpers.rel_err)"""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def _band(out, ref, rtol, atol, what):
    err = (out.double() - ref.double()).abs()
    bad = err > atol + rtol * ref.double().abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} outside rtol {rtol} atol {atol:.2e}, max err {err.max().item():.3e}"


def _case(dtype, D, Hq, Hkv, B, S, use_pos, seed):
    M = B * S
    qkv = _randn((M, (Hq + 2 * Hkv) * D), seed, dtype)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    wq = (0.5 + torch.rand(D, generator=g)).to(DEV).to(dtype)
    wk = (0.5 + torch.rand(D, generator=g)).to(DEV).to(dtype)
    cos_t, sin_t = _tables(N_POS, D)
    pos = torch.randint(0, N_POS, (M,), generator=g).to(torch.int32).to(DEV) if use_pos else None
    rows = pos.long() if use_pos else torch.arange(S, device=DEV).repeat(B)
    gq, gk, gv = _randn((B, Hq, S, D), seed + 2, dtype), _randn((B, Hkv, S, D), seed + 3, dtype), _randn((B, Hkv, S, D), seed + 4, dtype)

    q, k, v, rstd = K.qknorm_rope_split(qkv, wq, wk, EPS, cos_t, sin_t, pos, B, S, Hq, Hkv, D)
    dqkv, part = K.qknorm_rope_merge(gq, gk, gv, qkv, rstd, wq, wk, cos_t, sin_t, pos, B, S, Hq, Hkv, D)
    dw = K.colsum(part)
    got = dict(q=q, k=k, v=v, rstd=rstd, dqkv=dqkv, dwq=dw[:D], dwk=dw[D:])

    geo = (B, S, Hq, Hkv, D)
    ref = _with_grads(qkv.double(), wq.double(), wk.double(), gq.double(), gk.double(), gv.double(),
                      cos_t[rows].double(), sin_t[rows].double(), EPS, *geo, torch.float64)
    tag = f"{dtype} D {D} heads {Hq}/{Hkv} tokens {B}x{S} pos {use_pos}"
    assert torch.equal(got["v"].double(), ref["v"]), f"{tag}: v is a copy"
    _band(got["rstd"], ref["rstd"], 1e-5, 1e-5, f"{tag}: rstd")
    if dtype == torch.float32:
        for name, atol in (("q", 1e-5), ("k", 1e-5), ("dqkv", 2e-5), ("dwq", 1e-5 * math.sqrt(M * Hq)), ("dwk", 1e-5 * math.sqrt(M * Hkv))):
            _band(got[name], ref[name], 1e-5, atol, f"{tag}: {name}")
        return
    t16 = _with_grads(qkv, wq, wk, gq, gk, gv, cos_t[rows], sin_t[rows], EPS, *geo, torch.float32)
    for name in ("q", "k", "dqkv", "dwq", "dwk"):
        mine, torch_bf16 = _dist(got[name], ref[name]), _dist(t16[name], ref[name])
        assert mine <= 2.0 * torch_bf16, (f"{tag}: {name}: kernel is {mine:.3e} from the float64 formula, torch's bf16 evaluation of it "
                                         f"{torch_bf16:.3e} (allowed: twice that)")


@pytest.mark.parametrize("D", [32, 64, 128, 256])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_forward_and_backward_match_the_float64_formula(dtype, D):
    seed = 100
    for Hq, Hkv in HEADS:
        for B, S in ROWS:
            for use_pos in (False, True):
                seed += 10
                _case(dtype, D, Hq, Hkv, B, S, use_pos, seed)


def _unit_rms_rows(n_rows, D, seed):
    """rows of multiples of 1/8 whose squares sum to EXACTLY D (D - 4 random entries, the rest from a four-square decomposition of what
    is missing): every value, square and partial sum is exact in bf16 / fp32, so mean(x^2) is exactly 1 in the kernel too"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = torch.empty(n_rows, D, dtype=torch.float64)
    for r in range(n_rows):
        while True:
            k = torch.randint(-10, 11, (D - 4,), generator=g)
            rest = 64 * D - int((k * k).sum())
            four = None
            lim = math.isqrt(rest)
            for a in range(lim, -1, -1):
                for b in range(min(a, math.isqrt(rest - a * a)), -1, -1):
                    for c in range(min(b, math.isqrt(rest - a * a - b * b)), -1, -1):
                        d2 = rest - a * a - b * b - c * c
                        d = math.isqrt(d2)
                        if d * d == d2 and d <= c:
                            four = (a, b, c, d)
                            break
                    if four:
                        break
                if four:
                    break
            if four and max(four) <= 96:
                break
        ks = torch.cat([k, torch.tensor(four)])[torch.randperm(D, generator=g)]
        out[r] = ks.double() / 8
        assert float((out[r] ** 2).sum()) == D
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unit_weights_on_unit_rms_rows_reduce_to_rope_split(dtype):
    """q_norm_w = k_norm_w = 1 and heads whose RMS is exactly 1 (eps = 0): the norm is the identity, so the pass must give what
    dxa_rope_split gives for the same input, within 1 ulp of the output's dtype.
    The tables are rounded to multiples of 2^-12 here: with inputs of at most 7 significant bits every product and sum of the fp32
    rotation is then exact, so the comparison does not depend on which of the two products each kernel's compiled code happens to
    fold into an FMA (with full-precision tables that choice alone moves a cancelling output by more than its own ulp, in either
    kernel); in bf16 both kernels round every product explicitly and agree anyway."""
    B, S, Hq, Hkv, D = 2, 5, 4, 2, 128
    M, HS = B * S, Hq + 2 * Hkv
    rows = _unit_rms_rows(M * HS, D, 7).view(M, HS * D)
    qkv = rows.to(DEV).to(dtype)
    assert torch.equal(qkv.double().cpu(), rows), "the rows are exact in this dtype"
    one = torch.ones(D, device=DEV, dtype=dtype)
    cos_t, sin_t = (torch.round(t * 4096) / 4096 for t in _tables(S, D))
    q, k, v, rstd = K.qknorm_rope_split(qkv, one, one, 0.0, cos_t, sin_t, None, B, S, Hq, Hkv, D)
    q0, k0, v0 = K.rope_split(qkv, cos_t, sin_t, None, B, S, Hq, Hkv, D)
    _band(rstd, torch.ones_like(rstd), 0, 2.0 ** -23, "rstd of unit-RMS rows")
    ulp = 2.0 ** -23 if dtype == torch.float32 else 2.0 ** -7          # spacing of the dtype at [1, 2), scaled by the binade below
    for a, b, name in ((q, q0, "q"), (k, k0, "k")):
        a, b = a.double(), b.double()
        spacing = ulp * torch.exp2(torch.floor(torch.log2(torch.maximum(a.abs(), b.abs()).clamp_min(1e-30))))
        assert bool(((a - b).abs() <= spacing).all()), f"{name}: max difference {(a - b).abs().max().item():.3e}"
    assert torch.equal(v, v0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_weight_gradient_is_bit_reproducible(dtype):
    B, S, Hq, Hkv, D = 3, 11, 7, 1, 64
    qkv = _randn((B * S, (Hq + 2 * Hkv) * D), 1, dtype)
    wq, wk = _randn((D,), 2, dtype), _randn((D,), 3, dtype)
    cos_t, sin_t = _tables(S, D)
    gq, gk, gv = _randn((B, Hq, S, D), 4, dtype), _randn((B, Hkv, S, D), 5, dtype), _randn((B, Hkv, S, D), 6, dtype)
    _, _, _, rstd = K.qknorm_rope_split(qkv, wq, wk, EPS, cos_t, sin_t, None, B, S, Hq, Hkv, D)
    runs = []
    for _ in range(2):
        dqkv, part = K.qknorm_rope_merge(gq, gk, gv, qkv, rstd, wq, wk, cos_t, sin_t, None, B, S, Hq, Hkv, D)
        runs.append((dqkv.clone(), part.clone(), K.colsum(part).clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert runs[0][2].abs().max().item() > 0
    # frozen norm weights: no partial sums are asked for, dqkv is the same
    dqkv, part = K.qknorm_rope_merge(gq, gk, gv, qkv, rstd, wq, wk, cos_t, sin_t, None, B, S, Hq, Hkv, D, want_dw=False)
    assert part is None and torch.equal(dqkv, runs[0][0])


def test_unsupported_head_dim_is_refused_before_any_launch():
    B, S, Hq, Hkv, D = 1, 3, 2, 1, 48
    qkv = _randn((B * S, (Hq + 2 * Hkv) * D), 1)
    w = torch.ones(D, device=DEV)
    cos_t, sin_t = _tables(S, D)
    with pytest.raises(L.DxaError, match="head_dim"):
        K.qknorm_rope_split(qkv, w, w, EPS, cos_t, sin_t, None, B, S, Hq, Hkv, D)
    q = torch.full((B, Hq, S, D), 7.0, device=DEV)
    k = torch.full((B, Hkv, S, D), 7.0, device=DEV)
    v = torch.full((B, Hkv, S, D), 7.0, device=DEV)
    rc = L.lib.dxa_qknorm_rope_split(qkv.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), w.data_ptr(), w.data_ptr(), EPS, None,
                                     cos_t.data_ptr(), sin_t.data_ptr(), None, B, S, Hq, Hkv, D, L.F32, None)
    assert rc < 0 and "head_dim" in L.last_error()
    rstd = torch.ones((B * S, Hq + Hkv), device=DEV)
    dqkv = torch.full_like(qkv, 7.0)
    rc = L.lib.dxa_qknorm_rope_merge(q.data_ptr(), k.data_ptr(), v.data_ptr(), qkv.data_ptr(), rstd.data_ptr(), w.data_ptr(),
                                     w.data_ptr(), dqkv.data_ptr(), None, cos_t.data_ptr(), sin_t.data_ptr(), None, B, S, Hq, Hkv, D,
                                     L.F32, None)
    assert rc < 0 and "head_dim" in L.last_error()
    assert L.lib.dxa_qknorm_rope_merge_blocks(B * S, Hq, Hkv, D, L.F32) < 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (q, k, v, dqkv)), "nothing was written"
