"""The OFT diffusion kernels on the MI355X against the torch composition each replaces, restated on the CPU:
dxa_noisy_embed_fwd/bwd (Linear(1, d) + GELU(erf) of the noisy-action projector and its weight gradients), dxa_diffusion_put_fwd/bwd
(state row, time row and projected rows written into / read out of the reserved block) and dxa_ddim_step_embed (the two ends of a
DDIM step).

Bounds.  fp32: elementwise 1e-5 of the tensor's largest magnitude (erff / expf against torch's versions; the sums of the backward
have at most 17 terms here).  bf16: one bf16 ulp of the largest magnitude.  The put kernels are copies: bit-equal.  The backward's
sums are bit-identical over two runs.  The largest figures observed stand in the docstrings of the tests.

Shapes: d 96 and 520 (a column loop with a tail: 65 groups of 8 / 130 of 4 for 256 threads, two column blocks in the backward's fp32
first stage); R 1, 6 and 17 (one more than the backward's row chunk of 16); one sample with off = -1."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import kernels as K

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
CASES = [(d, R, dtype) for d in (96, 520) for R in (1, 6, 17) for dtype in (F32, BF)]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bound(ref: torch.Tensor, dtype) -> float:
    m = float(ref.abs().max())
    if dtype == F32:
        return 1e-5 * m
    return 2.0 ** (math.floor(math.log2(m)) - 7)                  # one bf16 ulp at the largest magnitude


def worst(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double().cpu() - ref.double()).abs().max())


def embed_case(d, R, dtype, seed=0):
    a = rnd(R, seed=seed + 1, scale=1.5)
    w1 = rnd(d, 1, seed=seed + 2).to(dtype)
    b1 = rnd(d, seed=seed + 3, scale=0.5).to(dtype)
    return a, w1, b1


def embed_composition(a, w1, b1, dtype):
    """what the reference's projector computes in ``dtype`` on the CPU: act_fn1(fc1(noisy_actions))"""
    return torch.nn.functional.gelu(torch.nn.functional.linear(a.to(dtype).view(-1, 1), w1, b1))


@pytest.mark.parametrize("d,R,dtype", CASES)
def test_noisy_embed_forward(d, R, dtype):
    """observed: fp32 at most 2.1e-7 of the largest magnitude (bound 1e-5); bf16 at most 3.8e-6 absolute from torch's bf16 composition
    (one ulp at the largest magnitude: 1.6e-2 to 6.3e-2)"""
    a, w1, b1 = embed_case(d, R, dtype)
    h = K.noisy_embed_fwd(a.to(DEV), w1.to(DEV), b1.to(DEV), dtype)
    want = embed_composition(a, w1, b1, dtype)
    assert h.shape == (R, d) and h.dtype == dtype
    e, bd = worst(h, want), bound(want, dtype)
    print(f"noisy_embed_fwd d{d} R{R} {str(dtype)[6:]}: worst {e:.3e} (bound {bd:.3e})")
    assert e <= bd
    # fp32 weights under bf16 activations (the shadow-less store): the same values
    if dtype == BF:
        h2 = K.noisy_embed_fwd(a.to(DEV), w1.float().to(DEV), b1.float().to(DEV), dtype)
        assert torch.equal(h2, h)


@pytest.mark.parametrize("d,R,dtype", CASES)
def test_noisy_embed_backward(d, R, dtype):
    """dw1 / db1 against fp64 on the CPU: dpre = dh gelu'(pre) with pre as the kernel forms it (rounded to the dtype), dw1 = sum_r dpre
    a_r, db1 = sum_r dpre; in fp32 also against torch's autograd of the composition.  Observed: at most 1.6e-7 of the largest magnitude
    in fp32; bf16 (fp32 sums over bf16 inputs) at most 2.0e-6 absolute, far inside one bf16 ulp.  Two runs: the same bits; ``accumulate`` adds."""
    a, w1, b1 = embed_case(d, R, dtype, seed=10)
    dh = rnd(R, d, seed=14).to(dtype)
    ar = a.to(dtype).double()
    pre = (ar[:, None] * w1.double().view(1, d) + b1.double()).to(dtype).double() if dtype == BF else \
        (a[:, None] * w1.view(1, d) + b1).double()
    cdf = 0.5 * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi)
    dpre = dh.double() * (cdf + pre * pdf)
    want_w, want_b = (dpre * ar[:, None]).sum(0), dpre.sum(0)
    args = (dh.to(DEV), a.to(DEV), w1.to(DEV), b1.to(DEV))
    dw1, db1 = K.noisy_embed_bwd(*args)
    assert dw1.dtype == db1.dtype == F32 and dw1.shape == db1.shape == (d,)
    ew, eb = worst(dw1, want_w), worst(db1, want_b)
    print(f"noisy_embed_bwd d{d} R{R} {str(dtype)[6:]}: dw1 {ew:.3e} (bound {bound(want_w, dtype):.3e}) db1 {eb:.3e} "
          f"(bound {bound(want_b, dtype):.3e})")
    assert ew <= bound(want_w, dtype) and eb <= bound(want_b, dtype)
    if dtype == F32:
        w_, b_ = w1.clone().requires_grad_(True), b1.clone().requires_grad_(True)
        embed_composition(a, w_, b_, F32).backward(dh)
        assert worst(dw1, w_.grad.view(-1)) <= bound(want_w, F32) and worst(db1, b_.grad) <= bound(want_b, F32)
    dw2, db2 = K.noisy_embed_bwd(*args)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    base_w, base_b = rnd(d, seed=15).to(DEV), rnd(d, seed=16).to(DEV)
    acc_w, acc_b = base_w.clone(), base_b.clone()
    K.noisy_embed_bwd(*args, dw1=acc_w, db1=acc_b, accumulate=True)
    assert torch.equal(acc_w, base_w + dw1) and torch.equal(acc_b, base_b + db1)
    K.noisy_embed_bwd(*args, dw1=acc_w, db1=acc_b, accumulate=False)
    assert torch.equal(acc_w, dw1) and torch.equal(acc_b, db1)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("d,R,dtype", CASES)
def test_diffusion_put_forward_and_backward(d, R, dtype, skip):
    """copies: bit-equal to torch indexing.  Sample 1 has off = -1 and sample 3 a block one row too long: both are left alone by the
    forward and come back as zero rows from the backward"""
    B, Q = 4, R + 1 + skip
    Sq = Q + 3
    off_h = torch.tensor([2, -1, Sq - Q, Sq - Q + 1], dtype=torch.int64)
    off = off_h.to(DEV)
    ok = [b for b in range(B) if 0 <= int(off_h[b]) and int(off_h[b]) + Q <= Sq]
    assert ok == [0, 2]
    proj, time, state = rnd(B * R, d, seed=1).to(dtype), rnd(B, d, seed=2).to(dtype), rnd(B, d, seed=3).to(dtype)
    x0 = rnd(B, Sq, d, seed=4).to(dtype)
    x = K.diffusion_put_(x0.to(DEV), proj.to(DEV), time.to(DEV), off, state.to(DEV) if skip else None)
    want = x0.clone()
    for b in ok:
        o = int(off_h[b])
        if skip:
            want[b, o] = state[b]
        want[b, o + skip] = time[b]
        want[b, o + skip + 1:o + Q] = proj[b * R:(b + 1) * R]
    assert torch.equal(x.cpu(), want)
    dx = rnd(B, Sq, d, seed=5).to(dtype)
    dproj, dstate = K.diffusion_put_bwd(dx.to(DEV), off, R, bool(skip), want_dstate=True)
    want_p, want_s = torch.zeros(B * R, d, dtype=dtype), torch.zeros(B, d, dtype=dtype)
    for b in ok:
        o = int(off_h[b])
        want_p[b * R:(b + 1) * R] = dx[b, o + skip + 1:o + Q]
        want_s[b] = dx[b, o]
    assert torch.equal(dproj.cpu(), want_p)
    assert (dstate is None) == (skip == 0) and (dstate is None or torch.equal(dstate.cpu(), want_s))
    dproj2, none = K.diffusion_put_bwd(dx.to(DEV), off, R, bool(skip), want_dstate=False)
    assert none is None and torch.equal(dproj2, dproj)


@pytest.mark.parametrize("d,dtype", [(d, t) for d in (96, 520) for t in (F32, BF)])
def test_ddim_step_embed(d, dtype):
    """x against a float64 evaluation of the step on inputs that land below, inside and above the clamp (observed: at most 7.2e-8 absolute,
    6e-8 of the largest magnitude); the time row bit-equal; the operand bit-equal to dxa_noisy_embed_fwd on the new x; the rows of the suffix
    behind the time row untouched; the null-eps form leaves x untouched"""
    n = 17
    c0, c1, c2, c3, clip = 1.5, 0.5, 0.8, 0.6, 1.0
    x_h = torch.tensor([-3.0, 3.0, 0.2, -0.6, 0.66, -0.67, 1.0, -1.0, 0.0] + [0.1 * i - 0.4 for i in range(8)])
    eps_h = rnd(n, seed=21).to(dtype)
    x0 = c0 * x_h.double() - c1 * eps_h.double()
    assert (x0 < -clip).any() and (x0 > clip).any() and ((x0 > -clip) & (x0 < clip)).any()
    want_x = c2 * x0.clamp(-clip, clip) + c3 * eps_h.double()
    _, w1, b1 = embed_case(d, n, dtype, seed=30)
    trow = rnd(d, seed=22).to(dtype)
    w1d, b1d, trowd = w1.to(DEV), b1.to(DEV), trow.to(DEV)

    def run(eps):
        x = x_h.to(DEV)
        suffix = torch.full((1 + n, d), 7.0, dtype=dtype, device=DEV)
        h = torch.empty((n, d), dtype=dtype, device=DEV)
        K.ddim_step_embed_(eps, x, (c0, c1, c2, c3), clip, trowd, w1d, b1d, suffix, h)
        assert torch.equal(suffix[0].cpu(), trow) and bool((suffix[1:] == 7.0).all())
        assert torch.equal(h, K.noisy_embed_fwd(x, w1d, b1d, dtype))
        want_h = embed_composition(x.cpu(), w1, b1, dtype)
        assert worst(h, want_h) <= bound(want_h, dtype)
        return x

    x = run(eps_h.to(DEV))
    e = worst(x, want_x)
    print(f"ddim_step_embed d{d} {str(dtype)[6:]}: x worst {e:.3e} (bound {1e-5 * float(want_x.abs().max()):.3e})")
    assert x.dtype == F32 and e <= 1e-5 * float(want_x.abs().max())       # the sampler state is fp32 in either dtype
    assert torch.equal(run(None).cpu(), x_h)
    # clip <= 0 switches the clamp off
    x2 = x_h.to(DEV)
    K.ddim_step_embed_(eps_h.to(DEV), x2, (c0, c1, c2, c3), 0.0, trowd, w1d, b1d, torch.empty((1, d), dtype=dtype, device=DEV),
                       torch.empty((n, d), dtype=dtype, device=DEV))
    assert worst(x2, c2 * x0 + c3 * eps_h.double()) <= 1e-5 * float((c2 * x0).abs().max())
