"""The GRPO kernels on the MI355X against fp64 arithmetic on the CPU of the SAME stored inputs, restated here: dxa_bin_logprob_fwd
(log-probability of the taken bin, entropy, logsumexp), dxa_bin_logprob_bwd (against autograd of log_softmax) and dxa_ppo_clip_fwd
(against autograd of the reference's clipped loss).

Bounds, from the count of fp32 roundings; u = 2^-24, Z = the row's largest |z|, z = x * inv_temperature with inv_temperature the
fp32 number the kernel is handed (the fp64 side uses that same number).  The kernels call expf and logf, whose documented error in
the HIP math library is at most 2 ulp and 1 ulp: 4u and 2u relative.
* z: one rounding, u Z absolute.  d = z - max: the two z errors and one rounding, at most 4 u Z.  e = expf(d): 4u + 4 u Z relative.
  s = sum e over NB positive terms, ceil(NB / 64) adds per lane and six butterfly levels: rho_s = u (4 + 4 Z + NB / 64 + 7) relative.
* lse = max + logf(s): rho_s absolute through the logarithm, 2 u log NB for logf, u |lse| for the add, u Z for the maximum:
  A_lse = u (11 + 5 Z + NB / 64 + 2 log NB + |lse|).
* logp = z[bin] - lse: A_lse + u (Z + |logp|).
* t = sum e z: every product e z carries e's error and two roundings, the sum the same adds as s; t / s adds rho_s and one rounding:
  at most Z u (25 + 8 Z + NB / 32) absolute.  entropy = lse - t / s: A_lse + Z u (25 + 8 Z + NB / 32) + u |entropy|.
* backward, element j: p = expf(z - lse) with the fp32 lse the forward stored: p (A_lse + u (4 + Z + |z - lse|)); g = coef gscale
  inv_temperature and the product g (onehot - p): four roundings of at most |g| each; a bf16 result is rounded once more, 2^-8
  relative (round to nearest with 8 significand bits, as fp32's u = 2^-24 with 24): |g| (p (A_lse + u (4 + Z + |z - lse|)) + 4 u) +
  2^-8 |result| [bf16].
* clipped loss, n tokens: ratio = expf(logp - old) is u |delta| + 4 u relative, a term -adv ratio two more roundings; a sum takes
  ceil(n / 1024) adds per thread, six butterfly levels and sixteen wave partials: sum |term| u (7 + |delta|max + ceil(n / 1024) + 22);
  the two counts are integers below 2^24: exact; coef: |coef| u (8 + |delta|).  Inputs keep every ratio 1e-3 away from the clip
  bounds (the fp32 ratio is within 1e-6 of the fp64 one), so both sides take the same branch and the clipped count is compared
  exactly; ratios exactly ON a bound are built from logp == old with a clip width of 0 (exp(0) = 1 = 1 + 0 in both arithmetics).
Each test prints the largest share of its bound that was used."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import kernels as K

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
U = 2.0 ** -24


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def inv32(temperature: float) -> float:
    return float(torch.tensor(1.0 / temperature, dtype=torch.float32))     # what ctypes hands the kernel


def strided(x_h, pad):
    """the [rows, NB] matrix as a view of a [rows, NB + pad] buffer on the device (NaN in the padding: never read)"""
    rows, NB = x_h.shape
    buf = torch.full((rows, NB + pad), float("nan"), dtype=x_h.dtype, device=DEV)
    buf[:, :NB] = x_h.to(DEV)
    return buf[:, :NB]


def fwd_reference(x_h, bins_h, temperature):
    z = x_h.double() * inv32(temperature)
    lse = torch.logsumexp(z, dim=-1)
    logp = torch.log_softmax(z, dim=-1).gather(-1, bins_h.clamp(0, x_h.shape[1] - 1).unsqueeze(-1)).squeeze(-1)
    ent = lse - (torch.softmax(z, dim=-1) * z).sum(-1)
    Z = z.abs().max(dim=-1).values
    NB = x_h.shape[1]
    a_lse = U * (11 + 5 * Z + NB / 64 + 2 * math.log(NB) + lse.abs())
    return z, lse, logp, ent, a_lse, a_lse + U * (Z + logp.abs()), a_lse + Z * U * (25 + 8 * Z + NB / 32) + U * ent.abs()


FWD_CASES = [(rows, NB, dtype, pad, temp, 1.0) for rows in (1, 6, 101) for NB in (1, 31, 255, 300) for dtype in (F32, BF)
             for pad, temp in ((0, 1.0), (8, 1.6))] + [(6, 255, F32, 0, 1.0, 80.0), (6, 255, BF, 8, 1.6, 80.0)]


@pytest.mark.parametrize("rows,NB,dtype,pad,temp,span", FWD_CASES)
def test_bin_logprob_forward(rows, NB, dtype, pad, temp, span):
    x_h = rnd(rows, NB, seed=rows + NB).to(dtype)
    if span != 1.0:                                                        # logits up to +-80: exp overflows without the max subtraction
        x_h = (x_h.float() / x_h.float().abs().max() * span).to(dtype)
    bins_h = torch.randint(0, NB, (rows,), generator=torch.Generator().manual_seed(1))
    x = strided(x_h, pad)
    assert x.stride(0) == NB + pad
    logp, ent, lse = K.bin_logprob_fwd(x, bins_h.to(DEV), temp)
    _, r_lse, r_logp, r_ent, b_lse, b_logp, b_ent = fwd_reference(x_h, bins_h, temp)
    shares = []
    for got, ref, bound in ((lse, r_lse, b_lse), (logp, r_logp, b_logp), (ent, r_ent, b_ent)):
        assert got.dtype == F32 and got.shape == (rows,)
        err = (got.double().cpu() - ref).abs()
        shares.append(float((err / bound).max()))
        assert (err <= bound).all()
    print(f"bin_logprob_fwd rows={rows} NB={NB} {dtype} ld={NB + pad} T={temp} span={span}: largest share of the bounds used "
          f"lse {shares[0]:.3f} logp {shares[1]:.3f} entropy {shares[2]:.3f}")
    again = K.bin_logprob_fwd(x, bins_h.to(DEV), temp)
    assert all(torch.equal(a, b) for a, b in zip(again, (logp, ent, lse)))                # two runs, the same bits


@pytest.mark.parametrize("dtype", [F32, BF])
def test_bin_out_of_range_gives_nan_and_leaves_the_other_rows_alone(dtype):
    rows, NB = 6, 31
    x_h = rnd(rows, NB, seed=4).to(dtype)
    bins_h = torch.randint(0, NB, (rows,), generator=torch.Generator().manual_seed(2))
    good = K.bin_logprob_fwd(x_h.to(DEV), bins_h.to(DEV), 1.6)
    bad_h = bins_h.clone()
    bad_h[1], bad_h[4] = NB, -1
    logp, ent, lse = K.bin_logprob_fwd(x_h.to(DEV), bad_h.to(DEV), 1.6)
    keep = torch.tensor([0, 2, 3, 5])
    assert bool(logp[[1, 4]].isnan().all()) and torch.equal(logp.cpu()[keep], good[0].cpu()[keep])
    assert torch.equal(ent, good[1]) and torch.equal(lse, good[2])         # the row's entropy does not depend on the bin


BWD_CASES = [(6, 31, F32, 0, 1.0), (6, 255, BF, 8, 1.6), (101, 300, F32, 8, 1.6), (101, 255, BF, 0, 1.0), (1, 1, F32, 0, 1.6)]


@pytest.mark.parametrize("rows,NB,dtype,pad,temp", BWD_CASES)
def test_bin_logprob_backward_against_autograd(rows, NB, dtype, pad, temp):
    x_h = rnd(rows, NB, seed=rows + NB, scale=2.0).to(dtype)
    bins_h = torch.randint(0, NB, (rows,), generator=torch.Generator().manual_seed(3))
    coef_h = rnd(rows, seed=5)
    coef_h[rows // 2] = 0.0                                                # a masked token: its row must come out as zeros
    gs_h = torch.tensor([0.37])
    x = strided(x_h, pad)
    bins, coef, gs = bins_h.to(DEV), coef_h.to(DEV), gs_h.to(DEV)
    _, _, lse = K.bin_logprob_fwd(x, bins, temp)
    out = K.bin_logprob_bwd(x, bins, lse, coef, gs, temp)
    assert out.dtype == dtype and out.shape == (rows, NB) and out.stride(0) == NB + pad
    # fp64 autograd of sum_r coef_r gscale logp_r
    x64 = x_h.double().requires_grad_(True)
    inv = inv32(temp)
    lp = torch.log_softmax(x64 * inv, dim=-1).gather(-1, bins_h.unsqueeze(-1)).squeeze(-1)
    (ref,) = torch.autograd.grad((lp * coef_h.double() * float(gs_h)).sum(), x64)
    z, r_lse, _, _, a_lse, _, _ = fwd_reference(x_h, bins_h, temp)
    g = (coef_h.double() * float(gs_h) * inv).abs().unsqueeze(-1)
    p = torch.softmax(z, dim=-1)
    Z = z.abs().max(dim=-1, keepdim=True).values
    bound = g * (p * (a_lse.unsqueeze(-1) + U * (4 + Z + (z - r_lse.unsqueeze(-1)).abs())) + 4 * U) + 1e-37
    if dtype == BF:
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)                    # the rounding acts on the fp32 result, not on ref
    err = (out.double().cpu() - ref).abs()
    print(f"bin_logprob_bwd rows={rows} NB={NB} {dtype} ld={NB + pad} T={temp}: largest share of the bound used {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert bool((out[rows // 2] == 0).all()) and (rows == 1 or bool((out != 0).any()))
    assert torch.equal(K.bin_logprob_bwd(x, bins, lse, coef, gs, temp), out)              # two runs, the same bits
    assert torch.equal(K.bin_logprob_bwd(x, bins, lse, coef, None, temp), K.bin_logprob_bwd(x, bins, lse, coef, torch.ones(1, device=DEV), temp))
    keep = x.clone()
    inplace = K.bin_logprob_bwd(x, bins, lse, coef, gs, temp, out=x)                      # in place: the same bits
    assert inplace.data_ptr() == x.data_ptr() and torch.equal(x, out) and not torch.equal(x, keep)
    # a zero-coef row is zeros whatever its logits and lse hold
    x2 = keep.clone()
    x2[rows // 2] = float("nan")
    assert bool((K.bin_logprob_bwd(x2, bins, lse, coef, gs, temp)[rows // 2] == 0).all())


def clip_case(n, seed, lo, hi, on_bound=False):
    """inputs whose fp64 ratio keeps 1e-3 (relative) away from both bounds; every fifth advantage is 0; ``on_bound``: every third
    token has logp == old (ratio exactly 1)"""
    old = rnd(n, seed=seed) - 2.0
    delta = rnd(n, seed=seed + 1, scale=0.3)
    for b in (lo, hi):
        near = ((delta.double().exp() - b).abs() < 2e-3 * b)
        delta[near] += 0.01
    logp = old + delta
    if on_bound:
        logp[::3] = old[::3]
    ratio = (logp.double() - old.double()).exp()
    ok = torch.minimum((ratio - lo).abs(), (ratio - hi).abs()) > 1e-3 * ratio
    assert bool((ok | (ratio == 1.0)).all())
    adv = rnd(n, seed=seed + 2)
    adv[::5] = 0.0
    mask = (torch.rand(n, generator=torch.Generator().manual_seed(seed + 3)) > 0.3).float()
    return logp, old, adv, mask


def clip_reference(logp, old, adv, mask, lo, hi, denom):
    lp = logp.double().requires_grad_(True)
    o, a, m = old.double(), adv.double(), mask.double()
    ratio = torch.exp(lp - o)
    pg1, pg2 = -a * ratio, -a * torch.clamp(ratio, lo, hi)
    terms = torch.max(pg1, pg2)
    cnt = float(m.sum())
    inv = (1.0 / denom) if denom is not None else (1.0 / cnt if cnt > 0 else 0.0)
    loss = (terms * m).sum() * inv
    (coef,) = torch.autograd.grad(loss, lp)
    sums = torch.stack([(terms * m).sum(), (torch.gt(pg2, pg1).double() * m).sum(), ((o - lp) * m).sum(), m.sum()]).detach()
    dmax = float((lp.detach() - o).abs().max())
    k = U * (7 + dmax + math.ceil(logp.numel() / 1024) + 22)
    b_sums = torch.stack([(terms.detach().abs() * m).sum() * k, torch.tensor(0.0, dtype=torch.float64),
                          ((o - lp.detach()).abs() * m).sum() * k, torch.tensor(0.0, dtype=torch.float64)])
    return loss.detach(), sums, coef, b_sums, coef.abs() * U * (8 + dmax) + 1e-37, inv


@pytest.mark.parametrize("n", [1, 7, 1500])
@pytest.mark.parametrize("clip_low,clip_high,on_bound", [(0.2, 0.28, False), (0.2, 0.0, True), (0.0, 0.28, True)])
@pytest.mark.parametrize("denom", [None, 18.0])
def test_ppo_clip_forward_against_autograd(n, clip_low, clip_high, on_bound, denom):
    lo, hi = float(torch.tensor(1.0) - torch.tensor(clip_low)), float(torch.tensor(1.0) + torch.tensor(clip_high))     # the kernel's fp32 bounds
    logp, old, adv, mask = clip_case(n, 10 * n, lo, hi, on_bound)
    if n == 1:
        mask[:] = 1.0
    r_loss, r_sums, r_coef, b_sums, b_coef, inv = clip_reference(logp, old, adv, mask, lo, hi, denom)
    args = [t.to(DEV) for t in (logp, old, adv)]
    loss, sums, coef = K.ppo_clip_fwd(*args, mask.to(DEV), clip_low, clip_high, denom)
    e_sums = (sums.double().cpu() - r_sums).abs()
    e_coef = (coef.double().cpu() - r_coef).abs()
    e_loss = abs(float(loss) - float(r_loss))
    b_loss = float(b_sums[0]) * inv + 2 * U * abs(float(r_loss))
    share = max(float((e_sums[[0, 2]] / b_sums[[0, 2]].clamp_min(1e-300)).max()), float((e_coef / b_coef).max()), e_loss / max(b_loss, 1e-300))
    print(f"ppo_clip_fwd n={n} clip=({clip_low}, {clip_high}) on_bound={on_bound} denom={denom}: clipped {int(sums[1])} of {int(sums[3])}, "
          f"largest share of a bound used {share:.3f}")
    assert sums[1] == r_sums[1] and sums[3] == r_sums[3] == mask.sum()                   # the counts: exact
    assert (e_sums <= b_sums).all() and (e_coef <= b_coef).all() and e_loss <= b_loss
    assert bool((coef.cpu()[mask == 0] == 0).all())
    if on_bound and n > 1:
        on = (logp == old) & (mask > 0) & (adv != 0)
        assert bool(on.any()) and torch.equal(coef.cpu()[on], (-adv[on]) * torch.tensor(inv, dtype=torch.float64).float())   # full gradient on the bound: -adv * 1 * inv
    l2, s2, c2 = K.ppo_clip_fwd(*args, mask.to(DEV), clip_low, clip_high, denom)
    assert torch.equal(l2, loss) and torch.equal(s2, sums) and torch.equal(c2, coef)      # two runs, the same bits
    for m2 in (mask.to(torch.uint8), mask.bool()):                                        # the mask as bytes: the same bits
        l3, s3, c3 = K.ppo_clip_fwd(*args, m2.to(DEV), clip_low, clip_high, denom)
        assert torch.equal(l3, loss) and torch.equal(s3, sums) and torch.equal(c3, coef)


@pytest.mark.parametrize("denom", [None, 18.0])
def test_ppo_clip_with_an_empty_mask_and_non_finite_masked_tokens(denom):
    n = 7
    logp, old, adv, mask = clip_case(n, 3, 0.8, 1.28)
    zero = torch.zeros(n)
    loss, sums, coef = K.ppo_clip_fwd(logp.to(DEV), old.to(DEV), adv.to(DEV), zero.to(DEV), 0.2, 0.28, denom)
    assert float(loss) == 0 and bool((sums == 0).all()) and bool((coef == 0).all())
    # a masked token whose log-prob is NaN (an out-of-range bin) changes nothing
    mask[:] = 1.0
    mask[2] = 0.0
    base = K.ppo_clip_fwd(logp.to(DEV), old.to(DEV), adv.to(DEV), mask.to(DEV), 0.2, 0.28, denom)
    logp[2] = float("nan")
    got = K.ppo_clip_fwd(logp.to(DEV), old.to(DEV), adv.to(DEV), mask.to(DEV), 0.2, 0.28, denom)
    assert all(torch.equal(a, b) for a, b in zip(got, base)) and float(got[2][2]) == 0
