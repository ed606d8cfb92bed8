"""The 256x256 ping-pong GEMM on v_mfma_f32_16x16x32_bf16 fragments, held EXACTLY: small-integer bf16 operands (values in
[-3, 3], K <= 4608) make every fp32 sum exact, so a misplaced 16x16 block, a wrong k-group pairing in the transposed reads or a
slab index slip shows as a wrong value, never as a rounding difference.  Outputs are compared with torch.equal against the fp64
product (bf16 outputs: the fp64 value rounded once, as the epilogue rounds its exact fp32 sum)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K

DEV = "cuda"


def ints(*shape, seed, lo=-3, hi=3, dtype=torch.bfloat16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype).to(DEV)


def operands(lay, M, N, Kd, seed):
    if lay == "nt":
        a, b = ints(M, Kd, seed=seed), ints(N, Kd, seed=seed + 1)
        return a, b, a.double() @ b.double().t(), K.mm_nt
    if lay == "nn":
        a, b = ints(M, Kd, seed=seed), ints(Kd, N, seed=seed + 1)
        return a, b, a.double() @ b.double(), K.mm_nn
    a, b = ints(Kd, M, seed=seed), ints(Kd, N, seed=seed + 1)
    return a, b, a.double().t() @ b.double(), K.mm_tn


def bf(x):
    return x.float().to(torch.bfloat16)


# (layout, M, N, K): the decoder's real shapes (M = 4592 tokens; the 256-CU round leaves a tail cut along K), ragged M / N, TN with
# K % 64 != 0, and NT shapes the dispatcher gives the 256-row ping-pong kernel (M > 1024, 256-row tiles no worse than 192-row ones)
CASES = [("nt", 4592, 4608, 3584), ("nt", 4592, 3584, 3584), ("nt", 1794, 520, 320), ("nt", 1536, 2048, 4608),
         ("nn", 4592, 3584, 4608), ("nn", 1000, 520, 1024), ("nn", 300, 264, 64),
         ("tn", 4608, 3584, 4592), ("tn", 520, 264, 1000), ("tn", 300, 136, 70), ("tn", 2304, 1024, 4112)]


@pytest.mark.parametrize("case", CASES)
def test_lean_bf16_out_with_bias_and_residual_is_exact(case):
    lay, M, N, Kd = case
    a, b, ref, fn = operands(lay, M, N, Kd, 11)
    bias, res = ints(N, seed=13, lo=-40, hi=40), ints(M, N, seed=14, lo=-40, hi=40)
    out = fn(a, b, bias=bias, residual=res)
    want = bf(ref + bias.double() + res.double())
    assert torch.equal(out, want), f"{case}: {(out != want).sum().item()} of {out.numel()} outputs differ"
    assert torch.equal(out, fn(a, b, bias=bias, residual=res))                       # run to run


@pytest.mark.parametrize("case", CASES)
def test_lean_f32_accumulate_mirror_sumsq_is_exact(case):
    lay, M, N, Kd = case
    a, b, ref, fn = operands(lay, M, N, Kd, 21)
    c0 = ints(M, N, seed=23, lo=-100, hi=100, dtype=torch.float32)
    out = c0.clone()
    mirror = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    part = torch.full((K.gemm_sumsq_slots(M, N),), float("nan"), device=DEV)
    fn(a, b, out=out, accumulate=True, mirror=mirror, sumsq=part)
    want = (ref + c0.double()).float()
    assert torch.equal(out, want), f"{case}: {(out != want).sum().item()} of {out.numel()} outputs differ"
    assert torch.equal(mirror, out.to(torch.bfloat16))
    ss = (want.double() ** 2).sum().item()
    assert abs(part.double().sum().item() - ss) <= 1e-5 * ss


@pytest.mark.parametrize("M,N,K1,K2", [(3584, 1024, 2296, 2296), (520, 264, 1000, 70)])
def test_tn_two_segments_is_exact(M, N, K1, K2):
    a, b, a2, b2 = ints(K1, M, seed=31), ints(K1, N, seed=32), ints(K2, M, seed=33), ints(K2, N, seed=34)
    out = torch.empty(M, N, device=DEV)
    K.mm_tn(a, b, out=out, a2=a2, b2=b2)
    want = (torch.cat([a, a2]).double().t() @ torch.cat([b, b2]).double()).float()
    assert torch.equal(out, want)


@pytest.mark.parametrize("M,N,Kd", [(1794, 1030, 320), (4592, 3584, 3584)])
def test_generic_epilogue_aux_and_ragged_n_is_exact(M, N, Kd):
    """NT off the lean path: an aux output (pre-activation) and / or a column count that is no multiple of 8"""
    a, b, ref, _ = operands("nt", M, N, Kd, 41)
    bias, res = ints(N, seed=43, lo=-40, hi=40), ints(M, N, seed=44, lo=-40, hi=40)
    aux = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    out = K.mm_nt(a, b, bias=bias, residual=res, aux_out=aux)
    pre = ref + bias.double()
    assert torch.equal(aux, bf(pre))
    assert torch.equal(out, bf(pre + res.double()))
    out32 = torch.empty(M, N, device=DEV)
    K.mm_nt(a, b, out=out32, bias=bias, aux_out=torch.empty(M, N, device=DEV))
    assert torch.equal(out32, pre.float())


def test_nn_mulgrad_epilogue_is_exact():
    """NN bf16 with the activation-gradient epilogue (ReLU: the gradient factor is 0 or 1)"""
    M, N, Kd = 4592, 3584, 4608
    a, b, ref, _ = operands("nn", M, N, Kd, 51)
    g = ints(M, N, seed=53, lo=-2, hi=2)
    out = K.mm_nn(a, b, mulgrad=g, act=L.ACT_RELU)
    want = bf(ref * (g.double() > 0))
    assert torch.equal(out, want)


def test_fp32_epilogue_operands_are_exact():
    """bf16 operands, fp32 output, fp32 bias / residual (the action head's split-bf16 products)"""
    M, N, Kd = 4592, 1024, 1536
    a, b, ref, _ = operands("nt", M, N, Kd, 61)
    bias, res = ints(N, seed=63, lo=-40, hi=40, dtype=torch.float32), ints(M, N, seed=64, lo=-40, hi=40, dtype=torch.float32)
    out = torch.empty(M, N, device=DEV)
    K.mm_nt(a, b, out=out, bias=bias, residual=res, epi_f32=True)
    assert torch.equal(out, (ref + bias.double() + res.double()).float())
    aux = torch.empty(M, N, device=DEV)
    K.mm_nt(a, b, out=out, bias=bias, aux_out=aux, epi_f32=True)
    assert torch.equal(aux, (ref + bias.double()).float())


@pytest.mark.parametrize("M,F_,Kd", [(4592, 18944, 3584), (1794, 1032, 320)])
def test_fused_swiglu_pre_activations_are_exact(M, F_, Kd):
    """FUSE = 1: the tile's gate / up columns come from the two halves of B; the stored pre-activations are the exact product"""
    x, w = ints(M, Kd, seed=71), ints(2 * F_, Kd, seed=72)
    assert K.swiglu_gemm_supported(x, w, keep_pre=False)
    out, pre = K.mm_nt_swiglu(x, w, keep_pre=True)
    want = bf(x.double() @ w.double().t())
    assert torch.equal(pre, want)
    assert torch.equal(out, K.mm_nt_swiglu(x, w, keep_pre=False)[0])
