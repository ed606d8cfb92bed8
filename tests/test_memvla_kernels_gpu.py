"""The MemVLA kernels (dexbotic_amd/csrc/memvla.hip) on the MI355X, each against a plain reference of the same operation:
dxa_dropout_mask bit for bit against the numpy Philox4x32-10 of tests/optim_mem_ref.py, dxa_bank_consolidate against float64
torch (similarities, first arg-max, exact merge, compaction), dxa_token_sum and dxa_add_rows against float64 / exact integer sums."""
import functools

import numpy as np
import pytest
import torch

from tests import optim_mem_ref as R
from tests.test_kernels_gpu import assert_close, rnd, tol_for

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ dropout mask
SEED, OFFSET = 0x123456789ABCDEF1, (5 << 32) | 77            # both with bits above 2^32
# dxa_dropout_mask launches min(ceil(quads / 256), 4096) blocks of 256 threads: 4 * 256 * 4096 elements fill the grid once, the
# 1201 elements above them (301 quads, the last one partial) are the second trip of the grid-stride loop
N_TWO_TRIPS = 4 * 256 * 4096 + 1201
PS = [0.0, 0.1, 0.5, 0.999]


@functools.lru_cache(maxsize=None)
def uniforms(n, seed, offset):
    return R.dropout_uniforms(n, seed, offset)


def want_mask(n, p, dtype, seed, offset):
    keep = torch.from_numpy(R.dropout_keep(n, p, seed, offset, u=uniforms(n, seed, offset))).to(DEV)
    scale = torch.tensor(float(R.keep_scale(p)), dtype=torch.float32, device=DEV).to(dtype)
    return torch.where(keep, scale, torch.zeros((), dtype=dtype, device=DEV)), keep, scale


def draw(n, p, dtype, seed, offset, pad=8):
    """the C entry on the first n elements of a NaN-filled buffer -> (mask [n], the pad elements behind it)"""
    buf = torch.full((n + pad,), float("nan"), dtype=dtype, device=DEV)
    L.check(L.lib.dxa_dropout_mask(buf.data_ptr(), n, float(p), seed, offset, K.dt(buf), K._stream()), "dxa_dropout_mask")
    return buf[:n], buf[n:]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099, N_TWO_TRIPS])
def test_dropout_mask_equals_philox_reference(n):
    for dtype in DTYPES:
        for p in PS:
            got, behind = draw(n, p, dtype, SEED, OFFSET)
            want, keep, scale = want_mask(n, p, dtype, SEED, OFFSET)
            assert same_bits(got, want), f"n={n} p={p} {dtype}: {int((got != want).sum())} elements differ from the reference"
            assert bool(torch.isnan(behind).all()), "wrote past n"
            assert bool(((got == 0) | (got == scale)).all())
            if p == 0.0:
                assert bool((got == 1).all())
    if n == N_TWO_TRIPS:
        # the draw is what the reference's CPU test bounds: within 4 standard errors of 1 - p
        for p in (0.1, 0.5):
            rate = float(want_mask(n, p, torch.float32, SEED, OFFSET)[1].float().mean())
            assert abs(rate - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5


def test_dropout_mask_seed_and_offset():
    n, p = 4099, 0.5
    a, _ = draw(n, p, torch.float32, SEED, OFFSET)
    b, _ = draw(n, p, torch.float32, SEED, OFFSET)
    assert same_bits(a, b)                                           # same (seed, offset): the same mask
    for seed, offset in ((SEED, OFFSET + 1), (SEED, OFFSET + (1 << 32)), (SEED + 1, OFFSET), (SEED + (1 << 32), OFFSET)):
        c, _ = draw(n, p, torch.float32, seed, offset)
        assert same_bits(c, want_mask(n, p, torch.float32, seed, offset)[0])
        assert not same_bits(a, c)                                   # each 32-bit half of seed and offset reaches the generator


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_mask_wrapper_advances_offset(dtype):
    shape, p, seed = (3, 7, 11), 0.1, 0xABCDEF0123456789
    m1 = K.dropout_mask(shape, p, dtype, DEV, seed=seed)
    off1 = K._MASK_STATE["offset"]
    m2 = K.dropout_mask(shape, p, dtype, DEV, seed=seed)
    off2 = K._MASK_STATE["offset"]
    assert off2 == off1 + 1 and m1.shape == shape and m1.dtype == dtype
    assert not same_bits(m1, m2)                                     # successive masks of one seed differ
    n = m1.numel()
    assert same_bits(m1.reshape(-1), want_mask(n, p, dtype, seed, off1)[0])
    assert same_bits(m2.reshape(-1), want_mask(n, p, dtype, seed, off2)[0])


# ------------------------------------------------------------------------------------------------ bank consolidation
BANK_SHAPES = [(2, 1, 1), (3, 3, 63), (4, 5, 64), (5, 4, 65), (6, 7, 200), (4, 256, 32)]


def sims_ref(feat, length):
    """float64: sims[i] = mean_n dot / (max(|a|, 1e-8) max(|b|, 1e-8)) over neighbouring entries of the stored values"""
    f = feat[:length].double()
    a, b = f[:-1], f[1:]
    den = a.norm(dim=-1).clamp_min(1e-8) * b.norm(dim=-1).clamp_min(1e-8)
    return ((a * b).sum(-1) / den).mean(-1)


def consolidated_ref(feat, ts, length, j):
    """entries j and j + 1 merged (fp32 arithmetic on the stored values, rounded to the storage type: exact), the rest moved down"""
    merged = (0.5 * feat[j].float() + 0.5 * feat[j + 1].float()).to(feat.dtype)
    f = torch.cat([feat[:j], merged[None], feat[j + 2:length]])
    t = torch.cat([ts[:j], (0.5 * (ts[j] + ts[j + 1]))[None], ts[j + 2:length]])
    return f, t


def bank(length, N, D, dtype, seed, plant=None):
    """capacity length + 2; plant = i: entry i + 1 is entry i plus a small perturbation (cosine ~0.99, unrelated entries ~0)"""
    feat = rnd(length + 2, N, D, dtype=torch.float32, seed=seed)
    if plant is not None:
        feat[plant + 1] = feat[plant] + 0.1 * rnd(N, D, seed=seed + 1)
    ts = torch.tensor([float(2 ** i + 1) for i in range(length + 2)], device=DEV)      # distinct, every mean exact
    return feat.to(dtype).contiguous(), ts


def run_bank(feat, ts, length, fifo=False):
    f, t = feat.clone(), ts.clone()
    sims = torch.full((length + 1,), float("nan"), device=DEV)
    K.bank_consolidate(f, t, length, sims, fifo=fifo)
    return f, t, sims


def check_bank(feat, ts, length, j, what, margin=True):
    D = feat.shape[2]
    f, t, sims = run_bank(feat, ts, length)
    want = sims_ref(feat, length)
    rtol, atol = tol_for(torch.float32, D)
    assert_close(sims[:length - 1], want, rtol, atol, f"{what}: sims")
    assert bool(torch.isnan(sims[length - 1:]).all()), f"{what}: sims written past length - 1"
    if margin and length > 2:
        top = want.sort(descending=True).values
        assert int(want.argmax()) == j and float(top[0] - top[1]) > 10 * (atol + rtol), f"{what}: no margin for the planted pair"
    wf, wt = consolidated_ref(feat, ts, length, j)
    assert same_bits(f[:length - 1], wf), f"{what}: entries"
    assert same_bits(t[:length - 1], wt), f"{what}: timesteps"
    assert same_bits(f[length:], feat[length:]) and same_bits(t[length:], ts[length:]), f"{what}: rows beyond length changed"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("length,N,D", BANK_SHAPES)
def test_bank_consolidate_planted_pair(length, N, D, dtype):
    for j in sorted({0, (length - 2) // 2, length - 2}):             # the best pair first, in the middle, last
        feat, ts = bank(length, N, D, dtype, seed=700 + j, plant=j if D > 1 else None)      # (D = 1: the one pair of (2,1,1))
        check_bank(feat, ts, length, j, f"({length},{N},{D}) {dtype} pair {j}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("length,N,D", BANK_SHAPES[1:])
def test_bank_consolidate_tie_takes_first(length, N, D, dtype):
    """entries [A, A, A, ...]: sims[0] and sims[1] come from identical data, the first pair wins (the timesteps tell which)"""
    feat, ts = bank(length, N, D, dtype, seed=710)
    feat[1], feat[2] = feat[0], feat[0]
    _, _, sims = run_bank(feat, ts, length)
    assert sims[0].item() == sims[1].item() and bool((sims[2:length - 1] < sims[0] - 0.5).all())
    check_bank(feat, ts, length, 0, f"tie ({length},{N},{D}) {dtype}", margin=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bank_consolidate_zero_token(dtype):
    """a token that is all zeros in one entry contributes a cosine of 0 to both of its pairs, not NaN"""
    length, N, D = 4, 5, 64
    feat, ts = bank(length, N, D, dtype, seed=720, plant=2)
    feat[1, 2] = 0
    feat[0, 4], feat[1, 4] = 0, 0                                    # and a token that is zero on both sides of a pair
    _, _, sims = run_bank(feat, ts, length)
    assert bool(torch.isfinite(sims[:length - 1]).all())
    check_bank(feat, ts, length, 2, f"zero token {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("length,N,D", BANK_SHAPES)
def test_bank_consolidate_fifo(length, N, D, dtype):
    feat, ts = bank(length, N, D, dtype, seed=730, plant=0 if D > 1 else None)
    f, t, sims = run_bank(feat, ts, length, fifo=True)
    assert bool(torch.isnan(sims).all())                             # neither read (a NaN would win no comparison) nor written
    assert same_bits(f[:length - 1], feat[1:length]) and same_bits(t[:length - 1], ts[1:length])
    assert same_bits(f[length:], feat[length:]) and same_bits(t[length:], ts[length:])


# ------------------------------------------------------------------------------------------------ token_sum / add_rows
RS, NNS, CS = [1, 3], [1, 7, 300], [1, 255, 256, 257, 520]


def f32(x):
    return float(np.float32(x))


@pytest.mark.parametrize("C_", CS)
def test_token_sum(C_):
    for R_ in RS:
        for Nn in NNS:
            g = torch.Generator(device="cpu")
            g.manual_seed(800 + Nn)
            xi = torch.randint(-3, 4, (R_, Nn, C_), generator=g).to(DEV)
            what = f"token_sum R={R_} Nn={Nn} C={C_}"
            # fp32 on integers: the sum is exact, the scaled sum one fp32 multiply
            assert same_bits(K.token_sum(xi.float()), xi.sum(1).float()), what
            inv = torch.tensor(1.0 / Nn, dtype=torch.float32, device=DEV)
            assert same_bits(K.token_sum(xi.float(), scale=1.0 / Nn), xi.sum(1).float() * inv), what + " scaled"
            for scale in (1.0, 1.0 / Nn):
                xb = rnd(R_, Nn, C_, dtype=torch.bfloat16, seed=801)
                out = K.token_sum(xb, scale=scale)
                assert out.dtype == torch.bfloat16 and out.shape == (R_, C_)
                assert_close(out, xb.double().sum(1) * f32(scale), *tol_for(torch.bfloat16), what + " bf16")


@pytest.mark.parametrize("dtype", DTYPES)
def test_token_sum_no_tokens(dtype):
    """Nn = 0: zeros (an empty torch tensor has no data pointer, so the C entry is called with a valid one)"""
    R_, C_ = 3, 257
    x = torch.ones(8, dtype=dtype, device=DEV)
    out = torch.full((R_, C_), float("nan"), dtype=dtype, device=DEV)
    L.check(L.lib.dxa_token_sum(x.data_ptr(), out.data_ptr(), R_, 0, C_, 1.0, K.dt(x), K._stream()), "dxa_token_sum")
    assert bool((out == 0).all())


@pytest.mark.parametrize("C_", CS)
def test_add_rows(C_):
    for R_ in RS:
        for Nn in NNS:
            for alpha in sorted({1.0, 1.0 / Nn}):
                what = f"add_rows R={R_} Nn={Nn} C={C_} alpha={alpha}"
                x, g = rnd(R_, Nn, C_, seed=810), rnd(R_, C_, seed=811)
                a32 = torch.tensor(alpha, dtype=torch.float32, device=DEV)
                out = K.add_rows(x, g, Nn, alpha)
                assert out.shape == (R_, Nn, C_)
                assert_close(out, x + a32 * g[:, None, :], *tol_for(torch.float32), what)
                assert_close(out, x.double() + f32(alpha) * g.double()[:, None, :], *tol_for(torch.float32), what + " f64")
                # x = None: the broadcast alone, one fp32 multiply
                assert same_bits(K.add_rows(None, g, Nn, alpha), (a32 * g)[:, None, :].expand(R_, Nn, C_).contiguous() + 0.0), what
                xb, gb = x.to(torch.bfloat16), g.to(torch.bfloat16)
                ref = xb.double() + f32(alpha) * gb.double()[:, None, :]
                assert_close(K.add_rows(xb, gb, Nn, alpha), ref, *tol_for(torch.bfloat16), what + " bf16")
                assert_close(K.add_rows(None, gb, Nn, alpha), (f32(alpha) * gb.double())[:, None, :].expand(R_, Nn, C_),
                             *tol_for(torch.bfloat16), what + " bf16 broadcast")
