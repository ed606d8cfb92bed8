"""dxa_flow_suffix_in / dxa_flow_euler_tail (csrc/flow.hip) against an fp64 torch evaluation of their formulas, written out below, in
fp32 and bf16: every shape dense (ldx = n A, a prog_min tensor of its own) and packed (ldx = n A + 1, prog_min in the last column, the
sampler's layout), every sample with its own progress, time embedding and starting minimum, sentinel guards around everything the
kernels write."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DA_LIMIT = 8192
#          B  n   A   da    p
SHAPES = [(1, 1, 1, 64, 0), (1, 1, 1, 64, 1),          # a single row
          (2, 6, 8, 64, 1),                            # the DM0-prog fixture
          (3, 5, 7, 72, 1),                            # odd A; da a multiple of 8 but not of 64
          (2, 3, 5, 21, 1),                            # the scalar path
          (1, 50, 32, 1024, 1),                        # the production row
          (1, 2, 4, DA_LIMIT, 1)]                      # the da limit
GUARD, SENT = 64, 777.0                                # guard elements (a multiple of 16 bytes in both dtypes) and their value
U = 2.0 ** -24
EPS, DT = 1e-6, -0.1
_CASES = {}


def case(shape, dtype):
    """operands of one (shape, dtype), built once and never written: fp32 x / progress / starting minimum, everything else rounded
    to ``dtype``.  With B > 1 the last sample's starting minimum is far below anything a step produces, so it must survive."""
    key = (shape, dtype)
    if key not in _CASES:
        B, n, A, da, p = shape
        gen = torch.Generator(device="cpu").manual_seed(sum(v * 31 ** i for i, v in enumerate(shape)))
        r = lambda *s: torch.randn(*s, generator=gen)
        c = dict(x=r(B, n * A), progress=torch.rand(B, 1, generator=gen) + torch.arange(B)[:, None].float(),
                 te=r(B, da).to(dtype), w_in=(r(da, A) / math.sqrt(A)).to(dtype), b_in=(0.1 * r(da)).to(dtype),
                 w_p=r(da, 1).to(dtype), b_p=(0.1 * r(da)).to(dtype),
                 h=(r(B * (p + n), da) * (1 + torch.arange(B * (p + n))[:, None].float())).to(dtype), g=(1 + 0.1 * r(da)).to(dtype),
                 w_out=(r(A, da) / math.sqrt(da)).to(dtype), b_out=(0.1 * r(A)).to(dtype),
                 w_q=(r(1, da) / math.sqrt(da)).to(dtype), b_q=(0.1 * r(1)).to(dtype),
                 pm0=torch.tensor(([float("inf"), 1e3, 0.5e3][:B - 1] + [-1e3]) if B > 1 else [float("inf")])[:, None])
        _CASES[key] = {k: v.to(DEV) for k, v in c.items()}
    return _CASES[key]


def state_buffers(c, shape, packed):
    """-> (buf, x view [B, n A], prog_min view [B, 1], mbuf): x (and, packed, the running minimum behind each sample) inside a guarded
    buffer; dense: the minimum in a guarded buffer of its own, two elements apart"""
    B, n, A, da, p = shape
    ld = n * A + (1 if packed else 0)
    buf = torch.full((GUARD + B * ld + GUARD,), SENT, device=DEV)
    body = buf[GUARD:GUARD + B * ld].view(B, ld)
    x = body[:, :n * A]
    x.copy_(c["x"])
    if packed:
        pm, mbuf = body[:, n * A:], None
    else:
        mbuf = torch.full((GUARD + 2 * B + GUARD,), SENT, device=DEV)
        pm = mbuf[GUARD:GUARD + 2 * B].view(B, 2)[:, :1]
    pm.copy_(c["pm0"])
    return buf, x, pm, mbuf


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flow_suffix_in(shape, dtype, packed):
    """row 0 (p = 1): progress[b] w_p + b_p; rows p + i: W_in rnd(x[b, i]) + b_in; every row's second half: te[b].  The output is
    stored in compute dtype: the bounds of test_rmsnorm (tests/test_kernels_gpu.py), fp32 1e-5 / 1e-5, bf16 1/64 / 1e-2"""
    from dexbotic_amd import kernels as K
    B, n, A, da, p = shape
    c = case(shape, dtype)
    buf, x, pm, mbuf = state_buffers(c, shape, packed)
    prog = torch.full((B, 3), SENT, device=DEV)                  # progress with a stride of its own
    prog[:, 1:2] = c["progress"]
    rows = B * (p + n)
    obuf = torch.full((GUARD + rows * 2 * da + GUARD,), SENT, device=DEV, dtype=dtype)
    out = K.flow_suffix_in(x, c["te"], c["w_in"], c["b_in"], n, A, prog[:, 1:2] if p else None, c["w_p"] if p else None,
                           c["b_p"] if p else None, out=obuf[GUARD:GUARD + rows * 2 * da].view(rows, 2 * da))
    torch.cuda.synchronize()
    # ---- the formulas in fp64
    xr = c["x"].to(dtype).double().view(B, n, A)
    act = torch.einsum("ck,bik->bic", c["w_in"].double(), xr) + c["b_in"].double()
    if p:
        pr = (c["progress"].double() * c["w_p"].double().view(1, da) + c["b_p"].double())[:, None, :]
        act = torch.cat([pr, act], dim=1)
    want = act.reshape(rows, da)
    rtol, atol = (1e-5, 1e-5) if dtype == torch.float32 else (1.0 / 64, 1e-2)
    err = (out[:, :da].double() - want).abs()
    print(f"suffix_in {shape} {dtype} max err {err.max().item():.3e} (max |want| {want.abs().max().item():.3e})")
    assert bool((err <= atol + rtol * want.abs()).all())
    assert torch.equal(out[:, da:].view(B, p + n, da), c["te"][:, None, :].expand(B, p + n, da))
    # ---- nothing else was written
    assert bool((obuf[:GUARD] == SENT).all()) and bool((obuf[-GUARD:] == SENT).all())
    assert torch.equal(x, c["x"]) and torch.equal(pm, c["pm0"])
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flow_euler_tail(shape, dtype, packed):
    """y = h rsqrt(mean(h^2) + eps) g; action rows x[b, i] += dt (W_out y + b_out); progress row prog_min[b] = min(prog_min[b],
    w_q y + b_q).  The results are fp32 from the given operands, so they are compared with the fp64 evaluation of the same operands:
    rtol 1e-5 plus an absolute bound from the kernel's own summation of the dot product.  Lane l of a wave adds the products
    W[a, k] y[k] of its chunks l VEC + 64 VEC j in ascending order with fma, T = VEC ceil(da / (64 VEC)) serial terms, and the 64
    lanes are then added by a shuffle tree of log2(64) = 6 levels: every product passes through at most T + 6 fp32 additions whose
    partial sums are at most sum |terms|, each rounding at most 2^-24 of it:
        |error| <= (T + 6) 2^-24 (sum_k |W[a, k] y[k]| + |b|) |dt|                (no |dt| for the progress prediction).
    The roundings outside that summation (the statistics, the two products that form y, the bias add and the final fma) are each
    2^-24 relative to a quantity no larger than sum |terms| or the result and are left to rtol = 167 x 2^-24."""
    from dexbotic_amd import kernels as K
    B, n, A, da, p = shape
    c = case(shape, dtype)
    buf, x, pm, mbuf = state_buffers(c, shape, packed)
    K.flow_euler_tail_(c["h"], c["g"], c["w_out"], c["b_out"], x, n, EPS, DT, pm if p else None, c["w_q"] if p else None,
                       c["b_q"] if p else None)
    torch.cuda.synchronize()
    # ---- the formulas in fp64
    h = c["h"].double().view(B, p + n, da)
    y = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS) * c["g"].double()
    ya = y[:, p:]                                                         # the action rows: x has no slot for the progress row
    v = torch.einsum("ak,bik->bia", c["w_out"].double(), ya) + c["b_out"].double()
    want = c["x"].double().view(B, n, A) + DT * v
    vec = 1 if da % (8 if dtype == torch.bfloat16 else 4) else (8 if dtype == torch.bfloat16 else 4)
    serial = vec * math.ceil(da / (64 * vec))
    mag = torch.einsum("ak,bik->bia", c["w_out"].double().abs(), ya.abs()) + c["b_out"].double().abs()
    bound = (serial + 6) * U * mag * abs(DT)
    err = (x.double().view(B, n, A) - want).abs()
    print(f"euler_tail {shape} {dtype} x: max err {err.max().item():.3e}, max err / (bound + rtol |want|) "
          f"{(err / (bound + 1e-5 * want.abs())).max().item():.3f}")
    assert bool((err <= bound + 1e-5 * want.abs()).all())
    assert float((x != c["x"]).float().mean()) > 0.99                   # the bound is not met by standing still
    if p:
        yp = y[:, 0]
        e = (yp * c["w_q"].double()).sum(-1, keepdim=True) + c["b_q"].double()
        ebound = (serial + 6) * U * ((yp.abs() * c["w_q"].double().abs()).sum(-1, keepdim=True) + c["b_q"].double().abs())
        wantm = torch.minimum(c["pm0"].double(), e)
        k = B - 1 if B > 1 else 0                                          # the samples whose start lies above the prediction
        assert bool((e[:max(k, 1)] < c["pm0"][:max(k, 1)].double() - 1).all())
        if B > 1:                                                         # a lower start survives, bit for bit
            assert bool((e[k] > c["pm0"][k].double() + 1).all()) and torch.equal(pm[k], c["pm0"][k])
        merr = (pm.double() - wantm).abs()
        print(f"euler_tail {shape} {dtype} prog_min: max err {merr.max().item():.3e}")
        assert bool((merr <= ebound + 1e-5 * wantm.abs()).all())
    else:
        assert torch.equal(pm, c["pm0"])                                   # p = 0 leaves the running minimum alone
    # ---- nothing else was written
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())
    if mbuf is not None:
        assert bool((mbuf[:GUARD] == SENT).all()) and bool((mbuf[-GUARD:] == SENT).all())
        assert bool((mbuf[GUARD:GUARD + 2 * B].view(B, 2)[:, 1] == SENT).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_flow_euler_tail_a_nan_prediction_wins(dtype):
    """torch.min over the stacked steps propagates a NaN: a NaN in one sample's progress row makes that sample's minimum NaN, whatever
    it held, and leaves the other samples and every action alone"""
    from dexbotic_amd import kernels as K
    shape = (3, 5, 7, 72, 1)
    B, n, A, da, p = shape
    c = case(shape, dtype)
    clean = state_buffers(c, shape, True)
    K.flow_euler_tail_(c["h"], c["g"], c["w_out"], c["b_out"], clean[1], n, EPS, DT, clean[2], c["w_q"], c["b_q"])
    h = c["h"].clone()
    h[1 * (p + n), 3] = float("nan")                                        # sample 1's progress row
    buf, x, pm, _ = state_buffers(c, shape, True)
    K.flow_euler_tail_(h, c["g"], c["w_out"], c["b_out"], x, n, EPS, DT, pm, c["w_q"], c["b_q"])
    torch.cuda.synchronize()
    assert bool(pm[1].isnan().all()) and torch.equal(pm[[0, 2]], clean[2][[0, 2]]) and torch.equal(x, clean[1])
    assert float(pm[2]) == -1e3 and float(pm[0]) < 1e3
    # and it stays NaN through a later, finite step
    K.flow_euler_tail_(c["h"], c["g"], c["w_out"], c["b_out"], x, n, EPS, DT, pm, c["w_q"], c["b_q"])
    assert bool(pm[1].isnan().all()) and not bool(pm[[0, 2]].isnan().any())
