"""dxa_adarms_fwd / dxa_adarms_bwd / dxa_gated_residual_fwd / dxa_gated_residual_bwd (csrc/norm.hip): the adaptive RMSNorm and the gated
residual of the pi0.5 action expert against an fp64 torch evaluation of their formulas, written out below.

    r = x + branch * gate_prev[s]                      y = r * rsqrt(mean(r^2) + eps) * (1 + scale[s]) + shift[s]
    g = dy * (1 + scale[s])                            dr = rstd * (g - xh * mean(g * xh)) (+ residual)
    dscale[s] = sum_rows dy * xh    dshift[s] = sum_rows dy    dbranch = dr * gate_prev[s]    dgate_prev[s] = sum_rows dr * branch

Tolerances: test_rmsnorm's (tests/test_kernels_gpu.py) — fp32 rtol 1e-5 / atol 1e-5, bf16 1/64 / 1e-2, dx atol x 2, the per-sample
sums atol x sqrt(rows_per_sample).

Shapes (B, rows_per_sample, cols): (1, 1, 64) a single row; (3, 3, 64) a 4-row workgroup spans samples 0 and 1; (2, 50, 1024) the
production row (the bf16 register-resident path, 50 % 4 != 0); (2, 5, 20) 8-byte bf16 / 16-byte fp32 accesses; (2, 5, 21) an odd
width: the scalar path; (2, 6, 8200) bf16 rows above the register-resident path's 8192.  Every sample has a modulation of its own,
so a wrong sample index cannot pass; every gate lives inside a wider [B, 3 cols] tensor (stride != cols)."""
import math

import pytest
import torch

from dexbotic_amd import kernels as K

from .test_kernels_gpu import assert_close, rnd

pytestmark = pytest.mark.gpu
EPS = 1e-6
SHAPES = [(1, 1, 64), (3, 3, 64), (2, 50, 1024), (2, 5, 20), (2, 5, 21), (2, 6, 8200)]
DTYPES = [torch.float32, torch.bfloat16]


def tol(dtype):
    return (1e-5, 1e-5) if dtype == torch.float32 else (1.0 / 64, 1e-2)


# the path each width takes, as the docstring states it: bf16 forward kernel, then elements per access for bf16 and for fp32
PATHS = {64: ("adarms_fwd_fast_k", 8, 4), 1024: ("adarms_fwd_fast_k", 8, 4), 20: ("adarms_fwd_k", 4, 4), 21: ("adarms_fwd_k", 1, 1),
         8200: ("adarms_fwd_k", 8, 4)}


def assert_path(entry, dtype, shape, gated, **ops):
    """dxa_norm_plan of the call just made takes the path PATHS names for its width"""
    B, rps, d = shape
    fam, vb, vf = PATHS[d]
    bf = dtype == torch.bfloat16
    vec, T, g = (vb if bf else vf), ("bf16" if bf else "float"), ("true" if gated else "false")
    want = {"adarms_fwd": (f"adarms_fwd_fast_k<{g}>" if bf and fam == "adarms_fwd_fast_k" else f"adarms_fwd_k<{T},{vec},{g}>"),
            "adarms_bwd": f"adarms_bwd_k<{T},{vec},{g}>", "gated_residual_fwd": f"gated_residual_fwd_k<{T},{vec}>",
            "gated_residual_bwd": f"gated_residual_bwd_k<{T},{vec}>"}[entry]
    p = K.norm_plan(entry, dtype=1 if bf else 0, rows=B * rps, rows_per_sample=rps, cols=d, **ops)
    assert p["kernel"] == want and p["vec"] == vec, (p, want)
    if entry.endswith("_bwd"):
        assert p["kernel2"] == f"adarms_fold_k<{T}>" and p["grid"][:2] == (K.lib.dxa_adarms_bwd_groups(rps), B)


def per_row(t, rps):
    """[B, cols] per-sample vectors -> [B * rps, cols] fp64"""
    return t.double().repeat_interleave(rps, dim=0)


def make(shape, dtype, seed):
    B, rps, d = shape
    rows = B * rps
    x = rnd(rows, d, dtype=dtype, seed=seed)
    branch = rnd(rows, d, dtype=dtype, seed=seed + 1)
    # distinct per sample: sample b's modulation is offset by b
    mod = (0.5 * rnd(B, 3 * d, seed=seed + 2) + 0.25 * torch.arange(B, device=x.device)[:, None]).to(dtype)
    mod_prev = (0.5 * rnd(B, 3 * d, seed=seed + 3) - 0.25 * torch.arange(B, device=x.device)[:, None]).to(dtype)
    return x, branch, mod, mod_prev


def ref_fwd(x, mod, rps, branch=None, gate=None):
    d = x.shape[1]
    r = x.double() if branch is None else x.double() + branch.double() * per_row(gate, rps)
    rstd = torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + EPS)
    return r * rstd * (1 + per_row(mod[:, :d], rps)) + per_row(mod[:, d:2 * d], rps), r


def ref_bwd(dy, r, mod, rps, residual=None, branch=None, gate=None):
    B, d = mod.shape[0], r.shape[1]
    r, dy = r.double(), dy.double()
    rstd = torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + EPS)
    xh = r * rstd
    g = dy * (1 + per_row(mod[:, :d], rps))
    dr = rstd * (g - xh * (g * xh).mean(-1, keepdim=True))
    if residual is not None:
        dr = dr + residual.double()
    out = dict(dr=dr, dscale=(dy * xh).view(B, rps, d).sum(1), dshift=dy.view(B, rps, d).sum(1))
    if branch is not None:
        out["dbranch"] = dr * per_row(gate, rps)
        out["dgate"] = (dr * branch.double()).view(B, rps, d).sum(1)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_adarms_forward_with_and_without_the_fused_gated_add(dtype, shape):
    B, rps, d = shape
    rtol, atol = tol(dtype)
    x, branch, mod, mod_prev = make(shape, dtype, 100)
    y, rstd, r = K.adarms_fwd(x, mod, EPS)
    assert r is None
    assert_path("adarms_fwd", dtype, shape, False, x=x, mod=mod, y=y, rstd=rstd)
    yr, rr = ref_fwd(x, mod, rps)
    assert_close(y, yr, rtol, atol, "adarms fwd")
    assert_close(rstd[:, None], torch.rsqrt(rr.pow(2).mean(-1, keepdim=True) + EPS), 1e-5, 1e-6, "adarms rstd")
    gate = mod_prev[:, 2 * d:]                                   # inside the wider tensor: row stride 3 d
    assert gate.stride(0) == 3 * d
    y2, rstd2, r2 = K.adarms_fwd(x, mod, EPS, branch=branch, gate_prev=gate)
    assert_path("adarms_fwd", dtype, shape, True, x=x, x2=branch, gate=gate, gate_ld=3 * d, mod=mod, aux=r2, y=y2, rstd=rstd2)
    yr2, rr2 = ref_fwd(x, mod, rps, branch, gate)
    assert_close(r2, rr2, rtol, atol, "adarms fwd r")
    assert_close(y2, yr2, rtol, atol, "adarms fwd fused")
    # the same gate as a tensor of its own (stride = cols): the same bits
    y3, rstd3, r3 = K.adarms_fwd(x, mod, EPS, branch=branch, gate_prev=gate.contiguous())
    assert torch.equal(y3, y2) and torch.equal(r3, r2) and torch.equal(rstd3, rstd2)
    # the fused launch against the two-step composition on the rounded r: the same bits
    y4, _, _ = K.adarms_fwd(r2, mod, EPS)
    assert torch.equal(y4, y2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_adarms_backward_with_and_without_residual_and_branch(dtype, shape):
    B, rps, d = shape
    rtol, atol = tol(dtype)
    x, branch, mod, mod_prev = make(shape, dtype, 200)
    dy = rnd(B * rps, d, dtype=dtype, seed=204)
    res = rnd(B * rps, d, dtype=dtype, seed=205)
    gate = mod_prev[:, 2 * d:]
    _, rstd, _ = K.adarms_fwd(x, mod, EPS)
    for residual in (None, res):
        want = ref_bwd(dy, x, mod, rps, residual)
        dmod = torch.full_like(mod, 7.0)
        dr, dbr = K.adarms_bwd(dy, x, mod, rstd, dmod, residual=residual)
        assert dbr is None
        assert_path("adarms_bwd", dtype, shape, False, dy=dy, x=x, mod=mod, rstd=rstd, residual=residual, dx=dr, dmod=dmod, partial=1 << 40,
                    partial_bytes=1 << 40)
        assert_close(dr, want["dr"], rtol, atol * 2, "adarms dr")
        assert_close(dmod[:, :d], want["dscale"], rtol, atol * math.sqrt(rps), "adarms dscale")
        assert_close(dmod[:, d:2 * d], want["dshift"], rtol, atol * math.sqrt(rps), "adarms dshift")
        assert bool((dmod[:, 2 * d:] == 7.0).all()), "the gate third belongs to the add the gate multiplies: not touched here"
    # the mid-layer step: the norm read r = x + branch * gate_prev; its backward also gives dbranch and dgate_prev
    _, rstd2, r = K.adarms_fwd(x, mod, EPS, branch=branch, gate_prev=gate)
    runs = []
    for residual in (None, res, res):
        want = ref_bwd(dy, r, mod, rps, residual, branch, gate)
        dmod, dmod_prev = torch.full_like(mod, 7.0), torch.full_like(mod_prev, 7.0)
        dr, dbr = K.adarms_bwd(dy, r, mod, rstd2, dmod, residual=residual, branch=branch, gate_prev=gate,
                               dgate_prev=dmod_prev[:, 2 * d:])
        assert_path("adarms_bwd", dtype, shape, True, dy=dy, x=r, mod=mod, rstd=rstd2, residual=residual, dx=dr, dmod=dmod, x2=branch,
                    gate=gate, gate_ld=3 * d, aux=dbr, dgate=dmod_prev[:, 2 * d:], dgate_ld=3 * d, partial=1 << 40, partial_bytes=1 << 40)
        assert_close(dr, want["dr"], rtol, atol * 2, "adarms dr (fused)")
        assert_close(dbr, want["dbranch"], rtol, atol * 2, "adarms dbranch")
        assert_close(dmod[:, :d], want["dscale"], rtol, atol * math.sqrt(rps), "adarms dscale (fused)")
        assert_close(dmod[:, d:2 * d], want["dshift"], rtol, atol * math.sqrt(rps), "adarms dshift (fused)")
        assert_close(dmod_prev[:, 2 * d:], want["dgate"], rtol, atol * math.sqrt(rps), "adarms dgate_prev")
        assert bool((dmod[:, 2 * d:] == 7.0).all()) and bool((dmod_prev[:, :2 * d] == 7.0).all())
        runs.append((dr, dbr, dmod, dmod_prev))
    # deterministic: two runs of the same backward agree bit for bit
    assert all(torch.equal(a, b) for a, b in zip(runs[1], runs[2]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_gated_residual_forward_and_backward(dtype, shape):
    B, rps, d = shape
    rtol, atol = tol(dtype)
    x, branch, mod, _ = make(shape, dtype, 300)
    dy = rnd(B * rps, d, dtype=dtype, seed=304)
    gate = mod[:, 2 * d:]
    y = K.gated_residual_fwd(x, branch, gate)
    assert_path("gated_residual_fwd", dtype, shape, False, x=x, x2=branch, gate=gate, gate_ld=3 * d, y=y)
    assert_close(y, x.double() + branch.double() * per_row(gate, rps), rtol, atol, "gated residual fwd")
    assert torch.equal(K.gated_residual_fwd(x, branch, gate.contiguous()), y)
    runs = []
    for _ in range(2):
        dmod = torch.full_like(mod, 7.0)
        dbr = K.gated_residual_bwd(dy, branch, gate, dmod[:, 2 * d:])
        assert_path("gated_residual_bwd", dtype, shape, False, dy=dy, x2=branch, gate=gate, gate_ld=3 * d, dx=dbr, dgate=dmod[:, 2 * d:],
                    dgate_ld=3 * d, partial=1 << 40, partial_bytes=1 << 40)
        assert_close(dbr, dy.double() * per_row(gate, rps), rtol, atol * 2, "gated residual dbranch")
        assert_close(dmod[:, 2 * d:], (dy.double() * branch.double()).view(B, rps, d).sum(1), rtol, atol * math.sqrt(rps),
                     "gated residual dgate")
        assert bool((dmod[:, :2 * d] == 7.0).all())
        runs.append((dbr, dmod))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
