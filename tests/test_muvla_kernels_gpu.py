"""The MuVLA row kernels on the MI355X against float64 torch formulas on the CPU: dxa_cross_entropy_rows_bwd,
dxa_ce_sample_reduce, dxa_add_layernorm_fwd/bwd and dxa_expectile_loss.  Bounds: those of tests/test_navila_kernels_gpu.py (its
cross-entropy and LayerNorm tolerances)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K

DEV = "cuda"
FP32_TOL = 1e-3
BF16_LN = (1.0 / 64, 2e-2)       # (rtol, atol) of the bf16 LayerNorm test in tests/test_kernels_gpu.py


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def rel_err(a, b) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def close(out, ref, rtol, atol, what):
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    err = (out - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max().item():.3e}"


# ------------------------------------------------------------- weighted cross-entropy backward, per-sample reduction
B_, L_ = 3, 5
_CE = {}


def ce_batch(V, dtype):
    """B = 3 samples x L = 5 rows of logits with a row stride above V; sample 1 has every label ignored; one reward negative.
    -> device inputs and the float64 reference (computed once per case and left unchanged)"""
    key = (V, dtype)
    if key in _CE:
        return _CE[key]
    ld = V + 9
    buf = rnd(B_ * L_, ld, dtype=dtype, scale=2.0, seed=V)
    z = buf[:, :V]
    labels = torch.randint(0, V, (B_, L_), generator=torch.Generator().manual_seed(V + 1))
    labels[0, 1] = -100
    labels[1, :] = -100                                        # n_1 = 0: clamped to 1, all-zero rows
    labels[2, 0] = V - 1
    labels[2, 4] = 0
    reward = torch.tensor([0.3, 0.8, -1.2])
    gscale = 0.7
    zr = z.detach().cpu().double().requires_grad_(True)
    lab = labels.reshape(-1)
    row = F.cross_entropy(zr, lab, reduction="none", ignore_index=-100).view(B_, L_)
    n = (labels != -100).sum(1).clamp(min=1).double()
    per = row.sum(1) / n
    w = 1.0 + torch.sigmoid(reward.double())
    loss_w, loss_1 = (per * w).mean(), per.mean()
    (gw,) = torch.autograd.grad(loss_w * gscale, zr, retain_graph=True)
    (g1,) = torch.autograd.grad(loss_1 * gscale, zr)
    out = dict(z=z, labels=lab.to(DEV), reward=reward.to(DEV), gscale=torch.tensor([gscale], device=DEV),
               loss_w=loss_w.detach(), loss_1=loss_1.detach(), dz_w=gw, dz_1=g1,
               row_w=(w / (n * B_)).repeat_interleave(L_), row_1=(1.0 / (n * B_)).repeat_interleave(L_))
    _CE[key] = out
    return out


CE_CASES = [(264, torch.float32), (264, torch.bfloat16), (1031, torch.float32), (1031, torch.bfloat16)]


@pytest.mark.parametrize("V,dtype", CE_CASES)
def test_ce_sample_reduce(V, dtype):
    c = ce_batch(V, dtype)
    row_loss, _ = K.cross_entropy_fwd(c["z"], c["labels"])
    loss, row_w = K.ce_sample_reduce(row_loss, c["labels"], c["reward"], B_, V)
    close(loss, c["loss_w"].view(1), 1e-5, 2e-5, "weighted loss")
    close(row_w, c["row_w"], 1e-5, 0.0, "row weights")
    assert torch.equal(row_w.view(B_, L_), row_w.view(B_, L_)[:, :1].expand(B_, L_))       # one weight per sample
    # reward = None: the plain per-sample mean
    loss1, row_1 = K.ce_sample_reduce(row_loss, c["labels"], None, B_, V)
    close(loss1, c["loss_1"].view(1), 1e-5, 2e-5, "unweighted loss")
    close(row_1, c["row_1"], 1e-6, 0.0, "unweighted row weights")
    # the same bits on a second run (one workgroup, fixed order)
    loss2, row_w2 = K.ce_sample_reduce(row_loss, c["labels"], c["reward"], B_, V)
    assert torch.equal(loss, loss2) and torch.equal(row_w, row_w2)


@pytest.mark.parametrize("V,dtype", CE_CASES)
def test_cross_entropy_rows_bwd(V, dtype):
    c = ce_batch(V, dtype)
    z, labels, gs = c["z"], c["labels"], c["gscale"]
    assert z.stride(0) > V
    row_loss, lse = K.cross_entropy_fwd(z, labels)
    _, row_w = K.ce_sample_reduce(row_loss, labels, c["reward"], B_, V)
    dz = K.cross_entropy_rows_bwd(z, labels, lse, gs, 1.0, row_w)
    # fp32 keeps ~1e-6 relative; a bf16 result is the fp32 value rounded once (2^-9 relative, 2^-8 allowed)
    rtol = 1e-4 if dtype == torch.float32 else 2.0 ** -8
    close(dz, c["dz_w"], rtol, 1e-7, "weighted dlogits")
    assert not dz.view(B_, L_, V)[1].any() and not dz[1].any()                            # ignored rows are zeros
    _, row_1 = K.ce_sample_reduce(row_loss, labels, None, B_, V)
    close(K.cross_entropy_rows_bwd(z, labels, lse, gs, 1.0, row_1), c["dz_1"], rtol, 1e-7, "unweighted dlogits")
    # row_w = None is cross_entropy_bwd, bit for bit
    assert torch.equal(K.cross_entropy_rows_bwd(z, labels, lse, gs, 0.25, None), K.cross_entropy_bwd(z, labels, lse, gs, 0.25))
    # in place (dlogits aliasing logits, the padded row stride kept) gives the same bits
    buf2 = torch.empty(B_ * L_, z.stride(0), device=DEV, dtype=dtype)
    z2 = buf2[:, :V]
    z2.copy_(z)
    assert torch.equal(K.cross_entropy_rows_bwd(z2, labels, lse, gs, 1.0, row_w, out=z2), dz)


# --------------------------------------------------------------------------------------------------- add + LayerNorm
@pytest.mark.parametrize("dtype,wdtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                          (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("cols", [70, 128, 1024])
@pytest.mark.parametrize("rows", [1, 5, 70])
def test_add_layernorm(rows, cols, dtype, wdtype):
    x = rnd(rows, cols, dtype=dtype, seed=1) + 0.5
    res = rnd(rows, cols, dtype=dtype, seed=2)
    w = (1 + 0.1 * rnd(cols, seed=3)).to(wdtype)
    b = (0.1 * rnd(cols, seed=4)).to(wdtype)
    dy = rnd(rows, cols, dtype=dtype, seed=5)
    y, mean, rstd = K.add_layernorm_fwd(x, res, w, b, 1e-5)
    assert y.shape == x.shape and y.dtype == dtype and mean.shape == rstd.shape == (rows,)
    xr, rr = x.cpu().double().requires_grad_(True), res.cpu().double().requires_grad_(True)
    wr, br = w.cpu().double().requires_grad_(True), b.cpu().double().requires_grad_(True)
    s = xr + rr
    yr = F.layer_norm(s, (cols,), wr, br, 1e-5)
    yr.backward(dy.cpu().double())
    assert torch.equal(xr.grad, rr.grad)
    dx, part = K.add_layernorm_bwd(dy, x, res, w, mean, rstd)
    assert dx.shape == x.shape and part.shape == (K.norm_bwd_blocks(rows), 2 * cols)
    f = K.colsum(part)
    dw, db = f[:cols], f[cols:]
    # the statistics are those of the UN-rounded sum
    close(mean, s.detach().mean(-1), 1e-5, 1e-5, "mean")
    close(rstd, torch.rsqrt(s.detach().var(-1, unbiased=False) + 1e-5), 1e-4, 1e-5, "rstd")
    if dtype == torch.float32:
        assert rel_err(y, yr) < FP32_TOL and rel_err(dx, xr.grad) < FP32_TOL
        assert rel_err(dw, wr.grad) < FP32_TOL and rel_err(db, br.grad) < FP32_TOL
    else:
        rtol, atol = BF16_LN
        close(y, yr, rtol, atol, "y")
        close(dx, xr.grad, rtol, atol * 2, "dx")
        close(dw, wr.grad, rtol, atol * math.sqrt(rows), "dw")
        close(db, br.grad, rtol, atol * math.sqrt(rows), "db")
    # res = 0 is layernorm_fwd, bit for bit (output and statistics)
    y0, m0, r0 = K.add_layernorm_fwd(x, torch.zeros_like(x), w, b, 1e-5)
    y1, m1, r1 = K.layernorm_fwd(x, w, b, 1e-5)
    assert torch.equal(y0, y1) and torch.equal(m0, m1) and torch.equal(r0, r1)


# ----------------------------------------------------------------------------------------------------- expectile loss
def expectile_ref(pred, target, tau, gscale):
    p = pred.cpu().double().requires_grad_(True)
    d = p - target.cpu().double()
    loss = (torch.where(d < 0, tau, 1 - tau) * d * d).mean()
    (g,) = torch.autograd.grad(loss * gscale, p)
    return loss.detach(), g


@pytest.mark.parametrize("n", [1, 2, 16, 300])
def test_expectile_loss(n):
    tau, gscale = 0.9, 0.5
    pred, target = rnd(n, seed=6), rnd(n, seed=7)
    cases = []
    if n == 1:                                               # one element: each sign and the exact zero in turn
        cases = [(pred, pred + 1.0), (pred, pred - 1.0), (pred, pred.clone())]
    else:
        target[0] = pred[0]                                  # an exact zero among both signs
        target[1] = pred[1] + (0.5 if n > 2 else -0.5)
        if n > 2:
            target[2] = pred[2] - 0.5
        cases = [(pred, target)]
    for p, t in cases:
        loss, dp = K.expectile_loss(p, t, tau, gscale)
        lr, gr = expectile_ref(p, t, tau, gscale)
        close(loss, lr.view(1), 1e-5, 1e-7, "loss")
        close(dp, gr, 1e-5, 1e-8, "dpred")
        zero = (p == t).cpu()
        assert not dp.cpu()[zero].any()                      # diff == 0: the 1 - tau branch, gradient 0
        loss2, none = K.expectile_loss(p, t, tau, gscale, want_grad=False)
        assert none is None and torch.equal(loss, loss2)
    if n > 2:
        d = (pred - target).cpu()
        assert (d < 0).any() and (d > 0).any() and (d == 0).any()


# ------------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_are_refused_with_a_message():
    st = torch.cuda.current_stream().cuda_stream
    rows, V = 4, 264
    z = rnd(rows, V, seed=8)
    labels = torch.zeros(rows, dtype=torch.int64, device=DEV)
    f32 = lambda n: torch.zeros(n, device=DEV)
    lse, rl, rw, loss, out = f32(rows), f32(rows), f32(rows), f32(1), torch.empty_like(z)
    p = lambda t: t.data_ptr()
    bwd = L.lib.dxa_cross_entropy_rows_bwd
    assert bwd(p(z), V, p(labels), p(lse), None, 1.0, p(rw), p(out), V, rows, V, -100, L.F32, st) == 0
    assert bwd(None, V, p(labels), p(lse), None, 1.0, p(rw), p(out), V, rows, V, -100, L.F32, st) == -1
    assert b"dxa_cross_entropy_rows_bwd" in L.lib.dxa_last_error()
    assert bwd(p(z), V, p(labels), p(lse), None, 1.0, p(rw), p(out), V - 1, rows, V, -100, L.F32, st) == -1
    assert bwd(p(z), V, p(labels), p(lse), None, 1.0, p(rw), p(out), V, rows, V, -100, 7, st) == -1
    red = L.lib.dxa_ce_sample_reduce
    assert red(p(rl), p(labels), None, p(rw), p(loss), 2, 2, V, -100, st) == 0
    assert red(p(rl), p(labels), None, None, p(loss), 2, 2, V, -100, st) == -1
    assert b"null" in L.lib.dxa_last_error()
    assert red(p(rl), p(labels), None, p(rw), p(loss), 0, 2, V, -100, st) == -1
    assert b"bad sizes" in L.lib.dxa_last_error()
    x = rnd(4, 8, seed=9)
    y, mean, rstd = torch.empty_like(x), f32(4), f32(4)
    fwd, bwdn = L.lib.dxa_add_layernorm_fwd, L.lib.dxa_add_layernorm_bwd
    assert fwd(p(x), p(x), None, None, p(y), p(mean), p(rstd), 4, 8, 1e-5, L.F32, L.F32, st) == 0
    assert fwd(p(x), None, None, None, p(y), p(mean), p(rstd), 4, 8, 1e-5, L.F32, L.F32, st) == -1
    assert b"null" in L.lib.dxa_last_error()
    assert fwd(p(x), p(x), None, None, p(y), p(mean), p(rstd), 4, 0, 1e-5, L.F32, L.F32, st) == -1
    assert b"bad sizes" in L.lib.dxa_last_error()
    assert fwd(p(x), p(x), None, None, p(y), p(mean), p(rstd), 4, 8, 1e-5, L.F32, L.BF16, st) == -2
    assert bwdn(p(x), p(x), p(x), p(x), p(mean), p(rstd), p(y), None, 4, 8, L.F32, L.F32, st) == -1
    assert b"partial_dwdb" in L.lib.dxa_last_error()
    assert bwdn(p(x), p(x), None, None, p(mean), p(rstd), p(y), None, 4, 8, L.F32, L.F32, st) == -1
    exp = L.lib.dxa_expectile_loss
    assert exp(p(rl), p(rw), p(loss), None, rows, 0.9, 1.0, st) == 0
    assert exp(p(rl), None, p(loss), None, rows, 0.9, 1.0, st) == -1
    assert b"null" in L.lib.dxa_last_error()
    assert exp(p(rl), p(rw), p(loss), None, 0, 0.9, 1.0, st) == -1
    assert exp(p(rl), p(rw), p(loss), None, rows, 1.0, 1.0, st) == -1
    assert b"tau" in L.lib.dxa_last_error()
    torch.cuda.synchronize()
    with pytest.raises(AssertionError):
        K.ce_sample_reduce(rl, labels, None, 3, V)          # 4 rows are not 3 samples of equal length
