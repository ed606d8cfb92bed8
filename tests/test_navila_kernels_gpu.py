"""The two NaVILA kernels on the MI355X against the same arithmetic composed from torch ops on the device:
dxa_downsample_layernorm_fwd/bwd (2x2 token merge + LayerNorm(4C)) and dxa_soft_cross_entropy_fwd/bwd."""
import ctypes as C
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
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def close(out, ref, rtol, atol, what):
    err = (out.double() - ref.double()).abs()
    bad = err > atol + rtol * ref.double().abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max().item():.3e}"


# --------------------------------------------------------------------------------- downsample + LayerNorm
def merge_ln(x, w, b, G, eps=1e-5):
    """x [N, G*G, C], token t = r*G + c -> zero pad to an even grid -> output token o = j*h + i (j column pair, i row pair) =
    [x(2i,2j) | x(2i,2j+1) | x(2i+1,2j) | x(2i+1,2j+1)] -> LayerNorm over the 4C columns"""
    N, T, C_ = x.shape
    Gp = G + (G & 1)
    h = Gp // 2
    g = F.pad(x.view(N, G, G, C_), (0, 0, 0, Gp - G, 0, Gp - G))            # [N, r, c, C]
    g = g.view(N, h, 2, h, 2, C_).permute(0, 3, 1, 2, 4, 5)                # [N, j, i, r & 1, c & 1, C]
    m = g.reshape(N, h * h, 4 * C_)
    return F.layer_norm(m, (4 * C_,), w, b, eps)


DS_CASES = [  # N, G, C, dtype, weight dtype
    (3, 3, 6, torch.float32, torch.float32),           # odd grid (padded), scalar path, three workgroups
    (3, 3, 6, torch.bfloat16, torch.bfloat16),
    (2, 4, 8, torch.float32, torch.float32),           # even grid, 16-byte path
    (2, 4, 8, torch.bfloat16, torch.float32),
    (2, 4, 8, torch.bfloat16, torch.bfloat16),
    (1, 5, 12, torch.float32, torch.float32),          # 16-byte path on an odd grid; 9 rows: a workgroup with one live wave
    (2, 27, 1152, torch.bfloat16, torch.bfloat16),     # the real tower's grid: 196 output tokens of width 4608
]
# the path of each case as its comment states it (dxa_norm_plan): the kernel's (T, TW, elements per access), both directions
DS_PATHS = {0: "float,float,1", 1: "bf16,bf16,1", 2: "float,float,4", 3: "bf16,float,8", 4: "bf16,bf16,8", 5: "float,float,4",
            6: "bf16,bf16,8"}


@pytest.mark.parametrize("N,G,C_,dtype,wdtype", DS_CASES)
def test_downsample_layernorm(N, G, C_, dtype, wdtype):
    h = (G + 1) // 2
    x = rnd(N, G * G, C_, dtype=dtype, seed=1) + 0.5
    w = (1 + 0.1 * rnd(4 * C_, seed=2)).to(wdtype)
    b = (0.1 * rnd(4 * C_, seed=3)).to(wdtype)
    dy = rnd(N, h * h, 4 * C_, dtype=dtype, seed=4)
    y, mean, rstd = K.downsample_layernorm_fwd(x, w, b, 1e-5)
    assert y.shape == (N, h * h, 4 * C_) and y.dtype == dtype and mean.shape == rstd.shape == (N * h * h,)
    xr = x.clone().requires_grad_(True)
    wr, br = w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)     # the composition runs in the row dtype
    yr = merge_ln(xr, wr, br, G)
    yr.backward(dy)
    dx = torch.full_like(x, float("nan"))                 # every element of the un-merged gradient must be written
    dx, part = K.downsample_layernorm_bwd(dy, x, w, mean, rstd, out=dx)
    assert dx.shape == x.shape and not torch.isnan(dx).any()
    assert part.shape == (K.norm_bwd_blocks(N * h * h), 8 * C_)
    path = DS_PATHS[DS_CASES.index((N, G, C_, dtype, wdtype))]
    dts = dict(dtype=int(dtype == torch.bfloat16), w_dtype=int(wdtype == torch.bfloat16), rows=N, G=G, cols=C_)
    pf = K.norm_plan("downsample_layernorm_fwd", x=x, w=w, b=b, y=y, mean=mean, rstd=rstd, **dts)
    pb = K.norm_plan("downsample_layernorm_bwd", dy=dy, x=x, w=w, mean=mean, rstd=rstd, dx=dx, partial=part, **dts)
    assert pf["kernel"] == f"ds_layernorm_fwd_k<{path}>" and pb["kernel"] == f"ds_layernorm_bwd_k<{path}>", (pf, pb)
    assert pb["lds"] == 8 * C_ * 4 and pb["grid"][0] == K.norm_bwd_blocks(N * h * h)    # the partial sums in LDS
    s = K.colsum(part)                                   # the fold dxa_layernorm_bwd's partials go through
    dw, db = s[:4 * C_], s[4 * C_:]
    rows = N * h * h
    if dtype == torch.float32:
        assert rel_err(y, yr) < FP32_TOL and rel_err(dx, xr.grad) < FP32_TOL
        assert rel_err(dw, wr.grad) < FP32_TOL and rel_err(db, br.grad) < FP32_TOL
    else:
        rtol, atol = BF16_LN
        close(y, yr, rtol, atol, "y")
        close(dx, xr.grad, rtol, atol * 2, "dx")
        close(dw, wr.grad, rtol, atol * math.sqrt(rows), "dw")
        close(db, br.grad, rtol, atol * math.sqrt(rows), "db")


def test_downsample_layernorm_statistics_and_bad_args():
    N, G, C_ = 2, 3, 6
    x = rnd(N, G * G, C_, seed=5)
    y, mean, rstd = K.downsample_layernorm_fwd(x, None, None, 1e-5)
    Gp, h = 4, 2
    m = F.pad(x.view(N, G, G, C_), (0, 0, 0, 1, 0, 1)).view(N, h, 2, h, 2, C_).permute(0, 3, 1, 2, 4, 5).reshape(N * h * h, 4 * C_)
    assert rel_err(mean, m.mean(-1)) < FP32_TOL                            # padded positions count as zeros
    assert rel_err(rstd, torch.rsqrt(m.var(-1, unbiased=False) + 1e-5)) < FP32_TOL
    st = torch.cuda.current_stream().cuda_stream
    p = x.data_ptr()
    assert L.lib.dxa_downsample_layernorm_fwd(None, None, None, y.data_ptr(), None, None, N, G, C_, 1e-5, L.F32, L.F32, st) == -1
    assert b"null" in L.lib.dxa_last_error()
    assert L.lib.dxa_downsample_layernorm_fwd(p, None, None, y.data_ptr(), None, None, N, 0, C_, 1e-5, L.F32, L.F32, st) == -1
    assert b"bad sizes" in L.lib.dxa_last_error()
    assert L.lib.dxa_downsample_layernorm_bwd(p, p, p, mean.data_ptr(), rstd.data_ptr(), p, None, N, G, C_, L.F32, L.F32, st) == -1
    assert b"partial_dwdb" in L.lib.dxa_last_error()
    assert L.lib.dxa_downsample_layernorm_fwd(p, None, None, y.data_ptr(), None, None, N, G, C_, 1e-5, L.F32, L.BF16, st) == -2
    with pytest.raises(L.DxaError):
        K.downsample_layernorm_fwd(rnd(1, 8, 4, seed=6), None, None, 1e-5)     # 8 tokens are not a square grid


# ------------------------------------------------------------------------------------ soft cross-entropy
def soft_ce_ref(z, labels, ids, std, gscale, scale):
    """log_softmax + dense targets from the closed form: rows labelled with a soft id get exp(-(y - s_k)^2 / (2 std^2)),
    normalised over the K ids; other rows their one-hot label; ignored rows nothing.  -> (row_loss, lse, dlogits), fp32"""
    zf = z.float().clone().requires_grad_(True)
    logp = torch.log_softmax(zf, dim=-1)
    rows, V = z.shape
    tgt = torch.zeros(rows, V, device=z.device)
    s = torch.tensor(ids, device=z.device, dtype=torch.int64)
    for r in range(rows):
        y = int(labels[r])
        if y == -100:
            continue
        if len(ids) and y in ids:
            e = torch.exp(-((y - s).float() ** 2) / (2 * std ** 2))
            tgt[r, s] = e / e.sum()
        else:
            tgt[r, y] = 1.0
    row_loss = -(tgt * logp).sum(-1)
    (row_loss.sum() * gscale * scale).backward()
    return row_loss.detach(), torch.logsumexp(zf.detach(), -1), zf.grad


SOFT_CASES = [  # V, rows, dtype, soft ids (out of order where it says so)
    (300, 16, torch.float32, [207, 200, 203, 201, 206, 202, 205, 204]),        # 16-byte path, ids out of order
    (301, 16, torch.float32, list(range(200, 208))),                          # scalar path
    (300, 16, torch.bfloat16, [5, 299, 0, 150]),                               # ids spread over the row, both ends of it
    (152064, 8, torch.bfloat16, [151700 + 2 * k for k in range(8)][::-1]),     # the real vocabulary; not contiguous
]


@pytest.mark.parametrize("V,rows,dtype,ids", SOFT_CASES)
def test_soft_cross_entropy(V, rows, dtype, ids):
    z = rnd(rows, V, dtype=dtype, scale=2.0, seed=7)
    g = torch.Generator().manual_seed(8)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[0], labels[1], labels[2] = min(ids), max(ids), ids[1]              # soft rows: both ends of the id range and one more
    labels[3] = -100                                                          # ignored rows mixed in
    labels[rows - 1] = -100
    for r in range(4, rows - 1):
        if int(labels[r]) in ids:
            labels[r] = (max(ids) + 1) % V if (max(ids) + 1) % V not in ids else 1
    labels = labels.to(DEV)
    soft = K.SoftTokens(ids, 1.0, DEV)
    gscale = torch.tensor([0.7], device=DEV)
    scale = 1.0 / 6
    row_loss, lse = K.soft_cross_entropy_fwd(z, labels, soft)
    dz = K.soft_cross_entropy_bwd(z, labels, lse, gscale, scale, soft)
    rl, ls, dr = soft_ce_ref(z, labels, ids, 1.0, 0.7, scale)
    # fp32 arithmetic on the same (fp32 or bf16) logits on both sides: what differs is the order of ~V additions and expf's last
    # bits, ~1e-6 relative on values of order 10
    close(lse, ls, 1e-5, 1e-5, "lse")
    close(row_loss, rl, 1e-5, 2e-5, "row loss")
    assert row_loss[3].item() == 0.0 and row_loss[rows - 1].item() == 0.0
    assert not dz[3].any() and not dz[rows - 1].any()
    # gradient: fp32 keeps ~1e-6 relative; a bf16 result is the fp32 value rounded once (2^-9 relative, 2^-8 allowed)
    rtol = 1e-4 if dtype == torch.float32 else 2.0 ** -8
    close(dz, dr, rtol, 1e-7, "dlogits")
    # in place (dlogits aliasing logits) gives the same bits
    z2 = z.clone()
    assert torch.equal(K.soft_cross_entropy_bwd(z2, labels, lse, gscale, scale, soft, out=z2), dz)
    # every row ignored: loss 0.0 and no gradient
    none = torch.full((rows,), -100, dtype=torch.int64, device=DEV)
    rl0, lse0 = K.soft_cross_entropy_fwd(z, none, soft)
    assert K.colsum(rl0.view(-1, 1)).item() == 0.0
    assert not K.soft_cross_entropy_bwd(z, none, lse0, gscale, scale, soft).any()


@pytest.mark.parametrize("V,dtype", [(300, torch.float32), (301, torch.bfloat16), (152064, torch.bfloat16)])
def test_soft_cross_entropy_without_soft_ids_is_cross_entropy(V, dtype):
    rows = 8
    z = rnd(rows, V, dtype=dtype, scale=2.0, seed=9)
    labels = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(10))
    labels[2] = -100
    labels = labels.to(DEV)
    gscale = torch.tensor([1.3], device=DEV)
    soft = K.SoftTokens([], 1.0, DEV)
    rl, lse = K.cross_entropy_fwd(z, labels)
    rl2, lse2 = K.soft_cross_entropy_fwd(z, labels, soft)
    assert torch.equal(rl, rl2) and torch.equal(lse, lse2)
    assert torch.equal(K.cross_entropy_bwd(z, labels, lse, gscale, 0.25), K.soft_cross_entropy_bwd(z, labels, lse, gscale, 0.25, soft))
    # ids no label of the batch hits change nothing either
    free = [i for i in range(V) if i not in set(labels.tolist())][:4]
    soft4 = K.SoftTokens(free, 1.0, DEV)
    rl3, lse3 = K.soft_cross_entropy_fwd(z, labels, soft4)
    assert torch.equal(rl, rl3) and torch.equal(lse, lse3)
    assert torch.equal(K.cross_entropy_bwd(z, labels, lse, gscale, 0.25), K.soft_cross_entropy_bwd(z, labels, lse, gscale, 0.25, soft4))


def test_soft_cross_entropy_refuses_bad_arguments():
    with pytest.raises(ValueError):
        K.SoftTokens([3, 4, 3], 1.0, DEV)                                      # duplicates: refused on the host
    rows, V = 4, 300
    z = rnd(rows, V, seed=11)
    labels = torch.zeros(rows, dtype=torch.int64, device=DEV)
    rl = torch.empty(rows, device=DEV)
    lse = torch.empty(rows, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    ids = torch.tensor([1, 2], dtype=torch.int64, device=DEV)
    host = (C.c_int64 * 2)(1, 2)
    hp = C.cast(host, C.c_void_p)
    fwd, bwd = L.lib.dxa_soft_cross_entropy_fwd, L.lib.dxa_soft_cross_entropy_bwd
    assert fwd(z.data_ptr(), V, labels.data_ptr(), rl.data_ptr(), lse.data_ptr(), rows, V, -100, ids.data_ptr(), hp, 2, 0.5, L.F32, st) == 0
    assert fwd(None, V, labels.data_ptr(), rl.data_ptr(), lse.data_ptr(), rows, V, -100, ids.data_ptr(), hp, 2, 0.5, L.F32, st) == -1
    assert b"dxa_soft_cross_entropy_fwd" in L.lib.dxa_last_error()
    assert fwd(z.data_ptr(), V - 1, labels.data_ptr(), rl.data_ptr(), lse.data_ptr(), rows, V, -100, ids.data_ptr(), hp, 2, 0.5, L.F32, st) == -1
    assert fwd(z.data_ptr(), V, labels.data_ptr(), rl.data_ptr(), lse.data_ptr(), rows, V, -100, None, None, 2, 0.5, L.F32, st) == -1
    assert b"required" in L.lib.dxa_last_error()
    big = (C.c_int64 * 2)(1, V)
    bp = C.cast(big, C.c_void_p)
    assert fwd(z.data_ptr(), V, labels.data_ptr(), rl.data_ptr(), lse.data_ptr(), rows, V, -100, ids.data_ptr(), bp, 2, 0.5, L.F32, st) == -1
    assert b"outside the vocabulary" in L.lib.dxa_last_error()
    out = torch.empty_like(z)
    assert bwd(z.data_ptr(), V, labels.data_ptr(), lse.data_ptr(), None, 1.0, out.data_ptr(), V, rows, V, -100, ids.data_ptr(), bp, 2, 0.5, L.F32, st) == -1
    assert b"outside the vocabulary" in L.lib.dxa_last_error()
    assert bwd(z.data_ptr(), V, labels.data_ptr(), lse.data_ptr(), None, 1.0, None, V, rows, V, -100, ids.data_ptr(), hp, 2, 0.5, L.F32, st) == -1
    assert bwd(z.data_ptr(), V, labels.data_ptr(), lse.data_ptr(), None, 1.0, out.data_ptr(), V - 1, rows, V, -100, ids.data_ptr(), hp, 2, 0.5, L.F32, st) == -1
    dup = (C.c_int64 * 2)(2, 2)
    assert fwd(z.data_ptr(), V, labels.data_ptr(), rl.data_ptr(), lse.data_ptr(), rows, V, -100, ids.data_ptr(), C.cast(dup, C.c_void_p), 2, 0.5, L.F32, st) == -1
    assert b"duplicate" in L.lib.dxa_last_error()
    assert fwd(z.data_ptr(), V, labels.data_ptr(), rl.data_ptr(), lse.data_ptr(), rows, V, -100, ids.data_ptr(), hp, 65, 0.5, L.F32, st) == -1
    with pytest.raises(L.DxaError):
        K.soft_cross_entropy_fwd(z, labels, K.SoftTokens([1, V], 1.0, DEV))
