"""dxa_rope2d_fwd / _bwd, dxa_layerscale_residual_fwd / _bwd, dxa_conv3x3s2_im2col / _col2im (csrc/pe.hip): the Perception Encoder
tower's kernels against an fp64 torch evaluation of their formulas, written out below.

    angle[t, :D/2] = repeat2((col(t) + s) * inv),  angle[t, D/2:] = repeat2((row(t) + s) * inv),  inv = theta ** -(arange(0, D/2, 2) / (D/2)),
    s = 1 with a CLS token, whose own row is all zero
    y[2i] = x[2i] cos - x[2i+1] sin,  y[2i+1] = x[2i+1] cos + x[2i] sin  on q and k;  the backward is the transpose
    y = x + gamma * h;   dh = gamma * dy,  dgamma = sum_rows dy * h
    conv: F.conv2d(x as [B, C, T, T], W [C', C, 3, 3], b, stride 2, padding 1), token-major in and out

Beside the shapes listed below: the rotation on a buffer that is not 16-byte aligned (the pair-wide path) and the convolution rows at
6 and 7 channels (the element-wise path), so every instantiation of the kernels runs.

Tolerances: those of tests/test_adarms_kernels_gpu.py — fp32 rtol 1e-5 / atol 1e-5, bf16 1/64 / 1e-2, dx atol x 2, column sums
(dgamma, dW, db) atol x sqrt(rows summed)."""
import math

import pytest
import torch
import torch.nn.functional as F

from dexbotic_amd import _lib as L
from dexbotic_amd import kernels as K

from .test_kernels_gpu import assert_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
THETA = 10000.0
# (N, grid_h, grid_w, H, D, cls, native grid or None)
ROPE_SHAPES = [(1, 1, 1, 1, 8, True, None),        # the smallest case
               (2, 3, 2, 2, 16, True, None),       # a non-square grid: swapped row / column angles cannot pass
               (1, 4, 4, 2, 64, False, None),      # the production head width, no CLS
               (2, 6, 6, 2, 64, True, None),       # 37 tokens
               (1, 3, 3, 1, 12, True, None),       # D % 8 != 0: the narrower access
               (2, 3, 2, 2, 16, True, (6, 6))]     # a 3 x 2 grid picked out of a 6 x 6 table
LS_SHAPES = [(1, 64), (5, 20), (5, 21), (74, 1024), (3, 8200)]
CONV_SHAPES = [(1, 1, 8), (2, 3, 8), (1, 4, 16), (2, 6, 24), (1, 26, 64)]


def tol(dtype):
    return (1e-5, 1e-5) if dtype == torch.float32 else (1.0 / 64, 1e-2)


# ------------------------------------------------------------------------------------------------ 2-D RoPE
def angles64(gh, gw, D, cls):
    """[T, D] fp64 from the formula in the module docstring (a picked grid has the angles of its own (row, col) positions)"""
    half = D // 2
    inv = THETA ** -(torch.arange(0, half, 2, dtype=torch.float64) / half)
    s = 1.0 if cls else 0.0
    rows = []
    for r in range(gh):
        for c in range(gw):
            rows.append(torch.cat([((c + s) * inv).repeat_interleave(2), ((r + s) * inv).repeat_interleave(2)]))
    a = torch.stack(rows)
    return torch.cat([torch.zeros(1, D, dtype=torch.float64), a]) if cls else a


def rot64(x, transpose=False):
    x1, x2 = x[..., 0::2], x[..., 1::2]
    pair = (x2, -x1) if transpose else (-x2, x1)
    return torch.stack(pair, dim=-1).flatten(-2)


def rope_ref(x, ang, backward=False):
    """x [N, T, 3, H, D] fp64 -> rotated q and k, v as it is"""
    c, s = ang.cos()[None, :, None, None, :].to(x.device), ang.sin()[None, :, None, None, :].to(x.device)
    qk = x[:, :, :2]
    out = x.clone()
    out[:, :, :2] = qk * c + (rot64(qk * s, True) if backward else rot64(qk) * s)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ROPE_SHAPES)
def test_rope2d_forward_backward_and_what_stays_untouched(dtype, shape):
    N, gh, gw, H, D, cls, native = shape
    rtol, atol = tol(dtype)
    T = gh * gw + int(cls)
    mh, mw = native or (gh, gw)
    cos_t, sin_t = K.rope2d_tables(gh, gw, D, mh, mw, cls, DEV)
    assert tuple(cos_t.shape) == (T, D)
    ang = angles64(gh, gw, D, cls)
    x = rnd(N, T, 3, H, D, dtype=dtype, seed=400 + D)
    y = K.rope2d_(x.clone(), cos_t, sin_t, N, T, H, D)
    assert_close(y, rope_ref(x.double(), ang), rtol, atol, "rope2d fwd")
    assert torch.equal(y[:, :, 2], x[:, :, 2]), "v is not touched"
    if cls:
        assert torch.equal(y[:, 0], x[:, 0]), "the CLS row has zero angles: bit-identical"
    if T > int(cls):
        assert not torch.equal(y[:, -1, :2], x[:, -1, :2])
    dy = rnd(N, T, 3, H, D, dtype=dtype, seed=500 + D)
    dx = K.rope2d_(dy.clone(), cos_t, sin_t, N, T, H, D, backward=True)
    assert_close(dx, rope_ref(dy.double(), ang, backward=True), rtol, atol, "rope2d bwd")
    assert torch.equal(dx[:, :, 2], dy[:, :, 2])
    # the adjoint identity <fwd(x), dy> = <x, bwd(dy)> in fp64 of the references, and bwd(fwd(x)) = x: the rotation is orthogonal
    back = K.rope2d_(y.clone(), cos_t, sin_t, N, T, H, D, backward=True)
    assert_close(back, x.double(), rtol, atol * 2, "rope2d bwd(fwd(x))")


def test_rope2d_row_and_column_angles_differ_on_a_non_square_grid():
    """token (r, c) = (2, 0) of a 3 x 2 grid: its first D/2 columns keep the angle of column 0, its last D/2 turn with row 2"""
    ang = angles64(3, 2, 16, True)
    t = 1 + 2 * 2 + 0
    assert torch.equal(ang[t, :8], ang[1, :8]) and not torch.equal(ang[t, 8:], ang[1, 8:])
    cos_t, _ = K.rope2d_tables(3, 2, 16, 3, 2, True, DEV)
    assert_close(cos_t, ang.cos().to(DEV), 1e-6, 1e-6, "rope2d table")


@pytest.mark.parametrize("dtype", DTYPES)
def test_rope2d_on_a_buffer_that_is_not_16_byte_aligned_takes_the_pair_path(dtype):
    """a contiguous view two elements into an allocation: 4 (bf16) or 8 (fp32) bytes off every wider alignment"""
    N, gh, gw, H, D = 2, 3, 2, 2, 16
    rtol, atol = tol(dtype)
    T = gh * gw + 1
    cos_t, sin_t = K.rope2d_tables(gh, gw, D, gh, gw, True, DEV)
    x = rnd(N, T, 3, H, D, dtype=dtype, seed=450)
    buf = torch.zeros(x.numel() + 2, device=DEV, dtype=dtype)
    view = buf[2:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % (4 * x.element_size()) != 0
    y = K.rope2d_(view, cos_t, sin_t, N, T, H, D)
    assert_close(y, rope_ref(x.double(), angles64(gh, gw, D, True)), rtol, atol, "rope2d fwd, pairs")
    assert torch.equal(y[:, :, 2], x[:, :, 2]) and torch.equal(y[:, 0], x[:, 0]) and not bool(buf[:2].any())
    # the same bits as the wide path on an aligned copy
    assert torch.equal(K.rope2d_(x.clone(), cos_t, sin_t, N, T, H, D), y)


def test_rope2d_refuses_a_head_width_that_is_not_a_multiple_of_4():
    x = torch.zeros(1, 2, 3, 1, 6, device=DEV)
    t = torch.zeros(2, 6, device=DEV)
    with pytest.raises(L.DxaError, match="multiple of 4"):
        K.rope2d_(x, t, t, 1, 2, 1, 6)


# ------------------------------------------------------------------------------------------------ LayerScale + residual
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", LS_SHAPES)
def test_layerscale_residual_forward_and_backward(dtype, shape):
    rows, cols = shape
    rtol, atol = tol(dtype)
    x, h, dy = (rnd(rows, cols, dtype=dtype, seed=600 + i) for i in range(3))
    gamma = (1.0 + 0.5 * rnd(cols, seed=603)).to(dtype)
    y = K.layerscale_residual_fwd(x, h, gamma)
    assert_close(y, x.double() + gamma.double() * h.double(), rtol, atol, "layerscale fwd")
    runs = []
    for _ in range(2):
        dh, part = K.layerscale_residual_bwd(dy, h, gamma)
        assert part.dtype == torch.float32 and part.shape == (L.lib.dxa_layerscale_bwd_rows(rows), cols)
        dgamma = K.colsum(part)
        assert_close(dh, dy.double() * gamma.double(), rtol, atol * 2, "layerscale dh")
        assert_close(dgamma, (dy.double() * h.double()).sum(0), rtol, atol * math.sqrt(rows), "layerscale dgamma")
        runs.append((dh, dgamma))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "deterministic: no atomics, one order"


# ------------------------------------------------------------------------------------------------ 3x3 stride-2 convolution
def conv_inputs(shape, dtype, seed):
    B, T, C_ = shape
    Co = 2 * C_
    x = rnd(B, T * T, C_, dtype=dtype, seed=seed)
    w = rnd(Co, C_, 3, 3, dtype=dtype, scale=(9 * C_) ** -0.5, seed=seed + 1)
    b = rnd(Co, dtype=dtype, seed=seed + 2)
    return x, w, b


def as_image(x, T):
    B, _, C_ = x.shape
    return x.double().view(B, T, T, C_).permute(0, 3, 1, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3x3s2_rows_times_weight_equal_conv2d_forward_and_backward(dtype, shape):
    B, T, C_ = shape
    rtol, atol = tol(dtype)
    x, w, b = conv_inputs(shape, dtype, 700 + T)
    Co, To = w.shape[0], K.conv_out_grid(T)
    xi = as_image(x, T).requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    want = F.conv2d(xi, w64, b64, stride=2, padding=1)
    assert want.shape == (B, Co, To, To)
    rows = K.conv3x3s2_im2col(x, T)
    assert rows.shape == (B * To * To, 9 * C_)
    # the rows themselves are copies: exact against unfold, whose column order is the weight's (c, ky, kx)
    unf = F.unfold(as_image(x, T), kernel_size=3, padding=1, stride=2).transpose(1, 2).reshape(B * To * To, 9 * C_)
    assert torch.equal(rows.double(), unf)
    y = K.mm_nt(rows, w.view(Co, 9 * C_), bias=b)
    assert_close(y.view(B, To, To, Co), want.permute(0, 2, 3, 1), rtol, atol, "conv fwd")
    dy = rnd(B * To * To, Co, dtype=dtype, seed=710 + T)
    want.backward(dy.double().view(B, To, To, Co).permute(0, 3, 1, 2))
    dx = K.conv3x3s2_col2im(K.mm_nn(dy, w.view(Co, 9 * C_)), B, T)
    assert_close(dx.view(B, T, T, C_), xi.grad.permute(0, 2, 3, 1), rtol, atol * 2, "conv dx")
    n = B * To * To
    dw = K.mm_tn(dy, rows, out_dtype=torch.float32)
    assert_close(dw.view(Co, C_, 3, 3), w64.grad, rtol, atol * math.sqrt(n), "conv dW in the parameter's layout")
    assert_close(K.colsum(dy), b64.grad, rtol, atol * math.sqrt(n), "conv db")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 5, 6), (1, 4, 7)])
def test_conv3x3s2_rows_and_adjoint_at_a_channel_count_that_is_no_multiple_of_4(dtype, shape):
    """the element-wise path (no product here: the GEMM wants 16-byte rows): rows against unfold, exactly; the adjoint against fold"""
    B, T, C_ = shape
    rtol, atol = tol(dtype)
    To = K.conv_out_grid(T)
    x = rnd(B, T * T, C_, dtype=dtype, seed=720 + C_)
    rows = K.conv3x3s2_im2col(x, T)
    unf = F.unfold(as_image(x, T), kernel_size=3, padding=1, stride=2)                          # [B, 9C, To*To]
    assert torch.equal(rows.double(), unf.transpose(1, 2).reshape(B * To * To, 9 * C_))
    dr = rnd(B * To * To, 9 * C_, dtype=dtype, seed=730 + C_)
    want = F.fold(dr.double().view(B, To * To, 9 * C_).transpose(1, 2), (T, T), kernel_size=3, padding=1, stride=2)
    assert_close(K.conv3x3s2_col2im(dr, B, T).view(B, T, T, C_), want.permute(0, 2, 3, 1), rtol, atol * 2, "col2im, element-wise")


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3x3s2_adjoint_of_all_ones_counts_the_taps_that_reach_each_element(dtype):
    """T = 3 (outputs at 0 and 2 per axis): with drows = 1 everywhere dx counts the (output, tap) pairs that read the element —
    even coordinates are read once per axis (the centre tap), the odd one by both neighbours: [[1, 2, 1], [2, 4, 2], [1, 2, 1]]"""
    B, T, C_ = 2, 3, 8
    To = K.conv_out_grid(T)
    dx = K.conv3x3s2_col2im(torch.ones(B * To * To, 9 * C_, device=DEV, dtype=dtype), B, T)
    want = torch.tensor([[1., 2., 1.], [2., 4., 2.], [1., 2., 1.]], device=DEV)
    assert torch.equal(dx.float().view(B, T, T, C_), want[None, :, :, None].expand(B, T, T, C_))
    # and im2col of all ones counts the taps inside the grid: corners of the output see 4 of 9
    rows = K.conv3x3s2_im2col(torch.ones(B, T * T, C_, device=DEV, dtype=dtype), T)
    assert rows.float().view(B, To, To, C_, 9).sum(-1).unique().tolist() == [4.0]
