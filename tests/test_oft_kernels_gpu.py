"""The OFT kernels on the MI355X against fp64 torch arithmetic on the CPU, restated here: dxa_action_put_fwd/bwd (query / state rows
written at per-sample offsets), dxa_action_layernorm_fwd/bwd (LayerNorm of the A*d wide rows read out of the decoder output at those
offsets) and dxa_l1_loss.

Bounds.  fp32 rows, forward: 2e-6 of the largest reference magnitude for y (the max-norm ratio the project's ``rel_err`` is), 2e-6 of
each value for mean / rstd (the inputs have mean 0.5, so no statistic sits near zero).  bf16 rows: half a bf16 unit in the last place
of the fp64 result — one rounding — plus the fp32 bound, because the fp32 value that is rounded is itself that far from the fp64 one.
Backward: the row sums run over up to 26,632 fp32 terms — about 104 sequential additions per thread, then a tree of 8 + 2 levels — so
their worst case is (104 + 10) x 2^-24 = 6.8e-6 relative; dx, dw and db are held to 1e-5 of the largest reference magnitude (bf16
rows: plus the one rounding)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import kernels as K

DEV = "cuda"
FWD_TOL = 2e-6
BWD_TOL = 1e-5


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bf16_half_ulp(ref: torch.Tensor) -> torch.Tensor:
    """half the spacing of bf16 numbers at |ref| (8 significant bits): the error of one correct rounding"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


def assert_close(out, ref, tol, what, rounded):
    """|out - ref| <= tol * max|ref| (+ half a bf16 ulp of ref when ``out`` was rounded to bf16)"""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    bound = tol * ref.abs().max() + (bf16_half_ulp(ref) if rounded else 0.0)
    err = (out - ref).abs()
    worst = float((err / bound).max()) if err.numel() else 0.0
    print(f"{what}: largest share of the bound used {worst:.3f} (max err {float(err.max()):.3e})")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())}/{err.numel()} off, worst share of the bound {worst:.3f}"


# ------------------------------------------------------------------------------------------------ action_put
PUT_CASES = [(d, dtype, qdtype, state) for d in (96, 35) for dtype, qdtype in ((torch.float32, torch.float32),
                                                                              (torch.bfloat16, torch.bfloat16),
                                                                              (torch.bfloat16, torch.float32))
             for state in (False, True)]


@pytest.mark.parametrize("d,dtype,qdtype,state", PUT_CASES)
def test_action_put_forward_and_backward(d, dtype, qdtype, state):
    B, Sq, nq = 3, 12, 6
    s = int(state)
    Q = nq + s
    off_h = torch.tensor([2, 0, Sq - Q], dtype=torch.int64)           # distinct; the last block ends exactly at the last row
    off = off_h.to(DEV)
    query = rnd(nq, d, seed=1).to(qdtype)
    st = rnd(B, d, seed=2).to(dtype) if state else None
    sentinel = 7.0
    x = torch.full((B, Sq, d), sentinel, dtype=dtype, device=DEV)
    K.action_put_(x, query.to(DEV), off, st.to(DEV) if state else None)
    want = torch.full((B, Sq, d), sentinel, dtype=dtype)
    for b in range(B):
        o = int(off_h[b])
        if state:
            want[b, o] = st[b]
        want[b, o + s:o + s + nq] = query.to(dtype)
    assert torch.equal(x.cpu(), want)                                  # rows outside the block untouched, the block exact
    # backward: the ascending-b fp32 sum, bit for bit; first write replaces, the next adds
    dx_h = rnd(B, Sq, d, seed=3).to(dtype)
    dx = dx_h.to(DEV)
    acc = torch.zeros(nq, d, dtype=torch.float32)
    for b in range(B):
        o = int(off_h[b])
        acc = acc + dx_h[b, o + s:o + s + nq].float()
    dq = torch.full((nq, d), float("nan"), dtype=torch.float32, device=DEV)
    _, dstate = K.action_put_bwd(dx, off, nq, state, dquery=dq, accumulate=False, want_dstate=state)
    assert torch.equal(dq.cpu(), acc)
    first = dq.clone()
    _, _ = K.action_put_bwd(dx, off, nq, state, dquery=dq, accumulate=True)
    assert torch.equal(dq.cpu(), acc + acc)                            # old + (sum over b): the store's accumulate convention
    again, dstate2 = K.action_put_bwd(dx, off, nq, state, want_dstate=state)
    assert torch.equal(again, first)                                   # two runs, same bits
    if state:
        want_ds = torch.stack([dx_h[b, int(off_h[b])] for b in range(B)])
        assert dstate.dtype == dtype and torch.equal(dstate.cpu(), want_ds) and torch.equal(dstate2.cpu(), want_ds)
    else:
        assert dstate is None and dstate2 is None


def test_action_put_leaves_a_sample_whose_block_does_not_fit_alone():
    """an offset that would put the block past the last row (or before the first): nothing of that sample is written or read"""
    B, Sq, nq, d = 3, 8, 6, 16
    off = torch.tensor([1, 3, -1], dtype=torch.int64, device=DEV)      # sample 1: 3 + 6 > 8; sample 2: negative
    x = torch.full((B, Sq, d), 7.0, device=DEV)
    q = rnd(nq, d, seed=1).to(DEV)
    K.action_put_(x, q, off)
    assert torch.equal(x[0, 1:7], q) and bool((x[1:] == 7.0).all()) and bool((x[0, 0] == 7.0).all()) and bool((x[0, 7] == 7.0).all())
    dq, _ = K.action_put_bwd(x, off, nq, False)
    assert torch.equal(dq, q)                                          # only sample 0 contributes


# ------------------------------------------------------------------------------------------------ action_layernorm
F32, BF = torch.float32, torch.bfloat16
LN_CASES = [  # B, Sq, d, T, A, skip, dtype, weight dtype
    (2, 19, 96, 2, 3, 0, F32, F32), (2, 19, 96, 2, 3, 1, F32, F32),          # 288 columns: one wave per row
    (2, 19, 96, 2, 3, 0, BF, BF), (2, 19, 96, 2, 3, 1, BF, BF), (2, 19, 96, 2, 3, 1, BF, F32),
    (2, 19, 35, 2, 3, 0, F32, F32), (2, 19, 35, 2, 3, 1, F32, F32),          # 105 columns, unaligned row starts: scalar path
    (2, 19, 35, 2, 3, 1, BF, BF),
    (1, 17, 3584, 2, 7, 0, BF, BF), (1, 17, 3584, 2, 7, 1, BF, BF),          # the real width: two rows of 25,088 columns
    (1, 17, 3584, 2, 7, 1, F32, F32),
    (1, 4, 4096, 2, 1, 0, F32, F32), (1, 4, 4096, 2, 1, 0, BF, BF),          # last width of the one-wave path ...
    (1, 4, 4104, 2, 1, 1, F32, F32), (1, 4, 4104, 2, 1, 1, BF, BF),          # ... first of the workgroup path, row in registers
    (1, 4, 26624, 2, 1, 0, F32, F32), (1, 4, 26624, 2, 1, 0, BF, BF),        # last width that stays in registers ...
    (1, 4, 26632, 2, 1, 1, F32, F32), (1, 4, 26632, 2, 1, 1, BF, BF),        # ... first that is read again
    (1, 4, 4099, 2, 1, 1, F32, F32), (1, 4, 4099, 2, 1, 0, BF, BF),          # a wide row on the scalar path
]


def action_rows(h, off, T, A, skip):
    """[B, Sq, d] -> [B T, A d]: the reference's extract_action_hidden_states, [:, 1:] with the state row, reshape"""
    B, Sq, d = h.shape
    return torch.stack([h[b, int(off[b]) + skip:int(off[b]) + skip + T * A].reshape(T, A * d) for b in range(B)]).reshape(B * T, A * d)


@pytest.mark.parametrize("B,Sq,d,T,A,skip,dtype,wdtype", LN_CASES)
def test_action_layernorm(B, Sq, d, T, A, skip, dtype, wdtype):
    cols, Q = A * d, T * A + skip
    off_h = torch.tensor([Sq - Q, 0][:B] if B > 1 else [Sq - Q - 1], dtype=torch.int64)       # distinct offsets, padding behind
    off = off_h.to(DEV)
    h_h = (rnd(B, Sq, d, seed=1) + 0.5).to(dtype)
    w_h, b_h = (1 + 0.1 * rnd(cols, seed=2)).to(wdtype), (0.1 * rnd(cols, seed=3)).to(wdtype)
    dy_h = rnd(B * T, cols, seed=4).to(dtype)
    h, w, b, dy = h_h.to(DEV), w_h.to(DEV), b_h.to(DEV), dy_h.to(DEV)
    rounded = dtype == BF
    # fp64 reference on the values the kernel reads
    x64 = action_rows(h_h.double(), off_h, T, A, skip).requires_grad_(True)
    w64, b64 = w_h.double().requires_grad_(True), b_h.double().requires_grad_(True)
    y64 = F.layer_norm(x64, (cols,), w64, b64, 1e-5)
    y64.backward(dy_h.double())
    mean64 = x64.detach().mean(dim=1)
    rstd64 = 1.0 / torch.sqrt(x64.detach().var(dim=1, unbiased=False) + 1e-5)

    y, mean, rstd = K.action_layernorm_fwd(h, off, w, b, T, A, bool(skip), 1e-5)
    assert y.shape == (B * T, cols) and y.dtype == dtype and mean.shape == rstd.shape == (B * T,) and mean.dtype == torch.float32
    tag = f"d{d} A{A} skip{skip} {str(dtype)[6:]}"
    assert_close(y, y64, FWD_TOL, f"action_layernorm y {tag}", rounded)
    for got, ref, nm in ((mean, mean64, "mean"), (rstd, rstd64, "rstd")):
        e = ((got.double().cpu() - ref) / ref).abs().max().item()
        print(f"action_layernorm {nm} {tag}: {e:.3e}")
        assert e <= FWD_TOL, (nm, e)

    dh = torch.full_like(h, float("nan"))                    # every element must be written: zero off the action rows
    dh, part = K.action_layernorm_bwd(dy, h, off, w, mean, rstd, T, A, bool(skip), out=dh)
    assert not torch.isnan(dh).any()
    act = torch.zeros(B, Sq, dtype=torch.bool)
    for bb in range(B):
        act[bb, int(off_h[bb]) + skip:int(off_h[bb]) + skip + T * A] = True
    dh_c = dh.cpu()
    assert not bool(dh_c[~act].any()), "a row that is no action row must come back exactly zero"
    assert_close(action_rows(dh_c, off_h, T, A, skip), x64.grad, BWD_TOL, f"action_layernorm dx {tag}", rounded)
    assert part.shape == (min(B * T, 64), 2 * cols) and part.dtype == torch.float32
    s = K.colsum(part)                                       # the fold dxa_layernorm_bwd's partials go through
    assert_close(s[:cols], w64.grad, BWD_TOL, f"action_layernorm dw {tag}", False)
    assert_close(s[cols:], b64.grad, BWD_TOL, f"action_layernorm db {tag}", False)
    # same bits on a second run
    y2, mean2, rstd2 = K.action_layernorm_fwd(h, off, w, b, T, A, bool(skip), 1e-5)
    dh2, part2 = K.action_layernorm_bwd(dy, h, off, w, mean, rstd, T, A, bool(skip))
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2) and torch.equal(dh, dh2) and torch.equal(part, part2)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("d,A", [(96, 3), (1024, 4)])
def test_action_layernorm_has_the_bits_of_layernorm_fwd_on_the_gathered_rows(dtype, d, A):
    """offsets 0 and A d <= 4096: the kernel walks a row in dxa_layernorm_fwd's order"""
    B, Sq, T = 2, 19, 2
    off = torch.zeros(B, dtype=torch.int64, device=DEV)
    h = (rnd(B, Sq, d, seed=5) + 0.5).to(dtype).to(DEV)
    w, b = (1 + 0.1 * rnd(A * d, seed=6)).to(dtype).to(DEV), (0.1 * rnd(A * d, seed=7)).to(dtype).to(DEV)
    y, mean, rstd = K.action_layernorm_fwd(h, off, w, b, T, A, False, 1e-5)
    rows = h[:, :T * A].reshape(B * T, A * d).contiguous()
    y0, mean0, rstd0 = K.layernorm_fwd(rows, w, b, 1e-5)
    assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)


def test_action_layernorm_many_rows_share_the_backward_workgroups():
    """B T = 80 rows over 64 workgroups: 16 of them take a second row, and their partial sums hold both"""
    B, Sq, d, T, A = 40, 9, 16, 2, 3
    off_h = torch.arange(B, dtype=torch.int64) % 3
    h_h, dy_h = rnd(B, Sq, d, seed=8) + 0.5, rnd(B * T, A * d, seed=9)
    w_h = 1 + 0.1 * rnd(A * d, seed=10)
    x64 = action_rows(h_h.double(), off_h, T, A, 1).requires_grad_(True)
    w64 = w_h.double().requires_grad_(True)
    b64 = torch.zeros(A * d, dtype=torch.float64, requires_grad=True)
    F.layer_norm(x64, (A * d,), w64, b64, 1e-5).backward(dy_h.double())
    h, off, w, dy = h_h.to(DEV), off_h.to(DEV), w_h.to(DEV), dy_h.to(DEV)
    _, mean, rstd = K.action_layernorm_fwd(h, off, w, torch.zeros_like(w), T, A, True, 1e-5)
    dh, part = K.action_layernorm_bwd(dy, h, off, w, mean, rstd, T, A, True)
    assert part.shape == (64, 2 * A * d)
    s = K.colsum(part)
    assert_close(action_rows(dh.cpu(), off_h, T, A, 1), x64.grad, BWD_TOL, "dx 80 rows", False)
    assert_close(s[:A * d], w64.grad, BWD_TOL, "dw 80 rows", False)
    assert_close(s[A * d:], b64.grad, BWD_TOL, "db 80 rows", False)


# ------------------------------------------------------------------------------------------------ L1 loss
@pytest.mark.parametrize("n", [1, 42, 65539])
def test_l1_loss(n):
    pred_h, target_h = rnd(n, seed=11), rnd(n, seed=12)
    tie = n // 2
    target_h[tie] = pred_h[tie]                                        # one deliberate tie: its gradient is exactly 0
    gscale = 0.5
    pred, target = pred_h.to(DEV), target_h.to(DEV)
    loss, dpred = K.l1_loss(pred, target, gscale, want_grad=True)
    d64 = pred_h.double() - target_h.double()
    ref = d64.abs().mean().item()
    if n == 1:
        assert loss.item() == 0.0 and dpred.item() == 0.0
    else:
        e = abs(loss.item() - ref) / ref
        print(f"l1_loss n={n}: loss {loss.item():.8f} reference {ref:.8f} ({e:.2e})")
        assert e <= 1e-6
    g = dpred.cpu()
    assert torch.equal(torch.sign(g), torch.sign(d64).float()) and g[tie].item() == 0.0          # the sign pattern is exact
    mag = g[g != 0].abs().double()
    if mag.numel():
        assert ((mag - gscale / n).abs() <= 1e-6 * gscale / n).all()
    loss2, dpred2 = K.l1_loss(pred, target, gscale, want_grad=True)
    assert torch.equal(loss, loss2) and torch.equal(dpred, dpred2)
    loss3, none = K.l1_loss(pred, target, gscale, want_grad=False)                               # NULL dpred: the loss alone
    assert none is None and torch.equal(loss3, loss)
