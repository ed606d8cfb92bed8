"""The OFT-discrete kernels on the MI355X against torch indexing and fp64 arithmetic on the CPU, restated here:
dxa_action_rows_fwd/bwd (the action rows as a dense operand, and its complete scatter back), dxa_action_fill_fwd/bwd (one shared row
written into every reserved row, and the fixed-order sum of their gradients) and dxa_action_bins_fwd (bin logits, first-index argmax
and action value in one launch).

Bounds.  rows / fill forward and the rows backward are copies: bit-equal.  ``drow`` is a sum of n = B R fp32 terms per column, added
one at a time (chunks of 16, then the chunks): at most n - 1 roundings of 2^-24 relative to a partial sum that never exceeds
sum |term|, so |drow - fp64| <= n 2^-24 sum |term| per element.  ``bin_logits``: a d-term dot product accumulated in fp32 (products of
bf16 operands are exact in fp32; fp32 operands: one fma rounding per term), in four strands that are then added: at most d roundings,
|logit - fp64| <= d 2^-24 sum_k |h_k w_k| per element, plus 2^-8 |x| for the one rounding of a bf16 output.  ``bin`` is compared with
the first-index argmax OF THE RETURNED LOGITS and ``action`` with the fp32 expression on the returned bins: both exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def blocks(off_h, B, Sq, R, s):
    """[(b, first action row)] of the samples whose block of s + R rows lies inside [0, Sq)"""
    return [(b, int(off_h[b]) + s) for b in range(B) if 0 <= int(off_h[b]) and int(off_h[b]) + s + R <= Sq]


# ------------------------------------------------------------------------------------------------ rows / fill
ROW_CASES = [(d, dtype, skip) for d in (96, 100) for dtype in (F32, BF) for skip in (0, 1)]


@pytest.mark.parametrize("d,dtype,skip", ROW_CASES)
def test_action_rows_forward_and_backward(d, dtype, skip):
    B, Sq, R = 3, 14, 6
    off_h = torch.tensor([2, Sq - R - skip, Sq - R - skip + 1], dtype=torch.int64)     # the last block is one row too long
    off = off_h.to(DEV)
    h_h = rnd(B, Sq, d, seed=1).to(dtype)
    y = K.action_rows_fwd(h_h.to(DEV), off, R, bool(skip))
    want = torch.zeros(B * R, d, dtype=dtype)
    ok = blocks(off_h, B, Sq, R, skip)
    assert [b for b, _ in ok] == [0, 1]
    for b, r0 in ok:
        want[b * R:(b + 1) * R] = h_h[b, r0:r0 + R]
    assert y.dtype == dtype and torch.equal(y.cpu(), want)                 # the out-of-range sample: zero rows
    dy_h = rnd(B * R, d, seed=2).to(dtype)
    dh = torch.full((B, Sq, d), float("nan"), dtype=dtype, device=DEV)
    out = K.action_rows_bwd(dy_h.to(DEV), off, B, Sq, R, bool(skip), out=dh)
    want_dh = torch.zeros(B, Sq, d, dtype=dtype)
    for b, r0 in ok:
        want_dh[b, r0:r0 + R] = dy_h[b * R:(b + 1) * R]
    assert out is dh and torch.equal(dh.cpu(), want_dh)                    # every element written: no NaN is left
    assert torch.equal(K.action_rows_bwd(dy_h.to(DEV), off, B, Sq, R, bool(skip)).cpu(), want_dh)


def fill_reference(dx_h, off_h, B, Sq, R, s):
    terms = [dx_h[b, r0:r0 + R].double() for b, r0 in blocks(off_h, B, Sq, R, s)]
    terms = torch.cat(terms) if terms else torch.zeros(0, dx_h.shape[-1], dtype=torch.float64)
    n = max(terms.shape[0], 1)
    return terms.sum(0), n * 2.0 ** -24 * terms.abs().sum(0)


@pytest.mark.parametrize("d,dtype,skip", ROW_CASES + [(96, F32, 2), (96, BF, 2)])
def test_action_fill_forward_and_backward(d, dtype, skip):
    """skip 2 stands for the large case: B R = 16 x 14 = 224 action rows with a state row, so the sum crosses 14 first-stage
    workgroups"""
    if skip == 2:
        B, Sq, R, s = 16, 20, 14, 1
        off_h = torch.arange(B, dtype=torch.int64) % 6                    # every block fits (5 + 15 <= 20)
    else:
        B, Sq, R, s = 3, 14, 6, skip
        off_h = torch.tensor([2, Sq - R - s, Sq - R - s + 1], dtype=torch.int64)
    off = off_h.to(DEV)
    ok = blocks(off_h, B, Sq, R, s)
    for row_dtype in ((dtype,) if dtype == F32 else (BF, F32)):
        row = rnd(d, seed=1).to(row_dtype)
        st = rnd(B, d, seed=2).to(dtype) if s else None
        x = torch.full((B, Sq, d), 7.0, dtype=dtype, device=DEV)
        K.action_fill_(x, row.to(DEV), off, R, st.to(DEV) if s else None)
        want = torch.full((B, Sq, d), 7.0, dtype=dtype)
        for b, r0 in ok:
            if s:
                want[b, r0 - 1] = st[b]
            want[b, r0:r0 + R] = row.to(dtype)
        assert torch.equal(x.cpu(), want)                                  # nothing else written, the out-of-range sample untouched
    dx_h = rnd(B, Sq, d, seed=3).to(dtype)
    dx = dx_h.to(DEV)
    ref, bound = fill_reference(dx_h, off_h, B, Sq, R, s)
    drow = torch.full((d,), float("nan"), dtype=torch.float32, device=DEV)
    _, dstate = K.action_fill_bwd(dx, off, R, bool(s), drow=drow, accumulate=False, want_dstate=bool(s))
    err = (drow.double().cpu() - ref).abs()
    print(f"fill bwd d={d} {dtype} rows={len(ok) * R}: largest share of the bound used {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    first = drow.clone()
    K.action_fill_bwd(dx, off, R, bool(s), drow=drow, accumulate=True)
    assert torch.equal(drow, first + first)                                # old + sum: accumulate doubles it
    again, dstate2 = K.action_fill_bwd(dx, off, R, bool(s), want_dstate=bool(s))
    assert torch.equal(again, first)                                       # two runs, the same bits
    if s:
        want_ds = torch.zeros(B, d, dtype=dtype)
        for b, r0 in ok:
            want_ds[b] = dx_h[b, r0 - 1]
        assert dstate.dtype == dtype and torch.equal(dstate.cpu(), want_ds) and torch.equal(dstate2.cpu(), want_ds)
    else:
        assert dstate is None and dstate2 is None


# ------------------------------------------------------------------------------------------------ bins
def bins_case(d, NB, rows, dtype, skip, seed=0):
    """B samples of R = rows / B action rows at distinct offsets; w_bins = the last NB rows of a larger [V, d] matrix"""
    B = 2 if rows == 6 else 8
    R = rows // B
    Sq = R + skip + 5
    off_h = (torch.arange(B, dtype=torch.int64) * 2) % 6
    h_h = rnd(B, Sq, d, seed=seed + 1).to(dtype)
    W_h = rnd(NB + 9, d, seed=seed + 2, scale=d ** -0.5).to(dtype)
    return B, R, Sq, off_h, h_h, W_h


def check_bins(logits, bins, action, h_h, W_h, off_h, B, Sq, R, skip, NB, dtype):
    d = h_h.shape[-1]
    rows_h = torch.zeros(B * R, d, dtype=torch.float64)
    for b, r0 in blocks(off_h, B, Sq, R, skip):
        rows_h[b * R:(b + 1) * R] = h_h[b, r0:r0 + R].double()
    w = W_h[W_h.shape[0] - NB:].double()
    ref = rows_h @ w.T
    bound = d * 2.0 ** -24 * (rows_h.abs() @ w.abs().T) + (2.0 ** -8 * ref.abs() if dtype == BF else 0.0)
    lg = logits.cpu()
    err = (lg.double() - ref).abs()
    share = float((err / bound.clamp_min(1e-300)).max())
    print(f"bins d={d} NB={NB} rows={B * R} {dtype}: largest share of the bound used {share:.3f}")
    assert lg.dtype == dtype and lg.shape == (B * R, NB) and (err <= bound).all()
    assert bins.dtype == torch.int64 and torch.equal(bins.cpu(), lg.float().argmax(dim=-1))    # first index of the returned row's maximum
    assert action.dtype == torch.float32 and torch.equal(action.cpu(), (bins.cpu().float() / NB) * 2 - 1)


BINS_CASES = [(96, 1, 6), (96, 31, 6), (96, 255, 6), (96, 31, 112), (3584, 255, 6), (3584, 255, 112), (3584, 31, 112), (3584, 1, 112),
              # the two sides of the threshold (1024 output tiles of 16 x 16) from which a workgroup computes 2 x 2 tiles: 63 x 16 tiles,
              # and 65 x 17 (both counts odd, so the last row group and the last bin group are half empty)
              (96, 255, 1008), (96, 270, 1040)]


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("d,NB,rows", BINS_CASES)
def test_action_bins(d, NB, rows, dtype):
    skip = rows == 112                                                     # the larger cases carry a state row
    B, R, Sq, off_h, h_h, W_h = bins_case(d, NB, rows, dtype, int(skip))
    W = W_h.to(DEV)
    w_bins = W[W.shape[0] - NB:]
    h, off = h_h.to(DEV), off_h.to(DEV)
    logits, bins, action = K.action_bins_fwd(h, off, w_bins, R, skip)
    check_bins(logits, bins, action, h_h, W_h, off_h, B, Sq, R, int(skip), NB, dtype)
    l2, b2, a2 = K.action_bins_fwd(h, off, w_bins, R, skip)
    assert torch.equal(l2, logits) and torch.equal(b2, bins) and torch.equal(a2, action)      # two runs, the same bits


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("d,rows", [(96, 6), (3584, 112), (96, 1024)])          # the last one: 2 x 2 tiles per workgroup
def test_action_bins_exact_ties_go_to_the_lower_index(d, rows, dtype):
    """operands on a coarse grid (multiples of 1/4 in h, of 1/8 in w, a few non-zero columns) make every logit exact in every
    summation order, and every weight row appears twice: each row's maximum is attained at least twice, exactly"""
    NB = 255
    B = 2 if rows == 6 else 8
    R, Sq = rows // B, rows // B + 4
    off_h = torch.arange(B, dtype=torch.int64) % 4
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    h_h = torch.zeros(B, Sq, d)
    h_h[..., :16] = torch.randint(-8, 9, (B, Sq, 16), generator=g).float() / 4
    half = torch.zeros(127, d)
    half[:, :16] = torch.randint(-8, 9, (127, 16), generator=g).float() / 8
    perm = torch.randperm(255, generator=g)
    W_h = torch.cat([half, half, half[:1]])[perm]                          # every weight row occurs twice (one three times), shuffled
    h_h, W_h = h_h.to(dtype), W_h.to(dtype)
    logits, bins, action = K.action_bins_fwd(h_h.to(DEV), off_h.to(DEV), W_h.to(DEV), R, False)
    rows_h = torch.cat([h_h[b, int(off_h[b]):int(off_h[b]) + R] for b in range(B)]).double()
    exact = rows_h @ W_h.double().T                                        # every partial sum is a multiple of 1/32 below 2^8
    assert torch.equal(exact.float().double(), exact)
    ref = exact.float().to(dtype).double()                                 # rounded once (bf16): equal values stay equal
    assert torch.equal(logits.cpu().double(), ref)
    top = ref.max(dim=-1, keepdim=True).values
    assert bool(((ref == top).sum(dim=-1) >= 2).all())                     # every row's maximum is attained at least twice
    assert torch.equal(bins.cpu(), ref.argmax(dim=-1))                     # torch: the first of them
    first = torch.tensor([int((ref[r] == top[r]).nonzero()[0]) for r in range(rows)])
    assert torch.equal(bins.cpu(), first)
    assert torch.equal(action.cpu(), (bins.cpu().float() / NB) * 2 - 1)


def test_action_bins_out_of_range_sample_and_argument_codes():
    d, NB, R, B, Sq = 96, 31, 6, 3, 10
    off_h = torch.tensor([1, 5, -2], dtype=torch.int64)                    # sample 1: 5 + 6 > 10; sample 2: negative
    h_h, W_h = rnd(B, Sq, d, seed=1), rnd(NB, d, seed=2, scale=0.1)
    logits, bins, action = K.action_bins_fwd(h_h.to(DEV), off_h.to(DEV), W_h.to(DEV), R, False)
    check_bins(logits, bins, action, h_h, W_h, off_h, B, Sq, R, 0, NB, F32)
    assert bool((logits[R:] == 0).all()) and bool((bins[R:] == 0).all()) and bool((action[R:] == -1).all())
    assert bool((logits[:R] != 0).any())
    # refused before any launch: a width the 16-byte operand loads cannot take, a misaligned weight view
    for bad_h, bad_w in ((rnd(B, Sq, 98), rnd(NB, 98)), (rnd(B, Sq, 100).to(BF), rnd(NB, 100).to(BF))):
        with pytest.raises(L.DxaError, match="multiple of"):
            K.action_bins_fwd(bad_h.to(DEV), off_h.to(DEV), bad_w.to(DEV), R, False)
    flat = rnd(NB * d + 1).to(DEV)
    with pytest.raises(L.DxaError, match="16-byte aligned"):
        K.action_bins_fwd(h_h.to(DEV), off_h.to(DEV), flat[1:].view(NB, d), R, False)
