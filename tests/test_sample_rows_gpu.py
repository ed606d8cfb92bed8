"""dxa_sample_rows on the GPU against the installed transformers' warpers (kept set, exactly) and a float64 CDF (the draw)."""
import pytest
import torch

from dexbotic_amd import kernels as K

from . import sample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
U_LAST = 1.0 - 2.0 ** -24                 # the largest fp32 below 1

# the reduced parameter sets of the one-row cases at the full vocabulary
BIG = ((0.7, 50, 1.0), (1.0, 0, 1.0), (0.7, 50, 0.9), (1.0, 0, 0.5))

CASES = [(V, 64, dt, "dense", None) for V in (1, 7, 257, 8192, 8200) for dt in (BF16, F32)] + [
    (257, 1, F32, "dense", None),
    (8192, 3, BF16, "dense", None),
    (8200, 3, BF16, "wide", None),            # ld = V + 24: rows of a slice of a wider tensor
    (8200, 3, F32, "wide", None),
    (8200, 3, BF16, "misaligned", None),      # a row pointer that is not 16-byte aligned
    (8200, 3, F32, "misaligned", None),
    (152064, 3, BF16, "dense", None),
    (152064, 1, BF16, "dense", BIG),
    (152064, 1, F32, "dense", BIG),
    (152064, 3, F32, "dense", BIG),
]


def on_device(x32, dtype, layout):
    rows, V = x32.shape
    if layout == "dense":
        return x32.to(DEV, dtype)
    if layout == "wide":
        wide = torch.full((rows, V + 24), 30.0, dtype=dtype, device=DEV)          # what lies beside the rows would win every draw
        wide[:, :V] = x32.to(DEV, dtype)
        x = wide[:, :V]
        assert x.stride(0) == V + 24
        return x
    flat = torch.full((rows * V + 8,), 30.0, dtype=dtype, device=DEV)
    x = flat[1:1 + rows * V].view(rows, V)
    x.copy_(x32.to(DEV, dtype))
    assert x.data_ptr() % 16 != 0
    return x


@pytest.mark.parametrize("V,rows,dtype,layout,combos", CASES,
                         ids=[f"V{c[0]}-r{c[1]}-{'bf16' if c[2] == BF16 else 'f32'}-{c[3]}{'-few' if c[4] else ''}" for c in CASES])
def test_kept_set_and_draw_match_hf(V, rows, dtype, layout, combos):
    combos = tuple(R.grid(V)) if combos is None else combos
    x32, top_idx = R.make_rows(V, rows, dtype, combos)
    R.assert_inputs(x32, top_idx, dtype, combos)
    x = on_device(x32, dtype, layout)
    g = torch.Generator().manual_seed(1234 + V)
    for T, k, p in combos:
        what = f"T={T} k={k} p={p}"
        keep = torch.isfinite(R.hf_warp(x32, T, k, p))
        pr, C = R.cdf64(x32, keep, T)
        for u in (torch.rand(rows, generator=g), torch.zeros(rows), torch.full((rows,), U_LAST)):
            token, kept, thresh, prob = K.sample_rows(x, u.to(DEV), T, k, p, return_info=True)
            mine = x32 >= thresh.cpu()[:, None]
            assert torch.equal(mine, keep), (what, "kept set", (mine != keep).sum(dim=-1))
            assert torch.equal(kept.cpu().long(), keep.sum(dim=-1)), what
            R.check_draw(token, prob, u, keep, pr, C, what)
            assert torch.equal(K.sample_rows(x, u.to(DEV), T, k, p), token)             # the optional outputs are optional


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_top_k_keeps_every_entry_tied_at_the_threshold(dtype):
    V, k = 300, 5
    x32 = torch.linspace(-6.0, -3.0, V).to(BF16).float().repeat(2, 1)
    x32[0, [17, 40, 99, 250]] = torch.tensor([4.0, 3.0, 2.5, 2.0])
    x32[0, [7, 120, 299]] = 1.5                                        # the 5th, 6th and 7th largest are equal
    x32[1, [0, 1, 2, 3, 4, 5]] = torch.tensor([1.5, 1.5, 1.5, 1.5, 1.5, 1.5])          # k-th value inside a run of six
    keep = torch.isfinite(R.hf_warp(x32, 1.0, k, 1.0))
    assert keep.sum(dim=-1).tolist() == [7, 6]                         # HF keeps all of them too
    u = torch.tensor([0.999, 0.5])
    token, kept, thresh, prob = K.sample_rows(x32.to(DEV, dtype), u.to(DEV), 1.0, k, 1.0, return_info=True)
    assert torch.equal(x32 >= thresh.cpu()[:, None], keep) and kept.tolist() == [7, 6]
    R.check_draw(token, prob, u, keep, *R.cdf64(x32, keep, 1.0))


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_degenerate_rows(dtype):
    V = 1000
    x = torch.full((3, V), -float("inf"))
    x[1, 5:9] = torch.tensor([0.5, float("nan"), 0.25, -float("inf")])        # a NaN (and -inf) among finite values
    x[2] = torch.randn(V, generator=torch.Generator().manual_seed(3))
    x[2, 0] = float("nan")
    x[2, 500] = float("nan")
    xd = x.to(DEV, dtype)
    for uval in (0.0, 0.3, 0.77, U_LAST):
        u = torch.full((3,), uval, device=DEV)
        for T, k, p in ((1.0, 0, 1.0), (0.7, 5, 1.0), (1.0, 0, 0.9), (0.7, 3, 0.5)):
            token, kept, thresh, prob = K.sample_rows(xd, u, T, k, p, return_info=True)
            assert int(token[0]) == 0 and int(kept[0]) == 0 and float(prob[0]) == 0.0          # all -inf: index 0
            assert int(token[1]) in (5, 7) and int(kept[1]) <= 2
            assert int(token[2]) not in (0, 500) and torch.isfinite(x[2, int(token[2])])
            assert int(kept[2]) <= V - 2


@pytest.mark.parametrize("V,dtype", [(257, F32), (8200, BF16), (152064, BF16)])
def test_top_k_1_is_argmax_for_every_u(V, dtype):
    rows = 3
    x32, _ = R.make_rows(V, rows, dtype, ((0.7, 1, 1.0),))               # the maximum of a built row is unique
    x = x32.to(DEV, dtype)
    want = K.argmax_rows(x)
    assert torch.equal(want.cpu(), x32.argmax(dim=-1))
    for uval in (0.0, 0.25, 0.5, 0.999, U_LAST):
        token, kept, _, prob = K.sample_rows(x, torch.full((rows,), uval, device=DEV), 0.7, 1, 1.0, return_info=True)
        assert torch.equal(token, want) and kept.tolist() == [1] * rows and prob.tolist() == [1.0] * rows


@pytest.mark.parametrize("V,rows,dtype", [(8200, 64, F32), (152064, 3, BF16)])
def test_same_call_gives_the_same_bits(V, rows, dtype):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, V, generator=g).to(DEV, dtype)                 # ties and all
    u = torch.rand(rows, generator=g).to(DEV)
    for T, k, p in ((0.7, 50, 1.0), (1.0, 0, 0.9), (0.7, 50, 0.9), (1.0, 0, 1.0)):
        first = K.sample_rows(x, u, T, k, p, return_info=True)
        for _ in range(2):
            again = K.sample_rows(x, u, T, k, p, return_info=True)
            assert all(torch.equal(a, b) for a, b in zip(first, again)), (T, k, p)
