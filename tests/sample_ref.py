"""CPU truth for the sampled-decoding tests: the installed transformers' logits warpers on fp32 CPU tensors, a float64 softmax /
cumulative sum for the draw, and rows of logits built so that the comparison with them is exact (see make_rows)."""
import functools

import numpy as np
import torch
from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

EPS_U = 2.0 ** -15        # draw: a 1024-thread block sums <= 149 fp32 terms per thread serially (149 * 2^-24 ~ 9e-6), plus about
#                           10 reduction levels and expf's few ulp
N_TOP = 256               # the largest entries of a built row that are pairwise distinct
P_MARGIN = 1e-4           # no ascending cumulative sum of a built row lies this close to 1 - top_p

TEMPERATURES = (0.7, 1.0, 0.05)
TOP_PS = (1.0, 0.9, 0.5)


def top_ks(V):
    return (0, 1, 5, 50, V + 3)


def grid(V):
    return [(T, k, p) for T in TEMPERATURES for k in top_ks(V) for p in TOP_PS]


def hf_warp(x32, T, k, p):
    """HF's warpers in generate()'s order on fp32 CPU scores [rows, V]; k <= 0 and p >= 1 mean off, as in generate()"""
    s = TemperatureLogitsWarper(float(T))(None, x32)
    if k > 0:
        s = TopKLogitsWarper(top_k=int(k))(None, s)
    if p < 1.0:
        s = TopPLogitsWarper(top_p=float(p))(None, s)
    return s


def cdf64(x32, keep, T):
    """float64 probabilities of the kept entries and their normalised cumulative sum in ascending index order"""
    z = x32.double() / T
    z = torch.where(keep, z, torch.full_like(z, -float("inf")))
    pr = torch.softmax(z, dim=-1)
    return pr, pr.cumsum(dim=-1)


def check_draw(token, prob, u, keep, pr, C, what=""):
    """the returned token j is kept, C[j-1] - eps <= u <= C[j] + eps, prob within 1e-5 + 1e-4 p of the float64 probability;
    (pr, C) = cdf64(x32, keep, T)"""
    rows = torch.arange(keep.shape[0])
    j = token.cpu().long()
    assert bool(keep[rows, j].all()), (what, "a token outside the kept set", j[~keep[rows, j]])
    hi = C[rows, j]
    lo = torch.where(j > 0, C[rows, (j - 1).clamp(min=0)], torch.zeros_like(hi))
    ud = u.cpu().double()
    bad = (ud < lo - EPS_U) | (ud > hi + EPS_U)
    assert not bool(bad.any()), (what, "draw outside its CDF interval", rows[bad], j[bad], lo[bad], ud[bad], hi[bad])
    if prob is not None:
        pj = pr[rows, j]
        err = (prob.cpu().double() - pj).abs()
        assert bool((err <= 1e-5 + 1e-4 * pj).all()), (what, "prob", err.max())


def _bf16_values():
    """every bf16 value v with 2^-3 <= |v| and -20 < v < 8, as fp32"""
    v = (np.arange(1 << 16, dtype=np.uint32) << 16).view(np.float32)
    return v[np.isfinite(v) & (np.abs(v) >= 0.125) & (v > -20) & (v < 8)]


def _one_row(V, dtype, rs):
    n = min(N_TOP, V)
    vals = _bf16_values()
    if dtype == torch.bfloat16:
        top = rs.choice(vals, n, replace=False)
    else:
        # fp32: few distinct upper halves and few distinct low bytes, so that entries share 16 and 24 leading bits
        while True:
            hi = rs.choice(vals[::16], n).view(np.uint32)
            bits = hi | rs.randint(0, 1024, n).astype(np.uint32) | (rs.randint(0, 4, n).astype(np.uint32) << 14)
            if len(np.unique(bits)) == n:
                break
        top = bits.view(np.float32)
    rest = top.min() - 1 - 8 * rs.random_sample(V - n).astype(np.float32)
    rest = torch.from_numpy(rest).to(torch.bfloat16).float().numpy()          # ties allowed (and many, at a large V)
    perm = rs.permutation(V)
    x = np.empty(V, dtype=np.float32)
    x[perm[:n]] = top
    x[perm[n:]] = rest
    return x, perm[:n]


def _rows_ok(x32, top_idx, combos):
    """per row: for every (T, k, p < 1), the nucleus lies inside the N_TOP distinct entries and no ascending cumulative sum is
    within P_MARGIN of 1 - top_p (float64)"""
    rows, V = x32.shape
    in_top = torch.zeros(rows, V, dtype=torch.bool)
    in_top.scatter_(1, top_idx, True)
    ok = torch.ones(rows, dtype=torch.bool)
    seen = set()
    for T, k, p in combos:
        k = 0 if k >= V else k
        if p >= 1.0 or (T, k, p) in seen:
            continue
        seen.add((T, k, p))
        pre = hf_warp(x32, T, k, 1.0)
        cs = torch.softmax(pre.double().sort(dim=-1).values, dim=-1).cumsum(dim=-1)
        ok &= ((cs - (1 - p)).abs() > P_MARGIN).all(dim=-1)
        kept = torch.isfinite(hf_warp(x32, T, k, p))
        ok &= ~(kept & ~in_top).any(dim=-1)
    return ok


@functools.lru_cache(maxsize=None)
def make_rows(V, rows, dtype, combos=None, seed=0):
    """fp32 CPU logits [rows, V], exactly representable in ``dtype``: the min(256, V) largest entries of a row are pairwise distinct
    values scattered by a seeded permutation, the rest lies below them with ties; row seeds are picked (in order, on the CPU) so that
    _rows_ok holds for every parameter set in ``combos`` (default: the whole grid).  Returns (x32, top_idx)."""
    combos = tuple(grid(V)) if combos is None else combos
    xs, tops = [None] * rows, [None] * rows
    todo, nxt = list(range(rows)), 0
    for _ in range(40):
        for r in todo:
            xs[r], tops[r] = _one_row(V, dtype, np.random.RandomState(1000 * seed + 7919 * V % 1000003 + nxt))
            nxt += 1
        x32 = torch.from_numpy(np.stack([xs[r] for r in todo]))
        ok = _rows_ok(x32, torch.from_numpy(np.stack([tops[r] for r in todo])).long(), combos)
        todo = [r for r, good in zip(todo, ok.tolist()) if not good]
        if not todo:
            break
    assert not todo, "no seed found for some rows"
    x32 = torch.from_numpy(np.stack(xs))
    top_idx = torch.from_numpy(np.stack(tops)).long()
    return x32, top_idx


def assert_inputs(x32, top_idx, dtype, combos):
    """the conditions on the inputs, stated in the tests that rely on them"""
    assert torch.equal(x32.to(dtype).float(), x32)                                        # exact in the tested dtype
    rows, V = x32.shape
    n = top_idx.shape[1]
    top = x32.gather(1, top_idx).to(dtype).float()
    assert all(len(torch.unique(top[r])) == n for r in range(rows))                       # pairwise distinct after rounding
    assert n == min(N_TOP, V)
    if n < V:
        rest_max = x32.scatter(1, top_idx, -float("inf")).max(dim=-1).values
        assert bool((rest_max < top.min(dim=-1).values).all())                            # and they are the largest
    assert bool(_rows_ok(x32, top_idx, combos).all())
