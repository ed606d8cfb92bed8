"""fp64 reference of the entry points of csrc/loss.hip that tests/loss_cases.py covers, from the formulas of
include/dexbotic_amd.h, computed from the stored (bf16 or fp32) inputs:

  forward        lse = M + log(sum_j exp(x_j - M)), M = max_j x_j (a -inf entry adds 0; nothing but -inf: lse = -inf; a NaN: NaN)
                 row_loss = lse - x[label]; a soft row (label among the K soft ids): lse - sum_k p_k x[s_k],
                 p_k = e_k / sum_k e_k, e_k = exp(-(label - s_k)^2 inv2s2); an ignored row (label == ignore_index or outside
                 [0, V)): 0
  backward       dlogits = rnd((exp(x - lse) - [j == label]) g), a soft row (exp(x - lse) - p_k) g at the soft ids;
                 g = gscale * scale (* row_w[r]); an ignored row: 0.  lse is what the kernel's own forward returned.
  sample reduce  w_b = 1 + 1 / (1 + exp(-reward_b)); den_b = max(n_b, 1) B; loss = sum_b w_b (sum_t row_loss[b, t]) / den_b over
                 the non-ignored labels; row_w[b, t] = w_b / den_b
  expectile      d = pred - target; w = tau if d < 0 else 1 - tau; loss = sum(w d^2) / n; dpred = (2 / n gscale) w d
  argmax         the first NaN's index, else the first index of the maximum (-0 == +0)

rnd rounds to the storage type (bf16; nothing for fp32).  ``mag`` of an output element is the sum of the absolute values of the
terms that made it, a term that went through exp() counted with (1 + |argument|) — the rounding of the argument is a relative
error of the value:
  lse        |M| + |log S| + sum_j p_j (1 + |x_j - M|)          (S = sum exp(x_j - M); the last sum is the relative error of S)
  row_loss   mag(lse) + |x[label]|; a soft row: mag(lse) + sum_k pm_k |x[s_k]|, pm_k = p_k (2 + a_k + sum_j p_j a_j), a = d^2 inv2s2
  dlogits    (p (1 + |x - lse|) + [j == label]) |g|; a soft column: (p (1 + |x - lse|) + pm_k) |g|
  sample     mw_b = 1 + s (2 + (1 - s)(1 + |reward_b|)), s the sigmoid (1 without rewards);  loss: sum_b mw_b sum_t |row_loss| / den_b;
             row_w: mw_b / den_b
  expectile  the value itself (its terms w d^2 have one sign; dpred is a product)
``emulate`` is the same formulas evaluated in plain fp32 torch on the CPU: what the slack constants of loss_cases.py are
measured from."""
import math

import torch

from tests import loss_cases as LC
from tests.norm_ref import ulp_bf16

TWO24 = 2.0 ** -24


def _rnd(t, dtype):
    return t.to(torch.bfloat16).to(t.dtype) if dtype == "bf16" else t


def _f32(v, ft):
    """a C float argument as the kernel receives it"""
    return torch.tensor(v, dtype=torch.float32).to(ft)


def _soft(lab, ids, ft):
    """soft targets of a row labelled ``lab``: (e_k, p_k, pm_k)"""
    d = (lab - ids).to(ft)                                    # exact: the integer difference
    a = (d * d) * _f32(LC.INV2S2, ft)
    e = torch.exp(-a)
    p = e / e.sum()
    return e, p, p * (2.0 + a + (p * a).sum())


def _zero_times(w, v):
    """w * v with 0 * inf = 0"""
    return torch.where(w > 0, w * v, torch.zeros_like(w))


def _ce_fwd(case, inp, ft):
    x = inp["logits"].to(ft)
    labels, V = inp["labels"], case["V"]
    ign = LC.ignored(labels, V, case["ignore_index"])
    ids = inp.get("soft_ids")
    M = x.max(1).values
    sh = torch.where(M == -math.inf, torch.zeros_like(M), M)
    e = torch.exp(x - sh[:, None])
    S = e.sum(1)
    lse = M + torch.log(S)
    mlse = M.abs() + torch.log(S).abs() + _zero_times(e, 1.0 + (x - sh[:, None]).abs()).sum(1) / S
    row_loss, mrl = torch.zeros_like(lse), torch.zeros_like(lse)
    for r in range(case["rows"]):
        lab = int(labels[r])
        if ign[r]:
            continue
        if ids is not None and lab in ids.tolist():
            e_k, _, pm = _soft(lab, ids, ft)
            row_loss[r] = lse[r] - (e_k * x[r, ids]).sum() / e_k.sum()
            mrl[r] = mlse[r] + (pm * x[r, ids].abs()).sum()
        else:
            row_loss[r] = lse[r] - x[r, lab]
            mrl[r] = mlse[r] + x[r, lab].abs()
    return {"lse": (lse, "lse", 0), "row_loss": (row_loss, "row_loss", 0)}, {"lse": mlse, "row_loss": mrl}


def _ce_bwd(case, inp, stats, ft):
    x = inp["logits"].to(ft)
    labels, V, dt = inp["labels"], case["V"], case["dtype"]
    ign = LC.ignored(labels, V, case["ignore_index"])
    ids = inp.get("soft_ids")
    l = stats["lse"].to(ft)
    g = (inp["gscale"].to(ft)[0] if "gscale" in inp else torch.ones((), dtype=ft)) * _f32(LC.SCALE, ft)
    g = g.expand(case["rows"]).clone()
    if "row_w" in inp:
        g = g * inp["row_w"].to(ft)
    g = torch.where(ign, torch.zeros_like(g), g)
    z = x - l[:, None]
    p = torch.where(ign[:, None], torch.zeros_like(x), torch.exp(z))
    tgt, tm = torch.zeros_like(x), torch.zeros_like(x)
    for r in range(case["rows"]):
        lab = int(labels[r])
        if ign[r]:
            continue
        if ids is not None and lab in ids.tolist():
            _, tgt[r, ids], tm[r, ids] = _soft(lab, ids, ft)
        else:
            tgt[r, lab] = tm[r, lab] = 1.0
    d = torch.where(ign[:, None], torch.zeros_like(x), (p - tgt) * g[:, None])
    mag = (_zero_times(p, 1.0 + z.abs()) + tm) * g.abs()[:, None]
    return {"dlogits": (_rnd(d, dt), "dlogits", 1 if dt == "bf16" else 0)}, {"dlogits": mag}


def _sample_reduce(case, inp, ft):
    B, L = case["B"], case["L"]
    rl = inp["row_loss"].to(ft).view(B, L)
    valid = (~LC.ignored(inp["labels"], LC.SAMPLE_V, -100)).view(B, L)
    n = valid.sum(1)
    s = (rl * valid).sum(1)
    sa = (rl.abs() * valid).sum(1)
    if "reward" in inp:
        r = inp["reward"].to(ft)
        sig = 1.0 / (1.0 + torch.exp(-r))
        w = 1.0 + sig
        mw = 1.0 + sig * (2.0 + (1.0 - sig) * (1.0 + r.abs()))
    else:
        w = mw = torch.ones(B, dtype=ft)
    den = torch.clamp(n, min=1).to(ft) * B
    outs = {"loss": ((w * s / den).sum().view(1), "sample_loss", 0), "row_w": ((w / den)[:, None].expand(B, L).reshape(-1), "row_w", 0)}
    mags = {"loss": (mw * sa / den).sum().view(1), "row_w": (mw / den)[:, None].expand(B, L).reshape(-1)}
    return outs, mags


def _expectile(case, inp, ft):
    n = case["n"]
    d = inp["pred"].to(ft) - inp["target"].to(ft)
    tau = _f32(case["tau"], ft)
    w = torch.where(d < 0, tau, 1.0 - tau)
    loss = ((w * d * d).sum() / n).view(1)
    outs, mags = {"loss": (loss, "expectile_loss", 0)}, {"loss": loss.abs()}
    if case["dpred"]:
        k = _f32(2.0, ft) / n * _f32(inp["gscale"], ft)
        outs["dpred"] = (k * w * d, "dpred", 0)
        mags["dpred"] = (k * w * d).abs()
    return outs, mags


def argmax_ref(x):
    """torch.argmax's rule, spelled out: the first NaN's index if the row holds one, else the first index of the maximum"""
    x = x.double()
    nan = torch.isnan(x)
    mx = torch.where(nan, torch.full_like(x, -math.inf), x).max(1, keepdim=True).values
    first = lambda m: torch.where(m.any(1), m.to(torch.int8).argmax(1), torch.zeros(m.shape[0], dtype=torch.int64))
    return torch.where(nan.any(1), first(nan), first(x == mx))


def formulas(case, inp, stats=None, ft=torch.float64):
    """outputs of the case's entry point computed in ``ft``: ``{name: (value, kind, U)}`` and ``{name: mag}``.  ``stats``: the
    forward's lse (fp32) for a backward case."""
    e = case["entry"]
    if e in LC.FWD:
        return _ce_fwd(case, inp, ft)
    if e in LC.BWD:
        return _ce_bwd(case, inp, stats, ft)
    if e == "sample_reduce":
        return _sample_reduce(case, inp, ft)
    if e == "expectile":
        return _expectile(case, inp, ft)
    raise AssertionError(e)


def reference(case, inp, stats=None):
    """fp64 reference: ``{name: (value, kind, U, mag)}``"""
    outs, mags = formulas(case, inp, stats, torch.float64)
    return {n: (v, k, U, mags[n]) for n, (v, k, U) in outs.items()}


def emulate(case, inp, stats=None):
    """the same formulas in plain fp32 (CPU torch): ``{name: value}`` (bf16 outputs rounded to bf16)"""
    outs, _ = formulas(case, inp, stats, torch.float32)
    return {n: v for n, (v, k, U) in outs.items()}


def forward_case(case):
    """the forward case whose lse a backward case takes: same sizes, layout of the logits, labels, soft ids and inputs"""
    return dict(case, entry="soft_fwd" if case["entry"] == "soft_bwd" else "ce_fwd")


def excess(got, ref, U, mag):
    """per element: the error beyond U ulp in units of 2^-24 * mag; inf where mag is 0 and the error is not, and where a
    non-finite reference element is not matched by the same non-finite value (or a finite one by a non-finite one)"""
    got = got.double()
    fin = torch.isfinite(ref)
    same = (torch.isnan(ref) & torch.isnan(got)) | (ref == got)
    r = torch.where(fin, ref, torch.zeros_like(ref))
    err = (torch.where(fin, got, torch.zeros_like(got)) - r).abs() - (U * ulp_bf16(r) if U else 0.0)
    err = torch.clamp(err, min=0.0)
    unit = TWO24 * torch.where(fin, mag, torch.ones_like(mag))
    ex = torch.where(err == 0, torch.zeros_like(err), err / torch.where(unit > 0, unit, torch.full_like(unit, math.nan))).nan_to_num(
        nan=math.inf)
    return torch.where(fin, ex, torch.where(same, torch.zeros_like(ex), torch.full_like(ex, math.inf)))


def not_bit_equal(got, ref):
    """elements of a bf16 output that differ from the reference rounded to bf16 (a NaN equals a NaN)"""
    g, r = got.to(torch.bfloat16), ref.to(torch.bfloat16)
    return int(((g.view(torch.int16) != r.view(torch.int16)) & ~(torch.isnan(g) & torch.isnan(r))).sum())
