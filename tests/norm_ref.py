"""fp64 reference of the norm entry points of csrc/norm.hip (RMSNorm, LayerNorm, add-LayerNorm forward and backward, dxa_colsum),
computed from the stored (bf16 or fp32) inputs, with the kernels' rounding points and no others:

  RMSNorm fwd     rstd = 1 / sqrt(sum(x^2) / C + eps);  y = rnd(w * rnd(x * rstd))
  RMSNorm bwd     xh = x * rstd;  c2 = sum(dy w xh) / C;  dx = rnd(rstd (dy w - xh c2) + res)   (one rounding)
                  dw = sum_rows dy * rnd(xh)
  LayerNorm fwd   mean, rstd = 1 / sqrt(sum((x - mean)^2) / C + eps);  y = rnd((x - mean) rstd w + b)
  LayerNorm bwd   xh = (x - mean) rstd;  c1 = sum(dy w) / C;  c2 = sum(dy w xh) / C;  dx = rnd(rstd (dy w - c1 - xh c2) + res)
                  dw = sum_rows dy * xh (xh NOT rounded),  db = sum_rows dy
  add-LayerNorm   LayerNorm of x + x2, the sum formed exactly and never rounded; the backward's dx is that of both addends
  colsum          out = sum_rows x (+ out)

rnd rounds to the storage type (bf16; nothing for fp32); mean / rstd and the weight gradients are fp32.  Every route of an entry
point rounds at the same points (norm.hip: rmsnorm_bwd_k, norm_bwd_fast_k, norm_bwd_fast8_k and rmsnorm_bwd_split_k all add
dy * rnd<T>(xh) to dw; the LayerNorm kernels add dy * xh).  The backward takes the mean / rstd the kernel's own forward
returned, so a backward case does not inherit the forward's error.

``mag`` of an output element is the sum of the absolute values of the terms that made it (row sums enter through their own
magnitudes: |x| + sum|x| / C for x - mean, sum|dy w xh| / C for c2, ...); for the column sums and weight gradients the sum over
rows.  ``emulate`` is the same formulas evaluated in plain fp32 torch on the CPU: what the slack constant of norm_cases.py is
measured from."""
import torch

from tests.norm_cases import EPS

TWO24 = 2.0 ** -24


def _rnd(t, dtype, on=True):
    return t.to(torch.bfloat16).to(t.dtype) if (on and dtype == "bf16") else t


def formulas(case, inp, stats=None, ft=torch.float64, rounding=True):
    """outputs of the case's entry point, computed in ``ft``: ``{name: (value, kind, U)}``, and with ft = fp64 also
    ``{name: mag}``.  ``stats``: the forward's mean / rstd (fp32 tensors) for a backward case."""
    e, C, dt = case["entry"], case["cols"], case["dtype"]
    U = 1 if dt == "bf16" else 0
    f = lambda n: inp[n].to(ft) if n in inp else None
    r = lambda t: _rnd(t, dt, rounding)
    outs, mags = {}, {}
    if e.startswith("downsample"):
        return _downsample(case, inp, stats, ft, rounding)
    if e.startswith(("adarms", "gated_residual")):
        return _adarms(case, inp, stats, ft, rounding)
    if e == "colsum":
        x = f("x")
        s = x.sum(0)
        m = x.abs().sum(0)
        if case["accumulate"]:
            s = s + f("y0")
            m = m + f("y0").abs()
        outs["out"] = (s, "colsum", 0)
        mags["out"] = m
        return outs, mags
    x = f("x")
    xa = x.abs()
    if e.startswith("add_"):
        x2 = f("x2")
        x, xa = x + x2, xa + x2.abs()
    w = f("w") if "w" in inp else torch.ones(C, dtype=ft)
    b = f("b") if "b" in inp else torch.zeros(C, dtype=ft)
    rms = e.startswith("rms")
    if e.endswith("_fwd"):
        if rms:
            rstd = 1.0 / torch.sqrt((x * x).sum(1) / C + EPS)
            xh = x * rstd[:, None]
            outs["y"] = (r(w * r(xh)), "y", U)
            mags["y"] = (w * xh).abs()
        else:
            mean = x.sum(1) / C
            d = x - mean[:, None]
            rstd = 1.0 / torch.sqrt((d * d).sum(1) / C + EPS)
            outs["y"] = (r(d * rstd[:, None] * w + b), "y", U)
            outs["mean"] = (mean, "stat", 0)
            mabs = xa.sum(1) / C
            mags["y"] = (xa + mabs[:, None]) * rstd[:, None] * w.abs() + b.abs()
            mags["mean"] = mabs
        outs["rstd"] = (rstd, "stat", 0)
        mags["rstd"] = rstd.abs()
        return outs, mags
    dy = f("dy")
    res = f("residual")
    rs = stats["rstd"].to(ft)[:, None]
    g = dy * w
    if rms:
        xh = x * rs
        xm = xa * rs
    else:
        mu = stats["mean"].to(ft)[:, None]
        xh = (x - mu) * rs
        xm = (xa + mu.abs()) * rs
    c2 = (g * xh).sum(1, keepdim=True) / C
    c2m = (g.abs() * xm).sum(1, keepdim=True) / C
    if rms:
        o = rs * (g - xh * c2)
        m = rs * (g.abs() + xm * c2m)
    else:
        c1 = g.sum(1, keepdim=True) / C
        o = rs * (g - c1 - xh * c2)
        m = rs * (g.abs() + g.abs().sum(1, keepdim=True) / C + xm * c2m)
    if res is not None:
        o, m = o + res, m + res.abs()
    outs["dx"] = (r(o), "dx", U)
    mags["dx"] = m
    if "w" in inp:
        if rms:
            t = dy * r(xh)
            outs["dw"] = (t.sum(0), "dw", 0)
            mags["dw"] = t.abs().sum(0)
        else:
            outs["dw"] = ((dy * xh).sum(0), "dw", 0)
            mags["dw"] = (dy.abs() * xm).sum(0)
            outs["db"] = (dy.sum(0), "dw", 0)
            mags["db"] = dy.abs().sum(0)
    return outs, mags


def merge(x, G):
    """[N, G*G, C] -> [N * h * h, 4C]: zero pad to an even grid, output token o = j*h + i (j column pair, i row pair) =
    [x(2i,2j) | x(2i,2j+1) | x(2i+1,2j) | x(2i+1,2j+1)]"""
    N, _, C = x.shape
    Gp = G + (G & 1)
    h = Gp // 2
    g = torch.nn.functional.pad(x.view(N, G, G, C), (0, 0, 0, Gp - G, 0, Gp - G))
    return g.view(N, h, 2, h, 2, C).permute(0, 3, 1, 2, 4, 5).reshape(N * h * h, 4 * C)


def unmerge(m, N, G, C):
    """the inverse of merge on the real tokens: [N * h * h, 4C] -> [N, G*G, C]"""
    Gp = G + (G & 1)
    h = Gp // 2
    g = m.reshape(N, h, h, 2, 2, C).permute(0, 2, 3, 1, 4, 5).reshape(N, Gp, Gp, C)
    return g[:, :G, :G].reshape(N, G * G, C)


def _downsample(case, inp, stats, ft, rounding):
    """2x2 token merge + LayerNorm(4C): LayerNorm of the merged rows (padded positions are zeros that count), the same rounding
    points; dx goes back to the un-merged layout (padded positions have none)"""
    N, G, C = case["rows"], case["G"], case["cols"]
    inner = dict(case, entry=case["entry"].replace("downsample_layernorm", "layernorm"), cols=4 * C, res=False)
    outs, mags = formulas(inner, dict(inp, x=merge(inp["x"], G)), stats, ft, rounding)
    if "dx" in outs:
        v, kind, U = outs["dx"]
        outs["dx"] = (unmerge(v, N, G, C), kind, U)
        mags["dx"] = unmerge(mags["dx"], N, G, C)
    return outs, mags


def _adarms(case, inp, stats, ft, rounding):
    """adaptive RMSNorm / gated residual (pi0.5), per sample s = row // rps, mod = [scale | shift | gate], gate = modp[s, 2C:]:
      adarms fwd      r = rnd(x + branch * gate) (gated; else r = x);  y = rnd(r rstd (1 + scale) + shift)
      adarms bwd      g = dy (1 + scale);  xh = r rstd;  o = rstd (g - xh sum(g xh) / C) + res;  dr = rnd(o)
                      dscale = rnd(sum_rows dy xh), dshift = rnd(sum_rows dy);  gated: dbranch = rnd(o gate), dgate = rnd(sum_rows o branch)
      gated residual  y = rnd(x + branch * gate);  dbranch = rnd(dy gate), dgate = rnd(sum_rows dy branch)
    (the per-sample sums are rounded once to the storage type)"""
    e, C, dt, rps, B = case["entry"], case["cols"], case["dtype"], case["rps"], case["B"]
    U = 1 if dt == "bf16" else 0
    rn = lambda t: _rnd(t, dt, rounding)
    rep = lambda t: t.repeat_interleave(rps, 0)
    per = lambda t: t.view(B, rps, C).sum(1)
    f = lambda n: inp[n].to(ft) if n in inp else None
    outs, mags = {}, {}
    gate = rep(f("modp")[:, 2 * C:]) if case["gated"] else None
    br = f("x2")
    if e.startswith("gated_residual"):
        if e.endswith("_fwd"):
            x = f("x")
            outs["y"] = (rn(x + br * gate), "y", U)
            mags["y"] = x.abs() + (br * gate).abs()
        else:
            dy = f("dy")
            outs["dx"] = (rn(dy * gate), "dx", U)
            mags["dx"] = (dy * gate).abs()
            outs["dgate"] = (rn(per(dy * br)), "dw", U)
            mags["dgate"] = per((dy * br).abs())
        return outs, mags
    mod = f("mod")
    sc, sh = rep(mod[:, :C]), rep(mod[:, C:2 * C])
    if e.endswith("_fwd"):
        x = f("x")
        if case["gated"]:
            r = rn(x + br * gate)
            outs["aux"] = (r, "y", U)
            mags["aux"] = x.abs() + (br * gate).abs()
        else:
            r = x
        rstd = 1.0 / torch.sqrt((r * r).sum(1) / C + EPS)
        xh = r * rstd[:, None]
        outs["y"] = (rn(xh * (1 + sc) + sh), "y", U)
        mags["y"] = xh.abs() * (1 + sc.abs()) + sh.abs()
        outs["rstd"] = (rstd, "stat", 0)
        mags["rstd"] = rstd.abs()
        return outs, mags
    r = stats["aux"].to(ft) if case["gated"] else f("x")       # the forward's r_out
    rs = stats["rstd"].to(ft)[:, None]
    dy, res = f("dy"), f("residual")
    g = dy * (1 + sc)
    xh = r * rs
    c2 = (g * xh).sum(1, keepdim=True) / C
    o = rs * (g - xh * c2)
    ga = dy.abs() * (1 + sc.abs())
    m = rs * (ga + xh.abs() * (ga * xh.abs()).sum(1, keepdim=True) / C)
    if res is not None:
        o, m = o + res, m + res.abs()
    outs["dx"] = (rn(o), "dx", U)
    mags["dx"] = m
    outs["dscale"] = (rn(per(dy * xh)), "dw", U)
    mags["dscale"] = per((dy * xh).abs())
    outs["dshift"] = (rn(per(dy)), "dw", U)
    mags["dshift"] = per(dy.abs())
    if case["gated"]:
        outs["aux"] = (rn(o * gate), "dx", U)
        mags["aux"] = m * gate.abs()
        outs["dgate"] = (rn(per(o * br)), "dw", U)
        mags["dgate"] = per(m * br.abs())
    return outs, mags


def reference(case, inp, stats=None):
    """fp64 reference: ``{name: (value, kind, U, mag)}``"""
    outs, mags = formulas(case, inp, stats, torch.float64)
    return {n: (v, k, U, mags[n]) for n, (v, k, U) in outs.items()}


def emulate(case, inp, stats=None):
    """the same formulas in plain fp32 (CPU torch): ``{name: value}`` (bf16 outputs rounded to bf16)"""
    outs, _ = formulas(case, inp, stats, torch.float32)
    return {n: v for n, (v, k, U) in outs.items()}


def ulp_bf16(ref):
    """spacing of bf16 numbers at |ref| (fp64), down to the subnormal spacing 2^-133 (also at an exact 0)"""
    _, e = torch.frexp(ref)
    e = torch.where(ref == 0, torch.full_like(e, -125), torch.clamp(e, min=-125))
    return torch.ldexp(torch.ones_like(ref), e - 8)


def excess(got, ref, U, mag):
    """per element: the error beyond U ulp, in units of 2^-24 * mag (inf where mag is 0 and the error is not)"""
    err = (got.double() - ref).abs() - (U * ulp_bf16(ref) if U else 0.0)
    err = torch.clamp(err, min=0.0)
    unit = TWO24 * mag
    return torch.where(err == 0, torch.zeros_like(err), err / torch.where(unit > 0, unit, torch.full_like(unit, float("nan")))).nan_to_num(
        nan=float("inf"))


def not_bit_equal(got, ref):
    """elements of a bf16 output that differ from the reference rounded to bf16"""
    return int((got.to(torch.bfloat16).view(torch.int16) != ref.to(torch.bfloat16).view(torch.int16)).sum())


def forward_case(case):
    """the forward case whose statistics a backward case uses: same entry family, rows, cols, dtypes, inputs"""
    fc = dict(case)
    fc["entry"] = case["entry"].replace("_bwd", "_fwd")
    return fc
