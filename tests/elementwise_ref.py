"""fp64 reference of the entry points of csrc/elementwise.hip, computed from the stored (bf16 / fp32) inputs with the kernels'
rounding points: rnd<T> (to bf16 for a bf16 kernel, nothing for fp32) wherever the kernel calls it or stores, and, in the outputs
held bit for bit, fp32 rounding after every fp32 add, multiply or divide the kernel does unfused.

  swiglu fwd      out = rnd(rnd(silu g) * u)                     silu g = g / (1 + exp(-g))
  swiglu bwd      s = 1 / (1 + exp(-g));  du = rnd(d * rnd(g s));  dg = rnd(d u s (1 + g (1 - s)))
  glu fwd / bwd   out = rnd(rnd(act g) * u);  du = rnd(d * rnd(act g));  dg = rnd(d u act'(g))
  act fwd / bwd   y = rnd(act x);  dx = rnd(dy act'(x))          (GELU-tanh through 1 - 2 / (1 + e^2u) in the kernel)
  RoPE split      c = rnd(cos), s = rnd(sin);  o1 = rnd(rnd(x1 c) + rnd(-x2 s)), o2 = rnd(rnd(x2 c) + rnd(x1 s))   (exact)
  RoPE merge      o1 = rnd(g1 c + g2 s), o2 = rnd(g2 c - g1 s), each product and the sum rounded to fp32    (exact)
  add / mul       rnd(a + b), rnd(a * b) of the fp32 result; axpby rnd(alpha a + beta b)
  vit_embed       x = rnd(rnd(base) + pos)                       (fp32 sum, exact)
  dit_assemble    h = (te + ze) + pos / xe + pos                 (fp32, exact)
  scatter, splice d_embed, token_drop dunc: fp32 sums in ascending row order (exact)
  qsample         xt = a x0 + s noise;  ddim: the kernel's chain;  timestep: cos / sin(t f);  mse: sum d^2 / n, dpred = 2 d / n gscale

``mag`` of a bounded output element is its formula evaluated on absolute values (subtractions become additions: the running
error bound of the operations), each exp / erf / tanh / cos / sin argument that the kernel forms by rounded operations weighted
by its own magnitude (1 + |arg|).  ``emulate`` evaluates the same formulas in fp32 (CPU torch, or on another device): the stand-ins
the slack constants of elementwise_cases.py are measured from."""
import math
import zlib

import torch

from tests import elementwise_cases as E

TWO24 = 2.0 ** -24
TINY = 2.0 ** -126
PAD = -(2 ** 63)
SENT = {"f32": -7777.0, "bf16": -7776.0}
F64 = torch.float64
BOUNDED_ENTRIES = ("swiglu_fwd", "swiglu_bwd", "glu_fwd", "glu_bwd", "act_fwd", "act_bwd", "axpby", "qsample", "ddim", "timestep",
                   "mse", "mse_rows")
GT_K = 0.79788456080286535588
GE_C = 0.70710678118654752440
QG_A = 1.702
ROPE_ENTRIES = ("rope_split", "rope_merge", "qknorm_split", "qknorm_merge")


def f32c(x):
    """a constant as the kernel's fp32 literal"""
    return float(torch.tensor(x, dtype=torch.float32))


def rnd(t, dt):
    return t.to(torch.bfloat16).to(t.dtype) if dt == "bf16" else t


def r32(t):
    return t.to(torch.float32).to(t.dtype)


def add32(a, b):
    return (a.float() + b.float()).to(a.dtype)


def mul32(a, b):
    return (a.float() * b.float()).to(a.dtype)


# ------------------------------------------------------------------------------------------------------------------ operands
def operands(case):
    """name -> (shape, dtype or "i64" / "i32" / "u8", role): role "in", "out" (sentinel-filled) or "inout" (given initial values)"""
    e, t, p = case["entry"], case["dtype"], case["p"]
    d2 = p.get("dst", t)
    if e in ("rope_split", "rope_merge", "qknorm_split", "qknorm_merge"):
        B, S, Hq, Hkv, D = p["B"], p["S"], p["Hq"], p["Hkv"], p["D"]
        Sc = p.get("S_cap", S)
        HS = Hq + 2 * Hkv
        o = dict(cos=((rope_positions(case), D // 2), "f32", "in"), sin=((rope_positions(case), D // 2), "f32", "in"))
        if p.get("pos"):
            o["pos"] = ((B * S,), "i32", "in")
        hm = "out" if e.endswith("split") else "in"
        tm = "in" if e.endswith("split") else "out"
        names = ("q", "k", "v") if e.endswith("split") else ("dq", "dk", "dv")
        o[names[0]] = ((B, Hq, Sc, D), t, hm)
        o[names[1]] = ((B, Hkv, Sc, D), t, hm)
        o[names[2]] = ((B, Hkv, Sc, D), t, hm)
        o["qkv" if e.endswith("split") else "dqkv"] = ((B * S, HS * D), t, tm)
        if e.startswith("qknorm"):
            o["wq"], o["wk"] = ((D,), t, "in"), ((D,), t, "in")
            if e == "qknorm_split":
                o["rstd"] = ((B * S, Hq + Hkv), "f32", "out")
            else:
                o["qkv"] = ((B * S, HS * D), t, "in")
                o["rstd"] = ((B * S, Hq + Hkv), "f32", "in")
        return o
    if e in ("swiglu_fwd", "glu_fwd"):
        return dict(gu=((p["rows"], 2 * p["F"]), t, "in"), out=((p["rows"], p["F"]), t, "out"))
    if e in ("swiglu_bwd", "glu_bwd"):
        return dict(gu=((p["rows"], 2 * p["F"]), t, "in"), dout=((p["rows"], p["F"]), t, "in"), dgu=((p["rows"], 2 * p["F"]), t, "out"))
    if e == "act_fwd":
        return dict(x=((p["n"],), t, "in"), y=((p["n"],), t, "out"))
    if e == "act_bwd":
        return dict(x=((p["n"],), t, "in"), dy=((p["n"],), t, "in"), dx=((p["n"],), t, "out"))
    if e in ("add", "axpby", "mul"):
        return dict(a=((p["n"],), t, "in"), b=((p["n"],), t, "in"), out=((p["n"],), t, "out"))
    if e == "mul_rows":
        return dict(x=((p["R"], p["Nn"], p["C"]), t, "in"), g=((p["R"], p["C"]), t, "in"), out=((p["R"], p["Nn"], p["C"]), t, "out"))
    if e == "cast":
        return dict(src=((p["n"],), t, "in"), dst=((p["n"],), d2, "out"))
    if e == "copy2d":
        return dict(src=((p["rows"], p["lds"]), t, "in"), dst=((p["rows"], p["ldd"]), d2, "out"))
    if e == "gather":
        return dict(x=((p["R"], p["d"]), t, "in"), idx=((p["n"],), "i64", "in"), out=((p["n"], p["d"]), d2, "out"))
    if e == "scatter":
        return dict(dout=((p["n"], p["d"]), t, "in"), idx=((p["n"],), "i64", "in"), dx=((p["R"], p["d"]), d2, "out"))
    if e == "im2col":
        gh, gw = p["H"] // p["P"], p["W"] // p["P"]
        return dict(images=((p["N"], 3, p["H"], p["W"]), t, "in"), rows=((p["N"] * gh * gw, p["ld"]), d2, "out"))
    if e == "splice_fwd":
        return dict(plan=((p["n_rows"],), "i64", "in"), embed=((p["V"], p["d"]), t, "in"), img=((p["n_img"], p["d"]), t, "in"),
                    out=((p["n_rows"], p["d"]), t, "out"))
    if e == "splice_bwd":
        o = dict(plan=((p["n_rows"],), "i64", "in"), dout=((p["n_rows"], p["d"]), t, "in"))
        if not p.get("no_embed"):
            o["d_embed"] = ((p["V"], p["d"]), "f32", "inout")
        if not p.get("no_img"):
            o["d_img"] = ((p["n_img"], p["d"]), t, "out")
        return o
    if e == "zero_rows":
        return dict(plan=((p["n_rows"],), "i64", "in"), g=((p["V"], p["d"]), "f32", "inout"))
    if e == "vit_embed_fwd":
        N, n, C = p["N"], p["np"], p["C"]
        return dict(patch=((N, n, C), t, "in"), cls=((C,), p["w"], "in"), pos=((n + 1, C), p["w"], "in"), x=((N, n + 1, C), t, "out"))
    if e == "vit_embed_bwd":
        N, n, C = p["N"], p["np"], p["C"]
        return dict(dx=((N, n + 1, C), t, "in"), dpatch=((N, n, C), t, "out"))
    if e == "qsample":
        N, per = p["N"], p["per"]
        return dict(x0=((N, per), t, "in"), noise=((N, per), t, "in"), a=((N,), t, "in"), s=((N,), t, "in"), xt=((N, per), t, "out"))
    if e == "timestep":
        return dict(t=((p["N"],), t, "in"), freqs=((p["half"],), t, "in"), out=((p["N"], 2 * p["half"]), t, "out"))
    if e == "dit_fwd":
        N, T_, hd = p["N"], p["T"], p["hd"]
        return dict(xe=((N, T_, hd), t, "in"), te=((N, hd), t, "in"), ze=((N, hd), t, "in"), pos=((T_ + 1, hd), t, "in"),
                    h=((N, T_ + 1, hd), t, "out"))
    if e == "dit_bwd":
        N, T_, hd = p["N"], p["T"], p["hd"]
        return dict(dh=((N, T_ + 1, hd), t, "in"), dxe=((N, T_, hd), t, "out"), dc=((N, hd), t, "out"))
    if e == "token_drop":
        return dict(z=((p["N"], p["d"]), t, "in"), unc=((p["d"],), t, "in"), drop=((p["N"],), "u8", "in"), out=((p["N"], p["d"]), t, "out"))
    if e == "token_drop_bwd":
        o = dict(dout=((p["N"], p["d"]), t, "in"), drop=((p["N"],), "u8", "in"))
        if not p.get("no_dz"):
            o["dz"] = ((p["N"], p["d"]), t, "out")
        o["dunc"] = ((p["d"],), t, "inout" if p["accumulate"] else "out")
        return o
    if e == "mse":
        return dict(pred=((p["n"],), t, "in"), target=((p["n"],), t, "in"), loss=((1,), t, "out"), dpred=((p["n"],), t, "out"))
    if e == "mse_rows":
        r, c = p["rows"], p["cols"]
        return dict(pred=((r, c), t, "in"), target=((r, c), t, "in"), row_w=((r,), t, "in"), loss=((1,), t, "out"),
                    dpred=((r, c), t, "out"))
    if e == "ddim":
        k = 2 if p["use_cfg"] else 1
        return dict(x=((k, p["B"], p["per"]), t, "inout"), mo=((k, p["B"], p["per"]), t, "in"))
    if e == "transpose":
        return dict(src=((p["R"], p["lds"]), t, "in"), dst=((p["C"], p["ldd"]), t, "out"))
    if e == "permute":
        B, S, H, D = p["B"], p["S"], p["H"], p["D"]
        bshd, bhsd = (B, S, H, D), (B, H, S, D)
        return dict(src=(bshd if p["to_head"] else bhsd, t, "in"), dst=(bhsd if p["to_head"] else bshd, t, "out"))
    raise AssertionError(e)


def rope_positions(case):
    """rows of the cos / sin tables: S, or S + 7 with a pos table (its positions reach past S)"""
    return case["p"]["S"] + (7 if case["p"].get("pos") else 0)


DDIM = dict(cfg_scale=1.5, ab_t=0.6, ab_prev=0.7)


def ddim_scalars():
    ab_t, ab_prev = DDIM["ab_t"], DDIM["ab_prev"]
    return dict(cfg_scale=f32c(DDIM["cfg_scale"]), c_recip=f32c(math.sqrt(1 / ab_t)), c_recipm1=f32c(math.sqrt(1 / ab_t - 1)),
                ab_prev=f32c(ab_prev))


# -------------------------------------------------------------------------------------------------------------------- inputs
SPECIAL = [20.0, 88.0, 89.0, 100.0, 0.0, 1e-20, 3e-19, 1.5, 0.25, 2.0 ** -70, 7.0, 0.75, 1e-3, 3.0, 0.0625, 12.0]
SPECIAL_ADD = [20.0, 88.0, 89.0, 100.0, 0.0, 1.5, 0.25, 7.0, 0.75, 0.0078125, 3.0, 0.0625, 12.0, 0.5, 2.5, 33.0]
NONFINITE = [float("nan"), float("inf"), -float("inf"), 3.3e38, -3.4e38, 1e-40, -0.0]


def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()) & 0x7FFFFFFF)


def special_values(shape, which, table=SPECIAL, nonfinite=False):
    """the special value set as a function of the element position alone (routes of a family of other widths see the same
    values at the same (row, column)): a sign and a table entry per element, every tenth element a normal draw"""
    n = 1
    for s in shape:
        n *= s
    idx = torch.arange(n, dtype=torch.int64)
    if len(shape) == 2:                                       # position-keyed: (row, column) independent of the row length
        idx = (torch.arange(shape[0])[:, None] * 1009 + torch.arange(shape[1])[None, :]).reshape(-1)
    h = (idx * 0x9E3779B1 + which * 0x85EBCA77) & 0x7FFFFFFF          # an integer hash: operands of other ``which`` independent
    h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & 0x7FFFFFFF
    h = ((h ^ (h >> 12)) * 0x297A2D39) & 0x7FFFFFFF
    h = h ^ (h >> 15)
    tab = torch.tensor(table, dtype=F64)
    v = tab[h % len(table)] * torch.where((h >> 7) % 2 == 0, 1.0, -1.0).to(F64)
    plain = ((h >> 11) % 2001 - 1000).to(F64) / 250.0             # an ordinary value in [-4, 4], also keyed by position
    v = torch.where(h % 10 == 3, plain, v)
    if nonfinite:
        nf = torch.tensor(NONFINITE, dtype=F64)
        v = torch.where(h % 7 == 2, nf[(h >> 3) % len(NONFINITE)], v)
        v[1:1 + min(n - 1, 2 * len(NONFINITE)):2] = nf.repeat(2)[: len(v[1:1 + min(n - 1, 2 * len(NONFINITE)):2])]    # every one
    return v.view(*shape)


def inputs(case):
    """the case's inputs on the CPU in their stored dtypes, and the initial contents of its inout operands (seeded by the id)"""
    e, t, p = case["entry"], case["dtype"], case["p"]
    g = _gen(case["id"])
    ops = operands(case)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    T = lambda dt: E.TORCH_DT[dt]
    out = {}
    special = case["values"] == "special"
    for n, (shape, dt, role) in ops.items():
        if role == "out" or dt in ("i64", "i32", "u8"):
            continue
        if special:
            table = SPECIAL_ADD if e == "add" else SPECIAL
            nonf = e not in BOUNDED_ENTRIES and e not in ("add", "mul", "mul_rows")
            which = zlib.crc32(n.encode()) & 0xFFFF
            if n == "gu":                     # gate and up keyed by (row, column of the output): routes of other F agree
                hf = (shape[0], shape[1] // 2)
                v = torch.cat([special_values(hf, which, table, nonf), special_values(hf, which + 1, table, nonf)], 1)
            else:
                v = special_values(shape, which, table, nonf)
        else:
            v = rn(*shape)
        out[n] = v.to(T(dt))
    if e == "add" and t == "bf16":
        # exponent spread of the addends <= 16: the fp32 sum is exact, so the stored sum is the correctly rounded one
        a, b = out["a"].double(), out["b"].double()
        ea, eb = torch.frexp(a)[1], torch.frexp(b)[1]
        far = (a != 0) & (b != 0) & ((ea - eb).abs() > 16)
        out["b"] = torch.where(far, torch.ldexp(torch.frexp(b)[0], ea), b).to(torch.bfloat16)
    if e in ROPE_ENTRIES:
        _rope_inputs(case, out, g)
    elif e == "gather":
        out["idx"] = torch.randint(0, p["R"], (p["n"],), generator=g)
        out["idx"][: min(3, p["n"])] = p["R"] - 1                     # repeated indices, the last row
    elif e == "scatter":
        idx = torch.randint(0, p["R"], (p["n"],), generator=g)
        idx[0] = idx[1] = min(2, p["R"] - 1)                           # repeated
        if p["n"] > 6:
            idx[3], idx[4], idx[5] = -1, p["R"], p["R"] + 5            # outside [0, R): contribute nothing
        out["idx"] = idx
    elif e in ("splice_fwd", "splice_bwd", "zero_rows"):
        out["plan"] = splice_plan(case, g)
    elif e in ("token_drop", "token_drop_bwd"):
        dr = torch.zeros(p["N"], dtype=torch.uint8)
        dr[1::2] = 1
        dr[-1] = 1
        out["drop"] = dr
    elif e == "qsample":
        out["a"] = torch.rand(p["N"], generator=g, dtype=F64).float()
        out["s"] = (1 - out["a"].double() ** 2).sqrt().float()
    elif e == "timestep":
        out["t"] = (torch.rand(p["N"], generator=g, dtype=F64) * 1000).floor().float()
        out["freqs"] = torch.exp(-math.log(10000) * torch.arange(p["half"], dtype=F64) / p["half"]).float()
    elif e == "mse_rows":
        out["row_w"] = torch.rand(p["rows"], generator=g, dtype=F64).float()
    return out


UNIT_ROW = [1.25, 1.25, 0.75, 0.75, 1.5, 1.0, 0.5, 0.5]            # squares add up to 8


def is_unit(case):
    """a q/k-norm case whose norm (split) or norm backward (merge) is the identity: q and k are rope_k's bit for bit"""
    return "unit" in case["id"].split("-")


def _rope_inputs(case, out, g):
    p, e, t = case["p"], case["entry"], case["dtype"]
    D, P = p["D"], rope_positions(case)
    half = D // 2
    inv = 1.0 / (10000.0 ** (torch.arange(0, half, dtype=torch.int64).float() * 2 / D))         # Qwen2RotaryEmbedding, fp32
    fr = torch.outer(torch.arange(P, dtype=torch.float32), inv)
    out["cos"], out["sin"] = fr.cos(), fr.sin()
    if p.get("pos"):
        n = p["B"] * p["S"]
        pos = torch.randperm(P, generator=g)[:n] if n <= P else torch.randint(0, P, (n,), generator=g)
        pos[0], pos[-1] = P - 1, 0                                      # a position past S first: not monotonic
        out["pos"] = pos.to(torch.int32)                                # not monotonic, reaching past S
    if is_unit(case):
        out["wq"] = torch.ones(D, dtype=E.TORCH_DT[t])
        out["wk"] = torch.ones(D, dtype=E.TORCH_DT[t])
        if e == "qknorm_split":
            # unit-RMS rows: per (token, head) D / 8 copies of UNIT_ROW, whose squares (multiples of 1 / 16) add up to 8 exactly
            # in fp32 in any order, with random signs in random order: sum x^2 / D is 1.0 exactly, so the norm is the identity,
            # while five of the eight values (1.25, 0.75, 1.5) make inexact fp32 products with a full-precision cos / sin: a
            # rotation contracted into an fma gives other bits (test_elementwise_ref.py counts them)
            B, S, HS = p["B"], p["S"], p["Hq"] + 2 * p["Hkv"]
            base = torch.tensor(UNIT_ROW, dtype=F64).repeat(D // 8)
            rows = B * S * HS
            perm = torch.argsort(torch.rand(rows, D, generator=g), dim=1)
            sign = torch.where(torch.rand(rows, D, generator=g) < 0.5, -1.0, 1.0).to(F64)
            out["qkv"] = (base[perm] * sign).view(B * S, HS * D).to(E.TORCH_DT[t])
        else:
            # the norm backward made transparent: pre-norm rows of zeros (x_hat = 0: nothing is projected out), unit weights
            # and rstd = 1, so dqkv = rstd * (w dy - x_hat * mean(w dy x_hat)) = dy, the un-rotated gradient itself
            out["qkv"] = torch.zeros_like(out["qkv"])
            out["rstd"] = torch.ones(p["B"] * p["S"], p["Hq"] + p["Hkv"])
    elif e.startswith("qknorm"):
        out["wq"] = (1 + 0.1 * torch.randn(D, generator=g, dtype=F64)).to(E.TORCH_DT[t])
        out["wk"] = (1 + 0.1 * torch.randn(D, generator=g, dtype=F64)).to(E.TORCH_DT[t])
        if e == "qknorm_merge":
            out["rstd"] = (0.5 + torch.rand(p["B"] * p["S"], p["Hq"] + p["Hkv"], generator=g, dtype=F64)).float()
    if e in ("rope_merge", "qknorm_merge"):
        # rows of the head-major tensors outside [s0, s0 + S) are NaN: the call must not read them
        s0, S = p.get("s0", 0), p["S"]
        for n in ("dq", "dk", "dv"):
            v = out[n].clone()
            v[:, :, :s0] = float("nan")
            v[:, :, s0 + S:] = float("nan")
            out[n] = v


def splice_plan(case, g):
    """token ids, image rows (-1 - j, each used once) and PAD rows; token 0 fills rows 0 .. 199 (whole waves of ballots, one id
    repeated across windows), token V - 1 first appears at row n_rows // 2 (r & 255 != 0)"""
    p = case["p"]
    n, V, ni = p["n_rows"], p["V"], p["n_img"]
    plan = torch.randint(1, V - 1, (n,), generator=g)
    if n >= 600:
        plan[:200] = 0
    plan[n // 2 + 1::7] = V - 1
    img_rows = torch.randperm(n - 1, generator=g)[: ni - 2] + 1
    img_rows = img_rows[(img_rows >= 200) | (n < 600)] if n >= 600 else img_rows
    plan[img_rows] = -1 - torch.randperm(ni, generator=g)[: img_rows.numel()]
    pads = torch.arange(n // 3 + 5, n, max(1, n // 6))
    plan[pads] = PAD
    plan[n // 2 + 1] = V - 1
    return plan


# ----------------------------------------------------------------------------------------------------------------- formulas
def _sig(x, a=1.0):
    """1 / (1 + e^-ax), and e^ax where e^-ax overflows (sigmoid_f in csrc/common.h)"""
    ax = a * x
    e = torch.exp(-ax)
    return torch.where(torch.isinf(e), torch.exp(ax), 1 / (1 + e))


def _silu(x, a=1.0):
    """x / (1 + e^-ax), and x e^ax where e^-ax overflows (silu_f)"""
    ax = a * x
    e = torch.exp(-ax)
    return torch.where(torch.isinf(e), x * torch.exp(ax), x / (1 + e))


def _act(act, x, exact):
    """(value, argument magnitude for mag, |value| terms) of the activation; ``exact``: tanh itself (reference) or the kernel's
    1 - 2 / (1 + e^2u) (emulation)"""
    a = E.ACT
    if act == a["gelu_erf"]:
        c = f32c(GE_C)
        z = x * c
        er = torch.erf(z)
        return 0.5 * x * (1 + er), 0.5 * x.abs() * (1 + er.abs()) + 0.5 * x.abs() * z.abs() * 1.1283791670955126 * torch.exp(-z * z)
    if act == a["gelu_tanh"]:
        k, c3 = f32c(GT_K), f32c(0.044715)
        u = k * (x + c3 * x * x * x)
        th = torch.tanh(u) if exact else 1 - 2 / (1 + torch.exp(2 * u))
        um = k * (x.abs() + c3 * x.abs() ** 3)
        return 0.5 * x * (1 + th), 0.5 * x.abs() * (1 + th.abs()) + 0.5 * x.abs() * (1 - th * th) * um
    if act == a["quick_gelu"]:
        ar = -f32c(QG_A) * x
        s = _sig(x, f32c(QG_A))
        y = _silu(x, f32c(QG_A))
        return y, y.abs() * (1 + ar.abs() * (1 - s))
    if act == a["silu"]:
        s = _sig(x)
        y = _silu(x)
        return y, y.abs() * (2 - s)
    if act == a["relu"]:
        y = torch.clamp(x, min=0)
        return y, y.abs()
    if act == a["sigmoid"]:
        s = _sig(x)
        return s, s * (2 - s)
    return x, x.abs()


def _act_grad(act, x, exact):
    a = E.ACT
    if act == a["gelu_erf"]:
        c = f32c(GE_C)
        z = x * c
        cdf = 0.5 * (1 + torch.erf(z))
        hx = -0.5 * x * x
        pdf = f32c(0.39894228040143267794) * torch.exp(hx)
        er = 2 * cdf - 1
        return cdf + x * pdf, 0.5 * (1 + er.abs()) + 0.5 * z.abs() * 1.1283791670955126 * torch.exp(-z * z) + (x * pdf).abs() * (2 + hx.abs())
    if act == a["gelu_tanh"]:
        k, c3 = f32c(GT_K), f32c(0.044715)
        u = k * (x + c3 * x * x * x)
        th = torch.tanh(u) if exact else 1 - 2 / (1 + torch.exp(2 * u))
        du = k * (1 + 3 * c3 * x * x)
        um = k * (x.abs() + c3 * x.abs() ** 3)
        g = 0.5 * (1 + th) + 0.5 * x * (1 - th * th) * du
        m = 0.5 * (1 + th.abs()) + 0.5 * x.abs() * (1 + th * th) * du.abs() + (0.5 + (x * th * du).abs()) * (1 - th * th) * um
        return g, m
    if act == a["quick_gelu"]:
        qa = f32c(QG_A)
        ar = -qa * x
        s = _sig(x, qa)
        g = s + x * qa * s * (1 - s)
        return g, (s + (x * qa).abs() * s * (1 + s)) * (1 + ar.abs() * (1 - s))
    if act == a["silu"]:
        s = _sig(x)
        g = s * (1 + x * (1 - s))
        return g, s * (1 + x.abs() * (1 + s)) * (1 + x.abs() * (1 - s))
    if act == a["relu"]:
        g = (x > 0).to(x.dtype)
        return g, g
    if act == a["sigmoid"]:
        s = _sig(x)
        return s * (1 - s), s * (1 + s) * (1 + x.abs() * (1 - s))
    return torch.ones_like(x), torch.ones_like(x)


def gelu_tanh_abs(act, x, grad):
    """the factor of GELU_TANH_ABS for an output of the GELU-tanh route (0 for other activations)"""
    if act != E.ACT["gelu_tanh"]:
        return torch.zeros_like(x)
    if not grad:
        return 0.5 * x.abs()
    k, c3 = f32c(GT_K), f32c(0.044715)
    u = k * (x + c3 * x * x * x)
    th = torch.tanh(u)
    return 0.5 + (x * th * k * (1 + 3 * c3 * x * x)).abs()


def _out(v, kind=None, mag=None, U=0, alt=(), ab=None, keep=None):
    return dict(v=v, kind=kind, mag=mag, U=U, alt=list(alt), abs=ab, keep=keep, exact=kind is None)


def _neighbours(a, m, dt, kind):
    """the bf16 neighbours an intermediate rnd<bf16>(a) may take when a lies within k 2^-24 m of a rounding boundary"""
    if dt != "bf16":
        return []
    tol = E.K_SLACK[kind] * TWO24 * m
    return [rnd(a - tol, dt), rnd(a + tol, dt)]


def formulas(case, inp, ft=F64, dev="cpu"):
    """the outputs of ``case`` from its inputs: ``{name: _out(...)}`` in ``ft`` (fp64: the reference; fp32: the stand-in)"""
    e, t, p = case["entry"], case["dtype"], case["p"]
    f = lambda n: inp[n].to(dev).to(ft)
    exact = ft == F64
    U = 1 if t == "bf16" else 0
    act = p.get("act", E.ACT["silu"])
    if e in ("swiglu_fwd", "glu_fwd", "swiglu_bwd", "glu_bwd"):
        F = p["F"]
        gu = f("gu")
        g, u = gu[:, :F], gu[:, F:]
        y, ym = _act(act, g, exact)
        ry = rnd(y, t)
        if e.endswith("fwd"):
            alts = [rnd(r * u, t) for r in _neighbours(y, ym, t, "glu")]
            return {"out": _out(rnd(ry * u, t), "glu", ym * u.abs(), U, alts, gelu_tanh_abs(act, g, False) * u.abs())}
        d = f("dout")
        if e == "swiglu_bwd":
            s = _sig(g)
            gs = g * s
            du_in, dum = gs, gs.abs() * (2 - s)
            gr = s * (1 + g * (1 - s))
            grm = s * (1 + g.abs() * (1 + s)) * (1 + g.abs() * (1 - s))
        else:
            du_in, dum = y, ym
            gr, grm = _act_grad(act, g, exact)
        du = rnd(d * rnd(du_in, t), t)
        alts_du = [rnd(d * r, t) for r in _neighbours(du_in, dum, t, "glu")]
        dg = rnd(d * u * gr, t)
        zero = torch.zeros_like(g)
        # dgu = [dg | du]: two outputs of their own kinds
        return {"dgu_g": _out(dg, "glu_grad", (d * u).abs() * grm, U, (), gelu_tanh_abs(act, g, True) * (d * u).abs()),
                "dgu_u": _out(du, "glu", d.abs() * dum, U, alts_du, gelu_tanh_abs(act, g, False) * d.abs() + zero)}
    if e == "act_fwd":
        x = f("x")
        y, ym = _act(act, x, exact)
        return {"y": _out(rnd(y, t), "act", ym, U, (), gelu_tanh_abs(act, x, False))}
    if e == "act_bwd":
        x, dy = f("x"), f("dy")
        gr, grm = _act_grad(act, x, exact)
        return {"dx": _out(rnd(dy * gr, t), "act_grad", dy.abs() * grm, U, (), gelu_tanh_abs(act, x, True) * dy.abs())}
    if e == "axpby":
        a, b = f("a"), f("b")
        al, be = f32c(p["alpha"]), f32c(p["beta"])
        return {"out": _out(rnd(al * a + be * b, t), "two_term", (al * a).abs() + (be * b).abs(), U)}
    if e == "qsample":
        x0, nz, a, s = f("x0"), f("noise"), f("a")[:, None], f("s")[:, None]
        return {"xt": _out(a * x0 + s * nz, "two_term", (a * x0).abs() + (s * nz).abs())}
    if e == "ddim":
        sc = ddim_scalars()
        x, mo = f("x"), f("mo")
        xv = x[0]
        if p["use_cfg"]:
            ec, eu = mo[0], mo[1]
            eps = eu + sc["cfg_scale"] * (ec - eu)
            epm = eu.abs() + sc["cfg_scale"] * (ec.abs() + eu.abs())
        else:
            eps, epm = mo[0], mo[0].abs()
        cr, cm = sc["c_recip"], sc["c_recipm1"]
        x0 = cr * xv - cm * eps
        x0m = cr * xv.abs() + cm * epm
        eps2 = (cr * xv - x0) / cm
        e2m = (cr * xv.abs() + x0m) / cm
        sa = math.sqrt(sc["ab_prev"])
        sb = math.sqrt(1 - sc["ab_prev"])           # 1 - ab_prev is exact in fp32 (Sterbenz)
        xn = x0 * sa + sb * eps2
        m = x0m * sa + sb * e2m
        if p["use_cfg"]:
            xn, m = torch.stack([xn, xn]), torch.stack([m, m])
        else:
            xn, m = xn[None], m[None]
        return {"x": _out(xn, "diffusion", m)}
    if e == "timestep":
        tt, fr = f("t"), f("freqs")
        arg = tt[:, None] * fr[None, :]
        am = 1 + arg.abs()
        return {"out": _out(torch.cat([torch.cos(arg), torch.sin(arg)], 1), "trig", torch.cat([am, am], 1))}
    if e in ("mse", "mse_rows"):
        pr, tg = f("pred"), f("target")
        d = pr - tg
        gs = f32c(p["gscale"])
        if e == "mse":
            n = d.numel()
            h = n / 1024 + 24                          # depth of the kernel's summation: per thread, the wave, 16 waves
            loss = (d * d).sum().reshape(1) / n
            return {"loss": _out(loss, "mse", loss * h),
                    "dpred": _out(2.0 / n * gs * d, "mse", (2.0 / n * gs * d).abs() * 2)}
        w = f("row_w")[:, None]
        cols = p["cols"]
        ws = w.sum() + f32c(1e-6)
        loss = (w * d * d).sum() / (cols * ws)
        h = d.numel() / 1024 + 24
        return {"loss": _out(loss.reshape(1), "mse", (loss.abs() * 2 * h).reshape(1)),
                "dpred": _out(2 * w * d / (cols * ws) * gs, "mse", (2 * w * d / (cols * ws) * gs).abs() * 2)}
    return exact_outputs(case, inp)


def exact_outputs(case, inp):
    """the outputs held bit for bit: fp64 values that are exactly the stored result (NaN as NaN)"""
    e, t, p = case["entry"], case["dtype"], case["p"]
    f = lambda n: inp[n].to(F64)
    d2 = p.get("dst", t)
    if e in ("rope_split", "qknorm_split"):
        return rope_split_ref(case, inp)
    if e in ("rope_merge", "qknorm_merge"):
        return rope_merge_ref(case, inp)
    if e == "add":
        return {"out": _out(rnd(add32(f("a"), f("b")), t))}
    if e == "mul":
        return {"out": _out(rnd(mul32(f("a"), f("b")), t))}
    if e == "mul_rows":
        return {"out": _out(rnd(mul32(f("x"), f("g")[:, None, :]), t))}
    if e == "cast":
        return {"dst": _out(rnd(f("src"), d2))}
    if e == "copy2d":
        src = f("src")
        o = torch.full((p["rows"], p["ldd"]), SENT[d2], dtype=F64)
        o[:, :p["cols"]] = rnd(src[:, :p["cols"]], d2)
        o[:, p["cols"]:p["cols_padded"]] = 0.0
        return {"dst": _out(o)}
    if e == "gather":
        return {"out": _out(rnd(f("x")[inp["idx"]], d2))}
    if e == "scatter":
        dout, idx = f("dout"), inp["idx"]
        s = torch.zeros(p["R"], p["d"], dtype=torch.float32)
        for i in range(p["n"]):
            r = int(idx[i])
            if 0 <= r < p["R"]:
                s[r] = s[r] + dout[i].float()
        return {"dx": _out(rnd(s.to(F64), d2))}
    if e == "im2col":
        img = f("images")
        N, H, W, P = p["N"], p["H"], p["W"], p["P"]
        gh, gw = H // P, W // P
        col = img.view(N, 3, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(N * gh * gw, 3 * P * P)
        o = torch.zeros(N * gh * gw, p["ld"], dtype=F64)
        o[:, :3 * P * P] = col
        return {"rows": _out(rnd(o, d2))}
    if e == "splice_fwd":
        plan, emb, img = inp["plan"], f("embed"), f("img")
        o = torch.zeros(p["n_rows"], p["d"], dtype=F64)
        tok = plan >= 0
        o[tok] = emb[plan[tok]]
        im = (plan < 0) & (plan != PAD)
        o[im] = img[-1 - plan[im]]
        return {"out": _out(o)}
    if e == "splice_bwd":
        plan, dout = inp["plan"], f("dout")
        res = {}
        if not p.get("no_embed"):
            de = inp["d_embed"].clone().float()
            acc = {}
            for r in range(p["n_rows"]):
                q = int(plan[r])
                if q >= 0:
                    acc[q] = acc[q] + dout[r].float() if q in acc else torch.zeros(p["d"]) + dout[r].float()
            for q, a in acc.items():
                de[q] = de[q] + a
            res["d_embed"] = _out(de.to(F64))
        if not p.get("no_img"):
            di = torch.full((p["n_img"], p["d"]), SENT[t], dtype=F64)
            im = (plan < 0) & (plan != PAD)
            di[-1 - plan[im]] = dout[im]
            res["d_img"] = _out(di)
        return res
    if e == "zero_rows":
        g = f("g").clone()
        plan = inp["plan"]
        g[plan[plan >= 0]] = 0.0
        return {"g": _out(g)}
    if e == "vit_embed_fwd":
        pa, cls, pos = f("patch"), f("cls"), f("pos")
        N = p["N"]
        base = torch.cat([cls[None, None, :].expand(N, 1, p["C"]), pa], 1)
        return {"x": _out(rnd(add32(rnd(base, t), pos[None].expand_as(base)), t))}
    if e == "vit_embed_bwd":
        return {"dpatch": _out(f("dx")[:, 1:])}
    if e == "dit_fwd":
        xe, te, ze, pos = f("xe"), f("te"), f("ze"), f("pos")
        base = torch.cat([add32(te, ze)[:, None], xe], 1)
        return {"h": _out(add32(base, pos[None].expand_as(base)))}
    if e == "dit_bwd":
        dh = f("dh")
        return {"dxe": _out(dh[:, 1:]), "dc": _out(dh[:, 0])}
    if e == "token_drop":
        z, unc, dr = f("z"), f("unc"), inp["drop"].bool()
        return {"out": _out(torch.where(dr[:, None], unc[None].expand_as(z), z))}
    if e == "token_drop_bwd":
        dout, dr = f("dout"), inp["drop"].bool()
        s = torch.zeros(p["d"], dtype=torch.float32)
        for n in range(p["N"]):
            if dr[n]:
                s = s + dout[n].float()
        res = {}
        if not p.get("no_dz"):
            res["dz"] = _out(torch.where(dr[:, None], torch.zeros_like(dout), dout))
        res["dunc"] = _out((inp["dunc"].float() + s).to(F64) if p["accumulate"] else s.to(F64))
        return res
    if e == "transpose":
        src = f("src")
        R, C_, Rp = p["R"], p["C"], p["Rp"]
        o = torch.full((C_, p["ldd"]), SENT[t], dtype=F64)
        o[:, :Rp] = 0.0
        o[:, :R] = src[:R, :C_].t()
        return {"dst": _out(o)}
    if e == "permute":
        return {"dst": _out(f("src").transpose(1, 2).contiguous())}
    raise AssertionError(e)


def _rope_tables(case, inp):
    p, t = case["p"], case["dtype"]
    B, S = p["B"], p["S"]
    pr = inp["pos"].long() if "pos" in inp else torch.arange(S).repeat(B)
    c = rnd(inp["cos"].to(F64)[pr], t)                     # [B*S, half], rounded to T as the kernel does
    s = rnd(inp["sin"].to(F64)[pr], t)
    return c, s


def rope_split_ref(case, inp):
    """q, k, v head-major (rows outside [s0, s0 + S) keep their sentinels); HF's arithmetic in T: every product rounded to T,
    then one add rounded to fp32 and stored in T"""
    p, t = case["p"], case["dtype"]
    B, S, Hq, Hkv, D = p["B"], p["S"], p["Hq"], p["Hkv"], p["D"]
    Sc, s0, half = p.get("S_cap", S), p.get("s0", 0), D // 2
    HS = Hq + 2 * Hkv
    x = inp["qkv"].to(F64).view(B * S, HS, D)
    c, s = _rope_tables(case, inp)
    c, s = c[:, None, :], s[:, None, :]
    x1, x2 = x[..., :half], x[..., half:]
    o1 = rnd(add32(rnd(mul32(x1, c.expand_as(x1)), t), rnd(mul32(-x2, s.expand_as(x2)), t)), t)
    o2 = rnd(add32(rnd(mul32(x2, c.expand_as(x2)), t), rnd(mul32(x1, s.expand_as(x1)), t)), t)
    rot = torch.cat([o1, o2], -1).view(B, S, HS, D)
    xs = x.view(B, S, HS, D)
    res = {}
    for n, lo, hi, src in (("q", 0, Hq, rot), ("k", Hq, Hq + Hkv, rot), ("v", Hq + Hkv, HS, xs)):
        o = torch.full((B, hi - lo, Sc, D), SENT[t], dtype=F64)
        o[:, :, s0:s0 + S] = src[:, :, lo:hi].permute(0, 2, 1, 3)
        res[n] = _out(o)
    if case["entry"] == "qknorm_split":
        res = res if is_unit(case) else {"v": res["v"]}
    return res


def rope_merge_ref(case, inp):
    """dqkv token-major: the inverse rotation g1 c + g2 s, g2 c - g1 s with each product and the sum rounded to fp32"""
    p, t = case["p"], case["dtype"]
    B, S, Hq, Hkv, D = p["B"], p["S"], p["Hq"], p["Hkv"], p["D"]
    s0, half = p.get("s0", 0), D // 2
    HS = Hq + 2 * Hkv
    hm = torch.cat([inp[n].to(F64)[:, :, s0:s0 + S] for n in ("dq", "dk", "dv")], 1)      # [B, HS, S, D]
    g = hm.permute(0, 2, 1, 3).reshape(B * S, HS, D)
    c, s = _rope_tables(case, inp)
    c, s = c[:, None, :].expand(B * S, HS, half), s[:, None, :].expand(B * S, HS, half)
    g1, g2 = g[..., :half], g[..., half:]
    o1 = add32(mul32(g1, c), mul32(g2, s))
    o2 = add32(mul32(g2, c), mul32(-g1, s))
    rot = torch.cat([o1, o2], -1)
    rot[:, Hq + Hkv:] = g[:, Hq + Hkv:]
    res = rnd(rot, t).view(B * S, HS * D)
    if case["entry"] == "qknorm_merge" and not is_unit(case):
        # only the dv third is held here (the RMSNorm backward of q / k: tests/test_qknorm_rope_gpu.py); a unit case holds the
        # un-rotation of dq and dk too
        keep = torch.zeros(B * S, HS, D, dtype=torch.bool)
        keep[:, Hq + Hkv:] = True
        return {"dqkv": _out(res, keep=keep.view(B * S, HS * D))}
    return {"dqkv": _out(res)}


def reference(case, inp):
    """fp64 reference: ``{name: _out}``; bounded outputs of swiglu / glu backward are split into their gate / up halves"""
    return formulas(case, inp, F64)


def emulate(case, inp, dev="cpu"):
    """the bounded outputs evaluated in fp32 with the same formulas and rounding points: ``{name: fp64 tensor on the CPU}``"""
    return {n: o["v"].double().cpu() for n, o in formulas(case, inp, torch.float32, dev).items() if not o["exact"]}


# ------------------------------------------------------------------------------------------------------------------- checks
def ulp(ref, dt):
    """spacing of ``dt`` numbers at |ref| (fp64), down to the subnormal spacing (also at an exact 0)"""
    _, e = torch.frexp(ref.nan_to_num(0.0))
    lo, m = (-125, 8) if dt == "bf16" else (-125, 24)
    e = torch.where(ref == 0, torch.full_like(e, lo), torch.clamp(e, min=lo))
    return torch.ldexp(torch.ones_like(ref), e - m)


def excess(got, o, dt, abs_coef=0.0):
    """per element: the error beyond U ulp, the 2^-126 term and the GELU-tanh term, in units of 2^-24 * mag (min over the
    reference and its neighbours; inf where mag is 0 and the error is not)"""
    got = got.double()
    best = None
    for ref in [o["v"]] + o["alt"]:
        err = (got - ref).abs() - (o["U"] * ulp(ref, dt) if o["U"] else 0.0) - TINY
        if o["abs"] is not None:
            err = err - abs_coef * o["abs"]
        err = torch.clamp(err, min=0.0)
        unit = TWO24 * o["mag"]
        ex = torch.where(err == 0, torch.zeros_like(err), err / torch.where(unit > 0, unit, torch.full_like(unit, float("nan"))))
        ex = ex.nan_to_num(nan=float("inf"))
        both_nan = torch.isnan(got) & torch.isnan(ref)
        ex = torch.where(both_nan, torch.zeros_like(ex), torch.where(torch.isnan(got) | torch.isnan(ref), torch.full_like(ex, float("inf")), ex))
        ex = torch.where((got == ref), torch.zeros_like(ex), ex)            # equal infinities
        best = ex if best is None else torch.minimum(best, ex)
    return best


def exact_mismatch(got, o, dt):
    """elements of an exact output that differ from the reference: bits (NaN as NaN); ``keep`` limits the held elements"""
    ref = o["v"].to(E.TORCH_DT[dt]) if dt in E.TORCH_DT else o["v"]
    iv = torch.int16 if dt == "bf16" else torch.int32
    g = got.to(ref.dtype)
    rn, gn = torch.isnan(ref), torch.isnan(g)
    bad = torch.where(rn, ~gn, gn | (g.view(iv) != ref.view(iv)))
    if o["keep"] is not None:
        bad = bad & o["keep"]
    return bad


def not_bit_equal(got, ref):
    """elements of a bf16 output that differ from the reference rounded to bf16 (NaN as NaN)"""
    r, g = ref.to(torch.bfloat16), got.to(torch.bfloat16)
    return int(((g.view(torch.int16) != r.view(torch.int16)) & ~(torch.isnan(g) & torch.isnan(r))).sum())


def share_keys(case):
    """the shares of the cap a case counts towards: a bf16 bounded case, GELU-tanh excluded, towards its entry point's, and with
    ordinary values towards that of its (entry point, kernel instantiation) as well, so that the million elements of a scalar
    second-trip case do not dilute a defect of the x8 or x4 route.  The special table is left out of the finer share: it has
    some thirty distinct values, each in about 3 % of a case's elements, so ONE value whose fp32 evaluation falls on the other
    side of a bf16 boundary is 3 % by itself (the fp32 stand-in does that in GLU); the bound and the agreement of the routes
    hold those cases."""
    if case["dtype"] != "bf16" or case["entry"] not in BOUNDED_ENTRIES or case["p"].get("act") == E.ACT["gelu_tanh"]:
        return ()
    return (case["entry"],) + (((case["entry"], case["kernel"]),) if case["values"] == "randn" else ())


def split_output(case, name, t):
    """a kernel output tensor -> the reference's outputs it holds (swiglu / glu backward: dgu = [dg | du])"""
    if case["entry"] in ("swiglu_bwd", "glu_bwd") and name == "dgu":
        F = case["p"]["F"]
        return {"dgu_g": t[:, :F], "dgu_u": t[:, F:]}
    return {name: t}


def out_dtype(case, name):
    ops = operands(case)
    if name.startswith("dgu"):
        name = "dgu"
    return ops[name][1]
