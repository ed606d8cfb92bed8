"""CPU checks of the norm reference (tests/norm_ref.py): without its rounding points it is torch's own LayerNorm / RMSNorm and
their autograd gradients in fp64, and the slack constants and share cap of tests/norm_cases.py hold for a plain fp32
evaluation of the same formulas over the whole case table (what they were measured from)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import norm_cases as NC
from tests import norm_ref as R


def _case(entry, rows, cols, w=True, res=True, dtype="f32"):
    return dict(id=f"t-{entry}-{rows}x{cols}", entry=entry, rows=rows, cols=cols, dtype=dtype, w_dtype=dtype, w=w, b=w,
                res=res and entry.endswith("_bwd") and not entry.startswith("add_"), mis=None, kernel=None, trips=None)


def _rel(a, b):
    return float((a - b).abs().max() / max(b.abs().max(), 1e-300))


@pytest.mark.parametrize("entry", ["layernorm", "add_layernorm", "rmsnorm"])
@pytest.mark.parametrize("w", [True, False])
def test_unrounded_reference_is_torch_autograd(entry, w):
    fc, bc = _case(entry + "_fwd", 7, 37, w), _case(entry + "_bwd", 7, 37, w)
    inp = {k: v.double() for k, v in NC.inputs(bc).items()}
    outs, _ = R.formulas(fc, inp, ft=torch.float64, rounding=False)
    x = (inp["x"] + inp["x2"] if entry.startswith("add") else inp["x"]).clone().requires_grad_(True)
    wt = inp["w"].clone().requires_grad_(True) if w else None
    bt = inp["b"].clone().requires_grad_(True) if (w and entry != "rmsnorm") else None
    if entry == "rmsnorm":
        y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + NC.EPS)
        y = y * wt if w else y
    else:
        y = F.layer_norm(x, (37,), wt, bt, NC.EPS)
        mean = x.detach().mean(-1)
        assert _rel(outs["mean"][0], mean) <= 1e-12
    assert _rel(outs["y"][0], y.detach()) <= 1e-12
    rstd = torch.rsqrt((x.detach() - (0 if entry == "rmsnorm" else x.detach().mean(-1, keepdim=True))).pow(2).mean(-1) + NC.EPS)
    assert _rel(outs["rstd"][0], rstd) <= 1e-12
    y.backward(inp["dy"])
    stats = {"rstd": outs["rstd"][0], "mean": outs["mean"][0] if "mean" in outs else None}
    g, _ = R.formulas(bc, inp, stats, ft=torch.float64, rounding=False)
    want_dx = x.grad + (inp["residual"] if bc["res"] else 0)
    assert _rel(g["dx"][0], want_dx) <= 1e-12
    if w:
        assert _rel(g["dw"][0], wt.grad) <= 1e-12
        if bt is not None:
            assert _rel(g["db"][0], bt.grad) <= 1e-12


def test_unrounded_downsample_reference_is_torch_autograd():
    bc = dict(NC.DS_CASES[-1], dtype="f32", w_dtype="f32", id="t-ds", G=3, rows=2)        # odd grid: padded quarters
    fc = dict(bc, entry="downsample_layernorm_fwd")
    inp = {k: v.double() for k, v in NC.inputs(bc).items()}
    x = inp["x"].clone().requires_grad_(True)
    w, b = inp["w"].clone().requires_grad_(True), inp["b"].clone().requires_grad_(True)
    y = F.layer_norm(R.merge(x, 3), (4 * bc["cols"],), w, b, NC.EPS)
    y.backward(inp["dy"])
    outs, _ = R.formulas(fc, inp, ft=torch.float64, rounding=False)
    assert _rel(outs["y"][0], y.detach()) <= 1e-12
    g, _ = R.formulas(bc, inp, {"mean": outs["mean"][0], "rstd": outs["rstd"][0]}, ft=torch.float64, rounding=False)
    assert _rel(g["dx"][0], x.grad) <= 1e-12 and _rel(g["dw"][0], w.grad) <= 1e-12 and _rel(g["db"][0], b.grad) <= 1e-12


@pytest.mark.parametrize("entry", ["adarms", "gated_residual"])
def test_unrounded_adarms_reference_is_torch_autograd(entry):
    bc = next(c for c in NC.AR_CASES if c["entry"] == entry + "_bwd" and c["gated"] and c["dtype"] == "f32")
    bc = dict(bc, res=False)
    fc = dict(bc, entry=entry + "_fwd")
    inp = {k: v.double() for k, v in NC.inputs(bc).items()}
    B, rps, C = bc["B"], bc["rps"], bc["cols"]
    x, br = inp["x"].clone().requires_grad_(True), inp["x2"].clone().requires_grad_(True)
    mod, modp = inp["mod"].clone().requires_grad_(True), inp["modp"].clone().requires_grad_(True)
    rep = lambda t: t.repeat_interleave(rps, 0)
    r = x + br * rep(modp[:, 2 * C:])
    if entry == "adarms":
        y = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + NC.EPS) * (1 + rep(mod[:, :C])) + rep(mod[:, C:2 * C])
    else:
        y = r
    y.backward(inp["dy"])
    outs, _ = R.formulas(fc, inp, ft=torch.float64, rounding=False)
    assert _rel(outs["y"][0], y.detach()) <= 1e-12
    g, _ = R.formulas(bc, inp, {"aux": r.detach(), "rstd": outs.get("rstd", (None,))[0]}, ft=torch.float64, rounding=False)
    if entry == "adarms":
        # dr is the gradient of r (the add's output); dbranch and dgate_prev follow it through the gated add
        assert _rel(g["dx"][0], x.grad) <= 1e-12 and _rel(g["aux"][0], br.grad) <= 1e-12
        assert _rel(g["dscale"][0], mod.grad[:, :C]) <= 1e-12 and _rel(g["dshift"][0], mod.grad[:, C:2 * C]) <= 1e-12
    else:
        assert _rel(g["dx"][0], br.grad) <= 1e-12
    assert _rel(g["dgate"][0], modp.grad[:, 2 * C:]) <= 1e-12


def test_colsum_reference():
    c = NC.COLSUM_CASES[-2]
    inp = NC.inputs(c)
    out = R.reference(c, inp)["out"]
    assert _rel(out[0], inp["x"].double().sum(0) + inp["y0"].double()) <= 1e-12
    assert torch.equal(out[3], inp["x"].double().abs().sum(0) + inp["y0"].double().abs())


def _emulated(case):
    inp = NC.inputs(case)
    stats = None
    if case["entry"].endswith("_bwd"):
        stats = R.emulate(R.forward_case(case), inp)
    return R.reference(case, inp, stats), R.emulate(case, inp, stats)


_MEASURED = {}


def measure():
    """largest excess (units of 2^-24 mag beyond the U ulp) of the fp32 emulation per output kind, and per entry point the share
    of bf16 output elements not bit-equal to the reference rounded to bf16"""
    if _MEASURED:
        return _MEASURED
    worst = {k: 0.0 for k in NC.K_SLACK}
    neq, tot = {}, {}
    for case in NC.ALL_CASES:
        ref, emu = _emulated(case)
        for n, (v, kind, U, mag) in ref.items():
            worst[kind] = max(worst[kind], float(R.excess(emu[n], v, U, mag).max()))
            if U:
                neq[case["entry"]] = neq.get(case["entry"], 0) + R.not_bit_equal(emu[n], v)
                tot[case["entry"]] = tot.get(case["entry"], 0) + v.numel()
    _MEASURED.update(worst=worst, share={e: neq[e] / tot[e] for e in tot})
    return _MEASURED


def test_slack_constants_cover_the_fp32_emulation():
    m = measure()
    print("fp32 emulation, largest excess per kind (2^-24 mag):", {k: round(v, 3) for k, v in m["worst"].items()})
    for kind, v in m["worst"].items():
        assert math.isfinite(v) and 4 * v <= NC.K_SLACK[kind], (kind, v)


def test_share_cap_holds_for_the_fp32_emulation():
    m = measure()
    print("fp32 emulation, share not bit-equal per entry point:", {k: f"{100 * v:.3f}%" for k, v in m["share"].items()})
    assert set(m["share"]) == {c["entry"] for c in NC.NORM_CASES} and len(m["share"]) == 12
    for e, s in m["share"].items():
        assert s <= NC.SHARE_CAP, (e, s)
