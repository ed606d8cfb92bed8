"""The fp64 reference of tests/elementwise_ref.py on the CPU: the backward formulas are torch autograd's in fp64, SwiGLU and RoPE are
torch's own bf16 / fp32 evaluation of the HF formulas bit for bit, the slack constants of tests/elementwise_cases.py cover the fp32
stand-in they were measured from, the share cap holds for it, and the share cap catches a dropped rounding point."""
import pytest
import torch
import torch.nn.functional as Fn

from tests import elementwise_cases as E
from tests import elementwise_ref as R

F64 = torch.float64
SMALL_F32 = [c for c in E.CASES if c["dtype"] == "f32" and not c["trip2"] and c["values"] == "randn"]


def _close(a, b, rtol=1e-12, atol=1e-300):
    assert torch.allclose(a.double(), b.double(), rtol=rtol, atol=atol), float((a.double() - b.double()).abs().max())


def _act_torch(act, x):
    """the activations with the kernels' fp32 constants, for autograd"""
    a = E.ACT
    if act == a["gelu_erf"]:
        return 0.5 * x * (1 + torch.erf(x * R.f32c(R.GE_C)))
    if act == a["gelu_tanh"]:
        return 0.5 * x * (1 + torch.tanh(R.f32c(R.GT_K) * (x + R.f32c(0.044715) * x ** 3)))
    if act == a["quick_gelu"]:
        return x * torch.sigmoid(R.f32c(R.QG_A) * x)
    if act == a["silu"]:
        return Fn.silu(x)
    if act == a["relu"]:
        return torch.relu(x)
    if act == a["sigmoid"]:
        return torch.sigmoid(x)
    return x


_BWD = [c for c in SMALL_F32 if c["entry"] in ("swiglu_bwd", "glu_bwd", "act_bwd", "rope_merge", "mse", "mse_rows", "splice_bwd",
                                                "scatter", "token_drop_bwd", "dit_bwd", "vit_embed_bwd")]


@pytest.mark.parametrize("case", _BWD, ids=lambda c: c["id"])
def test_backward_formulas_match_autograd_fp64(case):
    e, p = case["entry"], case["p"]
    inp = R.inputs(case)
    ref = R.reference(case, inp)
    f = lambda n: inp[n].to(F64).clone().requires_grad_(True)
    if e in ("swiglu_bwd", "glu_bwd"):
        F = p["F"]
        gu = f("gu")
        act = p.get("act", E.ACT["silu"])
        (_act_torch(act, gu[:, :F]) * gu[:, F:]).backward(inp["dout"].to(F64))
        # the kernels' derivative formulas carry exact constants (1 / sqrt(2 pi)) next to fp32 ones (1 / sqrt(2) in erf): ~1e-8 |dy|
        _close(ref["dgu_g"]["v"], gu.grad[:, :F], rtol=1e-6, atol=1e-6)
        _close(ref["dgu_u"]["v"], gu.grad[:, F:])
    elif e == "act_bwd":
        x = f("x")
        _act_torch(p["act"], x).backward(inp["dy"].to(F64))
        _close(ref["dx"]["v"], x.grad, rtol=1e-6, atol=1e-6)
    elif e == "rope_merge":
        B, S, Hq, Hkv, D, s0 = p["B"], p["S"], p["Hq"], p["Hkv"], p["D"], p["s0"]
        HS, half = Hq + 2 * Hkv, D // 2
        x = torch.zeros(B * S, HS, D, dtype=F64, requires_grad=True)
        c, s = (t.float().double() for t in R._rope_tables(case, inp))
        C_, S_ = torch.cat([c, c], -1)[:, None], torch.cat([s, s], -1)[:, None]
        rot = lambda t: torch.cat([-t[..., half:], t[..., :half]], -1)
        y = torch.cat([x[:, :Hq + Hkv] * C_ + rot(x[:, :Hq + Hkv]) * S_, x[:, Hq + Hkv:]], 1)
        g = torch.cat([inp[n].to(F64)[:, :, s0:s0 + S] for n in ("dq", "dk", "dv")], 1).permute(0, 2, 1, 3).reshape(B * S, HS, D)
        y.backward(g)
        ga = g.abs()
        mag = (ga * C_.abs() + torch.cat([ga[..., half:], ga[..., :half]], -1) * S_.abs()).reshape(B * S, HS * D)
        assert ((ref["dqkv"]["v"] - x.grad.reshape(B * S, HS * D)).abs() <= 2 * R.TWO24 * mag).all()    # 2 products, 1 sum in fp32
    elif e in ("mse", "mse_rows"):
        pr = f("pred")
        d = pr - inp["target"].to(F64)
        if e == "mse":
            loss = (d * d).mean()
        else:
            w = inp["row_w"].to(F64)[:, None]
            loss = (w * d * d).mean(1, keepdim=True).sum() / (w.sum() + R.f32c(1e-6))
        (loss * R.f32c(p["gscale"])).backward()
        _close(ref["dpred"]["v"], pr.grad, rtol=1e-10)
    elif e == "splice_bwd":
        emb = torch.zeros(p["V"], p["d"], dtype=F64, requires_grad=True)
        img = torch.zeros(p["n_img"], p["d"], dtype=F64, requires_grad=True)
        plan = inp["plan"]
        tok, im = plan >= 0, (plan < 0) & (plan != R.PAD)
        out = torch.zeros(p["n_rows"], p["d"], dtype=F64)
        out = out.index_put((tok.nonzero().flatten(),), emb[plan[tok]]).index_put((im.nonzero().flatten(),), img[-1 - plan[im]])
        out.backward(inp["dout"].to(F64))
        if "d_embed" in ref:
            # fp32 sums of up to n_rows terms: |error| <= n_rows 2^-24 (|d_embed| + sum |dout|)
            ea = torch.zeros_like(emb).index_add_(0, plan[tok], inp["dout"].to(F64)[tok].abs())
            bound = p["n_rows"] * R.TWO24 * (inp["d_embed"].to(F64).abs() + ea)
            assert ((ref["d_embed"]["v"] - inp["d_embed"].to(F64) - emb.grad).abs() <= bound).all()
        if "d_img" in ref:
            used = torch.zeros(p["n_img"], dtype=torch.bool)
            used[-1 - plan[im]] = True
            _close(ref["d_img"]["v"][used], img.grad[used])
    elif e == "scatter":
        x = torch.zeros(p["R"], p["d"], dtype=F64, requires_grad=True)
        idx = inp["idx"]
        ok = (idx >= 0) & (idx < p["R"])
        x[idx[ok]].backward(inp["dout"].to(F64)[ok])
        ea = torch.zeros_like(x).index_add_(0, idx[ok], inp["dout"].to(F64)[ok].abs())
        bound = p["n"] * R.TWO24 * ea + (R.ulp(ref["dx"]["v"], "bf16") if p["dst"] == "bf16" else 0)
        assert ((ref["dx"]["v"] - x.grad).abs() <= bound).all()
    elif e == "token_drop_bwd":
        z, unc = f("dout").detach().zero_().requires_grad_(True), torch.zeros(p["d"], dtype=F64, requires_grad=True)
        dr = inp["drop"].bool()[:, None]
        torch.where(dr, unc[None].expand(p["N"], p["d"]), z).backward(inp["dout"].to(F64))
        want = unc.grad + (inp["dunc"].to(F64) if p["accumulate"] else 0)
        bound = (p["N"] + 1) * R.TWO24 * (inp["dout"].to(F64).abs().sum(0) + (inp["dunc"].to(F64).abs() if p["accumulate"] else 0))
        assert ((ref["dunc"]["v"] - want).abs() <= bound).all()
        if "dz" in ref:
            _close(ref["dz"]["v"], z.grad)
    elif e == "dit_bwd":
        xe, te = f("dh").detach()[:, 1:].clone().requires_grad_(True), f("dh").detach()[:, 0].clone().requires_grad_(True)
        (torch.cat([te[:, None], xe], 1)).backward(inp["dh"].to(F64))
        _close(ref["dxe"]["v"], xe.grad)
        _close(ref["dc"]["v"], te.grad)
    elif e == "vit_embed_bwd":
        N, n, C = p["N"], p["np"], p["C"]
        pa = torch.zeros(N, n, C, dtype=F64, requires_grad=True)
        torch.cat([torch.zeros(N, 1, C, dtype=F64), pa], 1).backward(inp["dx"].to(F64))
        _close(ref["dpatch"]["v"], pa.grad)


# SwiGLU's bf16 outputs (an fp32 SwiGLU is a bounded output: silu itself is not correctly rounded); RoPE in both dtypes
_HF = [c for c in E.CASES if (c["entry"] == "rope_split" or c["entry"] == "swiglu_fwd" and c["dtype"] == "bf16") and
       c["values"] == "randn" and not c["trip2"]]


@pytest.mark.parametrize("case", _HF, ids=lambda c: c["id"])
def test_swiglu_and_rope_match_torch_bit_for_bit(case):
    """silu(g) * u and q * cos + rotate_half(q) * sin evaluated by torch in the case's dtype"""
    T, p = E.TORCH_DT[case["dtype"]], case["p"]
    inp = R.inputs(case)
    ref = R.reference(case, inp)
    iv = torch.int16 if T == torch.bfloat16 else torch.int32
    if case["entry"] == "swiglu_fwd":
        F = p["F"]
        gu = inp["gu"]
        want = Fn.silu(gu[:, :F]) * gu[:, F:]
        assert torch.equal(ref["out"]["v"].to(T).view(iv), want.view(iv))
        return
    B, S, Hq, Hkv, D, s0 = p["B"], p["S"], p["Hq"], p["Hkv"], p["D"], p["s0"]
    half = D // 2
    x = inp["qkv"].view(B, S, Hq + 2 * Hkv, D)
    pr = inp["pos"].long() if "pos" in inp else torch.arange(S).repeat(B)
    cos = torch.cat([inp["cos"][pr]] * 2, -1).to(T).view(B, S, 1, D)
    sin = torch.cat([inp["sin"][pr]] * 2, -1).to(T).view(B, S, 1, D)
    rot = lambda t: torch.cat([-t[..., half:], t[..., :half]], -1)
    y = x[:, :, :Hq + Hkv] * cos + rot(x[:, :, :Hq + Hkv]) * sin
    for n, lo, hi in (("q", 0, Hq), ("k", Hq, Hq + Hkv)):
        got = ref[n]["v"][:, :, s0:s0 + S].to(T)
        assert torch.equal(got.view(iv), y[:, :, lo:hi].permute(0, 2, 1, 3).contiguous().view(iv)), n


@pytest.mark.parametrize("case", [c for c in E.CASES if c["entry"] == "rope_merge" and c["dtype"] == "f32" and not c["trip2"]],
                         ids=lambda c: c["id"])
def test_fp32_rope_merge_is_autograd_in_fp32_bit_for_bit(case):
    p = case["p"]
    B, S, Hq, Hkv, D, s0 = p["B"], p["S"], p["Hq"], p["Hkv"], p["D"], p["s0"]
    HS, half = Hq + 2 * Hkv, D // 2
    inp = R.inputs(case)
    ref = R.reference(case, inp)
    pr = inp["pos"].long() if "pos" in inp else torch.arange(S).repeat(B)
    cos = torch.cat([inp["cos"][pr]] * 2, -1)[:, None]
    sin = torch.cat([inp["sin"][pr]] * 2, -1)[:, None]
    x = torch.zeros(B * S, Hq + Hkv, D, requires_grad=True)
    rot = lambda t: torch.cat([-t[..., half:], t[..., :half]], -1)
    y = x * cos + rot(x) * sin
    g = torch.cat([inp[n][:, :, s0:s0 + S] for n in ("dq", "dk")], 1).permute(0, 2, 1, 3).reshape(B * S, Hq + Hkv, D)
    y.backward(g)
    got = ref["dqkv"]["v"].float().view(B * S, HS, D)[:, :Hq + Hkv]
    assert torch.equal(got.view(torch.int32), x.grad.view(torch.int32))


def _fma32(a, b, c):
    """fma(a, b, c) of fp32 values held in fp64: the product is exact in fp64, then one fp64 add and the rounding to fp32 (the
    double rounding moves a last bit only at a near-tie: nothing to a share of several per cent)"""
    return R.r32(a * b + c)


_UNIT = [c for c in E.CASES if R.is_unit(c) and c["dtype"] == "f32" and not c["trip2"]]


@pytest.mark.parametrize("case", _UNIT, ids=lambda c: c["id"])
def test_unit_qknorm_cases_tell_a_contracted_rotation(case):
    """the fp32 unit cases of the q/k-norm kernels are there to hold the rotation uncontracted: on their inputs either way of
    contracting a product into the add changes a share of the q / k outputs, and the norm around the rotation is the identity"""
    p = case["p"]
    B, S, Hq, Hkv, D = p["B"], p["S"], p["Hq"], p["Hkv"], p["D"]
    HS, half = Hq + 2 * Hkv, D // 2
    inp = R.inputs(case)
    assert bool((inp["wq"] == 1).all() and (inp["wk"] == 1).all())
    c, s = (t[:, None, :].expand(B * S, Hq + Hkv, half) for t in R._rope_tables(case, inp))
    if case["entry"] == "qknorm_split":
        x = inp["qkv"].double().view(B * S, HS, D)
        sq = x * x
        assert torch.equal(sq * 16, (sq * 16).round()) and D <= 2 ** 20            # multiples of 1 / 16: every partial sum exact in fp32
        assert torch.equal(sq.sum(-1), torch.full((B * S, HS), float(D), dtype=F64))
        x = x[:, :Hq + Hkv]
        a1, a2 = x[..., :half], -x[..., half:]
        want = R.reference(case, inp)
        got = torch.cat([want[n]["v"].permute(0, 2, 1, 3) for n in ("q", "k")], 2).reshape(B * S, Hq + Hkv, D)[..., :half]
    else:
        assert bool((inp["qkv"] == 0).all() and (inp["rstd"] == 1).all())
        g = torch.cat([inp[n].double() for n in ("dq", "dk")], 1).permute(0, 2, 1, 3).reshape(B * S, Hq + Hkv, D)
        a1, a2 = g[..., :half], g[..., half:]
        got = R.reference(case, inp)["dqkv"]["v"].view(B * S, HS, D)[:, :Hq + Hkv, :half]
    plain = R.add32(R.mul32(a1, c), R.mul32(a2, s))
    assert torch.equal(plain, got)                                                    # the reference is the uncontracted form
    for fused in (_fma32(a1, c, R.mul32(a2, s)), _fma32(a2, s, R.mul32(a1, c))):
        share = float((fused != plain).double().mean())
        print(f"{case['id']}: a contracted rotation changes {100 * share:.1f} % of the first halves")
        # (position 0 and the slow dims of a short sequence have cos = 1, sin ~ 0 and rotate exactly: D = 32 at S = 5 is the floor)
        assert share > 0.02 and int((fused != plain).sum()) >= 8, share


_BOUNDED = [c for c in E.CASES if c["entry"] in R.BOUNDED_ENTRIES]


@pytest.fixture(scope="module")
def standin():
    """the fp32 CPU stand-in of every bounded case: id -> (reference, emulation)"""
    out = {}
    for c in _BOUNDED:
        inp = R.inputs(c)
        out[c["id"]] = (R.reference(c, inp), R.emulate(c, inp))
    return out


def test_slack_constants_cover_the_cpu_standin(standin):
    worst = {}
    for c in _BOUNDED:
        ref, em = standin[c["id"]]
        for n, v in em.items():
            ex = R.excess(v, ref[n], R.out_dtype(c, n), E.GELU_TANH_ABS)
            worst[ref[n]["kind"]] = max(worst.get(ref[n]["kind"], 0.0), float(ex.max()))
    print("worst fp32 stand-in error, x 2^-24 mag:", {k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == set(E.K_SLACK)
    assert all(worst[k] <= E.K_SLACK[k] / 4 for k in worst), worst


def test_gelu_tanh_term_covers_the_fast_formula():
    worst = 0.0
    for c in E.CASES:
        if c["p"].get("act") == E.ACT["gelu_tanh"] and not c["trip2"]:
            inp = R.inputs(c)
            x = (inp["x"] if "x" in inp else inp["gu"][:, :c["p"]["F"]]).float()
            u = R.f32c(R.GT_K) * (x + R.f32c(0.044715) * x * x * x)
            fast = 1 - 2 / (1 + torch.exp(2 * u))
            worst = max(worst, float((fast.double() - torch.tanh(u.double())).abs().max()))
    assert 0 < 4 * worst <= E.GELU_TANH_ABS, worst


def test_share_cap_holds_for_the_cpu_standin(standin):
    neq, tot = {}, {}
    for c in _BOUNDED:
        ref, em = standin[c["id"]]
        for n, v in em.items():
            for key in R.share_keys(c):                                  # per entry point, and per instantiation of it
                neq[key] = neq.get(key, 0) + R.not_bit_equal(v, ref[n]["v"])
                tot[key] = tot.get(key, 0) + v.numel()
    share = {e: neq[e] / tot[e] for e in tot}
    print("share not bit-equal (fp32 stand-in, bf16):", {str(e): f"{neq[e]}/{tot[e]} = {100 * s:.4f}%" for e, s in share.items()})
    assert all(s <= E.SHARE_CAP for s in share.values()), {e: s for e, s in share.items() if s > E.SHARE_CAP}
    # every bf16 instantiation of these entry points has a share of its own, resting on enough elements that the cap is not one
    # or two of them
    want = {(e, k) for k, i in E.INSTANTIATIONS.items() for e in i["entries"] if e in tot and i["targs"][0] == "bf16"}
    assert want == {k for k in tot if isinstance(k, tuple)}, want ^ {k for k in tot if isinstance(k, tuple)}
    assert all(tot[k] * E.SHARE_CAP >= 20 for k in tot), {k: tot[k] for k in tot if tot[k] * E.SHARE_CAP < 20}


def test_share_cap_catches_a_dropped_rounding_point():
    """SwiGLU without the rounding of silu to bf16, and bf16 RoPE with each half rotated in one rounding, leave the share cap"""
    neq, tot = {}, {}
    for c in E.CASES:
        if c["entry"] == "swiglu_fwd" and len(R.share_keys(c)) == 2:
            inp = R.inputs(c)
            F = c["p"]["F"]
            g, u = inp["gu"][:, :F].double(), inp["gu"][:, F:].double()
            seeded = R.rnd(R._silu(g) * u, "bf16")
            neq[c["kernel"]] = neq.get(c["kernel"], 0) + R.not_bit_equal(seeded, R.reference(c, inp)["out"]["v"])
            tot[c["kernel"]] = tot.get(c["kernel"], 0) + seeded.numel()
    assert len(tot) == 3                                                # x8, x4, x1: the defect in any one of them alone
    assert all(neq[k] / tot[k] > 10 * E.SHARE_CAP for k in tot), {k: neq[k] / tot[k] for k in tot}
    neq = tot = 0
    for c in E.CASES:
        if c["entry"] == "rope_split" and c["dtype"] == "bf16" and not c["trip2"]:
            p = c["p"]
            inp = R.inputs(c)
            half = p["D"] // 2
            x = inp["qkv"].double().view(p["B"] * p["S"], -1, p["D"])[:, :p["Hq"] + p["Hkv"]]
            cc, ss = (t[:, None] for t in R._rope_tables(c, inp))
            fused = R.rnd(x[..., :half] * cc - x[..., half:] * ss, "bf16")
            ref = R.rnd(R.add32(R.rnd(R.mul32(x[..., :half], cc.expand_as(fused)), "bf16"),
                                R.rnd(R.mul32(-x[..., half:], ss.expand_as(fused)), "bf16")), "bf16")
            neq += R.not_bit_equal(fused, ref)
            tot += fused.numel()
    assert neq / tot > 10 * E.SHARE_CAP, neq / tot
