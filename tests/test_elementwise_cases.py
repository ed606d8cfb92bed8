"""The elementwise case table (tests/elementwise_cases.py) on the CPU: it names every instantiation csrc/elementwise.hip can launch,
each case's route is the one the host conditions give, the second-trip cases exceed the capped grid, and the inputs claimed to make
exact sums make them."""
import os
import re

import torch

from tests import elementwise_cases as E
from tests import elementwise_ref as R

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dexbotic_amd", "csrc", "elementwise.hip")
# kernels without a grid-stride loop: one workgroup per row / tile / column block, or one workgroup in all
NO_GRID_STRIDE = ("splice_bwd_k", "zero_rows_k", "token_drop_bwd_k", "mse_loss_k", "mse_loss_rows_k", "transpose_k", "transpose8_bf16_k")


def test_launch_sites_match_the_recorded_number():
    src = open(SRC).read()
    assert len(re.findall(r"hipLaunchKernelGGL\(", src)) == E.LAUNCH_SITES


def test_every_kernel_template_of_the_file_is_listed():
    src = open(SRC).read()
    defined = set(re.findall(r"__global__\s+__launch_bounds__\(\w+\)\s+void\s+(\w+)\(", src))
    listed = {i["kernel"] for i in E.INSTANTIATIONS.values()}
    assert defined == listed, (defined - listed, listed - defined)


def test_every_instantiation_is_claimed_by_a_case():
    claimed = {c["kernel"] for c in E.CASES}
    assert claimed == set(E.INSTANTIATIONS), set(E.INSTANTIATIONS) - claimed
    assert len(E.INSTANTIATIONS) == 104
    assert len({c["id"] for c in E.CASES}) == len(E.CASES)


def test_each_case_takes_the_route_it_claims():
    bad = [(c["id"], E.route(c)) for c in E.CASES if E.route(c) != c["kernel"]]
    assert not bad, bad
    for c in E.CASES:
        assert c["entry"] in E.INSTANTIATIONS[c["kernel"]]["entries"], c["id"]


def test_vector_width_fallbacks_have_odd_size_and_under_aligned_cases():
    """each narrower route of a width-selecting entry point is reached by an odd size and by an under-aligned operand"""
    for e in ("swiglu_fwd", "swiglu_bwd", "glu_fwd", "glu_bwd", "act_fwd", "act_bwd", "add", "axpby", "mul", "cast", "splice_fwd",
              "splice_bwd"):
        for t in ("bf16", "f32"):
            cs = [c for c in E.CASES if c["entry"] == e and c["dtype"] == t]
            narrow = [c for c in cs if c["kernel"].endswith(",1>") or c["kernel"].endswith(",1,0>") or c["kernel"].endswith(",1,1>")]
            size = {"swiglu": "F", "glu": "F", "splice": "d"}.get(e.split("_")[0], "n")
            assert any(not c["off"] and c["p"][size] % 4 for c in narrow), (e, t, "odd size")
            assert any(c["off"] and c["p"][size] % 4 == 0 for c in narrow), (e, t, "under-aligned")
    # bf16 x4 of the gated MLPs: F % 4 == 0 but F % 8 != 0; bf16 RoPE narrow: D % 16 != 0 and an 8-byte aligned operand
    for e in ("swiglu_fwd", "swiglu_bwd", "glu_fwd", "glu_bwd"):
        assert any(c["kernel"].endswith("<bf16,4>") and c["p"]["F"] % 8 for c in E.CASES if c["entry"] == e)
    for e in ("rope_split", "rope_merge"):
        n = [c for c in E.CASES if c["entry"] == e and c["kernel"].endswith("<bf16," + ("true" if "merge" in e else "false") + ",4>")]
        assert any(c["p"]["D"] % 16 for c in n) and any(c["off"] for c in n)
    tv = {(c["dtype"], E.transpose_vec(c)) for c in E.CASES if c["kernel"].startswith("transpose_k")}
    assert tv == {("bf16", 0), ("bf16", 1), ("f32", 0), ("f32", 1)}
    assert {c["p"]["to_head"] for c in E.CASES if c["entry"] == "permute"} == {0, 1}


def test_rope_operands_are_aligned_as_documented():
    """fp32 operands 16-byte aligned, bf16 at least 8-byte aligned, cos / sin 16-byte aligned (never misaligned on purpose)"""
    for c in E.CASES:
        if c["entry"] in R.ROPE_ENTRIES:
            for n, off in c["off"].items():
                assert n not in ("cos", "sin") and (off * E.ES[c["dtype"]]) % (16 if c["dtype"] == "f32" else 8) == 0, c["id"]


def test_rope_edges_are_present():
    for e in ("rope_split", "rope_merge"):
        cs = [c for c in E.CASES if c["entry"] == e]
        assert {24, 64, 128, 256} <= {c["p"]["D"] for c in cs} and 72 in {c["p"]["D"] for c in cs}
        assert any(c["p"]["Hq"] == 7 and c["p"]["Hkv"] == 1 for c in cs) and any(c["p"]["Hq"] == 2 and c["p"]["Hkv"] == 2 for c in cs)
        assert any(c["p"]["S_cap"] > c["p"]["S"] and c["p"]["s0"] > 0 for c in cs)
        for c in cs:
            if c["p"]["pos"]:
                pos = R.inputs(c)["pos"].long()
                if pos.numel() > 1:
                    assert int(pos.max()) >= c["p"]["S"] and bool((pos[1:] < pos[:-1]).any()), c["id"]


def test_second_trip_cases():
    """more than the capped grid's work items with a partial last trip; one per kernel template and dtype with a grid-stride loop"""
    have = set()
    for c in E.CASES:
        n = E.work_items(c)
        if c["trip2"]:
            cap = E.grid_cap(c)
            assert n > cap and n % cap, (c["id"], n)
            have.add((E.INSTANTIATIONS[c["kernel"]]["kernel"], E.INSTANTIATIONS[c["kernel"]]["targs"][:1], c.get("p", {}).get("dst")))
    want = set()
    for i in E.INSTANTIATIONS.values():
        if i["kernel"] not in NO_GRID_STRIDE:
            dst = i["targs"][1] if i["kernel"] in ("cast_k", "copy2d_k", "gather_rows_k", "scatter_rows_k", "im2col_k") else None
            want.add((i["kernel"], i["targs"][:1], dst))
    # vit_embed_fwd: the weight dtype is the second argument
    have_v = {c["p"]["w"] for c in E.CASES if c["trip2"] and c["entry"] == "vit_embed_fwd"}
    assert have_v == {"bf16", "f32"}
    assert want <= have, want - have


def test_splice_backward_edges():
    cs = [c for c in E.CASES if c["entry"] == "splice_bwd"]
    assert {1028, 1030} <= {c["p"]["d"] for c in cs}
    assert any(c["p"].get("no_img") for c in cs) and any(c["p"].get("no_embed") for c in cs)
    for c in cs:
        plan = R.inputs(c)["plan"]
        assert bool((plan == R.PAD).any())
        img = plan[(plan < 0) & (plan != R.PAD)]
        assert img.unique().numel() == img.numel()                      # every image row used once
        if c["p"]["n_rows"] >= 600:
            assert c["p"]["n_rows"] > 2 * 256                           # three ballot windows
            rows0 = (plan == 0).nonzero().flatten()
            assert int(rows0.min()) < 256 and int(rows0.max()) >= 64 + 64    # one id over whole waves
            assert (plan[:200] == 0).all()                              # 200 duplicates: every lane of wave 0..2 of window 0
        last = (plan == c["p"]["V"] - 1).nonzero().flatten()
        assert int(last.min()) & 255 != 0 and bool((last >= 256).any() or c["p"]["n_rows"] <= 256)


def test_scatter_indices_outside_the_rows_and_gather_indices_inside():
    for c in E.CASES:
        if c["entry"] == "scatter" and c["p"]["n"] > 6:
            idx = R.inputs(c)["idx"]
            assert bool(((idx < 0) | (idx >= c["p"]["R"])).any()) and idx.unique().numel() < idx.numel()
        if c["entry"] == "gather":
            idx = R.inputs(c)["idx"]
            assert bool(((idx >= 0) & (idx < c["p"]["R"])).all()) and idx.unique().numel() < idx.numel()


def test_claimed_exact_sums_are_exact():
    """bf16 add: the exponent spread of the addends stays <= 16, so the fp32 sum is exact; bf16 RoPE: products of two bf16 values
    are exact in fp32; bf16 mul: products are exact in fp32 outside the subnormal range"""
    for c in E.CASES:
        if c["dtype"] != "bf16":
            continue
        if c["entry"] == "add":
            inp = R.inputs(c)
            a, b = inp["a"].double(), inp["b"].double()
            s = a + b
            assert torch.equal(s.float().double(), s), c["id"]
            if c["values"] == "special":
                nz = (a != 0) & (b != 0)
                ea, eb = torch.frexp(a[nz])[1], torch.frexp(b[nz])[1]
                assert int((ea - eb).abs().max()) <= 16, c["id"]
        if c["entry"] == "mul":
            inp = R.inputs(c)
            pr = inp["a"].double() * inp["b"].double()
            big = pr.abs() >= 2.0 ** -126
            assert torch.equal(pr[big].float().double(), pr[big]), c["id"]
    c = next(c for c in E.CASES if c["entry"] == "rope_split" and c["dtype"] == "bf16")
    inp = R.inputs(c)
    x = inp["qkv"].double()[:, : c["p"]["D"] // 2]
    cc = R._rope_tables(c, inp)[0]
    pr = x * cc
    assert torch.equal(pr.float().double(), pr)


def test_special_values_reach_every_bf16_route_of_a_family():
    """the special set through every bf16 route, with |x| in {20, 88, 89, 100}, +-0 and subnormal products"""
    for g, ids in E.ROUTE_GROUPS.items():
        ks = {next(c for c in E.CASES if c["id"] == i)["kernel"] for i in ids}
        e = g[0]
        want = {i for i in E.INSTANTIATIONS if e in E.INSTANTIATIONS[i]["entries"] and "<bf16," in i}
        assert ks == want, (g, ks, want)
    c = next(c for c in E.CASES if c["entry"] == "act_fwd" and c["values"] == "special")
    x = R.inputs(c)["x"].double()
    for v in (20.0, 88.0, 89.0, 100.0):
        assert bool((x == v).any() and (x == -v).any()), v
    assert bool((x == 0).any()) and bool((torch.signbit(x) & (x == 0)).any())
    c = next(c for c in E.CASES if c["entry"] == "mul" and c["values"] == "special")
    inp = R.inputs(c)
    pr = (inp["a"].double() * inp["b"].double()).abs()
    assert bool(((pr > 0) & (pr < 2.0 ** -126)).any())
    for e in ("cast", "transpose", "permute", "gather", "splice_fwd"):
        c = next(c for c in E.CASES if c["entry"] == e and c["values"] == "special")
        v = next(iter(t for n, t in R.inputs(c).items() if t.is_floating_point())).double()
        assert bool(torch.isnan(v).any() and torch.isinf(v).any()), e
