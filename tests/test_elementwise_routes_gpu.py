"""Every case of tests/elementwise_cases.py on the MI355X: the entry points of csrc/elementwise.hip called through the C ABI on the
test's own buffers, against the fp64 reference of tests/elementwise_ref.py.

Inputs are carved out of NaN-filled buffers, outputs out of sentinel-filled ones, each at the case's offset from a 256-byte-aligned
base.  Per case: the guards in front of and behind every output are intact and the inputs unchanged; the call, captured once into a
graph (never replayed), holds one kernel node whose function the runtime names with the case's instantiation, and a case that
claims a second grid-stride trip launched the capped grid; the eager call's outputs equal the reference bit for bit (exact outputs,
NaN as NaN) or hold
    |got - ref| <= ulp_T(ref) + k * 2^-24 * mag + 2^-126          (elementwise_cases.py: k = K_SLACK per output kind)
Over the bf16 bounded cases of one entry point (GELU-tanh excluded), and over those of one kernel instantiation of it, at most
SHARE_CAP of the elements differ from the reference rounded to bf16.  The torch-fp32-on-device stand-in that half of each K_SLACK
was measured from stays within K_SLACK / 4.  The bf16 routes of a family give the same bits on the same special inputs, and the splice backward repeats bit
for bit with another case in between."""
import ctypes as C
import time

import pytest
import torch

from tests import elementwise_cases as E
from tests import elementwise_ref as R
from tests.helpers import _captured_kernel

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import graphs

DEV = "cuda"
G = 256                                        # guard elements on each side (a multiple of 16 bytes for every dtype)
TD = dict(E.TORCH_DT, i64=torch.int64, i32=torch.int32, u8=torch.uint8)
IV = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int64: torch.int64, torch.int32: torch.int32, torch.uint8: torch.uint8}


class Carved:
    """an operand of ``shape`` carved out of a larger buffer filled with ``fill``: ``G + off`` guard elements in front, G behind"""

    def __init__(self, shape, dt, fill, off=0, value=None):
        n = 1
        for s in shape:
            n *= s
        self.dtype = TD[dt]
        self.buf = torch.full((2 * G + off + n,), fill, dtype=self.dtype, device=DEV)
        self.lo, self.hi = G + off, G + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if value is not None:
            self.t.copy_(value.to(DEV))
        self.before = self.buf.clone()

    def _iv(self, t):
        return t.view(IV[self.dtype])

    def guards_ok(self):
        b, a = self._iv(self.buf), self._iv(self.before)
        return torch.equal(b[:self.lo], a[:self.lo]) and torch.equal(b[self.hi:], a[self.hi:])

    def unchanged(self):
        return torch.equal(self._iv(self.buf), self._iv(self.before))


def _alloc(case, inp):
    ins, outs = {}, {}
    for n, (shape, dt, role) in R.operands(case).items():
        off = case["off"].get(n, 0)
        if role == "in":
            fill = 0 if dt in ("i64", "i32", "u8") else float("nan")
            ins[n] = Carved(shape, dt, fill, off, inp[n])
        elif role == "inout":
            outs[n] = Carved(shape, dt, R.SENT[dt], off, inp[n])
        else:
            outs[n] = Carved(shape, dt, R.SENT[dt], off)
    return ins, outs


def _call(case, o, stream):
    """the case's C entry point on operands ``o`` (name -> tensor)"""
    lib, e, t, p = L.lib, case["entry"], E.DT[case["dtype"]], case["p"]
    a = lambda n: o[n].data_ptr() if o.get(n) is not None else None
    d2 = E.DT[p.get("dst", case["dtype"])]
    if e in ("rope_split", "rope_merge"):
        B, S, Hq, Hkv, D = p["B"], p["S"], p["Hq"], p["Hkv"], p["D"]
        if e == "rope_split":
            return lib.dxa_rope_split_at(a("qkv"), a("q"), a("k"), a("v"), a("cos"), a("sin"), a("pos"), B, S, Hq, Hkv, D, p["S_cap"],
                                         p["s0"], t, stream)
        return lib.dxa_rope_merge_at(a("dq"), a("dk"), a("dv"), a("dqkv"), a("cos"), a("sin"), a("pos"), B, S, Hq, Hkv, D, p["S_cap"],
                                     p["s0"], t, stream)
    if e == "qknorm_split":
        B, S, Hq, Hkv, D = p["B"], p["S"], p["Hq"], p["Hkv"], p["D"]
        eps = 0.0 if "unit" in case["id"].split("-") else 1e-6
        return lib.dxa_qknorm_rope_split_at(a("qkv"), a("q"), a("k"), a("v"), a("wq"), a("wk"), eps, a("rstd"), a("cos"), a("sin"),
                                            a("pos"), B, S, Hq, Hkv, D, S, 0, S, 0, t, stream)
    if e == "qknorm_merge":
        B, S, Hq, Hkv, D = p["B"], p["S"], p["Hq"], p["Hkv"], p["D"]
        return lib.dxa_qknorm_rope_merge_from(a("dq"), a("dk"), a("dv"), a("qkv"), a("rstd"), a("wq"), a("wk"), a("dqkv"), None, a("cos"),
                                              a("sin"), a("pos"), B, S, Hq, Hkv, D, S, 0, t, stream)
    if e == "swiglu_fwd":
        return lib.dxa_swiglu_fwd(a("gu"), a("out"), p["rows"], p["F"], t, stream)
    if e == "swiglu_bwd":
        return lib.dxa_swiglu_bwd(a("gu"), a("dout"), a("dgu"), p["rows"], p["F"], t, stream)
    if e == "glu_fwd":
        return lib.dxa_glu_fwd(a("gu"), a("out"), p["rows"], p["F"], p["act"], t, stream)
    if e == "glu_bwd":
        return lib.dxa_glu_bwd(a("gu"), a("dout"), a("dgu"), p["rows"], p["F"], p["act"], t, stream)
    if e == "act_fwd":
        return lib.dxa_act_fwd(a("x"), a("y"), p["n"], p["act"], t, stream)
    if e == "act_bwd":
        return lib.dxa_act_bwd(a("x"), a("dy"), a("dx"), p["n"], p["act"], t, stream)
    if e == "add":
        return lib.dxa_add(a("a"), a("b"), a("out"), p["n"], t, stream)
    if e == "axpby":
        return lib.dxa_axpby(a("a"), a("b"), a("out"), p["n"], p["alpha"], p["beta"], t, stream)
    if e == "mul":
        return lib.dxa_mul(a("a"), a("b"), a("out"), p["n"], t, stream)
    if e == "mul_rows":
        return lib.dxa_mul_rows(a("x"), a("g"), a("out"), p["R"], p["Nn"], p["C"], t, stream)
    if e == "cast":
        return lib.dxa_cast(a("src"), a("dst"), p["n"], t, d2, stream)
    if e == "copy2d":
        return lib.dxa_copy2d(a("src"), p["lds"], a("dst"), p["ldd"], p["rows"], p["cols"], p["cols_padded"], t, d2, stream)
    if e == "gather":
        return lib.dxa_gather_rows(a("x"), a("idx"), a("out"), p["n"], p["d"], t, d2, stream)
    if e == "scatter":
        return lib.dxa_scatter_rows(a("dout"), a("idx"), a("dx"), p["n"], p["R"], p["d"], t, d2, stream)
    if e == "im2col":
        return lib.dxa_im2col(a("images"), a("rows"), p["N"], p["H"], p["W"], p["P"], p["ld"], t, d2, stream)
    if e == "splice_fwd":
        return lib.dxa_splice_fwd(a("plan"), a("embed"), a("img"), a("out"), p["n_rows"], p["d"], t, stream)
    if e == "splice_bwd":
        return lib.dxa_splice_bwd(a("plan"), a("dout"), a("d_embed"), a("d_img"), p["n_rows"], p["d"], t, stream)
    if e == "zero_rows":
        return lib.dxa_zero_rows(a("plan"), a("g"), p["n_rows"], p["d"], stream)
    if e == "vit_embed_fwd":
        return lib.dxa_vit_embed_fwd(a("patch"), a("cls"), a("pos"), a("x"), p["N"], p["np"], p["C"], t, E.DT[p["w"]], stream)
    if e == "vit_embed_bwd":
        return lib.dxa_vit_embed_bwd(a("dx"), a("dpatch"), p["N"], p["np"], p["C"], t, stream)
    if e == "qsample":
        return lib.dxa_qsample(a("x0"), a("noise"), a("a"), a("s"), a("xt"), p["N"], p["per"], stream)
    if e == "timestep":
        return lib.dxa_timestep_embedding(a("t"), a("freqs"), a("out"), p["N"], p["half"], stream)
    if e == "dit_fwd":
        return lib.dxa_dit_assemble_fwd(a("xe"), a("te"), a("ze"), a("pos"), a("h"), p["N"], p["T"], p["hd"], stream)
    if e == "dit_bwd":
        return lib.dxa_dit_assemble_bwd(a("dh"), a("dxe"), a("dc"), p["N"], p["T"], p["hd"], stream)
    if e == "token_drop":
        return lib.dxa_token_drop(a("z"), a("unc"), a("drop"), a("out"), p["N"], p["d"], stream)
    if e == "token_drop_bwd":
        return lib.dxa_token_drop_bwd(a("dout"), a("drop"), a("dz"), a("dunc"), p["N"], p["d"], p["accumulate"], stream)
    if e == "mse":
        return lib.dxa_mse_loss(a("pred"), a("target"), a("loss"), a("dpred"), p["n"], p["gscale"], stream)
    if e == "mse_rows":
        return lib.dxa_mse_loss_rows(a("pred"), a("target"), a("row_w"), a("loss"), a("dpred"), p["rows"], p["cols"], p["gscale"], stream)
    if e == "ddim":
        s = R.ddim_scalars()
        return lib.dxa_ddim_step(a("x"), a("mo"), p["B"], p["per"], p["use_cfg"], s["cfg_scale"], s["c_recip"], s["c_recipm1"],
                                 s["ab_prev"], stream)
    if e == "transpose":
        return lib.dxa_transpose(a("src"), p["lds"], a("dst"), p["ldd"], p["R"], p["C"], p["Rp"], t, stream)
    if e == "permute":
        return lib.dxa_permute_bshd(a("src"), a("dst"), p["B"], p["S"], p["H"], p["D"], p["to_head"], t, stream)
    raise AssertionError(e)


def _capture(case, ops, side):
    g = torch.cuda.CUDAGraph(keep_graph=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with graphs.capture(g, side):
            rc = _call(case, ops, side.cuda_stream)
    assert rc == 0, L.last_error()
    return _captured_kernel(g.raw_cuda_graph(), side.cuda_stream)


def _run(case, inp, side=None):
    """one guarded call -> (outputs on the CPU, problems, (kernel name, grid.x) of the captured call or None)"""
    ins, outs = _alloc(case, inp)
    ops = {n: c.t for n, c in {**ins, **outs}.items()}
    cap = _capture(case, ops, side) if side is not None else None
    L.check(_call(case, ops, torch.cuda.current_stream().cuda_stream), case["entry"])
    torch.cuda.synchronize()
    problems = [f"{n}: guard damaged" for n, c in outs.items() if not c.guards_ok()]
    problems += [f"{n}: input changed" for n, c in ins.items() if not c.unchanged()]
    got = {}
    for n, c in outs.items():
        got.update(R.split_output(case, n, c.t.cpu()))
    return got, problems, cap


_REPEAT_OTHER = next(c for c in E.CASES if c["entry"] == "splice_bwd" and c["p"]["d"] == 1028 and c["dtype"] == "f32")


class _Results(dict):
    """id -> record of the case run once (splice backward twice, another case in between), computed on first use"""

    def __init__(self):
        super().__init__()
        self.side = torch.cuda.Stream()

    def __missing__(self, cid):
        case = next(c for c in E.CASES if c["id"] == cid)
        inp = R.inputs(case)
        got, problems, cap = _run(case, inp, self.side)
        if case["entry"] == "splice_bwd":
            _run(_REPEAT_OTHER, R.inputs(_REPEAT_OTHER))
            got2, problems2, _ = _run(case, inp)
            problems += problems2
            if any(not torch.equal(got[n].view(IV[got[n].dtype]), got2[n].view(IV[got[n].dtype])) for n in got):
                problems.append("second run not bit-identical")
        rec = dict(got=got, problems=problems, cap=cap, ref=R.reference(case, inp))
        self[cid] = rec
        return rec


@pytest.fixture(scope="module")
def results():
    t0 = time.time()
    res = _Results()
    yield res
    torch.cuda.synchronize()
    print(f"\n{len(res)} cases in {time.time() - t0:.1f} s")


def _bad_values(case, got, ref):
    bad = []
    for n, o in ref.items():
        dt = R.out_dtype(case, n)
        if o["exact"]:
            mis = R.exact_mismatch(got[n], o, dt)
            if mis.any():
                i = int(mis.flatten().nonzero()[0])
                bad.append(f"{n}: {int(mis.sum())}/{mis.numel()} differ from the reference, first at flat {i}: got "
                           f"{float(got[n].flatten()[i]):.9g} want {float(o['v'].flatten()[i]):.9g}")
            continue
        ex = R.excess(got[n], o, dt, E.GELU_TANH_ABS)
        k = E.K_SLACK[o["kind"]]
        print(f"{case['id']} {n}: worst {float(ex.max()):.3g} x 2^-24 mag (k {k})")
        if not (ex <= k).all():
            i = int(torch.argmax(ex))
            bad.append(f"{n}: {int((ex > k).sum())}/{ex.numel()} over the bound, worst {float(ex.flatten()[i]):.3g} x 2^-24 mag (k {k}) "
                       f"at flat {i}: got {float(got[n].flatten()[i]):.9g} want {float(o['v'].flatten()[i]):.9g}")
    return bad


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c["id"])
def test_elementwise_route(case, results):
    rec = results[case["id"]]
    name, gx = rec["cap"]
    inst = E.INSTANTIATIONS[case["kernel"]]
    assert name is not None, "the runtime did not name the captured kernel"
    assert inst["mangled"] in name or inst["demangled"] in name, (name, case["kernel"])
    if case["trip2"]:
        assert gx == E.grid_cap(case) // 256, gx
    assert not rec["problems"], rec["problems"]
    if case["entry"] == "qknorm_split" and "unit" in case["id"].split("-"):
        rs = rec["got"]["rstd"]
        assert torch.equal(rs, torch.ones_like(rs)), f"rstd of the unit-RMS rows is not 1.0: {rs.unique()[:8].tolist()}"
    bad = _bad_values(case, rec["got"], rec["ref"])
    assert not bad, bad


def test_elementwise_share_not_bit_equal(results):
    """the cap per entry point, and per kernel instantiation of it (elementwise_ref.share_keys)"""
    neq, tot = {}, {}
    for case in E.CASES:
        if not R.share_keys(case):
            continue
        rec = results[case["id"]]
        for n, o in rec["ref"].items():
            if not o["exact"]:
                for key in R.share_keys(case):
                    neq[key] = neq.get(key, 0) + R.not_bit_equal(rec["got"][n], o["v"])
                    tot[key] = tot.get(key, 0) + o["v"].numel()
    share = {e: neq[e] / tot[e] for e in tot}
    print("share not bit-equal (bf16):", {str(e): f"{neq[e]}/{tot[e]} = {100 * s:.4f}%" for e, s in share.items()})
    assert share and all(s <= E.SHARE_CAP for s in share.values()), {e: s for e, s in share.items() if s > E.SHARE_CAP}


def test_slack_constants_cover_the_gpu_standin(results):
    """the second stand-in K_SLACK is measured from: the formulas and rounding points of the reference in torch fp32 operations
    on this device (its math library, not the kernels under test), against the fp64 reference, within K_SLACK / 4 per kind"""
    worst = {}
    for case in E.CASES:
        if case["entry"] not in R.BOUNDED_ENTRIES:
            continue
        ref = results[case["id"]]["ref"]
        for n, v in R.emulate(case, R.inputs(case), DEV).items():
            ex = float(R.excess(v, ref[n], R.out_dtype(case, n), E.GELU_TANH_ABS).max())
            worst[ref[n]["kind"]] = max(worst.get(ref[n]["kind"], 0.0), ex)
    print("worst torch-fp32-on-device stand-in error, x 2^-24 mag:", {k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == set(E.K_SLACK)
    assert all(worst[k] <= E.K_SLACK[k] / 4 for k in worst), worst


@pytest.mark.parametrize("group", sorted(E.ROUTE_GROUPS), ids=lambda g: g[0] + "-" + "-".join(f"{k}{v}" for k, v in g[1]))
def test_bf16_routes_agree_on_special_values(group, results):
    """the x8 stores (v_cvt_pk_bf16_f32) and the x4 / scalar ones (integer f2bf) give the same bits for the same inputs"""
    ids = E.ROUTE_GROUPS[group]
    kernels = {next(c for c in E.CASES if c["id"] == i)["kernel"] for i in ids}
    assert len(kernels) >= 2, ids
    outs = []
    for i in ids:
        got = results[i]["got"]
        F = min(next(c for c in E.CASES if c["id"] == j)["p"].get("F", 1 << 30) for j in ids)
        outs.append({n: (v[:, :F] if v.dim() == 2 else v) for n, v in got.items()})
    for o in outs[1:]:
        for n in outs[0]:
            a, b = outs[0][n].contiguous(), o[n].contiguous()
            same = (a.view(torch.int16) == b.view(torch.int16)) | (torch.isnan(a) & torch.isnan(b))
            assert same.all(), (n, ids, int((~same).sum()))
