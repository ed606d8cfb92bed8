"""Every case of tests/norm_cases.py on the MI355X: the norm entry points of csrc/norm.hip (RMSNorm, LayerNorm, add-LayerNorm,
downsample LayerNorm, adarms, gated residual, dxa_colsum) called through the C ABI on the test's own buffers, against the fp64
reference of tests/norm_ref.py.

Inputs are carved out of NaN-filled buffers (a read past a row or past the tensor poisons a sum), outputs and the partial slab out
of sentinel-filled ones.  Per case: the guards in front of and behind every output are intact, the inputs are unchanged, every
output element is finite, dxa_norm_plan gives the real call the kernel the case names, and every output element holds
    |got - ref| <= U * ulp_T(ref) + k * 2^-24 * mag      (norm_cases.py: U, k = K_SLACK per output kind, mag from norm_ref.py).
The backward takes the mean / rstd the kernel's own forward returned; its weight gradients are the partial slab folded by
dxa_colsum.  Each backward case runs twice with another case in between: dx, the slab and the folded dw are bit-identical.
Over the bf16 cases of one entry point at most SHARE_CAP of the output elements differ from the reference rounded to bf16.
A column sum is also bit-identical in its three forms: fused, fused again after a fused call of another grid (the arrival
counters were left zeroed), and the two-launch form, which a call captured on a stream that never ran a column sum (and so has
no counters) takes — the captured graph must hold exactly its two kernels — replayed once from a single-stream graph.  The gate
of adarms / gated residual is the last third of a [B, 3 cols] buffer whose other thirds are NaN; the thirds of dmod / dgate_prev
that belong to other gradients must keep their sentinels."""
import ctypes as C

import pytest
import torch

from tests import norm_cases as NC
from tests import norm_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import graphs
    from dexbotic_amd import kernels as K

DEV = "cuda"
G = 256                       # guard elements on each side (512 / 1024 bytes: the carved operand stays 16-byte aligned)
SENT = {torch.float32: -7777.0, torch.bfloat16: -7776.0}


class Carved:
    """an operand of ``shape`` carved out of a larger buffer filled with ``fill``: G guard elements in front (+ ``mis`` elements), G
    behind"""

    def __init__(self, shape, dtype, fill, mis=0, value=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((2 * G + mis + n,), fill, dtype=dtype, device=DEV)
        self.lo, self.hi = G + mis, G + mis + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if value is not None:
            self.t.copy_(value.to(DEV))
        self.before = self.buf.clone()

    def guards_ok(self):
        b, a = self.buf.view(torch.int16 if self.buf.dtype == torch.bfloat16 else torch.int32), \
            self.before.view(torch.int16 if self.buf.dtype == torch.bfloat16 else torch.int32)
        return torch.equal(b[:self.lo], a[:self.lo]) and torch.equal(b[self.hi:], a[self.hi:])

    def unchanged(self):
        iv = torch.int16 if self.buf.dtype == torch.bfloat16 else torch.int32
        return torch.equal(self.buf.view(iv), self.before.view(iv))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _call(entry, o, case, stream):
    """the C entry point of ``entry`` on operands ``o`` (name -> tensor or None)"""
    lib, R_, C_ = L.lib, case["rows"], case["cols"]
    dt, wdt = NC.DT[case["dtype"]], NC.DT[case["w_dtype"]]
    g = lambda n: _p(o.get(n))
    if entry == "rmsnorm_fwd":
        return lib.dxa_rmsnorm_fwd(g("x"), g("w"), g("y"), g("rstd"), R_, C_, NC.EPS, dt, wdt, stream)
    if entry == "rmsnorm_bwd":
        return lib.dxa_rmsnorm_bwd(g("dy"), g("x"), g("w"), g("rstd"), g("dx"), g("residual"), g("partial"), R_, C_, dt, wdt, stream)
    if entry == "layernorm_fwd":
        return lib.dxa_layernorm_fwd(g("x"), g("w"), g("b"), g("y"), g("mean"), g("rstd"), R_, C_, NC.EPS, dt, wdt, stream)
    if entry == "layernorm_bwd":
        return lib.dxa_layernorm_bwd(g("dy"), g("x"), g("w"), g("mean"), g("rstd"), g("dx"), g("residual"), g("partial"), R_, C_, dt,
                                     wdt, stream)
    if entry == "add_layernorm_fwd":
        return lib.dxa_add_layernorm_fwd(g("x"), g("x2"), g("w"), g("b"), g("y"), g("mean"), g("rstd"), R_, C_, NC.EPS, dt, wdt, stream)
    if entry == "add_layernorm_bwd":
        return lib.dxa_add_layernorm_bwd(g("dy"), g("x"), g("x2"), g("w"), g("mean"), g("rstd"), g("dx"), g("partial"), R_, C_, dt, wdt,
                                         stream)
    G = case.get("G")
    if entry == "downsample_layernorm_fwd":
        return lib.dxa_downsample_layernorm_fwd(g("x"), g("w"), g("b"), g("y"), g("mean"), g("rstd"), R_, G, C_, NC.EPS, dt, wdt, stream)
    if entry == "downsample_layernorm_bwd":
        return lib.dxa_downsample_layernorm_bwd(g("dy"), g("x"), g("w"), g("mean"), g("rstd"), g("dx"), g("partial"), R_, G, C_, dt, wdt,
                                                stream)
    rps, ld = case.get("rps"), 3 * C_
    pb = o["partial"].numel() * 4 if o.get("partial") is not None else 0
    if entry == "adarms_fwd":
        return lib.dxa_adarms_fwd(g("x"), g("x2"), g("gate"), ld, g("mod"), g("aux"), g("y"), g("rstd"), R_, rps, C_, NC.EPS, dt, stream)
    if entry == "gated_residual_fwd":
        return lib.dxa_gated_residual_fwd(g("x"), g("x2"), g("gate"), ld, g("y"), R_, rps, C_, dt, stream)
    if entry == "adarms_bwd":
        return lib.dxa_adarms_bwd(g("dy"), g("x"), g("mod"), g("rstd"), g("residual"), g("dx"), g("dmod"), g("x2"), g("gate"), ld, g("aux"),
                                  g("dgate"), ld, g("partial"), pb, R_, rps, C_, dt, stream)
    if entry == "gated_residual_bwd":
        return lib.dxa_gated_residual_bwd(g("dy"), g("x2"), g("gate"), ld, g("dx"), g("dgate"), ld, g("partial"), pb, R_, rps, C_, dt,
                                          stream)
    raise AssertionError(entry)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _shapes(case):
    """operand name -> shape of the case's entry point"""
    e, R_, C_ = case["entry"], case["rows"], case["cols"]
    if e.startswith("downsample"):
        rows = NC.ds_rows(case)
        x = (R_, case["G"] ** 2, C_)
        return dict(x=x, dx=x, dy=(rows, 4 * C_), y=(rows, 4 * C_), w=(4 * C_,), b=(4 * C_,), mean=(rows,), rstd=(rows,))
    sh = {n: (R_, C_) for n in ("x", "x2", "dy", "residual", "y", "dx", "aux")}
    sh.update(w=(C_,), b=(C_,), mean=(R_,), rstd=(R_,))
    if e in NC.SAMPLE_ENTRIES:
        sh.update(mod=(case["B"], 3 * C_), gate=(case["B"], 3 * C_), dmod=(case["B"], 3 * C_), dgate=(case["B"], 3 * C_))
    return sh


def _stats(case, inp):
    """what the backward takes from the kernel's own forward (plain fresh tensors): mean / rstd, and adarms' r_out"""
    e = case["entry"]
    if e.startswith("gated_residual"):
        return {}
    fc = R.forward_case(case)
    sh = _shapes(case)
    T = NC.TORCH_DT[case["dtype"]]
    o = {n: inp[n].to(DEV) for n in ("x", "x2", "w", "b", "mod") if n in inp}
    if "modp" in inp:
        o["gate"] = inp["modp"].to(DEV)[:, 2 * case["cols"]:]
        o["aux"] = torch.empty(*sh["aux"], dtype=T, device=DEV)
    o["y"] = torch.empty(*sh["y"], dtype=T, device=DEV)
    o["rstd"] = torch.empty(*sh["rstd"], dtype=torch.float32, device=DEV)
    if not e.startswith(("rms", "adarms")):
        o["mean"] = torch.empty(*sh["mean"], dtype=torch.float32, device=DEV)
    L.check(_call(fc["entry"], o, case, _stream()), fc["entry"])
    return {k: o[k] for k in ("mean", "rstd", "aux") if k in o}


_INPUTS = ("x", "x2", "dy", "residual", "w", "b", "mod", "gate")


def _run_norm(case, inp, stats):
    """one guarded call of a norm case -> (outputs on the CPU, problems, the slab, the plan of the real call)"""
    e, C_ = case["entry"], case["cols"]
    T, TW = NC.TORCH_DT[case["dtype"]], NC.TORCH_DT[case["w_dtype"]]
    bwd = e.endswith("_bwd")
    sh = _shapes(case)
    ins, outs = {}, {}
    nan, sent = float("nan"), SENT
    for n in NC.present(case):
        mis = int(n == case["mis"])
        if n == "gate":                          # the gate third of another sample modulation, the rest of it NaN
            ins[n] = Carved(sh[n], T, nan, mis)
            ins[n].t[:, 2 * C_:] = inp["modp"][:, 2 * C_:].to(DEV)
            ins[n].before = ins[n].buf.clone()
        elif n == "x" and e == "adarms_bwd" and case["gated"]:
            ins[n] = Carved(sh[n], T, nan, mis, stats["aux"])          # r: what the forward wrote
        elif n in _INPUTS:
            ins[n] = Carved(sh[n], TW if n in ("w", "b") else T, nan, mis, inp[n])
        elif n in ("mean", "rstd") and bwd:
            ins[n] = Carved(sh[n], torch.float32, nan, mis, stats[n])
        elif n in ("mean", "rstd"):
            outs[n] = Carved(sh[n], torch.float32, sent[torch.float32], mis)
        elif n == "partial":
            outs[n] = Carved((NC.partial_rows(case), NC.partial_cols(case)), torch.float32, sent[torch.float32], mis)
        else:                                    # y, dx, aux, dmod, dgate
            outs[n] = Carved(sh[n], T, sent[T], mis)
    ops = {n: c.t for n, c in {**ins, **outs}.items()}
    for n in ("gate", "dgate"):                  # [B, 3 cols] buffers: the operand is their last third
        if n in ops:
            ops[n] = ops[n][:, 2 * C_:]
    for n in NC.OPERANDS[e]:
        ops.setdefault(n, None)
    plan = K.norm_plan(e, **NC.plan_fields(case, lambda n: ops[n].data_ptr()))
    L.check(_call(e, ops, case, _stream()), e)
    torch.cuda.synchronize()
    problems = [f"{n}: guard damaged" for n, c in outs.items() if not c.guards_ok()]
    problems += [f"{n}: input changed" for n, c in ins.items() if not c.unchanged()]
    # the thirds of dmod / dgate_prev that belong to other gradients are not touched
    iv = torch.int16 if T == torch.bfloat16 else torch.int32
    for n, keep in (("dmod", slice(2 * C_, 3 * C_)), ("dgate", slice(0, 2 * C_))):
        if n in outs and not torch.equal(outs[n].t[:, keep].contiguous().view(iv), torch.full_like(outs[n].t[:, keep], sent[T]).view(iv)):
            problems.append(f"{n}: a third that is not this call's written")
    got = {}
    for n, c in outs.items():
        v = c.t
        if n == "dmod":
            got["dscale"], got["dshift"] = v[:, :C_].cpu(), v[:, C_:2 * C_].cpu()
        elif n == "dgate":
            got["dgate"] = v[:, 2 * C_:].cpu()
        else:
            got[n] = v.cpu()
    problems += [f"{n}: {int((~torch.isfinite(v.float())).sum())} non-finite" for n, v in got.items() if not torch.isfinite(v.float()).all()]
    slab = got.pop("partial", None)
    if slab is not None and e not in NC.SAMPLE_ENTRIES and ops.get("w") is not None:
        part = outs["partial"].t
        W = part.shape[1] // (1 if e.startswith("rms") else 2)
        got["dw"] = K.colsum(part[:, :W]).cpu()
        if not e.startswith("rms"):
            got["db"] = K.colsum(part[:, W:]).cpu()
    return got, problems, slab, plan


def _check_values(case, got, ref):
    bad = []
    for n, (v, kind, U, mag) in ref.items():
        ex = R.excess(got[n], v, U, mag)
        k = NC.K_SLACK[kind]
        if not (ex <= k).all():
            i = int(torch.argmax(torch.where(torch.isnan(ex), torch.full_like(ex, float("inf")), ex)))
            bad.append(f"{n}: {int((ex > k).sum())}/{ex.numel()} over the bound, worst {float(ex.flatten()[i]):.3g} x 2^-24 mag (k {k}) "
                       f"at flat {i}: got {float(got[n].flatten()[i]):.8g} want {float(v.flatten()[i]):.8g}")
    return bad


_OTHER = next(c for c in NC.NORM_CASES if c["entry"] == "layernorm_bwd" and c["rows"] == 4100)


@pytest.fixture(scope="module")
def norm_results():
    """every norm case run once (the backward ones twice, another case in between): id -> record"""
    out = {}
    for case in NC.NORM_CASES:
        inp = NC.inputs(case)
        stats = _stats(case, inp) if case["entry"].endswith("_bwd") else None
        got, problems, slab, plan = _run_norm(case, inp, stats)
        rec = dict(got=got, problems=problems, plan=plan, stats=stats)
        if stats is not None:
            oi = NC.inputs(_OTHER)
            _run_norm(_OTHER, oi, _stats(_OTHER, oi))
            got2, problems2, slab2, _ = _run_norm(case, inp, stats)
            rec["problems"] += problems2
            same = all(torch.equal(got[n], got2[n]) for n in got) and (slab is None or torch.equal(slab, slab2))
            if not same:
                rec["problems"].append("second run not bit-identical: " + ", ".join(n for n in got if not torch.equal(got[n], got2[n])))
        stats_cpu = {k: v.cpu() for k, v in stats.items()} if stats else None
        rec["ref"] = R.reference(case, inp, stats_cpu)
        out[case["id"]] = rec
    return out


@pytest.mark.parametrize("case", NC.NORM_CASES, ids=lambda c: c["id"])
def test_norm_route(case, norm_results):
    rec = norm_results[case["id"]]
    assert rec["plan"]["kernel"] == case["kernel"], rec["plan"]
    if case["trips"] is not None:
        assert rec["plan"]["trips"] == case["trips"]
    assert not rec["problems"], rec["problems"]
    bad = _check_values(case, rec["got"], rec["ref"])
    assert not bad, bad


def test_norm_share_not_bit_equal(norm_results):
    neq, tot = {}, {}
    for case in NC.NORM_CASES:
        rec = norm_results[case["id"]]
        for n, (v, kind, U, mag) in rec["ref"].items():
            if U:
                neq[case["entry"]] = neq.get(case["entry"], 0) + R.not_bit_equal(rec["got"][n], v)
                tot[case["entry"]] = tot.get(case["entry"], 0) + v.numel()
    share = {e: neq[e] / tot[e] for e in tot}
    print("share not bit-equal per entry point:", {e: f"{100 * s:.3f}%" for e, s in share.items()})
    assert len(share) == 12 and all(s <= NC.SHARE_CAP for s in share.values()), share


# ---------------------------------------------------------------------------------------------------------------- dxa_colsum
@pytest.fixture(scope="module")
def capture_stream():
    """a stream of this module's own that never runs an eager column sum, so dxa_colsum has no arrival counters for it; destroyed
    at the end of the module"""
    hip = C.CDLL("libamdhip64.so")
    h = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(h), C.c_uint(1)) == 0      # hipStreamNonBlocking
    yield torch.cuda.ExternalStream(h.value)
    torch.cuda.synchronize()
    assert hip.hipStreamDestroy(h) == 0


def _kernel_nodes(graph):
    """(number of nodes, number of kernel nodes) of a captured graph (hipGraph_t)"""
    hip = C.CDLL("libamdhip64.so")
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(C.c_void_p(graph), None, C.byref(n)) == 0
    nodes = (C.c_void_p * max(1, n.value))()
    assert hip.hipGraphGetNodes(C.c_void_p(graph), nodes, C.byref(n)) == 0
    kinds = []
    for i in range(n.value):
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
        kinds.append(t.value)
    return n.value, sum(k == 0 for k in kinds)              # hipGraphNodeTypeKernel = 0


def _colsum(case, x, out, scratch, stream):
    ld = NC.ld_of(case)[0]
    return L.lib.dxa_colsum(_p(x), ld, _p(out), case["rows"], case["cols"], NC.DT[case["dtype"]], int(case["accumulate"]), _p(scratch),
                            scratch.numel() * 4, stream)


@pytest.mark.parametrize("case", NC.COLSUM_CASES, ids=lambda c: c["id"])
def test_colsum_route(case, capture_stream):
    rows, cols = case["rows"], case["cols"]
    T = NC.TORCH_DT[case["dtype"]]
    ld, off = NC.ld_of(case)
    inp = NC.inputs(case)
    xb = Carved((rows, ld), T, float("nan"))
    xv = xb.t[:, off:off + cols]
    xv.copy_(inp["x"].to(DEV))
    xb.before = xb.buf.clone()
    y0 = inp.get("y0", torch.zeros(cols))
    outc = Carved((cols,), torch.float32, SENT[torch.float32], value=y0)
    nsplit = NC.colsum_nsplit(rows)
    scr = Carved((nsplit * cols,), torch.float32, SENT[torch.float32])
    plan = K.norm_plan("colsum", dtype=NC.DT[case["dtype"]], rows=rows, cols=cols, ld=ld, accumulate=int(case["accumulate"]), x=xv,
                       y=outc.t, partial=scr.t, partial_bytes=scr.t.numel() * 4, have_counters=1)
    assert plan["kernel"] == case["kernel"], plan
    L.check(_colsum(case, xv, outc.t, scr.t, _stream()), "dxa_colsum")
    torch.cuda.synchronize()
    assert outc.guards_ok() and scr.guards_ok() and xb.unchanged()
    got = outc.t.cpu()
    assert torch.isfinite(got).all()
    ref = R.reference(case, inp)
    bad = _check_values(case, {"out": got}, ref)
    assert not bad, bad
    if rows <= 32:
        return
    # fused again, after a fused call of another grid.x: the counters the first call used were left zeroed
    other = torch.randn(100, 3 * 256 + 1, device=DEV)
    K.colsum(other)
    outc.t.copy_(y0.to(DEV))
    L.check(_colsum(case, xv, outc.t, scr.t, _stream()), "dxa_colsum")
    torch.cuda.synchronize()
    assert torch.equal(outc.t.cpu(), got), "fused call after another grid differs"
    # the two-launch form: captured on a stream without counters (the graph holds the two kernels), replayed once
    s = capture_stream
    assert K.norm_plan("colsum", dtype=NC.DT[case["dtype"]], rows=rows, cols=cols, ld=ld, x=xv, y=outc.t, partial=scr.t,
                       partial_bytes=scr.t.numel() * 4, have_counters=0, capturing=1)["kernel"] == case["capture_kernel"]
    outc.t.copy_(y0.to(DEV))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.stream(s):
        with graphs.capture(g, s):
            rc = _colsum(case, xv, outc.t, scr.t, s.cuda_stream)
    assert rc == 0, L.last_error()
    assert _kernel_nodes(g.raw_cuda_graph()) == (2, 2), "the captured call did not take the two-launch form"
    g.instantiate()
    outc.t.copy_(y0.to(DEV))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert outc.guards_ok() and scr.guards_ok() and xb.unchanged()
    assert torch.equal(outc.t.cpu(), got), "two-launch form differs from the fused one"
