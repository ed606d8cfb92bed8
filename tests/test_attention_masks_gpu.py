"""dxa_attn_fwd / dxa_attn_bwd at the mask edges, at Sq != Sk and on the 8-wave kernels: every case of tests/attn_ref.py, on
inputs whose softmax weight sits on the keys next to each mask bound (a bound off by one key moves o by order 1, see
tests/test_attn_ref.py), against the fp64 reference and its autograd at the bounds tests/test_kernels_gpu.py uses.

Every output is a view with padded rows inside a larger buffer filled with NaN: what the kernels must write is written (no NaN
left), what they must not touch — the pad columns behind every row (the 72-of-128 columns, ragged last tiles), the guard rows
in front of and behind the tensor — still holds its NaN.  dxa_attn_plan on the descriptor that ran says which kernels ran."""
import ctypes as C
import math

import pytest
import torch

from . import attn_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K

DEV = "cuda"
GUARD = 256          # elements in front of and behind every output tensor
PAD = 8              # columns behind every output row

# (rtol, atol) of tests/test_kernels_gpu.py :: test_attention_fwd_bwd
TOL = {torch.bfloat16: dict(o=(1 / 64, 2e-2), lse=(1e-2, 3e-2), dq=(1 / 32, 6e-2), dk=(1 / 32, 1.2e-1), dv=(1 / 32, 1.2e-1)),
       torch.float32: dict(o=(2e-5, 2e-5), lse=(1e-4, 1e-4), dq=(1e-4, 1e-4), dk=(1e-4, 2e-4), dv=(1e-4, 2e-4))}


def worst(out, ref, tol):
    """largest error in units of the bound atol + rtol |ref|"""
    rtol, atol = tol
    return ((out.double() - ref.double()).abs() / (atol + rtol * ref.double().abs())).max().item()


def assert_close(out, ref, tol, what, widen=1.0):
    rtol, atol = tol
    out64, ref64 = out.double(), ref.double()
    err = (out64 - ref64).abs()
    bad = ~(err <= widen * (atol + rtol * ref64.abs()))        # (a NaN is bad)
    print(f"{what}: max err {err.max().item():.3e}, worst err / bound {worst(out, ref, tol):.3f} (allowed {widen:.3f})")
    if bad.any():
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {err.max().item():.3e} "
                             f"(ref max {ref64.abs().max().item():.3e}); first at {i}: got {out64[tuple(i)].item():.6e} "
                             f"want {ref64[tuple(i)].item():.6e}")


class Guarded:
    """a NaN-filled buffer, the tensor of `shape` in its middle, and the record of which elements the kernels own"""

    def __init__(self, shape, dtype):
        n = math.prod(shape)
        self.flat = torch.full((GUARD + n + GUARD,), float("nan"), device=DEV, dtype=dtype)
        self.owned_flat = torch.zeros(GUARD + n + GUARD, device=DEV, dtype=torch.bool)
        self.store = self.flat[GUARD:GUARD + n].view(shape)
        self.owned = self.owned_flat[GUARD:GUARD + n].view(shape)

    def claim(self, view):
        """view: function of the stored tensor -> the [B,H,S,D] view handed to the library"""
        view(self.owned).fill_(True)
        return view(self.store)

    def reset(self):
        self.flat.fill_(float("nan"))

    def check(self, what):
        assert not torch.isnan(self.flat[self.owned_flat]).any(), f"{what}: NaN left in the output"
        assert torch.isnan(self.flat[~self.owned_flat]).all(), f"{what}: written outside the tensor (pad columns or guard rows)"

    def values(self):
        return self.flat[self.owned_flat].clone()


_REF = {}


def reference(case):
    """(inputs on the GPU as fp32, fp64 o, lse, dq, dk, dv, vis): computed once per case, shared by the dtypes, never written"""
    if case.name not in _REF:
        q, k, v, do = (t.to(DEV) for t in R.edge_inputs(case))
        vis = case.vis().to(DEV)
        qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
        o, lse = R.attention_ref(qr, kr, vr, vis, case.scale)
        o.backward(do.double())
        _REF[case.name] = ((q, k, v, do), o.detach(), lse.detach(), qr.grad, kr.grad, vr.grad, vis)
    return _REF[case.name]


class Problem:
    """the case's tensors in the case's memory layout and the descriptor over them"""

    def __init__(self, case, dtype, force_generic):
        c = self.case = case
        (q, k, v, do), *_ = reference(case)
        hm = lambda t: t.permute(0, 2, 1, 3)                                    # [B,S,H,D] storage -> [B,H,S,D] view
        cols = lambda t: t[..., :c.D]
        self.bufs = {}

        def out(name, shape, view):
            if name not in self.bufs:
                self.bufs[name] = Guarded(shape, dtype)
            return self.bufs[name].claim(view)

        if c.layout == "fused_qkv":                                             # [B,S,3,H,D]: q, k, v of one projection
            assert c.Hq == c.Hkv and c.Sq == c.Sk
            qkv = torch.stack([hm(q), hm(k), hm(v)], 2).to(dtype).contiguous()
            self.q, self.k, self.v = (hm(qkv[:, :, i]) for i in range(3))
            self.do = hm(hm(do).to(dtype).contiguous())
            shape = (c.B, c.Sq, 3, c.Hq, c.D + PAD)
            self.dq, self.dk, self.dv = (out("dqkv", shape, lambda t, i=i: cols(hm(t[:, :, i]))) for i in range(3))
        else:
            self.q, self.do = q.to(dtype).contiguous(), do.to(dtype).contiguous()
            self.dq = out("dq", (c.B, c.Hq, c.Sq, c.D + PAD), cols)
            if c.layout == "packed_kv":                                         # [B,Sk,2,H,D]: k, v of one projection (cross-attention)
                kv = torch.stack([hm(k), hm(v)], 2).to(dtype).contiguous()
                self.k, self.v = hm(kv[:, :, 0]), hm(kv[:, :, 1])
                shape = (c.B, c.Sk, 2, c.Hkv, c.D + PAD)
                self.dk, self.dv = (out("dkv", shape, lambda t, i=i: cols(hm(t[:, :, i]))) for i in range(2))
            else:
                self.k, self.v = k.to(dtype).contiguous(), v.to(dtype).contiguous()
                self.dk = out("dk", (c.B, c.Hkv, c.Sk, c.D + PAD), cols)
                self.dv = out("dv", (c.B, c.Hkv, c.Sk, c.D + PAD), cols)
        self.o = out("o", (c.B, c.Sq, c.Hq, c.D + PAD), lambda t: cols(hm(t)))   # token-major: the o_proj input
        self.lse = Guarded((c.B, c.Hq, c.Sq), torch.float32)
        self.bufs["lse"] = self.lse
        self.lse.claim(lambda t: t)
        self.masks = {key: (None if m is None else m.to(DEV)) for key, m in case.masks().items()}
        self.force_generic = force_generic

    def desc(self, v=None):
        c = self.case
        d = K._attn_desc(self.q, self.k, self.v if v is None else v, self.o, self.lse.store, c.causal, c.scale, self.masks["kv_start"],
                         self.masks["kv_end"], self.masks["q_limit"], self.masks["key_valid"])
        d.force_generic = int(self.force_generic)
        d.d_o, (d.do_sb, d.do_sh, d.do_ss) = K._ptr(self.do), K._bhsd_strides(self.do)
        d.dq, (d.dq_sb, d.dq_sh, d.dq_ss) = K._ptr(self.dq), K._bhsd_strides(self.dq)
        d.dk, (d.dk_sb, d.dk_sh, d.dk_ss) = K._ptr(self.dk), K._bhsd_strides(self.dk)
        d.dv, (d.dv_sb, d.dv_sh, d.dv_ss) = K._ptr(self.dv), K._bhsd_strides(self.dv)
        return d

    def forward(self, d):
        nbytes = int(L.lib.dxa_attn_fwd_workspace(C.byref(d)))
        ws = torch.empty(max(nbytes, 1), device=DEV, dtype=torch.uint8)
        L.check(L.lib.dxa_attn_fwd_ws(C.byref(d), K._ptr(ws), nbytes, K._stream()), "dxa_attn_fwd_ws")

    def backward(self, d):
        nbytes = int(L.lib.dxa_attn_bwd_workspace(C.byref(d)))
        ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
        L.check(L.lib.dxa_attn_bwd(C.byref(d), K._ptr(ws), nbytes, K._stream()), "dxa_attn_bwd")

    def run(self):
        for g in self.bufs.values():
            g.reset()
        d = self.desc()
        self.forward(d)
        self.backward(d)
        torch.cuda.synchronize()
        return {name: g.values() for name, g in self.bufs.items()}


def check_case(case, dtype, force_generic):
    inputs, ref_o, ref_lse, ref_dq, ref_dk, ref_dv, vis = reference(case)
    pb = Problem(case, dtype, force_generic)
    # ---- which kernels this runs: the plan of the descriptor that runs
    d = pb.desc()
    if force_generic:
        f, b = R.check_route_fp32_generic(L, case, d)
    else:
        f, b = R.check_route(L, case, d)
    print(f"route: {case.name} [{'bf16' if dtype == torch.bfloat16 else 'fp32 force_generic'}]: {R.route_text(f, b)}")
    first = pb.run()
    # ---- nothing unwritten, nothing written outside
    for name, g in pb.bufs.items():
        g.check(f"{case.name}: {name}")
    # ---- the numbers
    tol = TOL[dtype]
    refs = dict(o=ref_o, lse=ref_lse, dq=ref_dq, dk=ref_dk, dv=ref_dv)
    widen = {}
    if dtype == torch.bfloat16 and case.emulated:
        emu = R.attention_ref_bf16(*inputs, vis, case.scale)
        for name in case.emulated:                                              # 2 x what bf16 itself costs on these inputs
            widen[name] = max(1.0, 2 * worst(emu[name], refs[name], tol[name]))
    failures = []
    for name, got in (("o", pb.o), ("lse", pb.lse.store), ("dq", pb.dq), ("dk", pb.dk), ("dv", pb.dv)):
        try:
            assert_close(got, refs[name], tol[name], name, widen.get(name, 1.0))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    # ---- queries that see nothing, keys that nobody sees: exact zeros
    dead = ~vis.any(-1)                                                         # [B, Sq]
    unseen = ~vis.any(1)                                                        # [B, Sk]
    rows = dead[:, None].expand(-1, case.Hq, -1)
    keys = unseen[:, None].expand(-1, case.Hkv, -1)
    assert torch.all(pb.o[rows] == 0) and torch.all(pb.lse.store[rows] == 0) and torch.all(pb.dq[rows] == 0), "dead query rows"
    assert torch.all(pb.dk[keys] == 0) and torch.all(pb.dv[keys] == 0), "keys no query sees"
    # ---- the same bits again
    second = pb.run()
    for name in first:
        assert torch.equal(first[name], second[name]), f"{name} differs between two calls"
    return pb, first


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_attention_mask_edges_bf16(case):
    """forward and fused backward on the route the case names; then the forward again with a V that is 8-byte but not 16-byte
    aligned (attn_fwd_flash_k, V transposed through registers), which adds every element in the same order: the same bits.

    dk of c03 and c08 (Case.emulated): the project's bound 1/32 |ref| + 1.2e-1 is below bf16 itself there.  A key on a mask edge
    is a target of hundreds of queries, its dk sums that many dS q terms of order 1 that cancel (|dk| up to 138), and dS goes
    into that product as bf16.  tests/attn_ref.py :: attention_ref_bf16 — fp64 with P, dS and the outputs rounded to bf16, no
    kernel involved — is 1.58 x the bound off the fp64 reference at c03 (max error 0.411) and 1.71 x at c08 (0.274); the kernels
    measured 1.60 x (0.427) and 1.31 x (0.287) on the MI355X.  These two get 2 x the emulation's error, computed in the test:
    3.17 x and 3.42 x the bound.  Every other output of every case, c03's and c08's o, dq and dv included, holds the project's
    bounds (worst: dk of c02 at 0.71, emulation 0.88)."""
    pb, first = check_case(case, torch.bfloat16, 0)
    buf = torch.empty(pb.v.numel() + 4, device=DEV, dtype=torch.bfloat16)
    v8 = buf[4:].view(pb.v.shape)
    v8.copy_(pb.v)
    assert v8.data_ptr() % 16 == 8
    d8 = pb.desc(v=v8)
    R.check_route(L, case, d8, fwd_family="flash", backward=False)
    pb.bufs["o"].reset()
    pb.lse.reset()
    pb.forward(d8)
    torch.cuda.synchronize()
    assert torch.equal(pb.bufs["o"].values(), first["o"]) and torch.equal(pb.lse.values(), first["lse"])
    pb.bufs["o"].check("o, 8-byte aligned V")


@pytest.mark.parametrize("case", [c for c in R.CASES if c.fp32_generic], ids=[c.name for c in R.CASES if c.fp32_generic])
def test_attention_mask_edges_fp32_generic(case):
    """the one-wave-per-row forward and the GEMM-composed backward under the same masks, GQA and Sq != Sk, at the fp32 bounds"""
    check_case(case, torch.float32, 1)
