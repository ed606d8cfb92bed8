"""fp64 restatement (TEST INFRASTRUCTURE, not product code) of masked attention as include/dexbotic_amd.h :: dxa_attn_desc
defines it, the mask-edge cases the GPU sweep runs, and inputs that make an off-by-one mask visible.

The rule, written once: key j is visible to query i of batch row b when

    kv_start[b] <= j < min(kv_end[b], q_limit[b, i])   and   key_valid[b, j]   and   (not causal or j <= i + (Sk - Sq))

A query that sees no key gives o = 0 and lse = 0 (the library's convention).

Why the inputs are built and not drawn: with N(0,1) q and k the softmax is nearly flat over hundreds of keys, one key wrongly
added or dropped moves o by |v| / N, and that is below the bf16 tolerance.  edge_inputs() puts every row's softmax weight on
the keys next to the places where its mask flips, so that the last visible and the first hidden key both score `gain` above
the rest: including the one or dropping the other moves o by order 1.  tests/test_attn_ref.py holds that property as a
condition on the inputs (no GPU); tests/test_attention_masks_gpu.py runs the kernels on them."""
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

GAIN = 8.0
NOISE = 0.3
TARGETS = 8          # edge keys a row aims at (c10: kv_start, a key_valid hole and the upper bound are 7 keys; 6 dropped kv_start)


# ------------------------------------------------------------------------------------------------ the rule
def visibility(B, Sq, Sk, causal, kv_start=None, kv_end=None, q_limit=None, key_valid=None, diag=0):
    """bool [B, Sq, Sk].  kv_start / kv_end: [B] ints or None; q_limit: [B, Sq] or None; key_valid: [B, Sk] or None;
    diag shifts the causal diagonal (0 = the library's: the last query sees the last key)"""
    j = torch.arange(Sk).view(1, 1, Sk)
    i = torch.arange(Sq).view(1, Sq, 1)
    vis = torch.ones(B, Sq, Sk, dtype=torch.bool)
    if kv_start is not None:
        vis = vis & (j >= torch.as_tensor(kv_start).view(B, 1, 1))
    if kv_end is not None:
        vis = vis & (j < torch.as_tensor(kv_end).view(B, 1, 1))
    if q_limit is not None:
        vis = vis & (j < torch.as_tensor(q_limit).view(B, Sq, 1))
    if key_valid is not None:
        vis = vis & torch.as_tensor(key_valid).bool().view(B, 1, Sk)
    if causal:
        vis = vis & (j <= i + (Sk - Sq) + diag)
    return vis


def attention_ref(q, k, v, vis, scale):
    """q [B,Hq,Sq,D], k / v [B,Hkv,Sk,D], vis bool [B,Sq,Sk] -> (o [B,Hq,Sq,D], lse [B,Hq,Sq]) in fp64; differentiable"""
    G = q.shape[1] // k.shape[1]
    kk = k.double().repeat_interleave(G, 1)
    vv = v.double().repeat_interleave(G, 1)
    s = q.double() @ kk.transpose(-1, -2) * scale
    vis = vis.to(s.device)[:, None]
    live = vis.any(-1, keepdim=True)
    s = s.masked_fill(~vis, float("-inf")).masked_fill(~live, 0.0)       # a dead row: constants, no NaN and no gradient
    o = (torch.softmax(s, -1) @ vv) * live
    lse = torch.logsumexp(s, -1) * live[..., 0]
    return o, lse


def attention_ref_bf16(q, k, v, do, vis, scale):
    """The same attention with the roundings a correct bf16 flash kernel cannot avoid, everything else in fp64: the
    unnormalised weights exp(s - max) rounded to bf16 in front of P V; o, dq, dk, dv rounded to bf16; P and
    dS = P (dP - delta) scale, with delta = rowsum(dO o) of the ROUNDED o, rounded to bf16 in front of their products.
    -> dict o, dq, dk, dv (fp64).  A yardstick for a tolerance where the project's bound is tighter than bf16 itself on these
    inputs (see Case.emulated), never a reference: tests/test_attention_masks_gpu.py compares with attention_ref only."""
    bf = lambda t: t.to(torch.bfloat16).double()
    B, Hq, Sq, _ = q.shape
    G = Hq // k.shape[1]
    q, k, v, do = (t.double() for t in (q, k, v, do))
    kk, vv = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    vis = vis.to(q.device)[:, None]
    live = vis.any(-1, keepdim=True)
    s = (q @ kk.transpose(-1, -2) * scale).masked_fill(~vis, float("-inf")).masked_fill(~live, 0.0)
    e = torch.exp(s - s.amax(-1, keepdim=True)) * vis
    l = e.sum(-1, keepdim=True)
    p = e / l.clamp_min(1e-300)
    o = bf(bf(e) @ vv / l.clamp_min(1e-300))
    ds = bf(p * (do @ vv.transpose(-1, -2) - (do * o).sum(-1, keepdim=True)) * scale)
    fold = lambda t: t.reshape(B, Hq // G, G, *t.shape[2:]).sum(2)                # the query heads of a kv head
    return dict(o=o, dq=bf(ds @ kk), dk=bf(fold(ds.transpose(-1, -2) @ q)), dv=bf(fold(bf(p).transpose(-1, -2) @ do)))


# ------------------------------------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    name: str
    B: int
    Hq: int
    Hkv: int
    Sq: int
    Sk: int
    D: int
    causal: bool = False
    kv_start: Optional[Sequence[int]] = None
    kv_end: Optional[Sequence[int]] = None
    q_limit: Optional[Sequence[Sequence[int]]] = None      # per batch row: (first query, limit) runs, see _q_limit
    holes: Optional[Sequence[Sequence[int]]] = None        # per batch row: invalid keys
    layout: str = "head"          # "head": q, k, v head-major [B,H,S,D]; "packed_kv": k, v from one [B,Sk,2,H,D]; "fused_qkv": [B,S,3,H,D]
    fp32_generic: bool = False    # also run in fp32 with force_generic = 1
    # the route the case is there to reach (dxa_attn_plan): forward family, forward / dQ waves, dK/dV waves, dK/dV prefetch, key ranges
    fwd: str = "tr"
    nw: int = 4
    nw_dkv: int = 4
    pf: int = 1
    nsplit: int = 1
    tile: int = 0                 # staged tile width (0: head_dim)
    # outputs whose bf16 bound is 2 x the error of attention_ref_bf16 on this case instead of the project's (where that is
    # more): the project's bound sits below what bf16 rounding of dS alone gives these inputs — see the GPU test's docstring
    emulated: Sequence[str] = ()

    @property
    def scale(self):
        return self.D ** -0.5

    def masks(self):
        """dict of int32 / uint8 tensors (or None) in the shapes the descriptor takes"""
        t = lambda x: None if x is None else torch.tensor(list(x), dtype=torch.int32)
        ql = None
        if self.q_limit is not None:
            ql = torch.empty(self.B, self.Sq, dtype=torch.int32)
            for b, runs in enumerate(self.q_limit):
                for first, lim in runs:
                    ql[b, first:] = lim
        kvalid = None
        if self.holes is not None:
            kvalid = torch.ones(self.B, self.Sk, dtype=torch.uint8)
            for b, hs in enumerate(self.holes):
                kvalid[b, list(hs)] = 0
        return dict(kv_start=t(self.kv_start), kv_end=t(self.kv_end), q_limit=ql, key_valid=kvalid)

    def vis(self, diag=0, **override):
        m = self.masks()
        m.update(override)
        return visibility(self.B, self.Sq, self.Sk, self.causal, diag=diag, **m)


_R = lambda *a: tuple(range(*a))
_BLOCKS = ((0, 128), (128, 200), (200, 300))                 # q_limit blocks [128 | 200 | 300]
_BLOCKS_DEAD = ((0, 128), (5, 0), (6, 128), (128, 200), (200, 300))   # ... with one query (5) that sees nothing
_HOLES_300 = _R(60, 70) + (130,)                             # 60:70 crosses a 64-key tile edge and holds key 64

CASES = [
    Case("c01 causal kv_start+kv_end hd128", 2, 4, 2, 150, 150, 128, causal=True, kv_start=(0, 37), kv_end=(150, 141),
         fp32_generic=True, nw_dkv=8),
    Case("c02 q_limit+key_valid hd256", 2, 8, 1, 300, 300, 256, q_limit=(_BLOCKS, _BLOCKS_DEAD), holes=(_HOLES_300, _HOLES_300),
         nw_dkv=8, pf=0),
    Case("c03 q_limit+key_valid hd256 8 waves", 11, 8, 2, 300, 300, 256, q_limit=(_BLOCKS, _BLOCKS_DEAD) + (_BLOCKS,) * 9,
         holes=(_HOLES_300,) * 11, nw=8, nw_dkv=8, pf=0, emulated=("dk",)),
    Case("c04 cross Sq<Sk kv_end hd64 packed kv", 2, 4, 4, 40, 333, 64, kv_end=(333, 129), layout="packed_kv", fp32_generic=True),
    Case("c05 causal Sk>Sq key_valid hd128", 2, 4, 2, 70, 200, 128, causal=True, holes=(_R(60, 70) + (150,), (0, 1, 2, 131, 199)),
         fp32_generic=True, nw_dkv=8),
    Case("c06 causal Sq>Sk hd64", 1, 2, 2, 200, 70, 64, causal=True, fp32_generic=True),
    Case("c07 empty and one-tile key ranges hd128", 3, 4, 1, 96, 160, 128, kv_start=(0, 64, 100), kv_end=(160, 64, 128),
         fp32_generic=True, nw_dkv=8),
    Case("c08 kv_end+key_valid hd72 8 waves fused qkv", 8, 16, 16, 250, 250, 72, kv_end=(250, 249, 200, 129, 128, 64, 1, 250),
         holes=(_R(120, 130), (), (63, 64), (128,), (0,), (), (), (249,)), layout="fused_qkv", nw=8, tile=128, emulated=("dk",)),
    Case("c09 causal kv_start hd72", 2, 3, 3, 130, 130, 72, causal=True, kv_start=(0, 67), tile=128),
    Case("c10 split forward hd256", 2, 8, 1, 17, 833, 256, kv_start=(0, 70), kv_end=(833, 600),
         q_limit=(((0, 817), (1, 833)), ((0, 470), (8, 833))), holes=(_R(120, 136), (300,)),
         nw_dkv=8, pf=0, nsplit=14),
]


# ------------------------------------------------------------------------------------------------ the inputs
def _targets(vis):
    """float [B, Sq, Sk]: 1 at the (at most TARGETS) keys of each row that sit on a mask edge — both sides of every flip of the
    row, key 0 and key Sk-1 when visible — nearest the row's last visible key"""
    B, Sq, Sk = vis.shape
    flip = vis[..., 1:] != vis[..., :-1]
    cand = torch.zeros_like(vis)
    cand[..., 1:] |= flip
    cand[..., :-1] |= flip
    cand[..., 0] |= vis[..., 0]
    cand[..., -1] |= vis[..., -1]
    j = torch.arange(Sk).expand(B, Sq, Sk)
    upper = torch.where(vis, j, torch.full_like(j, -1)).amax(-1, keepdim=True)
    dist = torch.where(cand, (j - upper).abs(), torch.full_like(j, 1 << 30))
    near = dist.topk(min(TARGETS, Sk), dim=-1, largest=False).indices
    w = torch.zeros(B, Sq, Sk).scatter_(-1, near, 1.0)
    return w * cand


def edge_inputs(case, seed=0, gain=GAIN, noise=NOISE):
    """-> q [B,Hq,Sq,D], k, v [B,Hkv,Sk,D], do [B,Hq,Sq,D]: fp32 CPU tensors holding bf16-representable values"""
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c = case
    r = (gain / c.scale) ** 0.5
    u = rn(c.B, c.Hkv, c.Sk, c.D)
    u = u / u.norm(dim=-1, keepdim=True)
    w = _targets(c.vis()).double()                                         # [B, Sq, Sk]
    aim = (w[:, None] @ u).repeat_interleave(c.Hq // c.Hkv, 1)             # [B, Hq, Sq, D]: sum of the row's target directions
    q = noise * rn(c.B, c.Hq, c.Sq, c.D) + r * aim
    k = r * u
    v, do = rn(c.B, c.Hkv, c.Sk, c.D), rn(c.B, c.Hq, c.Sq, c.D)
    return tuple(t.to(torch.bfloat16).float() for t in (q, k, v, do))


def normal_inputs(case, seed=0):
    """the N(0,1) inputs of tests/test_kernels_gpu.py, for the record of why they do not see a mask edge"""
    g = torch.Generator().manual_seed(2000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = case
    return tuple(t.to(torch.bfloat16).float() for t in (rn(c.B, c.Hq, c.Sq, c.D), rn(c.B, c.Hkv, c.Sk, c.D), rn(c.B, c.Hkv, c.Sk, c.D),
                                                        rn(c.B, c.Hq, c.Sq, c.D)))


def perturbations(case):
    """yields (name, vis) with one bound of the case's mask moved by one key; only the bounds the case sets"""
    m = case.masks()
    for key in ("kv_end", "kv_start", "q_limit"):
        if m[key] is not None:
            for step in (-1, 1):
                yield f"{key}{step:+d}", case.vis(**{key: m[key] + step})
    if case.causal:
        for step in (-1, 1):
            yield f"diagonal{step:+d}", case.vis(diag=step)
    if m["key_valid"] is not None:
        yield "key_valid ignored", case.vis(key_valid=None)
        yield "key_valid shifted", case.vis(key_valid=torch.roll(m["key_valid"], 1, dims=1))


def sensitivity(case, inputs, vis_p, delta=0.08):
    """-> (affected rows, rows among them whose o moves by more than delta in some column): rows are (b, i) with a changed
    mask row, o is taken over all heads"""
    q, k, v, _ = inputs
    vis = case.vis()
    o0, _ = attention_ref(q, k, v, vis, case.scale)
    o1, _ = attention_ref(q, k, v, vis_p, case.scale)
    affected = (vis != vis_p).any(-1)                                      # [B, Sq]
    moved = ((o1 - o0).abs().amax(-1).amax(1) > delta) & affected
    return int(affected.sum()), int(moved.sum())


# ------------------------------------------------------------------------------------------------ the routes
def plan(L, d, backward):
    """dxa_attn_plan of descriptor d (L = dexbotic_amd._lib)"""
    import ctypes as C
    info = L.AttnPlanInfo()
    rc = L.lib.dxa_attn_plan(C.byref(d), int(backward), C.byref(info))
    assert rc == 0, L.last_error()
    return info


def check_route(L, case, d, fwd_family=None, backward=True):
    """the plan of descriptor d is the route the case names -> (forward plan, backward plan or None)"""
    import ctypes as C
    tile = case.tile or case.D
    f = plan(L, d, False)
    got = (f.family.decode(), f.D, f.DV, f.nw, f.nsplit)
    assert got == (fwd_family or case.fwd, tile, case.D, case.nw, case.nsplit), (case.name, "forward", got)
    assert f.workspace == L.lib.dxa_attn_fwd_workspace(C.byref(d)) and (f.workspace > 0) == (case.nsplit > 1)
    if not backward:
        return f, None
    b = plan(L, d, True)
    got = (b.family.decode(), b.D, b.DV, b.nw, b.nw_dkv, b.pf)
    assert got == ("flash", tile, case.D, case.nw, case.nw_dkv, case.pf), (case.name, "backward", got)
    assert b.workspace == L.lib.dxa_attn_bwd_workspace(C.byref(d)) == (case.B * case.Hq * case.Sq * 4 + 255) // 256 * 256
    return f, b


def check_route_fp32_generic(L, case, d):
    """fp32 with force_generic = 1: one wave per query row forward, GEMM-composed backward"""
    import ctypes as C
    f, b = plan(L, d, False), plan(L, d, True)
    assert (f.family.decode(), f.vec, f.nsplit, f.workspace) == ("generic", 4, 1, 0), case.name
    assert (b.family.decode(), b.nw_dkv) == ("composed", 0), case.name
    assert b.workspace == L.lib.dxa_attn_bwd_workspace(C.byref(d)) > 3 * case.B * case.Hq * case.Sq * case.Sk * 4
    return f, b


def route_text(f, b):
    """one line for the log: the kernels the two plans name"""
    fam = f.family.decode()
    fwd = {"tr": f"attn_fwd_tr_k<{f.D},{f.nw},{f.DV}>", "flash": f"attn_fwd_flash_k<{f.D},{f.nw},{f.DV}>",
           "generic": f"attn_fwd_generic_k<vec {f.vec}>"}.get(fam, fam)
    if f.nsplit > 1:
        fwd += f" x {f.nsplit} key ranges + attn_split_combine_k"
    bwd = b.family.decode()
    if bwd == "flash":
        bwd = f"attn_bwd_dq_k<{b.D},{b.nw},{b.DV}> + attn_bwd_dkv_k<{b.D},{b.DV},{b.nw_dkv},{'PF' if b.pf else 'noPF'}>"
    return f"forward {fwd} (workspace {f.workspace}) | backward {bwd} (workspace {b.workspace})"
