"""dxa_qknorm_rope_split_at / dxa_qknorm_rope_merge_from: the fused per-head q/k RMSNorm + RoPE pass writing into / reading from
head-major tensors that several calls share (the two Qwen3 experts of DM0's mixture layer; a sampler's key / value buffer whose
prefix is cached), against the float64 formula and the bands of tests/test_qknorm_rope_gpu.py (imported, not restated).

Shapes: B = 2, S = 5 — at every (dtype, D, heads) here the item count is no multiple of the 256-thread workgroup, so tail lanes take
the "re-read item 0, store nothing" path beside a window that does not start at 0; D = 32 and 128 are the narrowest and the common
head; (7, 1) heads make the q / k / v boundaries odd.  Destinations are filled with a sentinel first: everything outside the window
must come back bit for bit.
"""
import math

import pytest
import torch

from .test_qknorm_rope_gpu import DEV, EPS, N_POS, _band, _dist, _formula, _randn, _tables, _with_grads

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K

B, S = 2, 5
SENTINEL = -77.0          # exact in bf16 and fp32
HEADS = [(4, 2), (7, 1)]
# (Sq_cap, q0, Skv_cap, kv0): the sampler's shape (queries alone, keys at 0 / in the middle / flush with the end), then the training
# shape (one capacity, one offset)
WINDOWS = [(5, 0, 13, 0), (5, 0, 13, 3), (5, 0, 13, 8), (13, 3, 13, 3)]


def _inputs(dtype, D, Hq, Hkv, S_, seed):
    M = B * S_
    qkv = _randn((M, (Hq + 2 * Hkv) * D), seed, dtype)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    wq = (0.5 + torch.rand(D, generator=g)).to(DEV).to(dtype)
    wk = (0.5 + torch.rand(D, generator=g)).to(DEV).to(dtype)
    pos = torch.randint(0, N_POS, (M,), generator=g).to(torch.int32).to(DEV)
    return qkv, wq, wk, pos


def _check_forward(got, ref, dtype, t16, tag):
    assert torch.equal(got["v"].double(), ref["v"]), f"{tag}: v is a copy"
    if got["rstd"] is not None:
        _band(got["rstd"], ref["rstd"], 1e-5, 1e-5, f"{tag}: rstd")
    for name in ("q", "k"):
        if dtype == torch.float32:
            _band(got[name], ref[name], 1e-5, 1e-5, f"{tag}: {name}")
        else:
            mine, torch_bf16 = _dist(got[name], ref[name]), _dist(t16[name], ref[name])
            assert mine <= 2.0 * torch_bf16, f"{tag}: {name}: kernel {mine:.3e} from the float64 formula, torch's bf16 {torch_bf16:.3e}"


@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_split_writes_its_window_and_nothing_else(dtype, D):
    cos_t, sin_t = _tables(N_POS, D)
    seed = 500
    for Hq, Hkv in HEADS:
        seed += 10
        qkv, wq, wk, pos = _inputs(dtype, D, Hq, Hkv, S, seed)
        geo = (B, S, Hq, Hkv, D)
        rows = pos.long()
        ref = dict(zip(("q", "k", "v", "rstd"),
                       _formula(qkv.double(), wq.double(), wk.double(), cos_t[rows].double(), sin_t[rows].double(), EPS, *geo, torch.float64)))
        t16 = None
        if dtype == torch.bfloat16:
            t16 = dict(zip(("q", "k", "v", "rstd"), _formula(qkv, wq, wk, cos_t[rows], sin_t[rows], EPS, *geo, torch.float32)))
        q1, k1, v1, rstd1 = K.qknorm_rope_split(qkv, wq, wk, EPS, cos_t, sin_t, pos, *geo)            # the offset-free entry point
        for Sq_cap, q0, Skv_cap, kv0 in WINDOWS:
            for want_rstd in (True, False):
                tag = f"{dtype} D {D} heads {Hq}/{Hkv} q {q0}/{Sq_cap} kv {kv0}/{Skv_cap} rstd {want_rstd}"
                q = torch.full((B, Hq, Sq_cap, D), SENTINEL, device=DEV, dtype=dtype)
                k = torch.full((B, Hkv, Skv_cap, D), SENTINEL, device=DEV, dtype=dtype)
                v = torch.full((B, Hkv, Skv_cap, D), SENTINEL, device=DEV, dtype=dtype)
                rstd = K.qknorm_rope_split_into(qkv, q, k, v, q0, kv0, wq, wk, EPS, cos_t, sin_t, pos, *geo, want_rstd=want_rstd)
                assert (rstd is None) == (not want_rstd)
                win = dict(q=q[:, :, q0:q0 + S], k=k[:, :, kv0:kv0 + S], v=v[:, :, kv0:kv0 + S], rstd=rstd)
                _check_forward(win, ref, dtype, t16, tag)
                for name, mine, plain in (("q", win["q"], q1), ("k", win["k"], k1), ("v", win["v"], v1)):
                    assert torch.equal(mine, plain), f"{tag}: {name} differs from the offset-free entry point"
                if want_rstd:
                    assert torch.equal(rstd, rstd1), tag
                for name, t, lo in (("q", q, q0), ("k", k, kv0), ("v", v, kv0)):
                    outside = torch.ones(t.shape[2], dtype=torch.bool, device=DEV)
                    outside[lo:lo + S] = False
                    assert bool((t[:, :, outside] == SENTINEL).all()), f"{tag}: {name} was written outside its window"


@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_merge_reads_each_segment_of_shared_gradients(dtype, D):
    """two segments (S = 5 at 0, S = 8 at 5) of one dq / dk / dv with norm weights of their own, as the two experts of a layer"""
    S_cap = 13
    segs = [(5, 0), (8, 5)]
    cos_t, sin_t = _tables(N_POS, D)
    seed = 900
    for Hq, Hkv in HEADS:
        seed += 10
        gq, gk, gv = (_randn((B, Hq, S_cap, D), seed + 2, dtype), _randn((B, Hkv, S_cap, D), seed + 3, dtype),
                      _randn((B, Hkv, S_cap, D), seed + 4, dtype))
        for i, (Sn, s0) in enumerate(segs):
            qkv, wq, wk, pos = _inputs(dtype, D, Hq, Hkv, Sn, seed + 100 * (i + 1))
            geo = (B, Sn, Hq, Hkv, D)
            M = B * Sn
            rows = pos.long()
            sl = [t[:, :, s0:s0 + Sn].contiguous() for t in (gq, gk, gv)]
            q = torch.empty((B, Hq, S_cap, D), device=DEV, dtype=dtype)
            k = torch.empty((B, Hkv, S_cap, D), device=DEV, dtype=dtype)
            v = torch.empty((B, Hkv, S_cap, D), device=DEV, dtype=dtype)
            rstd = K.qknorm_rope_split_into(qkv, q, k, v, s0, s0, wq, wk, EPS, cos_t, sin_t, pos, *geo)
            runs = []
            for _ in range(2):
                dqkv, part = K.qknorm_rope_merge_from(gq, gk, gv, s0, qkv, rstd, wq, wk, cos_t, sin_t, pos, *geo)
                runs.append((dqkv.clone(), part.clone(), K.colsum(part).clone()))
            assert all(torch.equal(a, b) for a, b in zip(*runs)), "the same inputs give the same bits"
            dqkv, _, dw = runs[0]
            got = dict(dqkv=dqkv, dwq=dw[:D], dwk=dw[D:])
            ref = _with_grads(qkv.double(), wq.double(), wk.double(), *(t.double() for t in sl),
                              cos_t[rows].double(), sin_t[rows].double(), EPS, *geo, torch.float64)
            tag = f"{dtype} D {D} heads {Hq}/{Hkv} segment {Sn} at {s0}"
            if dtype == torch.float32:
                for name, atol in (("dqkv", 2e-5), ("dwq", 1e-5 * math.sqrt(M * Hq)), ("dwk", 1e-5 * math.sqrt(M * Hkv))):
                    _band(got[name], ref[name], 1e-5, atol, f"{tag}: {name}")
            else:
                t16 = _with_grads(qkv, wq, wk, *sl, cos_t[rows], sin_t[rows], EPS, *geo, torch.float32)
                for name in ("dqkv", "dwq", "dwk"):
                    mine, torch_bf16 = _dist(got[name], ref[name]), _dist(t16[name], ref[name])
                    assert mine <= 2.0 * torch_bf16, (f"{tag}: {name}: kernel is {mine:.3e} from the float64 formula, torch's bf16 "
                                                     f"evaluation of it {torch_bf16:.3e} (allowed: twice that)")
            # the offset-free entry point on the slice gives the same bits
            dqkv0, part0 = K.qknorm_rope_merge(*sl, qkv, rstd, wq, wk, cos_t, sin_t, pos, *geo)
            assert torch.equal(dqkv0, dqkv) and torch.equal(part0, runs[0][1]), tag


def test_windows_outside_the_capacity_are_refused_before_any_launch():
    Hq, Hkv, D = 4, 2, 32
    qkv, wq, wk, pos = _inputs(torch.float32, D, Hq, Hkv, S, 1)
    cos_t, sin_t = _tables(N_POS, D)
    q = torch.full((B, Hq, 5, D), SENTINEL, device=DEV)
    k = torch.full((B, Hkv, 13, D), SENTINEL, device=DEV)
    v = torch.full((B, Hkv, 13, D), SENTINEL, device=DEV)
    geo = (B, S, Hq, Hkv, D)
    with pytest.raises(L.DxaError, match="outside"):
        K.qknorm_rope_split_into(qkv, q, k, v, 0, 9, wq, wk, EPS, cos_t, sin_t, pos, *geo)             # kv0 + S = 14 > 13
    with pytest.raises(L.DxaError, match="outside"):
        K.qknorm_rope_split_into(qkv, q, k, v, 0, -1, wq, wk, EPS, cos_t, sin_t, pos, *geo)
    with pytest.raises(L.DxaError, match="outside"):
        K.qknorm_rope_split_into(qkv, q, k, v, 1, 0, wq, wk, EPS, cos_t, sin_t, pos, *geo)             # q0 + S = 6 > 5
    rstd = torch.ones((B * S, Hq + Hkv), device=DEV)
    dq = torch.full((B, Hq, 13, D), SENTINEL, device=DEV)
    with pytest.raises(L.DxaError, match="outside"):
        K.qknorm_rope_merge_from(dq, k, v, 9, qkv, rstd, wq, wk, cos_t, sin_t, pos, *geo)
    with pytest.raises(L.DxaError, match="outside"):
        K.qknorm_rope_merge_from(dq, k, v, -2, qkv, rstd, wq, wk, cos_t, sin_t, pos, *geo)
    # a head_dim the kernel does not take
    D2 = 48
    qkv2 = _randn((B * S, (Hq + 2 * Hkv) * D2), 2)
    w2 = torch.ones(D2, device=DEV)
    c2, s2 = _tables(N_POS, D2)
    q2 = torch.full((B, Hq, 5, D2), SENTINEL, device=DEV)
    k2 = torch.full((B, Hkv, 13, D2), SENTINEL, device=DEV)
    v2 = torch.full((B, Hkv, 13, D2), SENTINEL, device=DEV)
    with pytest.raises(L.DxaError, match="head_dim"):
        K.qknorm_rope_split_into(qkv2, q2, k2, v2, 0, 3, w2, w2, EPS, c2, s2, pos, B, S, Hq, Hkv, D2)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (q, k, v, dq, q2, k2, v2)), "nothing was written"
