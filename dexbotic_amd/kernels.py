"""Tensor-level wrappers over the C ABI (no autograd here — see functional.py).

Every function takes torch tensors living on the MI355X, passes raw device pointers + sizes + the
current HIP stream to libdexbotic_amd.so and returns torch tensors allocated by torch's caching
allocator (PyTorch = device memory and streams only).  Nothing here computes with torch ops.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import lib

F32, BF16 = L.F32, L.BF16


def dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise L.DxaError(f"unsupported dtype {t.dtype} (fp32 / bf16 only)")


def torch_dtype(code: int) -> torch.dtype:
    return torch.bfloat16 if code == BF16 else torch.float32


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """raw handle of the calling thread's current stream on the current device (what every launch below is enqueued on).  The two
    torch._C calls cost ~0.3 us against ~1.5 us for torch.cuda.current_stream().cuda_stream (a Stream object per call) — on a step of
    2,000 - 7,700 launches that is host time the launch-bound stretches wait for"""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise L.DxaError("dexbotic_amd kernels need device tensors (no CPU fallback exists)")
    return t.data_ptr()


def _row_major(t: torch.Tensor, name: str) -> int:
    """leading dimension of a 2-D tensor whose last dim is contiguous"""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise L.DxaError(f"{name}: expected a 2-D tensor with contiguous rows, got shape {tuple(t.shape)} "
                         f"strides {t.stride()}")
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))


# ------------------------------------------------------------------------------------------------ GEMM
# How fp32 x fp32 NT products of >= 128 rows are computed: "exact" = fp32 MFMA (v_mfma_f32_16x16x4_f32, 157 TF/s peak);
# "bf16x3" = three-term split-bf16 product on the bf16 ring kernel (16 mantissa bits per operand, ~1e-5 relative; the
# reference's trainer runs the same fp32 head matmuls as TF32, base_exp.py:254).  Set by NativeTrainer.step /
# inference_action from the model config; parity tests in fp32 mode leave it at "exact".
F32_GEMM_MODE = "exact"


@contextlib.contextmanager
def f32_gemm_mode(mode: str):
    global F32_GEMM_MODE
    if mode not in ("exact", "bf16x3"):
        raise L.DxaError(f"unknown fp32 GEMM mode {mode!r}")
    prev, F32_GEMM_MODE = F32_GEMM_MODE, mode
    try:
        yield
    finally:
        F32_GEMM_MODE = prev


def split3(x: torch.Tensor, rows: int, cols: int, ld: int, side: int) -> torch.Tensor:
    """fp32 [rows, cols] -> bf16 [rows, 3*cols] = [hi | hi | lo] (side 0) or [hi | lo | hi] (side 1), x = hi + lo"""
    out = torch.empty((rows, 3 * cols), device=x.device, dtype=torch.bfloat16)
    L.check(lib.dxa_split3(_ptr(x), ld, _ptr(out), rows, cols, side, _stream()), "dxa_split3")
    return out


def split3_t(x: torch.Tensor, pad_to: int, side: int) -> torch.Tensor:
    """fp32 [R, C] -> bf16 [C, 3 * Rp] = split3 of x^T (Rp = R rounded up to ``pad_to``, zero filled) in ONE launch"""
    R, C_ = x.shape
    Rp = (R + pad_to - 1) // pad_to * pad_to
    out = torch.empty((C_, 3 * Rp), device=x.device, dtype=torch.bfloat16)
    L.check(lib.dxa_split3_t(_ptr(x), _row_major(x, "x"), _ptr(out), R, C_, Rp, side, _stream()), "dxa_split3_t")
    return out


def split3_pair(a: torch.Tensor, a_t: bool, b: torch.Tensor, b_t: bool, pad_to: int = 1, a_dims=None, b_dims=None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """both operands of one bf16x3 product in ONE launch (dxa_split3_pair): ``a`` as the A operand (hi | hi | lo), ``b`` as the B operand
    (hi | lo | hi); ``*_t``: the split of the TRANSPOSE ([R, C] -> [C, 3 Rp], Rp = R rounded up to ``pad_to``) as split3_t writes it;
    ``*_dims`` = (rows, cols, ld) of an operand that is not simply a row-major 2-D tensor (gemm()'s explicit extents)"""
    ops, outs = [], []
    for x, t, side, dims in ((a, a_t, 0, a_dims), (b, b_t, 1, b_dims)):
        R, C_, ld = dims if dims is not None else (x.shape[0], x.shape[1], _row_major(x, "x"))
        o = L.Split3Op()
        o.src, o.ld, o.rows, o.cols, o.side, o.transposed = _ptr(x), ld, R, C_, side, int(t)
        if t:
            Rp = (R + pad_to - 1) // pad_to * pad_to
            out = torch.empty((C_, 3 * Rp), device=x.device, dtype=torch.bfloat16)
            o.pad = Rp
        else:
            out = torch.empty((R, 3 * C_), device=x.device, dtype=torch.bfloat16)
            o.pad = 0
        o.dst = _ptr(out)
        ops.append(o)
        outs.append(out)
    L.check(lib.dxa_split3_pair(C.byref(ops[0]), C.byref(ops[1]), _stream()), "dxa_split3_pair")
    return outs[0], outs[1]


def _x3_t_ok(M: int, N: int, Kc: int, out: torch.Tensor) -> bool:
    """the split-bf16 NT product is admissible for these extents (same rule as _x3_eligible; Kc = contraction length)"""
    return (F32_GEMM_MODE == "bf16x3" and out.dtype == torch.float32 and M >= 128 and N >= 128 and Kc >= 64 and Kc % 32 == 0
            and 6 * max(M, N) * Kc < (1 << 31))


def mm_tn_f32(a: torch.Tensor, b: torch.Tensor, *, out: torch.Tensor, **kw) -> torch.Tensor:
    """out[M,N] = a[K,M]^T @ b[K,N] for fp32 operands as an NT product of the transposes (the fp32 heads' dW).  bf16x3 mode: the
    transposed split operands come out of ONE launch each (dxa_split3_t); exact mode: fp32 transposes + the fp32 MFMA kernel."""
    Kc, M = a.shape
    N = b.shape[1]
    if a.dtype == torch.float32 and b.dtype == torch.float32 and _x3_t_ok(M, N, (Kc + 31) // 32 * 32, out):
        a3, b3 = split3_pair(a, True, b, True, pad_to=32)
        Kp = a3.shape[1] // 3
        kw = _ld_kwargs(kw, out)
        return gemm(L.NT, a3, b3, M, N, 3 * Kp, 3 * Kp, 3 * Kp, out, _row_major(out, "out"), epi_f32=True, **kw)
    return mm_nt(transpose(a, 4), transpose(b, 4), out=out, **kw)


def mm_nn_f32(a: torch.Tensor, b: torch.Tensor, **kw) -> torch.Tensor:
    """a[M,K] @ b[K,N] for fp32 operands as an NT product against b^T (the fp32 heads' dX = dY W)"""
    M, Kc = a.shape
    N = b.shape[1]
    out = kw.get("out")
    if (a.dtype == torch.float32 and b.dtype == torch.float32 and Kc % 32 == 0 and a.is_contiguous() and a.data_ptr() % 16 == 0
            and Kc % 4 == 0 and (out is None or out.dtype == torch.float32)):
        if out is None:
            out = kw["out"] = torch.empty((M, N), device=a.device, dtype=torch.float32)
        if _x3_t_ok(M, N, Kc, out):
            a3, b3 = split3_pair(a, False, b, True)
            kw2 = _ld_kwargs({k: v for k, v in kw.items() if k != "out"}, out)
            return gemm(L.NT, a3, b3, M, N, 3 * Kc, 3 * Kc, 3 * Kc, out, _row_major(out, "out"), epi_f32=True, **kw2)
    return mm_nt(a, transpose(b, 1), **kw)


def _x3_eligible(layout, a, b, out, M, N, K, lda, ldb, nb) -> bool:
    return (F32_GEMM_MODE == "bf16x3" and layout == L.NT and a.dtype == torch.float32 and b.dtype == torch.float32
            and out.dtype == torch.float32 and tuple(nb) == (1, 1, 1) and M >= 128 and N >= 128 and K >= 64 and K % 32 == 0
            and lda % 4 == 0 and ldb % 4 == 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
            and 6 * max(M, N) * K < (1 << 31))


_NB1 = (1, 1, 1)


def gemm(layout: int, a: torch.Tensor, b: torch.Tensor, M: int, N: int, K: int, lda: int, ldb: int,
         out: torch.Tensor, ldc: int, *, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, ldr: int = 0, act: int = L.ACT_NONE,
         aux_out: Optional[torch.Tensor] = None, mulgrad: Optional[torch.Tensor] = None, ldg: int = 0,
         alpha: float = 1.0, accumulate: bool = False, nb: Sequence[int] = _NB1,
         sA: Sequence[int] = (0, 0, 0), sB: Sequence[int] = (0, 0, 0), sC: Sequence[int] = (0, 0, 0),
         sR: Sequence[int] = (0, 0, 0), sG: Sequence[int] = (0, 0, 0), epi_f32: bool = False,
         mirror: Optional[torch.Tensor] = None, sumsq: Optional[torch.Tensor] = None,
         a2: Optional[torch.Tensor] = None, b2: Optional[torch.Tensor] = None) -> torch.Tensor:
    if not epi_f32 and a2 is None and _x3_eligible(layout, a, b, out, M, N, K, lda, ldb, nb):
        a3, b3 = split3_pair(a, False, b, False, a_dims=(M, K, lda), b_dims=(N, K, ldb))
        return gemm(L.NT, a3, b3, M, N, 3 * K, 3 * K, 3 * K, out, ldc, bias=bias, residual=residual, ldr=ldr, act=act,
                    aux_out=aux_out, mulgrad=mulgrad, ldg=ldg, alpha=alpha, accumulate=accumulate, epi_f32=True,
                    mirror=mirror, sumsq=sumsq)
    d = L.GemmDesc()
    d.layout, d.in_dtype, d.out_dtype, d.act = layout, dt(a), dt(out), act
    d.epi_f32 = int(epi_f32)
    if dt(b) != d.in_dtype:
        raise L.DxaError("gemm: A and B dtypes differ")
    for t, n in ((bias, "bias"), (residual, "residual"), (mulgrad, "mulgrad")):
        if t is not None and dt(t) != (F32 if epi_f32 else d.in_dtype):
            raise L.DxaError(f"gemm: {n} dtype must equal the input dtype")
    if aux_out is not None and dt(aux_out) != d.out_dtype:
        raise L.DxaError("gemm: aux_out dtype must equal the output dtype")
    d.M, d.N, d.K = M, N, K
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc = _ptr(a), lda, _ptr(b), ldb, _ptr(out), ldc
    d.bias, d.residual, d.ldr = _ptr(bias), _ptr(residual), ldr
    d.aux_out, d.mulgrad, d.ldg = _ptr(aux_out), _ptr(mulgrad), ldg
    d.alpha, d.accumulate = alpha, int(accumulate)
    if mirror is not None:
        if mirror.dtype != torch.bfloat16 or out.dtype != torch.float32 or tuple(nb) != (1, 1, 1) or \
                _row_major(mirror, "mirror") != ldc:
            raise L.DxaError("gemm: mirror must be a bf16 [M, N] view with the output's leading dimension (fp32 output)")
        d.mirror = _ptr(mirror)
    if sumsq is not None:
        if sumsq.dtype != torch.float32 or tuple(nb) != (1, 1, 1) or not sumsq.is_contiguous() \
                or sumsq.numel() != gemm_sumsq_slots(M, N):
            raise L.DxaError("gemm: sumsq must be gemm_sumsq_slots(M, N) contiguous floats (unbatched output)")
        d.sumsq = _ptr(sumsq)
    if nb is _NB1 or tuple(nb) == (1, 1, 1):         # (a fresh descriptor is zeroed: the strides of an unbatched product stay 0)
        d.nb[0] = d.nb[1] = d.nb[2] = 1
    else:
        for i in range(3):
            d.nb[i], d.sA[i], d.sB[i], d.sC[i], d.sR[i], d.sG[i] = nb[i], sA[i], sB[i], sC[i], sR[i], sG[i]
    K_all = K
    if a2 is not None:                         # TN: a second pair of operands contracted into the same product
        if layout != L.TN or b2 is None or a2.shape[1] != M or b2.shape[1] != N or a2.shape[0] != b2.shape[0] \
                or dt(a2) != d.in_dtype or dt(b2) != d.in_dtype or _row_major(a2, "a2") != lda or _row_major(b2, "b2") != ldb:
            raise L.DxaError("gemm: a2 / b2 are a second [K2, M] / [K2, N] pair of a TN product (same dtypes and leading dimensions)")
        d.A2, d.B2, d.K2 = _ptr(a2), _ptr(b2), a2.shape[0]
        K_all = K + a2.shape[0]
    prof = GEMM_PROFILE
    if prof is not None and prof.wants(layout, d.in_dtype, d.out_dtype):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.dxa_gemm(C.byref(d), _stream()), "dxa_gemm")
        e1.record()
        batches = nb[0] * nb[1] * nb[2]
        esz = {L.BF16: 2, L.F32: 4}
        prof.add((layout, d.in_dtype, d.out_dtype), e0, e1, 2.0 * M * N * K_all * batches,
                 float((M * K_all + N * K_all) * esz.get(d.in_dtype, 2) + M * N * esz.get(d.out_dtype, 2)) * batches)
        return out
    L.check(lib.dxa_gemm(C.byref(d), _stream()), "dxa_gemm")
    return out


class GemmProfile:
    """HIP-event timing of launches of the chosen gemm instantiations — keys (layout, in dtype, out dtype) — on the
    stream they are launched on: bench.py's live roofline measurement.  Per timed launch it also records the algorithmic
    flops (2 M N K) and the algorithmic bytes (A and B read once, C written once).  ``stride`` = s: every s-th launch of a key
    is timed (a deterministic sample spread over the whole region; s coprime with the 4 products a transformer layer launches
    per layout, so every product is sampled equally often) — a pair of event records costs the stream ~4 us, and 1240 pairs per
    step were 2 % of the step they were there to measure.  ``seen`` counts every launch of a key, timed or not."""

    def __init__(self, *keys, stride: int = 1):
        if len(keys) == 3 and all(isinstance(k, int) for k in keys):
            keys = (tuple(keys),)
        self.keys = set(tuple(k) for k in keys)
        self.events = []
        self.stride = max(1, int(stride))
        self.seen = {k: 0 for k in self.keys}

    def wants(self, layout, in_dtype, out_dtype) -> bool:
        key = (layout, in_dtype, out_dtype)
        if key not in self.keys:
            return False
        n = self.seen[key]
        self.seen[key] = n + 1
        return n % self.stride == 0

    def add(self, key, e0, e1, flops: float, nbytes: float = 0.0) -> None:
        self.events.append((key, e0, e1, flops, nbytes))

    def summary(self, key=None):
        """(timed launches, their total_ms, total_flops, total_algorithmic_bytes), of one key or of all — call after a device sync"""
        ev = [e for e in self.events if key is None or e[0] == tuple(key)]
        ms = sum(a.elapsed_time(b) for _, a, b, _, _ in ev)
        return len(ev), ms, sum(e[3] for e in ev), sum(e[4] for e in ev)

    def launches(self, key=None) -> int:
        """every launch of the key(s) inside the profiled region, timed or not"""
        return self.seen[tuple(key)] if key is not None else sum(self.seen.values())


GEMM_PROFILE: Optional[GemmProfile] = None


def _out2d(M: int, N: int, like: torch.Tensor, out: Optional[torch.Tensor], out_dtype: Optional[torch.dtype]):
    if out is None:
        out = torch.empty((M, N), device=like.device, dtype=out_dtype or like.dtype)
    return out


def mm_nt(a: torch.Tensor, b: torch.Tensor, *, out=None, out_dtype=None, **kw) -> torch.Tensor:
    """out[M,N] = a[M,K] @ b[N,K]^T  (+ fused epilogue options of gemm())"""
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K, (a.shape, b.shape)
    out = _out2d(M, N, a, out, out_dtype)
    kw = _ld_kwargs(kw, out)
    return gemm(L.NT, a, b, M, N, K, _row_major(a, "a"), _row_major(b, "b"), out, _row_major(out, "out"), **kw)


def mm_nn(a: torch.Tensor, b: torch.Tensor, *, out=None, out_dtype=None, **kw) -> torch.Tensor:
    """out[M,N] = a[M,K] @ b[K,N]"""
    M, K = a.shape
    N = b.shape[1]
    assert b.shape[0] == K, (a.shape, b.shape)
    out = _out2d(M, N, a, out, out_dtype)
    kw = _ld_kwargs(kw, out)
    return gemm(L.NN, a, b, M, N, K, _row_major(a, "a"), _row_major(b, "b"), out, _row_major(out, "out"), **kw)


def mm_tn(a: torch.Tensor, b: torch.Tensor, *, out=None, out_dtype=None, **kw) -> torch.Tensor:
    """out[M,N] = a[K,M]^T @ b[K,N]"""
    K, M = a.shape
    N = b.shape[1]
    assert b.shape[0] == K, (a.shape, b.shape)
    out = _out2d(M, N, a, out, out_dtype)
    kw = _ld_kwargs(kw, out)
    return gemm(L.TN, a, b, M, N, K, _row_major(a, "a"), _row_major(b, "b"), out, _row_major(out, "out"), **kw)


def swiglu_gemm_supported(x: torch.Tensor, w: torch.Tensor, keep_pre: bool = False) -> bool:
    """should / can mm_nt_swiglu take this gated-MLP product (dxa_gemm_desc.fuse = DXA_FUSE_SWIGLU)?  bf16, >= 129 rows, K % 64 == 0,
    F % 8 == 0, F >= 128.  Default: the serving paths (no pre-activations kept: one output stream); the training forward, which also
    stores the [M, 2F] pre-activations from the epilogue (three 8-byte store streams and 87 M SiLUs that nothing overlaps), measured
    235.5 against 236.1 ms per step with it — inside the noise, and the product's own rate drops — so it stays on the two-launch
    form (profiles/r06_swiglu_fuse_ab.txt)."""
    if keep_pre:
        return False
    M, K_ = x.shape
    F_ = w.shape[0] // 2
    return (x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.is_cuda and
            M >= 129 and K_ % 64 == 0 and K_ >= 64 and F_ % 8 == 0 and F_ >= 128 and w.shape[0] % 2 == 0 and
            x.is_contiguous() and w.is_contiguous() and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and
            M * 2 * F_ * 2 < (1 << 31) and w.numel() * 2 < (1 << 31))


def mm_nt_swiglu(x: torch.Tensor, w: torch.Tensor, keep_pre: bool = True):
    """gated MLP input half in ONE launch: x [M, K] @ [gate ; up]^T ([2F, K], gate rows first) -> (silu(gate) * up [M, F],
    pre-activations [M, 2F] or None).  Bit-identical to ``swiglu_fwd(mm_nt(x, w))`` (same tiles, same K order, same rounding points);
    HF Qwen2MLP (qwen2/modeling_qwen2.py:35-48 under cogact_arch.py:97-106)."""
    M, K_ = x.shape
    N = w.shape[0]
    F_ = N // 2
    out = torch.empty((M, F_), device=x.device, dtype=x.dtype)
    pre = torch.empty((M, N), device=x.device, dtype=x.dtype) if keep_pre else None
    d = L.GemmDesc()
    d.layout, d.in_dtype, d.out_dtype, d.act = L.NT, L.BF16, L.BF16, L.ACT_NONE
    d.M, d.N, d.K = M, N, K_
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc = _ptr(x), K_, _ptr(w), K_, _ptr(out), F_
    d.aux_out, d.ld_aux = _ptr(pre), N
    d.alpha, d.fuse = 1.0, L.FUSE_SWIGLU
    for i in range(3):
        d.nb[i] = 1
    prof = GEMM_PROFILE
    if prof is not None and prof.wants(L.NT, L.BF16, L.BF16):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.dxa_gemm(C.byref(d), _stream()), "dxa_gemm (swiglu)")
        e1.record()
        prof.add((L.NT, L.BF16, L.BF16), e0, e1, 2.0 * M * N * K_, float((M * K_ + N * K_) * 2 + M * (N + F_) * 2))
        return out, pre
    L.check(lib.dxa_gemm(C.byref(d), _stream()), "dxa_gemm (swiglu)")
    return out, pre


def _ld_kwargs(kw: dict, out: torch.Tensor) -> dict:
    kw = dict(kw)
    if kw.get("residual") is not None:
        kw["ldr"] = _row_major(kw["residual"], "residual")
    if kw.get("mulgrad") is not None:
        kw["ldg"] = _row_major(kw["mulgrad"], "mulgrad")
    if kw.get("aux_out") is not None and _row_major(kw["aux_out"], "aux_out") != _row_major(out, "out"):
        raise L.DxaError("gemm: aux_out must share the output leading dimension")
    return kw


# ------------------------------------------------------------------------------------- MemVLA memory path
_MASK_STATE = {"seed": None, "offset": 0}


def dropout_mask(shape, p: float, dtype: torch.dtype, device, seed: Optional[int] = None) -> torch.Tensor:
    """a dropout mask (0 | 1/(1-p)) drawn on the device in ONE launch; successive masks advance a process-wide counter, the
    key comes from torch's seed (torch.manual_seed makes runs repeatable)"""
    n = 1
    for v in shape:
        n *= int(v)
    out = torch.empty(tuple(int(v) for v in shape), device=device, dtype=dtype)
    if _MASK_STATE["seed"] is None or seed is not None:
        _MASK_STATE["seed"] = int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
    _MASK_STATE["offset"] += 1
    L.check(lib.dxa_dropout_mask(_ptr(out), n, float(p), _MASK_STATE["seed"], _MASK_STATE["offset"], dt(out), _stream()),
            "dxa_dropout_mask")
    return out


def bank_consolidate(feat: torch.Tensor, ts: torch.Tensor, length: int, sims: torch.Tensor, fifo: bool = False) -> None:
    """token-merge of the most similar neighbouring pair (fifo: drop of the oldest entry) among the first ``length`` entries of
    feat [cap, N, D] / ts [cap] (in place; afterwards the first length - 1 entries are the bank)"""
    assert feat.is_contiguous() and ts.is_contiguous() and ts.dtype == torch.float32 and sims.dtype == torch.float32
    assert feat.dim() == 3 and length <= feat.shape[0] and sims.numel() >= length - 1
    L.check(lib.dxa_bank_consolidate(_ptr(feat), _ptr(ts), int(length), feat.shape[1], feat.shape[2], dt(feat), int(fifo),
                                     _ptr(sims), _stream()), "dxa_bank_consolidate")


def _bank_dims(feat: torch.Tensor, ts: torch.Tensor, counts: torch.Tensor):
    B, cap, N, D = feat.shape
    assert feat.is_contiguous() and ts.is_contiguous() and ts.dtype == torch.float32 and ts.shape == (B, cap)
    assert counts.is_contiguous() and counts.dtype == torch.int32 and counts.shape == (B,) and counts.device == feat.device
    return B, cap, N, D


def bank_stage_fwd(feat: torch.Tensor, ts: torch.Tensor, counts: torch.Tensor, tokens: torch.Tensor, timesteps: torch.Tensor):
    """what one 'parallel_stream' step retrieves from, for all B slots in ONE launch: feat [B, cap, N, D], ts [B, cap], counts [B]
    int32, tokens [B, N, D], timesteps [B] fp32 -> fresh (mem [B, cap, N, D], ts_eff [B, cap], kv_len [B] int32); a slot without
    history holds its own tokens as entry 0, everything behind kv_len is zero"""
    B, cap, N, D = _bank_dims(feat, ts, counts)
    assert tokens.is_contiguous() and tokens.shape == (B, N, D) and tokens.dtype == feat.dtype
    assert timesteps.is_contiguous() and timesteps.dtype == torch.float32 and timesteps.shape == (B,)
    mem = torch.empty_like(feat)
    ts_eff = torch.empty_like(ts)
    kv_len = torch.empty(B, device=feat.device, dtype=torch.int32)
    L.check(lib.dxa_bank_stage_fwd(_ptr(feat), _ptr(ts), _ptr(counts), _ptr(tokens), _ptr(timesteps), _ptr(mem), _ptr(ts_eff),
                                   _ptr(kv_len), B, cap, N, D, dt(feat), _stream()), "dxa_bank_stage_fwd")
    return mem, ts_eff, kv_len


def bank_stage_bwd(dmem: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """dtokens [B, N, D] = dmem[:, 0] for the slots without history, 0 for the others"""
    B, cap, N, D = dmem.shape
    assert dmem.is_contiguous() and counts.is_contiguous() and counts.dtype == torch.int32 and counts.shape == (B,)
    out = torch.empty((B, N, D), device=dmem.device, dtype=dmem.dtype)
    L.check(lib.dxa_bank_stage_bwd(_ptr(dmem), _ptr(counts), _ptr(out), B, cap, N, D, dt(dmem), _stream()), "dxa_bank_stage_bwd")
    return out


def bank_append(feat: torch.Tensor, ts: torch.Tensor, counts: torch.Tensor, src: torch.Tensor, timesteps: torch.Tensor) -> None:
    """feat[b, counts[b]] = src[b], ts[b, counts[b]] = timesteps[b] for all B slots in ONE launch (in place)"""
    B, cap, N, D = _bank_dims(feat, ts, counts)
    assert src.is_contiguous() and src.shape == (B, N, D) and src.dtype == feat.dtype
    assert timesteps.is_contiguous() and timesteps.dtype == torch.float32 and timesteps.shape == (B,)
    L.check(lib.dxa_bank_append(_ptr(feat), _ptr(ts), _ptr(counts), _ptr(src), _ptr(timesteps), B, cap, N, D, dt(feat), _stream()),
            "dxa_bank_append")


def bank_consolidate_batched(feat: torch.Tensor, ts: torch.Tensor, counts: torch.Tensor, count_add: int, mem_length: int,
                             sims: Optional[torch.Tensor], fifo: bool = False) -> None:
    """bank_consolidate on every slot whose length counts[b] + count_add exceeds mem_length, the others untouched (in place; two
    launches for all B slots; per slot bit-identical to bank_consolidate).  sims: B * (cap - 1) floats of scratch."""
    B, cap, N, D = _bank_dims(feat, ts, counts)
    assert fifo or (sims is not None and sims.dtype == torch.float32 and sims.is_contiguous() and sims.numel() >= B * (cap - 1))
    L.check(lib.dxa_bank_consolidate_batched(_ptr(feat), _ptr(ts), _ptr(counts), int(count_add), int(mem_length), int(fifo),
                                             _ptr(sims), B, cap, N, D, dt(feat), _stream()), "dxa_bank_consolidate_batched")


def _bank_at_dims(feat: torch.Tensor, ts: torch.Tensor, slot_ids: torch.Tensor, counts: torch.Tensor):
    """the _at calls: banks of S slots, R <= S rows.  ``slot_ids`` / ``counts`` [R] int32 on the device; the ids are DISTINCT —
    the caller that owns the host list checks (a duplicate there is a ValueError), nothing is read back here"""
    S, cap, N, D = feat.shape
    R = slot_ids.shape[0]
    assert feat.is_contiguous() and ts.is_contiguous() and ts.dtype == torch.float32 and ts.shape == (S, cap)
    for t in (slot_ids, counts):
        assert t.is_contiguous() and t.dtype == torch.int32 and t.shape == (R,) and t.device == feat.device
    assert 0 < R <= S, (R, S)
    return R, S, cap, N, D


def distinct_slots(slots, S: int):
    """host-side check of a slot list before it is uploaded for the _at calls: ints in [0, S), no duplicates (ValueError)"""
    ids = [int(s) for s in slots]
    if len(set(ids)) != len(ids):
        raise ValueError(f"duplicate slot ids in one call: {ids}")
    if any(s < 0 or s >= S for s in ids):
        raise ValueError(f"slot ids {ids} outside [0, {S})")
    return ids


def bank_stage_fwd_at(feat: torch.Tensor, ts: torch.Tensor, slot_ids: torch.Tensor, counts: torch.Tensor, tokens: torch.Tensor,
                      timesteps: torch.Tensor):
    """bank_stage_fwd on rows ``slot_ids`` of feat [S, cap, N, D] / ts [S, cap]: counts [R], tokens [R, N, D], timesteps [R] ->
    fresh (mem [R, cap, N, D], ts_eff [R, cap], kv_len [R]); row r reads slot slot_ids[r]"""
    R, S, cap, N, D = _bank_at_dims(feat, ts, slot_ids, counts)
    assert tokens.is_contiguous() and tokens.shape == (R, N, D) and tokens.dtype == feat.dtype
    assert timesteps.is_contiguous() and timesteps.dtype == torch.float32 and timesteps.shape == (R,)
    mem = torch.empty((R, cap, N, D), device=feat.device, dtype=feat.dtype)
    ts_eff = torch.empty((R, cap), device=feat.device, dtype=torch.float32)
    kv_len = torch.empty(R, device=feat.device, dtype=torch.int32)
    L.check(lib.dxa_bank_stage_fwd_at(_ptr(feat), _ptr(ts), _ptr(slot_ids), _ptr(counts), _ptr(tokens), _ptr(timesteps), _ptr(mem),
                                      _ptr(ts_eff), _ptr(kv_len), R, S, cap, N, D, dt(feat), _stream()), "dxa_bank_stage_fwd_at")
    return mem, ts_eff, kv_len


def bank_append_at(feat: torch.Tensor, ts: torch.Tensor, slot_ids: torch.Tensor, counts: torch.Tensor, src: torch.Tensor,
                   timesteps: torch.Tensor) -> None:
    """feat[slot_ids[r], counts[r]] = src[r], ts[slot_ids[r], counts[r]] = timesteps[r] in ONE launch; other slots untouched"""
    R, S, cap, N, D = _bank_at_dims(feat, ts, slot_ids, counts)
    assert src.is_contiguous() and src.shape == (R, N, D) and src.dtype == feat.dtype
    assert timesteps.is_contiguous() and timesteps.dtype == torch.float32 and timesteps.shape == (R,)
    L.check(lib.dxa_bank_append_at(_ptr(feat), _ptr(ts), _ptr(slot_ids), _ptr(counts), _ptr(src), _ptr(timesteps), R, S, cap, N, D,
                                   dt(feat), _stream()), "dxa_bank_append_at")


def bank_consolidate_batched_at(feat: torch.Tensor, ts: torch.Tensor, slot_ids: torch.Tensor, counts: torch.Tensor, count_add: int,
                                mem_length: int, sims: Optional[torch.Tensor], fifo: bool = False) -> None:
    """bank_consolidate_batched on rows ``slot_ids``: slot slot_ids[r] is consolidated when counts[r] + count_add exceeds
    mem_length.  sims: R * (cap - 1) floats of scratch, indexed by the row (two rows never share it)."""
    R, S, cap, N, D = _bank_at_dims(feat, ts, slot_ids, counts)
    assert fifo or (sims is not None and sims.dtype == torch.float32 and sims.is_contiguous() and sims.numel() >= R * (cap - 1))
    L.check(lib.dxa_bank_consolidate_batched_at(_ptr(feat), _ptr(ts), _ptr(slot_ids), _ptr(counts), int(count_add), int(mem_length),
                                                int(fifo), _ptr(sims), R, S, cap, N, D, dt(feat), _stream()),
            "dxa_bank_consolidate_batched_at")


def add_rows(x: Optional[torch.Tensor], g: torch.Tensor, Nn: int, alpha: float = 1.0) -> torch.Tensor:
    """x [R, Nn, C] + alpha * g [R, C] broadcast over the tokens (x None: the broadcast alone)"""
    R, C_ = g.shape
    assert g.is_contiguous() and (x is None or (x.is_contiguous() and x.shape == (R, Nn, C_) and x.dtype == g.dtype))
    out = torch.empty((R, Nn, C_), device=g.device, dtype=g.dtype)
    L.check(lib.dxa_add_rows(_ptr(x), _ptr(g), _ptr(out), R, Nn, C_, float(alpha), dt(g), _stream()), "dxa_add_rows")
    return out


def token_sum(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """scale * sum over the token axis: [R, Nn, C] -> [R, C] (same dtype, fp32 accumulation)"""
    R, Nn, C_ = x.shape
    assert x.is_contiguous()
    out = torch.empty((R, C_), device=x.device, dtype=x.dtype)
    L.check(lib.dxa_token_sum(_ptr(x), _ptr(out), R, Nn, C_, float(scale), dt(x), _stream()), "dxa_token_sum")
    return out


# ----------------------------------------------------------------------------------------------- norms
def rmsnorm_fwd(x: torch.Tensor, w: Optional[torch.Tensor], eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    x2 = x.reshape(-1, x.shape[-1])
    assert x2.is_contiguous()
    y = torch.empty_like(x2)
    rstd = torch.empty(x2.shape[0], device=x.device, dtype=torch.float32)
    L.check(lib.dxa_rmsnorm_fwd(_ptr(x2), _ptr(w), _ptr(y), _ptr(rstd), x2.shape[0], x2.shape[1], eps, dt(x2),
                                dt(w) if w is not None else dt(x2), _stream()), "dxa_rmsnorm_fwd")
    return y.view(x.shape), rstd


def norm_bwd_blocks(rows: int) -> int:
    return int(lib.dxa_norm_bwd_blocks(rows))


def norm_plan(entry: str, **fields) -> dict:
    """the launch dxa_norm_plan gives a call of dxa_<entry> (L.NORM_ENTRIES); ``fields`` are dxa_norm_desc's by name, a pointer
    role as a tensor, an address (int) or None.  Host arithmetic only: answers without a GPU."""
    d = L.NormDesc()
    d.entry = L.NORM_ENTRIES.index(entry)
    for k, v in fields.items():
        setattr(d, k, _ptr(v) if isinstance(v, torch.Tensor) else v)
    info = L.NormPlanInfo()
    L.check(lib.dxa_norm_plan(C.byref(d), C.byref(info)), "dxa_norm_plan")
    s = lambda p: p.decode() if p is not None else None
    return {"kernel": s(info.kernel), "kernel2": s(info.kernel2), "mode": s(info.mode), "vec": info.vec, "grid": tuple(info.grid),
            "block": info.block, "lds": info.lds, "nsplit": info.nsplit, "trips": info.trips}


def norm_kernel_names() -> list:
    """every instantiation the norm launchers can launch (dxa_norm_kernel_name)"""
    names = []
    while lib.dxa_norm_kernel_name(len(names)) is not None:
        names.append(lib.dxa_norm_kernel_name(len(names)).decode())
    return names


def _residual2d(residual, x2):
    if residual is None:
        return None
    r2 = residual.reshape(-1, x2.shape[-1])
    assert r2.is_contiguous() and r2.shape == x2.shape and r2.dtype == x2.dtype
    return r2


def rmsnorm_bwd(dy, x, w, rstd, dw_out: Optional[torch.Tensor] = None, accumulate: bool = False,
                want_dw: bool = True, residual: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """returns (dx, dw_fp32 or None); dw is (accumulated) into dw_out when given.  `residual` (the gradient that bypassed
    the normalised sub-block) is added to dx inside the kernel."""
    x2 = x.reshape(-1, x.shape[-1])
    dy2 = dy.reshape(-1, x.shape[-1])
    assert x2.is_contiguous() and dy2.is_contiguous()
    rows, cols = x2.shape
    dx = torch.empty_like(x2)
    part = None
    if w is not None and want_dw:
        part = torch.empty((norm_bwd_blocks(rows), cols), device=x.device, dtype=torch.float32)
    # w is still needed for dx even when its gradient is not (frozen norm): pass a throw-away slab
    if w is not None and part is None:
        part = torch.empty((norm_bwd_blocks(rows), cols), device=x.device, dtype=torch.float32)
        want_dw = False
    L.check(lib.dxa_rmsnorm_bwd(_ptr(dy2), _ptr(x2), _ptr(w), _ptr(rstd), _ptr(dx), _ptr(_residual2d(residual, x2)), _ptr(part),
                                rows, cols, dt(x2),
                                dt(w) if w is not None else dt(x2), _stream()), "dxa_rmsnorm_bwd")
    dw = colsum(part, out=dw_out, accumulate=accumulate) if (part is not None and want_dw) else None
    return dx.view(x.shape), dw


def layernorm_fwd(x, w, b, eps):
    x2 = x.reshape(-1, x.shape[-1])
    assert x2.is_contiguous()
    y = torch.empty_like(x2)
    mean = torch.empty(x2.shape[0], device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    L.check(lib.dxa_layernorm_fwd(_ptr(x2), _ptr(w), _ptr(b), _ptr(y), _ptr(mean), _ptr(rstd), x2.shape[0],
                                  x2.shape[1], eps, dt(x2), dt(w) if w is not None else dt(x2), _stream()),
            "dxa_layernorm_fwd")
    return y.view(x.shape), mean, rstd


def layernorm_bwd(dy, x, w, mean, rstd, dw_out=None, db_out=None, accumulate: bool = False, want_dw: bool = True,
                  residual: Optional[torch.Tensor] = None, return_part: bool = False):
    """returns (dx, dw_fp32 or None, db_fp32 or None); dw/db are (accumulated) into dw_out/db_out when given; `residual` is
    added to dx inside the kernel.  ``return_part``: (dx, the kernel's per-row-block partial sums [blocks, dw | db]) — the caller folds them"""
    x2 = x.reshape(-1, x.shape[-1])
    dy2 = dy.reshape(-1, x.shape[-1])
    assert x2.is_contiguous() and dy2.is_contiguous()
    rows, cols = x2.shape
    dx = torch.empty_like(x2)
    part = None
    if w is not None:
        part = torch.empty((norm_bwd_blocks(rows), 2 * cols), device=x.device, dtype=torch.float32)
    L.check(lib.dxa_layernorm_bwd(_ptr(dy2), _ptr(x2), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dx),
                                  _ptr(_residual2d(residual, x2)), _ptr(part), rows, cols, dt(x2), dt(w) if w is not None else dt(x2), _stream()), "dxa_layernorm_bwd")
    if return_part:
        return dx.view(x.shape), part
    if part is None or not want_dw:
        return dx.view(x.shape), None, None
    if dw_out is not None:
        if db_out is not None and db_out.data_ptr() == dw_out.data_ptr() + 4 * cols:
            # weight and bias gradient slots lie back to back (they are registered as one group): one column sum
            both = torch.as_strided(dw_out, (2 * cols,), (1,))
            colsum(part, out=both, accumulate=accumulate)
        else:
            colsum(part[:, :cols], out=dw_out, accumulate=accumulate)
            colsum(part[:, cols:], out=db_out, accumulate=accumulate)
        return dx.view(x.shape), dw_out, db_out
    s = colsum(part)
    return dx.view(x.shape), s[:cols], s[cols:]


def add_layernorm_fwd(x, res, w, b, eps):
    """y = LayerNorm(x + res) in one launch; the sum is never written -> (y, mean [rows], rstd [rows])"""
    x2 = x.reshape(-1, x.shape[-1])
    r2 = res.reshape(-1, x.shape[-1])
    assert x2.is_contiguous() and r2.is_contiguous() and r2.shape == x2.shape and r2.dtype == x2.dtype
    y = torch.empty_like(x2)
    mean = torch.empty(x2.shape[0], device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    L.check(lib.dxa_add_layernorm_fwd(_ptr(x2), _ptr(r2), _ptr(w), _ptr(b), _ptr(y), _ptr(mean), _ptr(rstd), x2.shape[0],
                                      x2.shape[1], eps, dt(x2), dt(w) if w is not None else dt(x2), _stream()),
            "dxa_add_layernorm_fwd")
    return y.view(x.shape), mean, rstd


def add_layernorm_bwd(dy, x, res, w, mean, rstd):
    """-> (dx, the gradient of BOTH addends; partial sums [blocks, dw | db] fp32 or None without w): the caller folds the partials"""
    x2 = x.reshape(-1, x.shape[-1])
    r2 = res.reshape(-1, x.shape[-1])
    dy2 = dy.reshape(-1, x.shape[-1])
    assert x2.is_contiguous() and r2.is_contiguous() and dy2.is_contiguous() and r2.shape == x2.shape == dy2.shape
    assert r2.dtype == x2.dtype == dy2.dtype
    rows, cols = x2.shape
    dx = torch.empty_like(x2)
    part = None
    if w is not None:
        part = torch.empty((norm_bwd_blocks(rows), 2 * cols), device=x.device, dtype=torch.float32)
    L.check(lib.dxa_add_layernorm_bwd(_ptr(dy2), _ptr(x2), _ptr(r2), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(part), rows,
                                      cols, dt(x2), dt(w) if w is not None else dt(x2), _stream()), "dxa_add_layernorm_bwd")
    return dx.view(x.shape), part


def _gate_view(gate: torch.Tensor, B: int, cols: int, like: torch.Tensor) -> int:
    """gate [B, cols], usually the last third of a [B, 3 * cols] modulation tensor: a view with contiguous columns -> its row stride"""
    assert gate.shape == (B, cols) and gate.dtype == like.dtype and gate.stride(1) == 1 and gate.stride(0) >= cols, \
        (gate.shape, gate.stride(), gate.dtype)
    return gate.stride(0)


def _adarms_rows(x: torch.Tensor, mod: torch.Tensor):
    x2 = x.reshape(-1, x.shape[-1])
    rows, cols = x2.shape
    assert x2.is_contiguous() and mod.is_contiguous() and mod.dim() == 2 and mod.shape[1] == 3 * cols and mod.dtype == x.dtype
    B = mod.shape[0]
    assert B > 0 and rows % B == 0, (rows, B)
    return x2, rows, cols, B


def adarms_fwd(x: torch.Tensor, mod: torch.Tensor, eps: float, branch: Optional[torch.Tensor] = None,
               gate_prev: Optional[torch.Tensor] = None):
    """adaptive RMSNorm with the per-sample modulation mod [B, 3 * cols] = [scale | shift | gate] (rows / B rows per sample).
    With ``branch`` and ``gate_prev`` [B, cols] (a view into another modulation tensor): r = x + branch * gate_prev[sample] first,
    in the same launch.  -> (y, rstd [rows], r or None)"""
    x2, rows, cols, B = _adarms_rows(x, mod)
    y = torch.empty_like(x2)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    r, b2, gate_ld = None, None, 0
    if branch is not None:
        b2 = branch.reshape(-1, cols)
        assert b2.is_contiguous() and b2.shape == x2.shape and b2.dtype == x2.dtype
        gate_ld = _gate_view(gate_prev, B, cols, x2)
        r = torch.empty_like(x2)
    L.check(lib.dxa_adarms_fwd(_ptr(x2), _ptr(b2), _ptr(gate_prev) if branch is not None else None, gate_ld, _ptr(mod), _ptr(r),
                               _ptr(y), _ptr(rstd), rows, rows // B, cols, eps, dt(x2), _stream()), "dxa_adarms_fwd")
    return y.view(x.shape), rstd, (r.view(x.shape) if r is not None else None)


def gated_residual_fwd(x: torch.Tensor, branch: torch.Tensor, gate: torch.Tensor) -> torch.Tensor:
    """x + branch * gate[sample]; gate [B, cols] may be a view into a modulation tensor"""
    x2 = x.reshape(-1, x.shape[-1])
    b2 = branch.reshape(-1, x.shape[-1])
    rows, cols = x2.shape
    B = gate.shape[0]
    assert x2.is_contiguous() and b2.is_contiguous() and b2.shape == x2.shape and b2.dtype == x2.dtype and rows % B == 0
    y = torch.empty_like(x2)
    L.check(lib.dxa_gated_residual_fwd(_ptr(x2), _ptr(b2), _ptr(gate), _gate_view(gate, B, cols, x2), _ptr(y), rows, rows // B, cols,
                                       dt(x2), _stream()), "dxa_gated_residual_fwd")
    return y.view(x.shape)


def _adarms_partial(B: int, rows: int, n: int, cols: int, device) -> torch.Tensor:
    return torch.empty(B * 4 * int(lib.dxa_adarms_bwd_groups(rows // B)) * n * cols, device=device, dtype=torch.float32)


def adarms_bwd(dy, r, mod, rstd, dmod: torch.Tensor, residual=None, branch=None, gate_prev=None, dgate_prev=None):
    """backward of adarms_fwd on the row it normalised (``r``: x, or the gated sum).  Writes the scale and shift thirds of ``dmod``
    [B, 3 * cols]; with ``branch``: also ``dgate_prev`` [B, cols] (a view into the other modulation tensor's gradient).
    -> (dr (+ residual), dbranch or None)"""
    r2, rows, cols, B = _adarms_rows(r, mod)
    dy2 = dy.reshape(-1, cols)
    assert dy2.is_contiguous() and dy2.shape == r2.shape and dy2.dtype == r2.dtype
    assert dmod.is_contiguous() and dmod.shape == mod.shape and dmod.dtype == mod.dtype
    dr = torch.empty_like(r2)
    b2 = dbranch = None
    gate_ld = dgate_ld = 0
    if branch is not None:
        b2 = branch.reshape(-1, cols)
        assert b2.is_contiguous() and b2.shape == r2.shape and b2.dtype == r2.dtype
        gate_ld, dgate_ld = _gate_view(gate_prev, B, cols, r2), _gate_view(dgate_prev, B, cols, r2)
        dbranch = torch.empty_like(r2)
    part = _adarms_partial(B, rows, 3 if branch is not None else 2, cols, r.device)
    L.check(lib.dxa_adarms_bwd(_ptr(dy2), _ptr(r2), _ptr(mod), _ptr(rstd), _ptr(_residual2d(residual, r2)), _ptr(dr), _ptr(dmod),
                               _ptr(b2), _ptr(gate_prev) if branch is not None else None, gate_ld, _ptr(dbranch),
                               _ptr(dgate_prev) if branch is not None else None, dgate_ld, _ptr(part), part.numel() * 4, rows,
                               rows // B, cols, dt(r2), _stream()), "dxa_adarms_bwd")
    return dr.view(r.shape), (dbranch.view(r.shape) if dbranch is not None else None)


def gated_residual_bwd(dy, branch, gate, dgate: torch.Tensor) -> torch.Tensor:
    """backward of gated_residual_fwd: -> dbranch = dy * gate[sample]; ``dgate`` [B, cols] (a view) receives sum_rows dy * branch"""
    dy2 = dy.reshape(-1, dy.shape[-1])
    b2 = branch.reshape(-1, dy.shape[-1])
    rows, cols = dy2.shape
    B = gate.shape[0]
    assert dy2.is_contiguous() and b2.is_contiguous() and b2.shape == dy2.shape and b2.dtype == dy2.dtype and rows % B == 0
    dbranch = torch.empty_like(dy2)
    part = _adarms_partial(B, rows, 1, cols, dy.device)
    L.check(lib.dxa_gated_residual_bwd(_ptr(dy2), _ptr(b2), _ptr(gate), _gate_view(gate, B, cols, dy2), _ptr(dbranch), _ptr(dgate),
                                       _gate_view(dgate, B, cols, dy2), _ptr(part), part.numel() * 4, rows, rows // B, cols, dt(dy2),
                                       _stream()), "dxa_gated_residual_bwd")
    return dbranch.view(dy.shape)


def downsample_grid(n_tokens: int) -> Tuple[int, int]:
    """(G, h) of the 2x2 token merge: n_tokens = G*G input tokens per image, h*h = ceil(G/2)^2 merged tokens"""
    G = int(round(n_tokens ** 0.5))
    if G * G != n_tokens or G < 1:
        raise L.DxaError(f"downsample: {n_tokens} tokens per image are not a square grid")
    return G, (G + 1) // 2


def downsample_layernorm_fwd(x, w, b, eps):
    """x [N, G*G, C] -> (y [N, h*h, 4C], mean [N*h*h], rstd [N*h*h]): 2x2 token merge (column-pair major, odd grids zero padded)
    + LayerNorm over the 4C merged columns in one launch"""
    assert x.dim() == 3 and x.is_contiguous()
    N, T, C_ = x.shape
    G, h = downsample_grid(T)
    y = torch.empty((N, h * h, 4 * C_), device=x.device, dtype=x.dtype)
    mean = torch.empty(N * h * h, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    L.check(lib.dxa_downsample_layernorm_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(y), _ptr(mean), _ptr(rstd), N, G, C_, eps, dt(x),
                                             dt(w) if w is not None else dt(x), _stream()), "dxa_downsample_layernorm_fwd")
    return y, mean, rstd


def downsample_layernorm_bwd(dy, x, w, mean, rstd, out: Optional[torch.Tensor] = None):
    """-> (dx [N, G*G, C] in the un-merged layout, partial sums [blocks, dw | db] fp32 or None without w); the caller folds the
    partials (colsum).  ``out``: destination for dx (every element is written)"""
    assert x.dim() == 3 and x.is_contiguous()
    N, T, C_ = x.shape
    G, h = downsample_grid(T)
    dy2 = dy.reshape(N * h * h, 4 * C_)
    assert dy2.is_contiguous() and dy2.dtype == x.dtype
    dx = torch.empty_like(x) if out is None else out
    assert dx.shape == x.shape and dx.dtype == x.dtype and dx.is_contiguous()
    part = None
    if w is not None:
        part = torch.empty((norm_bwd_blocks(N * h * h), 8 * C_), device=x.device, dtype=torch.float32)
    L.check(lib.dxa_downsample_layernorm_bwd(_ptr(dy2), _ptr(x), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(part), N, G, C_,
                                             dt(x), dt(w) if w is not None else dt(x), _stream()), "dxa_downsample_layernorm_bwd")
    return dx, part


# ------------------------------------------------------------------------------------------------- OFT
def _action_off(off: torch.Tensor, B: int) -> torch.Tensor:
    assert off.dtype == torch.int64 and off.is_contiguous() and off.numel() == B, (off.dtype, off.shape, B)
    return off


def action_put_(x: torch.Tensor, query: torch.Tensor, off: torch.Tensor, state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, Sq, d] in place: x[b, off[b] + s + j] = query[j] (query [n, d] in x's dtype or fp32, shared by the batch); with ``state``
    [B, d]: x[b, off[b]] = state[b] and s = 1, else s = 0.  ``off`` [B] int64 on the device."""
    B, Sq, d = x.shape
    assert x.is_contiguous() and query.is_contiguous() and query.dim() == 2 and query.shape[1] == d
    if state is not None:
        assert state.is_contiguous() and state.shape == (B, d) and state.dtype == x.dtype
    L.check(lib.dxa_action_put_fwd(_ptr(x), _ptr(query), _ptr(state), _ptr(_action_off(off, B)), B, Sq, d, query.shape[0], dt(x),
                                   dt(query), _stream()), "dxa_action_put_fwd")
    return x


def action_put_bwd(dx: torch.Tensor, off: torch.Tensor, n_query: int, skip: bool, dquery: Optional[torch.Tensor] = None,
                   accumulate: bool = False, want_dstate: bool = False):
    """-> (dquery [n_query, d] fp32 = sum over the samples in ascending order, written to / accumulated into ``dquery`` when given;
    dstate [B, d] in dx's dtype or None)"""
    B, Sq, d = dx.shape
    assert dx.is_contiguous()
    if dquery is None:
        dquery = torch.empty((n_query, d), device=dx.device, dtype=torch.float32)
        accumulate = False
    assert dquery.dtype == torch.float32 and dquery.is_contiguous() and dquery.numel() == n_query * d
    dstate = torch.empty((B, d), device=dx.device, dtype=dx.dtype) if (want_dstate and skip) else None
    L.check(lib.dxa_action_put_bwd(_ptr(dx), _ptr(_action_off(off, B)), _ptr(dquery), _ptr(dstate), B, Sq, d, n_query, int(skip),
                                   int(accumulate), dt(dx), _stream()), "dxa_action_put_bwd")
    return dquery, dstate


def action_layernorm_fwd(h: torch.Tensor, off: torch.Tensor, w, b, T: int, A: int, skip: bool, eps: float):
    """h [B, Sq, d] -> (y [B*T, A*d], mean [B*T], rstd [B*T]): row (b, t) = LayerNorm of the A*d elements from h[b, off[b] + skip + t*A]"""
    B, Sq, d = h.shape
    assert h.is_contiguous()
    y = torch.empty((B * T, A * d), device=h.device, dtype=h.dtype)
    mean = torch.empty(B * T, device=h.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    L.check(lib.dxa_action_layernorm_fwd(_ptr(h), _ptr(_action_off(off, B)), _ptr(w), _ptr(b), _ptr(y), _ptr(mean), _ptr(rstd), B, Sq,
                                         d, T, A, int(skip), eps, dt(h), dt(w) if w is not None else dt(h), _stream()),
            "dxa_action_layernorm_fwd")
    return y, mean, rstd


def action_layernorm_bwd(dy: torch.Tensor, h: torch.Tensor, off: torch.Tensor, w, mean, rstd, T: int, A: int, skip: bool,
                         out: Optional[torch.Tensor] = None):
    """-> (dh [B, Sq, d], every element written: dx on the action rows, zero elsewhere; partial sums [blocks, dw | db] fp32 or None
    without w: the caller folds them with colsum)"""
    B, Sq, d = h.shape
    dy2 = dy.reshape(B * T, A * d)
    assert h.is_contiguous() and dy2.is_contiguous() and dy2.dtype == h.dtype
    dh = torch.empty_like(h) if out is None else out
    assert dh.shape == h.shape and dh.dtype == h.dtype and dh.is_contiguous()
    part = None
    if w is not None:
        part = torch.empty((int(lib.dxa_action_layernorm_bwd_blocks(B * T)), 2 * A * d), device=h.device, dtype=torch.float32)
    L.check(lib.dxa_action_layernorm_bwd(_ptr(dy2), _ptr(h), _ptr(_action_off(off, B)), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dh),
                                         _ptr(part), B, Sq, d, T, A, int(skip), dt(h), dt(w) if w is not None else dt(h), _stream()),
            "dxa_action_layernorm_bwd")
    return dh, part


def l1_loss(pred, target, gscale: float = 1.0, want_grad: bool = True):
    """mean |pred - target| -> (loss [1], dpred = sign(pred - target) gscale / n or None)"""
    assert pred.is_contiguous() and target.is_contiguous() and pred.dtype == torch.float32 and target.dtype == torch.float32
    assert pred.numel() == target.numel()
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred) if want_grad else None
    L.check(lib.dxa_l1_loss(_ptr(pred), _ptr(target), _ptr(loss), _ptr(dpred), pred.numel(), gscale, _stream()), "dxa_l1_loss")
    return loss, dpred


def action_rows_fwd(h: torch.Tensor, off: torch.Tensor, n_rows: int, skip: bool) -> torch.Tensor:
    """h [B, Sq, d] -> y [B * n_rows, d]: y[b * n_rows + j] = h[b, off[b] + skip + j]; zero rows for an out-of-range sample"""
    B, Sq, d = h.shape
    assert h.is_contiguous()
    y = torch.empty((B * n_rows, d), device=h.device, dtype=h.dtype)
    L.check(lib.dxa_action_rows_fwd(_ptr(h), _ptr(_action_off(off, B)), _ptr(y), B, Sq, d, n_rows, int(skip), dt(h), _stream()),
            "dxa_action_rows_fwd")
    return y


def action_rows_bwd(dy: torch.Tensor, off: torch.Tensor, B: int, Sq: int, n_rows: int, skip: bool,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dy [B * n_rows, d] -> dh [B, Sq, d], every element written: the dy rows on the action rows, zero elsewhere"""
    d = dy.shape[-1]
    assert dy.is_contiguous() and dy.numel() == B * n_rows * d
    dh = torch.empty((B, Sq, d), device=dy.device, dtype=dy.dtype) if out is None else out
    assert dh.shape == (B, Sq, d) and dh.dtype == dy.dtype and dh.is_contiguous()
    L.check(lib.dxa_action_rows_bwd(_ptr(dy), _ptr(_action_off(off, B)), _ptr(dh), B, Sq, d, n_rows, int(skip), dt(dy), _stream()),
            "dxa_action_rows_bwd")
    return dh


def action_fill_(x: torch.Tensor, row: torch.Tensor, off: torch.Tensor, n_rows: int, state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, Sq, d] in place: x[b, off[b] + s + j] = row for j < n_rows (row [d] in x's dtype or fp32); with ``state`` [B, d]:
    x[b, off[b]] = state[b] and s = 1, else s = 0"""
    B, Sq, d = x.shape
    assert x.is_contiguous() and row.is_contiguous() and row.numel() == d
    if state is not None:
        assert state.is_contiguous() and state.shape == (B, d) and state.dtype == x.dtype
    L.check(lib.dxa_action_fill_fwd(_ptr(x), _ptr(row), _ptr(state), _ptr(_action_off(off, B)), B, Sq, d, n_rows, dt(x), dt(row),
                                    _stream()), "dxa_action_fill_fwd")
    return x


def action_fill_bwd(dx: torch.Tensor, off: torch.Tensor, n_rows: int, skip: bool, drow: Optional[torch.Tensor] = None,
                    accumulate: bool = False, want_dstate: bool = False):
    """-> (drow [d] fp32 = sum over every sample's action rows of dx, in a fixed order, written to / accumulated into ``drow`` when
    given; dstate [B, d] in dx's dtype or None)"""
    B, Sq, d = dx.shape
    assert dx.is_contiguous()
    if drow is None:
        drow = torch.empty(d, device=dx.device, dtype=torch.float32)
        accumulate = False
    assert drow.dtype == torch.float32 and drow.is_contiguous() and drow.numel() == d
    dstate = torch.empty((B, d), device=dx.device, dtype=dx.dtype) if (want_dstate and skip) else None
    partial = torch.empty((int(lib.dxa_action_fill_bwd_blocks(B * n_rows)), d), device=dx.device, dtype=torch.float32)
    L.check(lib.dxa_action_fill_bwd(_ptr(dx), _ptr(_action_off(off, B)), _ptr(drow), _ptr(dstate), _ptr(partial), B, Sq, d, n_rows,
                                    int(skip), int(accumulate), dt(dx), _stream()), "dxa_action_fill_bwd")
    return drow, dstate


def action_bins_fwd(h: torch.Tensor, off: torch.Tensor, w_bins: torch.Tensor, n_rows: int, skip: bool):
    """h [B, Sq, d], w_bins [NB, d] (contiguous rows: the tail of lm_head.weight) -> (bin_logits [B * n_rows, NB] in h's dtype,
    bin int64 [B * n_rows] = first index of the row's maximum, action fp32 [B * n_rows] = bin / NB * 2 - 1).  Semantics:
    include/dexbotic_amd.h"""
    B, Sq, d = h.shape
    assert h.is_contiguous() and w_bins.is_contiguous() and w_bins.dim() == 2 and w_bins.shape[1] == d and w_bins.dtype == h.dtype
    NB, rows = w_bins.shape[0], B * n_rows
    logits = torch.empty((rows, NB), device=h.device, dtype=h.dtype)
    bins = torch.empty(rows, device=h.device, dtype=torch.int64)
    action = torch.empty(rows, device=h.device, dtype=torch.float32)
    counters = torch.empty(int(lib.dxa_action_bins_counters(rows)), device=h.device, dtype=torch.int32)
    L.check(lib.dxa_action_bins_fwd(_ptr(h), _ptr(_action_off(off, B)), _ptr(w_bins), _ptr(logits), _ptr(bins), _ptr(action),
                                    _ptr(counters), B, Sq, d, n_rows, int(skip), NB, dt(h), _stream()), "dxa_action_bins_fwd")
    return logits, bins, action


def _embed_args(a: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor) -> int:
    d = w1.numel()
    assert a.dtype == torch.float32 and a.is_contiguous() and w1.is_contiguous() and b1.is_contiguous()
    assert b1.numel() == d and w1.dtype == b1.dtype
    return d


def noisy_embed_fwd(a: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """a fp32 (R scalars, any shape), w1 [d, 1] / b1 [d] -> h [R, d] in ``dtype``: gelu_erf(a_r w1 + b1) with a and the pre-activation
    rounded to ``dtype``.  Semantics: include/dexbotic_amd.h"""
    d = _embed_args(a, w1, b1)
    h = torch.empty((a.numel(), d), device=a.device, dtype=dtype)
    L.check(lib.dxa_noisy_embed_fwd(_ptr(a), _ptr(w1), _ptr(b1), _ptr(h), a.numel(), d, dt(h), dt(w1), _stream()), "dxa_noisy_embed_fwd")
    return h


def noisy_embed_bwd(dh: torch.Tensor, a: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, dw1: Optional[torch.Tensor] = None,
                    db1: Optional[torch.Tensor] = None, accumulate: bool = False):
    """-> (dw1 [d], db1 [d]) fp32, fixed-order sums over the R rows, written to / accumulated into ``dw1`` / ``db1`` when given"""
    d = _embed_args(a, w1, b1)
    R = a.numel()
    assert dh.is_contiguous() and dh.shape == (R, d)
    if dw1 is None or db1 is None:
        dw1, db1 = (torch.empty(d, device=dh.device, dtype=torch.float32) for _ in range(2))
        accumulate = False
    for t in (dw1, db1):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == d
    partial = torch.empty((int(lib.dxa_noisy_embed_bwd_blocks(R)), 2 * d), device=dh.device, dtype=torch.float32)
    L.check(lib.dxa_noisy_embed_bwd(_ptr(dh), _ptr(a), _ptr(w1), _ptr(b1), _ptr(dw1), _ptr(db1), _ptr(partial), R, d, int(accumulate),
                                    dt(dh), dt(w1), _stream()), "dxa_noisy_embed_bwd")
    return dw1, db1


def diffusion_put_(x: torch.Tensor, proj: torch.Tensor, time: torch.Tensor, off: torch.Tensor,
                   state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, Sq, d] in place, at the block off[b]: [state[b], when given] [time[b]] [proj[b * R + j], j < R]; proj [B R, d], time [B, d]"""
    B, Sq, d = x.shape
    assert x.is_contiguous() and proj.is_contiguous() and time.is_contiguous() and proj.dtype == x.dtype and time.dtype == x.dtype
    assert proj.dim() == 2 and proj.shape[1] == d and proj.shape[0] % max(B, 1) == 0 and time.shape == (B, d)
    if state is not None:
        assert state.is_contiguous() and state.shape == (B, d) and state.dtype == x.dtype
    L.check(lib.dxa_diffusion_put_fwd(_ptr(x), _ptr(proj), _ptr(time), _ptr(state), _ptr(_action_off(off, B)), B, Sq, d,
                                      proj.shape[0] // max(B, 1), dt(x), _stream()), "dxa_diffusion_put_fwd")
    return x


def diffusion_put_bwd(dx: torch.Tensor, off: torch.Tensor, n_rows: int, skip: bool, want_dstate: bool = False):
    """-> (dproj [B n_rows, d], dstate [B, d] or None) in dx's dtype; zero rows for an out-of-range sample"""
    B, Sq, d = dx.shape
    assert dx.is_contiguous()
    dproj = torch.empty((B * n_rows, d), device=dx.device, dtype=dx.dtype)
    dstate = torch.empty((B, d), device=dx.device, dtype=dx.dtype) if (want_dstate and skip) else None
    L.check(lib.dxa_diffusion_put_bwd(_ptr(dx), _ptr(_action_off(off, B)), _ptr(dproj), _ptr(dstate), B, Sq, d, n_rows, int(skip),
                                      dt(dx), _stream()), "dxa_diffusion_put_bwd")
    return dproj, dstate


def ddim_step_embed_(eps: Optional[torch.Tensor], x: torch.Tensor, coef, clip: float, time_row: torch.Tensor, w1: torch.Tensor,
                     b1: torch.Tensor, suffix: torch.Tensor, h: torch.Tensor) -> None:
    """x [n] fp32 in place: with ``eps`` [n] (h's dtype) the DDIM update with ``coef`` = (c0, c1, c2, c3) and the clamp at +-``clip``;
    then suffix[0] = time_row and h [n, d] = the projector's fc2 operand of the new x.  Semantics: include/dexbotic_amd.h"""
    n, d = h.shape
    assert _embed_args(x, w1, b1) == d and x.numel() == n and h.is_contiguous()
    assert time_row.is_contiguous() and time_row.numel() == d and time_row.dtype == h.dtype
    assert suffix.dtype == h.dtype and suffix.shape[-1] == d and suffix.stride(-1) == 1
    if eps is not None:
        assert eps.is_contiguous() and eps.numel() == n and eps.dtype == h.dtype
    c0, c1, c2, c3 = (float(c) for c in coef)
    L.check(lib.dxa_ddim_step_embed(_ptr(eps), _ptr(x), c0, c1, c2, c3, float(clip), _ptr(time_row), _ptr(w1), _ptr(b1), _ptr(suffix),
                                    _ptr(h), n, d, dt(h), dt(w1), _stream()), "dxa_ddim_step_embed")


def bin_logprob_fwd(logits: torch.Tensor, bins: torch.Tensor, temperature: float = 1.0):
    """logits [rows, NB] (fp32 / bf16, rows contiguous, any row stride), bins [rows] int64 BIN indices -> (logp, entropy, lse), each
    [rows] fp32, of softmax(logits / temperature).  Semantics: include/dexbotic_amd.h"""
    rows, NB = logits.shape
    ld = _row_major(logits, "bin_logprob_fwd: logits")
    assert bins.dtype == torch.int64 and bins.is_contiguous() and bins.numel() == rows
    logp, entropy, lse = (torch.empty(rows, device=logits.device, dtype=torch.float32) for _ in range(3))
    L.check(lib.dxa_bin_logprob_fwd(_ptr(logits), ld, _ptr(bins), 1.0 / float(temperature), _ptr(logp), _ptr(entropy), _ptr(lse),
                                    rows, NB, dt(logits), _stream()), "dxa_bin_logprob_fwd")
    return logp, entropy, lse


def bin_logprob_bwd(logits: torch.Tensor, bins: torch.Tensor, lse: torch.Tensor, coef: torch.Tensor, gscale: Optional[torch.Tensor],
                    temperature: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dlogits = coef[r] gscale[0] / temperature (onehot(bin) - softmax(logits / temperature)); ``out`` may be ``logits`` itself (in
    place) and otherwise has its row stride"""
    rows, NB = logits.shape
    ld = _row_major(logits, "bin_logprob_bwd: logits")
    if out is None:
        out = torch.empty_strided(logits.shape, logits.stride(), device=logits.device, dtype=logits.dtype)
    assert out.shape == logits.shape and out.dtype == logits.dtype and _row_major(out, "bin_logprob_bwd: out") == ld
    for t in (lse, coef):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == rows
    assert bins.dtype == torch.int64 and bins.is_contiguous() and bins.numel() == rows
    assert gscale is None or (gscale.dtype == torch.float32 and gscale.numel() == 1)
    L.check(lib.dxa_bin_logprob_bwd(_ptr(logits), ld, _ptr(bins), _ptr(lse), _ptr(coef), _ptr(gscale), 1.0 / float(temperature),
                                    _ptr(out), rows, NB, dt(logits), _stream()), "dxa_bin_logprob_bwd")
    return out


def ppo_clip_fwd(logp: torch.Tensor, old_logp: torch.Tensor, adv: torch.Tensor, mask: torch.Tensor, clip_low: float, clip_high: float,
                 denom: Optional[float] = None):
    """the clipped policy loss over n tokens (fp32; ``mask`` fp32 0/1, uint8 or bool) -> (loss [1] = sums[0] / denom, sums [4] =
    (sum max(pg1, pg2), clipped count, sum (old - logp), valid count), coef [n] = d loss / d logp).  ``denom`` None: the mask's own
    count (a masked mean; an empty mask gives loss 0 and coef 0).  Semantics: include/dexbotic_amd.h"""
    n = logp.numel()
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    assert mask.dtype in (torch.float32, torch.uint8) and mask.is_contiguous() and mask.numel() == n
    for t in (logp, old_logp, adv):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    if denom is not None and not denom > 0:
        raise L.DxaError(f"ppo_clip_fwd: denom {denom} (a positive number, or None for the mask's own count)")
    sums = torch.empty(4, device=logp.device, dtype=torch.float32)
    loss = torch.empty(1, device=logp.device, dtype=torch.float32)
    coef = torch.empty(n, device=logp.device, dtype=torch.float32)
    L.check(lib.dxa_ppo_clip_fwd(_ptr(logp), _ptr(old_logp), _ptr(adv), _ptr(mask), int(mask.dtype == torch.uint8), n, float(clip_low),
                                 float(clip_high), 0.0 if denom is None else 1.0 / float(denom), _ptr(sums), _ptr(loss), _ptr(coef),
                                 _stream()), "dxa_ppo_clip_fwd")
    return loss, sums, coef


def _sample_rows(t: torch.Tensor, B: int, cols: int, name: str) -> int:
    """sample stride (elements) of an fp32 [B, cols] view whose rows are contiguous: a dense tensor or columns of a wider one"""
    if t.dtype != torch.float32 or t.shape != (B, cols) or (cols > 1 and t.stride(1) != 1):
        raise L.DxaError(f"{name}: expected fp32 [{B}, {cols}] with contiguous rows, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0) if B > 1 else max(cols, t.stride(0))


def flow_suffix_in(x: torch.Tensor, te: torch.Tensor, w_in: torch.Tensor, b_in: torch.Tensor, n: int, A: int,
                   progress: Optional[torch.Tensor] = None, w_p: Optional[torch.Tensor] = None,
                   b_p: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x fp32 [B, n * A] (rows may be columns of a wider tensor), te [B, da], w_in [da, A], b_in [da] -> the input of
    action_time_mlp_in [B * (p + n), 2 * da] in te's dtype; ``progress`` fp32 [B, 1] with w_p [da, 1] / b_p [da] puts the progress
    row in front of every sample's action rows (p = 1).  Semantics: include/dexbotic_amd.h"""
    B, da = te.shape
    p = 0 if progress is None else 1
    assert te.is_contiguous() and w_in.is_contiguous() and b_in.is_contiguous() and w_in.shape == (da, A) and b_in.numel() == da
    assert w_in.dtype == te.dtype == b_in.dtype
    ldx = _sample_rows(x, B, n * A, "flow_suffix_in x")
    ldp = 0
    if p:
        assert w_p is not None and b_p is not None and w_p.is_contiguous() and b_p.is_contiguous()
        assert w_p.numel() == da == b_p.numel() and w_p.dtype == te.dtype == b_p.dtype
        ldp = _sample_rows(progress, B, 1, "flow_suffix_in progress")
    if out is None:
        out = torch.empty((B * (p + n), 2 * da), device=te.device, dtype=te.dtype)
    assert out.is_contiguous() and out.shape == (B * (p + n), 2 * da) and out.dtype == te.dtype
    L.check(lib.dxa_flow_suffix_in(_ptr(x), ldx, _ptr(progress), ldp, _ptr(te), _ptr(w_in), _ptr(b_in), _ptr(w_p) if p else None,
                                   _ptr(b_p) if p else None, _ptr(out), B, n, A, da, p, dt(te), _stream()), "dxa_flow_suffix_in")
    return out


def flow_euler_tail_(h: torch.Tensor, g: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, x: torch.Tensor, n: int, eps: float,
                     dt_: float, prog_min: Optional[torch.Tensor] = None, w_q: Optional[torch.Tensor] = None,
                     b_q: Optional[torch.Tensor] = None) -> torch.Tensor:
    """h [B * (p + n), da] (the expert's rows before its final norm), g [da], w_out [A, da], b_out [A]; x fp32 [B, n * A] IN PLACE:
    x += dt * action_out_proj(rmsnorm(h)) on the action rows; with ``prog_min`` fp32 [B, 1] (p = 1, w_q [1, da], b_q [1]) the
    progress row's prediction is folded into the running minimum in place.  Semantics: include/dexbotic_amd.h"""
    A, da = w_out.shape
    p = 0 if prog_min is None else 1
    B = h.shape[0] // (p + n)
    assert h.is_contiguous() and h.shape == (B * (p + n), da) and g.is_contiguous() and g.numel() == da
    assert w_out.is_contiguous() and b_out.is_contiguous() and b_out.numel() == A and h.dtype == g.dtype == w_out.dtype == b_out.dtype
    ldx = _sample_rows(x, B, n * A, "flow_euler_tail_ x")
    ldm = 0
    if p:
        assert w_q is not None and b_q is not None and w_q.is_contiguous() and w_q.numel() == da and b_q.numel() == 1
        assert w_q.dtype == h.dtype == b_q.dtype
        ldm = _sample_rows(prog_min, B, 1, "flow_euler_tail_ prog_min")
    L.check(lib.dxa_flow_euler_tail(_ptr(h), _ptr(g), _ptr(w_out), _ptr(b_out), _ptr(w_q) if p else None, _ptr(b_q) if p else None,
                                    _ptr(x), ldx, _ptr(prog_min), ldm, B, n, A, da, p, eps, dt_, dt(h), _stream()),
            "dxa_flow_euler_tail")
    return x


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """out[c] (+)= sum_r x[r, c]  (fp32 result)"""
    ld = _row_major(x, "x")
    rows, cols = x.shape
    if out is None:
        out = torch.empty(cols, device=x.device, dtype=torch.float32)
        accumulate = False
    nsplit = max(1, min(64, (rows + 31) // 32))
    scratch = torch.empty(nsplit * cols, device=x.device, dtype=torch.float32)
    L.check(lib.dxa_colsum(_ptr(x), ld, _ptr(out), rows, cols, dt(x), int(accumulate), _ptr(scratch),
                           scratch.numel() * 4, _stream()), "dxa_colsum")
    return out


# ------------------------------------------------------------------------------------------------ RoPE
def rope_split(qkv: torch.Tensor, cos_t, sin_t, pos, B, S, Hq, Hkv, D):
    assert qkv.is_contiguous() and qkv.shape == (B * S, (Hq + 2 * Hkv) * D)
    q = torch.empty((B, Hq, S, D), device=qkv.device, dtype=qkv.dtype)
    k = torch.empty((B, Hkv, S, D), device=qkv.device, dtype=qkv.dtype)
    v = torch.empty((B, Hkv, S, D), device=qkv.device, dtype=qkv.dtype)
    L.check(lib.dxa_rope_split(_ptr(qkv), _ptr(q), _ptr(k), _ptr(v), _ptr(cos_t), _ptr(sin_t), _ptr(pos), B, S, Hq,
                               Hkv, D, dt(qkv), _stream()), "dxa_rope_split")
    return q, k, v


def rope_split_into(qkv: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, s0: int, cos_t, sin_t, pos, B, S, Hq, Hkv, D) -> None:
    """rope_split writing its S tokens at positions s0 .. s0 + S - 1 of SHARED contiguous q [B, Hq, S_cap, D], k / v [B, Hkv, S_cap, D]"""
    S_cap = q.shape[2]
    assert qkv.is_contiguous() and qkv.shape == (B * S, (Hq + 2 * Hkv) * D)
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous() and q.shape == (B, Hq, S_cap, D) and \
        k.shape == (B, Hkv, S_cap, D) == v.shape and q.dtype == k.dtype == v.dtype == qkv.dtype
    L.check(lib.dxa_rope_split_at(_ptr(qkv), _ptr(q), _ptr(k), _ptr(v), _ptr(cos_t), _ptr(sin_t), _ptr(pos), B, S, Hq, Hkv, D,
                                  S_cap, s0, dt(qkv), _stream()), "dxa_rope_split_at")


def rope_merge_from(dq, dk, dv, s0: int, cos_t, sin_t, pos, B, S, Hq, Hkv, D):
    """rope_merge of positions s0 .. s0 + S - 1 of SHARED contiguous dq [B, Hq, S_cap, D], dk / dv [B, Hkv, S_cap, D]"""
    S_cap = dq.shape[2]
    assert dq.is_contiguous() and dk.is_contiguous() and dv.is_contiguous() and dq.shape == (B, Hq, S_cap, D)
    dqkv = torch.empty((B * S, (Hq + 2 * Hkv) * D), device=dq.device, dtype=dq.dtype)
    L.check(lib.dxa_rope_merge_at(_ptr(dq), _ptr(dk), _ptr(dv), _ptr(dqkv), _ptr(cos_t), _ptr(sin_t), _ptr(pos), B, S, Hq, Hkv, D,
                                  S_cap, s0, dt(dq), _stream()), "dxa_rope_merge_at")
    return dqkv


def rope_merge(dq, dk, dv, cos_t, sin_t, pos, B, S, Hq, Hkv, D):
    assert dq.is_contiguous() and dk.is_contiguous() and dv.is_contiguous()
    dqkv = torch.empty((B * S, (Hq + 2 * Hkv) * D), device=dq.device, dtype=dq.dtype)
    L.check(lib.dxa_rope_merge(_ptr(dq), _ptr(dk), _ptr(dv), _ptr(dqkv), _ptr(cos_t), _ptr(sin_t), _ptr(pos), B, S,
                               Hq, Hkv, D, dt(dq), _stream()), "dxa_rope_merge")
    return dqkv


QKNORM_HEAD_DIMS = (32, 64, 128, 256)      # csrc/elementwise.hip qknorm_rope_*_k


def qknorm_rope_split(qkv: torch.Tensor, q_norm_w: torch.Tensor, k_norm_w: torch.Tensor, eps: float, cos_t, sin_t, pos, B, S, Hq, Hkv,
                      D, want_rstd: bool = True):
    """rope_split with Qwen3's per-head RMSNorm of q and k (weights [D] in qkv's dtype) in the same pass
    -> (q, k, v, rstd [B*S, Hq+Hkv] fp32 or None): what qknorm_rope_merge needs besides qkv itself"""
    assert qkv.is_contiguous() and qkv.shape == (B * S, (Hq + 2 * Hkv) * D)
    assert q_norm_w.dtype == qkv.dtype == k_norm_w.dtype and q_norm_w.numel() == D == k_norm_w.numel()
    q = torch.empty((B, Hq, S, D), device=qkv.device, dtype=qkv.dtype)
    k = torch.empty((B, Hkv, S, D), device=qkv.device, dtype=qkv.dtype)
    v = torch.empty((B, Hkv, S, D), device=qkv.device, dtype=qkv.dtype)
    rstd = torch.empty((B * S, Hq + Hkv), device=qkv.device, dtype=torch.float32) if want_rstd else None
    L.check(lib.dxa_qknorm_rope_split(_ptr(qkv), _ptr(q), _ptr(k), _ptr(v), _ptr(q_norm_w), _ptr(k_norm_w), float(eps), _ptr(rstd),
                                      _ptr(cos_t), _ptr(sin_t), _ptr(pos), B, S, Hq, Hkv, D, dt(qkv), _stream()),
            "dxa_qknorm_rope_split")
    return q, k, v, rstd


def qknorm_rope_merge(dq, dk, dv, qkv: torch.Tensor, rstd: torch.Tensor, q_norm_w, k_norm_w, cos_t, sin_t, pos, B, S, Hq, Hkv, D,
                      want_dw: bool = True):
    """-> (dqkv [B*S, (Hq+2Hkv)*D] token-major, partial sums [blocks, dw_q | dw_k] fp32 or None): rope_merge followed by the
    per-head RMSNorm backward, one launch; the caller folds the partials (colsum)"""
    assert dq.is_contiguous() and dk.is_contiguous() and dv.is_contiguous() and qkv.is_contiguous() and rstd.is_contiguous()
    assert qkv.shape == (B * S, (Hq + 2 * Hkv) * D) and dq.shape == (B, Hq, S, D) and dk.shape == (B, Hkv, S, D) == dv.shape
    assert dq.dtype == dk.dtype == dv.dtype == qkv.dtype == q_norm_w.dtype == k_norm_w.dtype
    assert rstd.shape == (B * S, Hq + Hkv) and rstd.dtype == torch.float32
    dqkv = torch.empty_like(qkv)
    part = None
    if want_dw:
        nblk = int(lib.dxa_qknorm_rope_merge_blocks(B * S, Hq, Hkv, D, dt(qkv)))
        if nblk < 0:
            L.check(nblk, "dxa_qknorm_rope_merge_blocks")
        part = torch.empty((nblk, 2 * D), device=qkv.device, dtype=torch.float32)
    L.check(lib.dxa_qknorm_rope_merge(_ptr(dq), _ptr(dk), _ptr(dv), _ptr(qkv), _ptr(rstd), _ptr(q_norm_w), _ptr(k_norm_w), _ptr(dqkv),
                                      _ptr(part), _ptr(cos_t), _ptr(sin_t), _ptr(pos), B, S, Hq, Hkv, D, dt(qkv), _stream()),
            "dxa_qknorm_rope_merge")
    return dqkv, part


def qknorm_rope_split_into(qkv: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q0: int, kv0: int, q_norm_w, k_norm_w,
                           eps: float, cos_t, sin_t, pos, B, S, Hq, Hkv, D, want_rstd: bool = True):
    """qknorm_rope_split writing its S tokens at positions q0 .. q0 + S - 1 of SHARED contiguous q [B, Hq, Sq_cap, D] and at
    kv0 .. kv0 + S - 1 of k / v [B, Hkv, Skv_cap, D] (capacities and offsets of q and of k / v apart: a sampler's queries are the
    suffix alone, its keys land behind the cached prefix) -> rstd [B*S, Hq+Hkv] fp32 or None"""
    Sq_cap, Skv_cap = q.shape[2], k.shape[2]
    assert qkv.is_contiguous() and qkv.shape == (B * S, (Hq + 2 * Hkv) * D)
    assert q_norm_w.dtype == qkv.dtype == k_norm_w.dtype and q_norm_w.numel() == D == k_norm_w.numel()
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous() and q.shape == (B, Hq, Sq_cap, D) and \
        k.shape == (B, Hkv, Skv_cap, D) == v.shape and q.dtype == k.dtype == v.dtype == qkv.dtype
    rstd = torch.empty((B * S, Hq + Hkv), device=qkv.device, dtype=torch.float32) if want_rstd else None
    L.check(lib.dxa_qknorm_rope_split_at(_ptr(qkv), _ptr(q), _ptr(k), _ptr(v), _ptr(q_norm_w), _ptr(k_norm_w), float(eps), _ptr(rstd),
                                         _ptr(cos_t), _ptr(sin_t), _ptr(pos), B, S, Hq, Hkv, D, Sq_cap, q0, Skv_cap, kv0, dt(qkv),
                                         _stream()), "dxa_qknorm_rope_split_at")
    return rstd


def qknorm_rope_merge_from(dq, dk, dv, s0: int, qkv: torch.Tensor, rstd: torch.Tensor, q_norm_w, k_norm_w, cos_t, sin_t, pos, B, S, Hq,
                           Hkv, D, want_dw: bool = True):
    """qknorm_rope_merge of positions s0 .. s0 + S - 1 of SHARED contiguous dq [B, Hq, S_cap, D], dk / dv [B, Hkv, S_cap, D];
    qkv and rstd are these S tokens' own -> (dqkv, partial sums or None)"""
    S_cap = dq.shape[2]
    assert dq.is_contiguous() and dk.is_contiguous() and dv.is_contiguous() and qkv.is_contiguous() and rstd.is_contiguous()
    assert qkv.shape == (B * S, (Hq + 2 * Hkv) * D) and dq.shape == (B, Hq, S_cap, D) and dk.shape == (B, Hkv, S_cap, D) == dv.shape
    assert dq.dtype == dk.dtype == dv.dtype == qkv.dtype == q_norm_w.dtype == k_norm_w.dtype
    assert rstd.shape == (B * S, Hq + Hkv) and rstd.dtype == torch.float32
    dqkv = torch.empty_like(qkv)
    part = None
    if want_dw:
        nblk = int(lib.dxa_qknorm_rope_merge_blocks(B * S, Hq, Hkv, D, dt(qkv)))
        if nblk < 0:
            L.check(nblk, "dxa_qknorm_rope_merge_blocks")
        part = torch.empty((nblk, 2 * D), device=qkv.device, dtype=torch.float32)
    L.check(lib.dxa_qknorm_rope_merge_from(_ptr(dq), _ptr(dk), _ptr(dv), _ptr(qkv), _ptr(rstd), _ptr(q_norm_w), _ptr(k_norm_w),
                                           _ptr(dqkv), _ptr(part), _ptr(cos_t), _ptr(sin_t), _ptr(pos), B, S, Hq, Hkv, D, S_cap, s0,
                                           dt(qkv), _stream()), "dxa_qknorm_rope_merge_from")
    return dqkv, part


# ------------------------------------------------------------------------------------------- attention
def _bhsd_strides(t: torch.Tensor) -> Tuple[int, int, int]:
    """t is a [B,H,S,D] VIEW (any memory order) with D contiguous -> (sb, sh, ss)"""
    assert t.dim() == 4 and (t.shape[3] == 1 or t.stride(3) == 1), (t.shape, t.stride())
    return t.stride(0), t.stride(1), t.stride(2)


def _attn_desc(q, k, v, o, lse, causal, scale, kv_start, kv_end, q_limit=None, key_valid=None, drop_mask=None) -> L.AttnDesc:
    d = L.AttnDesc()
    B, Hq, Sq, D = q.shape
    _, Hkv, Sk, _ = k.shape
    d.dtype, d.B, d.Hq, d.Hkv, d.Sq, d.Sk, d.D = dt(q), B, Hq, Hkv, Sq, Sk, D
    d.causal, d.scale = int(causal), scale
    d.q, (d.q_sb, d.q_sh, d.q_ss) = _ptr(q), _bhsd_strides(q)
    d.k, (d.k_sb, d.k_sh, d.k_ss) = _ptr(k), _bhsd_strides(k)
    d.v, (d.v_sb, d.v_sh, d.v_ss) = _ptr(v), _bhsd_strides(v)
    d.o, (d.o_sb, d.o_sh, d.o_ss) = _ptr(o), _bhsd_strides(o)
    d.lse, d.kv_start, d.kv_end = _ptr(lse), _ptr(kv_start), _ptr(kv_end)
    if q_limit is not None:
        assert q_limit.dtype == torch.int32 and q_limit.is_contiguous() and q_limit.shape == (B, Sq)
    if key_valid is not None:
        assert key_valid.dtype == torch.uint8 and key_valid.is_contiguous() and key_valid.shape == (B, Sk)
    d.q_limit, d.key_valid = _ptr(q_limit), _ptr(key_valid)
    if drop_mask is not None:
        assert drop_mask.dtype == q.dtype and drop_mask.is_contiguous() and drop_mask.shape == (B, Hq, Sq, Sk)
        d.drop_mask = _ptr(drop_mask)
    return d


def attn_fwd(q, k, v, o, *, causal: bool, scale: float, kv_start=None, kv_end=None, force_generic=False,
             q_limit=None, key_valid=None, drop_mask=None):
    """q/k/v/o: [B,H,S,D] views (token-major or head-major memory); returns lse [B,Hq,Sq] fp32"""
    B, Hq, Sq, _ = q.shape
    lse = torch.empty((B, Hq, Sq), device=q.device, dtype=torch.float32)
    d = _attn_desc(q, k, v, o, lse, causal, scale, kv_start, kv_end, q_limit, key_valid, drop_mask)
    d.force_generic = int(force_generic)
    nbytes = int(lib.dxa_attn_fwd_workspace(C.byref(d)))
    if nbytes:
        # large non-flash problem (fp32, or attention dropout): scores materialised through the batched GEMMs
        ws = torch.empty(nbytes, device=q.device, dtype=torch.uint8)
        L.check(lib.dxa_attn_fwd_ws(C.byref(d), _ptr(ws), nbytes, _stream()), "dxa_attn_fwd_ws")
    else:
        L.check(lib.dxa_attn_fwd(C.byref(d), _stream()), "dxa_attn_fwd")
    return lse


def attn_bwd(q, k, v, o, lse, do, dq, dk, dv, *, causal: bool, scale: float, kv_start=None, kv_end=None,
             force_generic=False, q_limit=None, key_valid=None, drop_mask=None):
    d = _attn_desc(q, k, v, o, lse, causal, scale, kv_start, kv_end, q_limit, key_valid, drop_mask)
    d.force_generic = int(force_generic)
    d.d_o, (d.do_sb, d.do_sh, d.do_ss) = _ptr(do), _bhsd_strides(do)
    d.dq, (d.dq_sb, d.dq_sh, d.dq_ss) = _ptr(dq), _bhsd_strides(dq)
    d.dk, (d.dk_sb, d.dk_sh, d.dk_ss) = _ptr(dk), _bhsd_strides(dk)
    d.dv, (d.dv_sb, d.dv_sh, d.dv_ss) = _ptr(dv), _bhsd_strides(dv)
    nbytes = int(lib.dxa_attn_bwd_workspace(C.byref(d)))
    ws = torch.empty(nbytes, device=q.device, dtype=torch.uint8)
    L.check(lib.dxa_attn_bwd(C.byref(d), _ptr(ws), nbytes, _stream()), "dxa_attn_bwd")


# ----------------------------------------------------------------------------------------- elementwise
def swiglu_fwd(gu: torch.Tensor) -> torch.Tensor:
    rows, F2 = gu.shape
    assert gu.is_contiguous() and F2 % 2 == 0
    out = torch.empty((rows, F2 // 2), device=gu.device, dtype=gu.dtype)
    L.check(lib.dxa_swiglu_fwd(_ptr(gu), _ptr(out), rows, F2 // 2, dt(gu), _stream()), "dxa_swiglu_fwd")
    return out


def swiglu_bwd(gu: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
    rows, F2 = gu.shape
    assert gu.is_contiguous() and dout.is_contiguous()
    dgu = torch.empty_like(gu)
    L.check(lib.dxa_swiglu_bwd(_ptr(gu), _ptr(dout), _ptr(dgu), rows, F2 // 2, dt(gu), _stream()), "dxa_swiglu_bwd")
    return dgu


def axpby(a: torch.Tensor, b: torch.Tensor, alpha: float, beta: float) -> torch.Tensor:
    assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape and a.dtype == b.dtype
    out = torch.empty_like(a)
    L.check(lib.dxa_axpby(_ptr(a), _ptr(b), _ptr(out), a.numel(), alpha, beta, dt(a), _stream()), "dxa_axpby")
    return out


def mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape and a.dtype == b.dtype
    out = torch.empty_like(a)
    L.check(lib.dxa_mul(_ptr(a), _ptr(b), _ptr(out), a.numel(), dt(a), _stream()), "dxa_mul")
    return out


def mul_rows(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """x [R, N, C] * g [R, C] (broadcast over N)"""
    R, Nn, C_ = x.shape
    assert x.is_contiguous() and g.is_contiguous() and g.shape == (R, C_) and g.dtype == x.dtype
    out = torch.empty_like(x)
    L.check(lib.dxa_mul_rows(_ptr(x), _ptr(g), _ptr(out), R, Nn, C_, dt(x), _stream()), "dxa_mul_rows")
    return out


def glu_fwd(gu: torch.Tensor, act: int) -> torch.Tensor:
    """act(gate) * up for [rows, 2F] = [gate ; up] (GeGLU with act = ACT_GELU_TANH)"""
    rows, F2 = gu.shape
    assert gu.is_contiguous() and F2 % 2 == 0
    out = torch.empty((rows, F2 // 2), device=gu.device, dtype=gu.dtype)
    L.check(lib.dxa_glu_fwd(_ptr(gu), _ptr(out), rows, F2 // 2, act, dt(gu), _stream()), "dxa_glu_fwd")
    return out


def glu_bwd(gu: torch.Tensor, dout: torch.Tensor, act: int) -> torch.Tensor:
    rows, F2 = gu.shape
    assert gu.is_contiguous() and dout.is_contiguous()
    dgu = torch.empty_like(gu)
    L.check(lib.dxa_glu_bwd(_ptr(gu), _ptr(dout), _ptr(dgu), rows, F2 // 2, act, dt(gu), _stream()), "dxa_glu_bwd")
    return dgu


def act_fwd(x: torch.Tensor, act: int) -> torch.Tensor:
    assert x.is_contiguous()
    y = torch.empty_like(x)
    L.check(lib.dxa_act_fwd(_ptr(x), _ptr(y), x.numel(), act, dt(x), _stream()), "dxa_act_fwd")
    return y


def act_bwd(x: torch.Tensor, dy: torch.Tensor, act: int) -> torch.Tensor:
    assert x.is_contiguous() and dy.is_contiguous()
    dx = torch.empty_like(x)
    L.check(lib.dxa_act_bwd(_ptr(x), _ptr(dy), _ptr(dx), x.numel(), act, dt(x), _stream()), "dxa_act_bwd")
    return dx


def add(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape and a.dtype == b.dtype
    if out is None:
        out = torch.empty_like(a)
    L.check(lib.dxa_add(_ptr(a), _ptr(b), _ptr(out), a.numel(), dt(a), _stream()), "dxa_add")
    return out


def cast(src: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert src.is_contiguous()
    if out is None:
        out = torch.empty(src.shape, device=src.device, dtype=dtype)
    L.check(lib.dxa_cast(_ptr(src), _ptr(out), src.numel(), dt(src), dt(out), _stream()), "dxa_cast")
    return out


def copy2d(src: torch.Tensor, dst: torch.Tensor, cols: int, cols_padded: int) -> torch.Tensor:
    L.check(lib.dxa_copy2d(_ptr(src), _row_major(src, "src"), _ptr(dst), _row_major(dst, "dst"), src.shape[0], cols,
                           cols_padded, dt(src), dt(dst), _stream()), "dxa_copy2d")
    return dst


def transpose(x: torch.Tensor, pad_to: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[R, C] -> [C, Rp] with Rp = R rounded up to `pad_to` (zero filled)"""
    R, C_ = x.shape
    Rp = (R + pad_to - 1) // pad_to * pad_to
    if out is None:
        out = torch.empty((C_, Rp), device=x.device, dtype=x.dtype)
    L.check(lib.dxa_transpose(_ptr(x), _row_major(x, "x"), _ptr(out), _row_major(out, "out"), R, C_, Rp, dt(x), _stream()),
            "dxa_transpose")
    return out


def permute_bshd(x: torch.Tensor, B: int, S: int, H: int, D: int, to_head: bool) -> torch.Tensor:
    assert x.is_contiguous() and x.numel() == B * S * H * D
    out = torch.empty((B, H, S, D) if to_head else (B, S, H, D), device=x.device, dtype=x.dtype)
    L.check(lib.dxa_permute_bshd(_ptr(x), _ptr(out), B, S, H, D, int(to_head), dt(x), _stream()), "dxa_permute_bshd")
    return out


def splice_fwd(plan: torch.Tensor, embed: torch.Tensor, img: Optional[torch.Tensor]) -> torch.Tensor:
    assert plan.dtype == torch.int64 and plan.is_contiguous() and embed.is_contiguous()
    n, d = plan.numel(), embed.shape[1]
    out = torch.empty((n, d), device=embed.device, dtype=embed.dtype)
    L.check(lib.dxa_splice_fwd(_ptr(plan), _ptr(embed), _ptr(img), _ptr(out), n, d, dt(embed), _stream()),
            "dxa_splice_fwd")
    return out


def splice_bwd(plan: torch.Tensor, dout: torch.Tensor, d_embed: Optional[torch.Tensor],
               d_img: Optional[torch.Tensor]) -> None:
    n, d = dout.shape
    assert dout.is_contiguous() and (d_embed is None or d_embed.dtype == torch.float32)
    L.check(lib.dxa_splice_bwd(_ptr(plan), _ptr(dout), _ptr(d_embed), _ptr(d_img), n, d, dt(dout), _stream()),
            "dxa_splice_bwd")


def zero_rows(plan: torch.Tensor, g: torch.Tensor) -> None:
    """g[plan[r], :] = 0 for every token entry (plan[r] >= 0) of the plan; g fp32 [V, d]"""
    assert plan.dtype == torch.int64 and plan.is_contiguous() and g.dtype == torch.float32 and g.is_contiguous()
    L.check(lib.dxa_zero_rows(_ptr(plan), _ptr(g), plan.numel(), g.shape[1], _stream()), "dxa_zero_rows")


def gather_rows(x: torch.Tensor, idx: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    assert x.is_contiguous() and idx.dtype == torch.int64
    out = torch.empty((idx.numel(), x.shape[1]), device=x.device, dtype=dtype)
    L.check(lib.dxa_gather_rows(_ptr(x), _ptr(idx), _ptr(out), idx.numel(), x.shape[1], dt(x), dt(out), _stream()),
            "dxa_gather_rows")
    return out


def scatter_rows(dout: torch.Tensor, idx: torch.Tensor, R: int, dtype: torch.dtype) -> torch.Tensor:
    assert dout.is_contiguous()
    dx = torch.empty((R, dout.shape[1]), device=dout.device, dtype=dtype)
    L.check(lib.dxa_scatter_rows(_ptr(dout), _ptr(idx), _ptr(dx), idx.numel(), R, dout.shape[1], dt(dout), dt(dx),
                                 _stream()), "dxa_scatter_rows")
    return dx


def im2col(images: torch.Tensor, P: int, ld: int, dtype: torch.dtype) -> torch.Tensor:
    assert images.is_contiguous() and images.dim() == 4 and images.shape[1] == 3
    N, _, H, W = images.shape
    rows = torch.empty((N * (H // P) * (W // P), ld), device=images.device, dtype=dtype)
    L.check(lib.dxa_im2col(_ptr(images), _ptr(rows), N, H, W, P, ld, dt(images), dt(rows), _stream()), "dxa_im2col")
    return rows


def vit_embed_fwd(patch: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, N: int, np_: int) -> torch.Tensor:
    C_ = patch.shape[-1]
    x = torch.empty((N, np_ + 1, C_), device=patch.device, dtype=patch.dtype)
    L.check(lib.dxa_vit_embed_fwd(_ptr(patch), _ptr(cls), _ptr(pos), _ptr(x), N, np_, C_, dt(patch), dt(cls),
                                  _stream()), "dxa_vit_embed_fwd")
    return x


def vit_embed_bwd(dx: torch.Tensor, N: int, np_: int) -> torch.Tensor:
    C_ = dx.shape[-1]
    assert dx.is_contiguous()
    dpatch = torch.empty((N * np_, C_), device=dx.device, dtype=dx.dtype)
    L.check(lib.dxa_vit_embed_bwd(_ptr(dx), _ptr(dpatch), N, np_, C_, dt(dx), _stream()), "dxa_vit_embed_bwd")
    return dpatch


# ------------------------------------------------------------------------- Perception Encoder tower pieces
def rope2d_tables(grid_h: int, grid_w: int, D: int, max_h: int, max_w: int, cls: bool, device, theta: float = 10000.0):
    """fp32 (cos, sin) [T, D] of the reference's Rope2D (pe_model.py:75-128) for a grid_h x grid_w input on a tower whose native
    grid is max_h x max_w: the native table's rows picked at r * max_w + c.  Host-side, once per grid (callers cache it)."""
    half = D // 2
    inv = 1.0 / (theta ** (torch.arange(0, half, 2)[: half // 2].float() / half))
    hr, wr = torch.arange(max_h, dtype=torch.float), torch.arange(max_w, dtype=torch.float)
    if cls:
        hr, wr = hr + 1, wr + 1
    fh = (hr[:, None] * inv[None, :]).repeat_interleave(2, dim=-1)[:, None].expand(max_h, max_w, -1)
    fw = (wr[:, None] * inv[None, :]).repeat_interleave(2, dim=-1)[None, :].expand(max_h, max_w, -1)
    freqs = torch.cat([fw, fh], dim=-1).reshape(max_h * max_w, -1)
    if (grid_h, grid_w) != (max_h, max_w):
        rows = (torch.arange(grid_h).view(-1, 1) * max_w + torch.arange(grid_w).view(1, -1)).reshape(-1)
        freqs = freqs.index_select(0, rows)
    if cls:
        freqs = torch.cat([torch.zeros(1, freqs.shape[-1]), freqs], dim=0)
    return freqs.cos().contiguous().to(device), freqs.sin().contiguous().to(device)


def rope2d_(qkv: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor, N: int, T: int, H: int, D: int, backward: bool = False):
    """in-place 2-D RoPE of the q and k thirds of qkv [N, T, 3, H, D] (``backward``: the transposed rotation, on dqkv)"""
    assert qkv.is_contiguous() and qkv.numel() == N * T * 3 * H * D
    assert cos_t.dtype == torch.float32 and sin_t.dtype == torch.float32 and cos_t.is_contiguous() and sin_t.is_contiguous()
    assert tuple(cos_t.shape) == (T, D) and tuple(sin_t.shape) == (T, D)
    fn = lib.dxa_rope2d_bwd if backward else lib.dxa_rope2d_fwd
    L.check(fn(_ptr(qkv), _ptr(cos_t), _ptr(sin_t), N, T, H, D, dt(qkv), _stream()), "dxa_rope2d_bwd" if backward else "dxa_rope2d_fwd")
    return qkv


def layerscale_residual_fwd(x: torch.Tensor, h: torch.Tensor, gamma: torch.Tensor) -> torch.Tensor:
    """x + gamma[c] * h"""
    x2, h2 = x.reshape(-1, x.shape[-1]), h.reshape(-1, x.shape[-1])
    rows, cols = x2.shape
    assert x2.is_contiguous() and h2.is_contiguous() and h2.shape == x2.shape and h2.dtype == x2.dtype
    assert gamma.is_contiguous() and gamma.numel() == cols and gamma.dtype == x2.dtype
    y = torch.empty_like(x2)
    L.check(lib.dxa_layerscale_residual_fwd(_ptr(x2), _ptr(h2), _ptr(gamma), _ptr(y), rows, cols, dt(x2), _stream()),
            "dxa_layerscale_residual_fwd")
    return y.view(x.shape)


def layerscale_residual_bwd(dy: torch.Tensor, h: torch.Tensor, gamma: torch.Tensor):
    """-> (dh = gamma * dy, partial sums [p, cols] fp32 of dy * h: the caller folds them into dgamma with colsum)"""
    dy2, h2 = dy.reshape(-1, dy.shape[-1]), h.reshape(-1, dy.shape[-1])
    rows, cols = dy2.shape
    assert dy2.is_contiguous() and h2.is_contiguous() and h2.shape == dy2.shape and h2.dtype == dy2.dtype
    assert gamma.is_contiguous() and gamma.numel() == cols and gamma.dtype == dy2.dtype
    dh = torch.empty_like(dy2)
    part = torch.empty((int(lib.dxa_layerscale_bwd_rows(rows)), cols), device=dy.device, dtype=torch.float32)
    L.check(lib.dxa_layerscale_residual_bwd(_ptr(dy2), _ptr(h2), _ptr(gamma), _ptr(dh), _ptr(part), part.numel() * 4, rows, cols,
                                            dt(dy2), _stream()), "dxa_layerscale_residual_bwd")
    return dh.view(dy.shape), part


def conv_out_grid(T: int) -> int:
    """output side of a 3x3 / stride 2 / pad 1 convolution over a T x T grid"""
    return (T - 1) // 2 + 1


def conv3x3s2_im2col(x: torch.Tensor, T: int) -> torch.Tensor:
    """x [B, T*T, C] token-major -> rows [B*To*To, 9*C], column order (c, ky, kx)"""
    assert x.dim() == 3 and x.is_contiguous() and x.shape[1] == T * T
    B, _, C_ = x.shape
    To = conv_out_grid(T)
    rows = torch.empty((B * To * To, 9 * C_), device=x.device, dtype=x.dtype)
    L.check(lib.dxa_conv3x3s2_im2col(_ptr(x), _ptr(rows), B, T, C_, dt(x), _stream()), "dxa_conv3x3s2_im2col")
    return rows


def conv3x3s2_col2im(drows: torch.Tensor, B: int, T: int) -> torch.Tensor:
    """adjoint of conv3x3s2_im2col: drows [B*To*To, 9*C] -> dx [B, T*T, C]"""
    To = conv_out_grid(T)
    assert drows.dim() == 2 and drows.is_contiguous() and drows.shape[0] == B * To * To and drows.shape[1] % 9 == 0
    C_ = drows.shape[1] // 9
    dx = torch.empty((B, T * T, C_), device=drows.device, dtype=drows.dtype)
    L.check(lib.dxa_conv3x3s2_col2im(_ptr(drows), _ptr(dx), B, T, C_, dt(drows), _stream()), "dxa_conv3x3s2_col2im")
    return dx


# ------------------------------------------------------------------------------------- diffusion glue
def qsample(x0, noise, a, s):
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (x0, noise, a, s))
    xt = torch.empty_like(x0)
    N = x0.shape[0]
    L.check(lib.dxa_qsample(_ptr(x0), _ptr(noise), _ptr(a), _ptr(s), _ptr(xt), N, x0.numel() // N, _stream()),
            "dxa_qsample")
    return xt


def timestep_embedding(t: torch.Tensor, freqs: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.float32 and freqs.dtype == torch.float32
    half = freqs.numel()
    out = torch.empty((t.numel(), 2 * half), device=t.device, dtype=torch.float32)
    L.check(lib.dxa_timestep_embedding(_ptr(t), _ptr(freqs), _ptr(out), t.numel(), half, _stream()),
            "dxa_timestep_embedding")
    return out


def dit_assemble_fwd(xe, te, ze, pos):
    N, T, hd = xe.shape
    h = torch.empty((N, T + 1, hd), device=xe.device, dtype=torch.float32)
    L.check(lib.dxa_dit_assemble_fwd(_ptr(xe), _ptr(te), _ptr(ze), _ptr(pos), _ptr(h), N, T, hd, _stream()),
            "dxa_dit_assemble_fwd")
    return h


def dit_assemble_bwd(dh):
    N, T1, hd = dh.shape
    assert dh.is_contiguous()
    dxe = torch.empty((N, T1 - 1, hd), device=dh.device, dtype=torch.float32)
    dc = torch.empty((N, hd), device=dh.device, dtype=torch.float32)
    L.check(lib.dxa_dit_assemble_bwd(_ptr(dh), _ptr(dxe), _ptr(dc), N, T1 - 1, hd, _stream()), "dxa_dit_assemble_bwd")
    return dxe, dc


def token_drop(z, uncond, drop):
    N, d = z.shape
    assert drop.dtype == torch.uint8 and z.is_contiguous()
    out = torch.empty_like(z)
    L.check(lib.dxa_token_drop(_ptr(z), _ptr(uncond), _ptr(drop), _ptr(out), N, d, _stream()), "dxa_token_drop")
    return out


def token_drop_bwd(dout, drop, want_dz=True):
    N, d = dout.shape
    assert dout.is_contiguous()
    dz = torch.empty_like(dout) if want_dz else None
    dunc = torch.empty(d, device=dout.device, dtype=torch.float32)
    L.check(lib.dxa_token_drop_bwd(_ptr(dout), _ptr(drop), _ptr(dz), _ptr(dunc), N, d, 0, _stream()),
            "dxa_token_drop_bwd")
    return dz, dunc


def mse_loss(pred, target, gscale: float = 1.0, want_grad: bool = True):
    assert pred.is_contiguous() and target.is_contiguous() and pred.dtype == torch.float32
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred) if want_grad else None
    L.check(lib.dxa_mse_loss(_ptr(pred), _ptr(target), _ptr(loss), _ptr(dpred), pred.numel(), gscale, _stream()),
            "dxa_mse_loss")
    return loss, dpred


def mse_loss_rows(pred, target, row_w, gscale: float = 1.0, want_grad: bool = True):
    """sum_r w_r mean_c(d^2) / (sum w + 1e-6) over pred/target [rows, ...]; row_w [rows] fp32"""
    assert pred.is_contiguous() and target.is_contiguous() and pred.dtype == torch.float32
    rows = pred.shape[0]
    assert row_w.dtype == torch.float32 and row_w.is_contiguous() and row_w.numel() == rows
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred) if want_grad else None
    L.check(lib.dxa_mse_loss_rows(_ptr(pred), _ptr(target), _ptr(row_w), _ptr(loss), _ptr(dpred), rows,
                                  pred.numel() // rows, gscale, _stream()), "dxa_mse_loss_rows")
    return loss, dpred


def expectile_loss(pred, target, tau: float, gscale: float = 1.0, want_grad: bool = True):
    """mean(w d^2), w = tau where d = pred - target < 0 and 1 - tau elsewhere -> (loss [1], dpred or None)"""
    assert pred.is_contiguous() and target.is_contiguous() and pred.dtype == torch.float32 and target.dtype == torch.float32
    assert pred.numel() == target.numel()
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred) if want_grad else None
    L.check(lib.dxa_expectile_loss(_ptr(pred), _ptr(target), _ptr(loss), _ptr(dpred), pred.numel(), float(tau), gscale,
                                   _stream()), "dxa_expectile_loss")
    return loss, dpred


def ddim_step(x, model_out, B, use_cfg, cfg_scale, c_recip, c_recipm1, ab_prev):
    per = x.numel() // x.shape[0]
    L.check(lib.dxa_ddim_step(_ptr(x), _ptr(model_out), B, per, int(use_cfg), cfg_scale, c_recip, c_recipm1, ab_prev,
                              _stream()), "dxa_ddim_step")
    return x


# --------------------------------------------------------------------------------------------- optimizer
def sumsq(x: torch.Tensor, out: torch.Tensor, scratch: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    assert x.is_contiguous() and scratch.dtype == torch.float64 and scratch.numel() >= 4096
    L.check(lib.dxa_sumsq(_ptr(x), x.numel(), dt(x), _ptr(scratch), _ptr(out), int(accumulate), _stream()), "dxa_sumsq")
    return out


def sumsq_ranges(base: torch.Tensor, starts: torch.Tensor, lens: torch.Tensor, out: torch.Tensor, scratch: torch.Tensor,
                 accumulate: bool = False) -> torch.Tensor:
    """out (+)= sum over the slices base[starts[i] : starts[i] + lens[i]] of x^2 (int64 device arrays, <= 4096 slices)"""
    assert base.is_contiguous() and starts.dtype == torch.int64 and lens.dtype == torch.int64 and starts.numel() == lens.numel()
    assert scratch.dtype == torch.float64 and scratch.numel() >= 4096
    L.check(lib.dxa_sumsq_ranges(_ptr(base), dt(base), _ptr(starts), _ptr(lens), starts.numel(), _ptr(scratch), _ptr(out),
                                 int(accumulate), _stream()), "dxa_sumsq_ranges")
    return out


def sum_f32(x: torch.Tensor, out: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    assert x.is_contiguous() and x.dtype == torch.float32 and out.dtype == torch.float32
    L.check(lib.dxa_sum_f32(_ptr(x), x.numel(), _ptr(out), int(accumulate), _stream()), "dxa_sum_f32")
    return out


def gemm_sumsq_slots(M: int, N: int) -> int:
    return int(lib.dxa_gemm_sumsq_slots(M, N))


def clip_coef(sumsq_t, max_norm: float, norm_out, coef_out, grad_scale: float = 1.0):
    if grad_scale == 1.0:
        L.check(lib.dxa_clip_coef(_ptr(sumsq_t), max_norm, _ptr(norm_out), _ptr(coef_out), _stream()), "dxa_clip_coef")
    else:
        L.check(lib.dxa_clip_coef_scaled(_ptr(sumsq_t), max_norm, grad_scale, _ptr(norm_out), _ptr(coef_out), _stream()),
                "dxa_clip_coef_scaled")


def scale_(x: torch.Tensor, s: float) -> torch.Tensor:
    assert x.dtype == torch.float32 and x.is_contiguous()
    L.check(lib.dxa_scale(_ptr(x), x.numel(), s, _stream()), "dxa_scale")
    return x


def scale_dev_(x: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """x *= s[0], s a device fp32 scalar"""
    assert x.dtype == torch.float32 and x.is_contiguous() and s.dtype == torch.float32 and s.numel() == 1
    L.check(lib.dxa_scale_dev(_ptr(x), x.numel(), _ptr(s), _stream()), "dxa_scale_dev")
    return x


def adamw(p, g, m, v, shadow, chunk_start, chunk_len, chunk_grp, lrs, wds, beta1, beta2, eps, step, clip=None, chunk_state=None,
          chunk_mv_start=None):
    """``chunk_mv_start``: m / v are PACKED (the sharded optimizer state of engine.FusedAdamW(ranges=...)): chunk c's moments start
    at element chunk_mv_start[c] of m and v; p, g and shadow keep the arena offset chunk_start[c]"""
    d = L.AdamWDesc()
    if chunk_mv_start is not None:
        assert chunk_mv_start.dtype == torch.int64 and chunk_mv_start.numel() == chunk_start.numel() and chunk_mv_start.is_contiguous()
    d.chunk_mv_start = _ptr(chunk_mv_start)
    if chunk_state is not None:
        assert chunk_state.dtype == torch.uint8 and chunk_state.numel() == chunk_start.numel() and chunk_state.is_contiguous()
    d.chunk_state = _ptr(chunk_state)
    d.p, d.g, d.m, d.v, d.shadow = _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(shadow)
    d.g_dtype = dt(g)
    d.chunk_start, d.chunk_len, d.chunk_grp = _ptr(chunk_start), _ptr(chunk_len), _ptr(chunk_grp)
    d.n_chunks = chunk_start.numel()
    assert len(lrs) <= 8 and len(lrs) == len(wds)
    for i, (lr, wd) in enumerate(zip(lrs, wds)):
        d.lr[i], d.wd[i] = lr, wd
    d.beta1, d.beta2, d.eps = beta1, beta2, eps
    d.bc1, d.bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    d.clip_coef = _ptr(clip)
    L.check(lib.dxa_adamw(C.byref(d), _stream()), "dxa_adamw")


# ------------------------------------------------------------------------------------- LM head (row A10)
def cross_entropy_fwd(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100):
    """logits [rows, V] (fp32/bf16, rows contiguous), labels [rows] int64 (already shifted) ->
    (row_loss [rows] fp32, lse [rows] fp32)"""
    rows, V = logits.shape
    assert logits.stride(1) == 1 and labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == rows
    row_loss = torch.empty(rows, device=logits.device, dtype=torch.float32)
    lse = torch.empty(rows, device=logits.device, dtype=torch.float32)
    L.check(lib.dxa_cross_entropy_fwd(_ptr(logits), logits.stride(0), _ptr(labels), _ptr(row_loss), _ptr(lse), rows, V,
                                      ignore_index, dt(logits), _stream()), "dxa_cross_entropy_fwd")
    return row_loss, lse


def cross_entropy_bwd(logits: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor, gscale: Optional[torch.Tensor],
                      scale: float, out: Optional[torch.Tensor] = None, ignore_index: int = -100) -> torch.Tensor:
    """dlogits = (softmax - onehot) * gscale[0] * scale; ``out`` may be ``logits`` itself (in place)"""
    rows, V = logits.shape
    if out is None:
        out = torch.empty_like(logits)
    assert out.shape == logits.shape and out.dtype == logits.dtype and out.stride(1) == 1
    L.check(lib.dxa_cross_entropy_bwd(_ptr(logits), logits.stride(0), _ptr(labels), _ptr(lse), _ptr(gscale), float(scale),
                                      _ptr(out), out.stride(0), rows, V, ignore_index, dt(logits), _stream()),
            "dxa_cross_entropy_bwd")
    return out


def cross_entropy_rows_bwd(logits: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor, gscale: Optional[torch.Tensor],
                           scale: float, row_w: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
                           ignore_index: int = -100) -> torch.Tensor:
    """dlogits = (softmax - onehot) * row_w[r] * gscale[0] * scale; ``row_w`` [rows] fp32 (None: cross_entropy_bwd's result)"""
    rows, V = logits.shape
    if out is None:
        out = torch.empty_like(logits)
    assert out.shape == logits.shape and out.dtype == logits.dtype and out.stride(1) == 1
    if row_w is not None:
        assert row_w.dtype == torch.float32 and row_w.is_contiguous() and row_w.numel() == rows
    L.check(lib.dxa_cross_entropy_rows_bwd(_ptr(logits), logits.stride(0), _ptr(labels), _ptr(lse), _ptr(gscale), float(scale),
                                           _ptr(row_w), _ptr(out), out.stride(0), rows, V, ignore_index, dt(logits), _stream()),
            "dxa_cross_entropy_rows_bwd")
    return out


def ce_sample_reduce(row_loss: torch.Tensor, labels: torch.Tensor, reward: Optional[torch.Tensor], B: int, V: int,
                     ignore_index: int = -100):
    """row_loss / labels [B*L] (cross_entropy_fwd's), reward [B] fp32 on the device or None -> (loss [1], row_w [B*L]):
    loss = mean_b w_b sum_t row_loss[b, t] / max(n_b, 1), row_w[b, t] = w_b / (max(n_b, 1) B), w_b = 1 + sigmoid(reward_b) or 1"""
    assert row_loss.dtype == torch.float32 and row_loss.is_contiguous() and labels.dtype == torch.int64 and labels.is_contiguous()
    n = row_loss.numel()
    assert labels.numel() == n and B > 0 and n % B == 0
    if reward is not None:
        assert reward.dtype == torch.float32 and reward.is_contiguous() and reward.numel() == B and reward.device == row_loss.device
    loss = torch.empty(1, device=row_loss.device, dtype=torch.float32)
    row_w = torch.empty(n, device=row_loss.device, dtype=torch.float32)
    L.check(lib.dxa_ce_sample_reduce(_ptr(row_loss), _ptr(labels), _ptr(reward), _ptr(row_w), _ptr(loss), B, n // B, V,
                                     ignore_index, _stream()), "dxa_ce_sample_reduce")
    return loss, row_w


class SoftTokens:
    """the K soft ("time") token ids of the soft-target cross-entropy, on the host (checked by every call) and on the device, with
    1 / (2 std^2).  Duplicate ids are refused: the reference's result for them is an accident of write order."""

    def __init__(self, ids: Sequence[int], std: float, device):
        ids = [int(i) for i in ids]
        if len(set(ids)) != len(ids):
            raise ValueError(f"soft token ids must be distinct, got {ids}")
        if not float(std) > 0.0:
            raise ValueError(f"soft-target std must be positive, got {std}")
        self.K = len(ids)
        self.host = (C.c_int64 * max(self.K, 1))(*ids)
        self.dev = torch.tensor(ids, dtype=torch.int64, device=device) if self.K else None
        self.inv2s2 = 1.0 / (2.0 * float(std) ** 2)


def soft_cross_entropy_fwd(logits: torch.Tensor, labels: torch.Tensor, soft: SoftTokens, ignore_index: int = -100):
    """cross_entropy_fwd with Gaussian soft targets over ``soft``'s ids for the rows labelled with one of them"""
    rows, V = logits.shape
    assert logits.stride(1) == 1 and labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == rows
    row_loss = torch.empty(rows, device=logits.device, dtype=torch.float32)
    lse = torch.empty(rows, device=logits.device, dtype=torch.float32)
    L.check(lib.dxa_soft_cross_entropy_fwd(_ptr(logits), logits.stride(0), _ptr(labels), _ptr(row_loss), _ptr(lse), rows, V,
                                           ignore_index, _ptr(soft.dev), C.cast(soft.host, C.c_void_p) if soft.K else None,
                                           soft.K, soft.inv2s2, dt(logits), _stream()), "dxa_soft_cross_entropy_fwd")
    return row_loss, lse


def soft_cross_entropy_bwd(logits: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor, gscale: Optional[torch.Tensor],
                           scale: float, soft: SoftTokens, out: Optional[torch.Tensor] = None,
                           ignore_index: int = -100) -> torch.Tensor:
    """dlogits = (softmax - target) * gscale[0] * scale, target = one-hot or the soft row; ``out`` may be ``logits`` itself"""
    rows, V = logits.shape
    if out is None:
        out = torch.empty_like(logits)
    assert out.shape == logits.shape and out.dtype == logits.dtype and out.stride(1) == 1
    L.check(lib.dxa_soft_cross_entropy_bwd(_ptr(logits), logits.stride(0), _ptr(labels), _ptr(lse), _ptr(gscale), float(scale),
                                           _ptr(out), out.stride(0), rows, V, ignore_index, _ptr(soft.dev),
                                           C.cast(soft.host, C.c_void_p) if soft.K else None, soft.K, soft.inv2s2,
                                           dt(logits), _stream()), "dxa_soft_cross_entropy_bwd")
    return out


def argmax_rows(x: torch.Tensor) -> torch.Tensor:
    """first index of each row's maximum (torch.argmax semantics) -> int64 [rows]"""
    rows, cols = x.shape
    assert x.stride(1) == 1
    out = torch.empty(rows, device=x.device, dtype=torch.int64)
    L.check(lib.dxa_argmax_rows(_ptr(x), x.stride(0), _ptr(out), rows, cols, dt(x), _stream()), "dxa_argmax_rows")
    return out


def sample_rows(logits: torch.Tensor, u: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                return_info: bool = False):
    """one token per row drawn from softmax(logits / temperature) after HF's top-k (0 = off) and top-p (1 = off) warpers, with the
    uniform ``u[r]`` in [0, 1) deciding row r's draw -> int64 [rows]; ``return_info``: (token, kept int32 = size of the kept
    set, thresh fp32 = its smallest logit, prob fp32 = probability of the token).  Semantics: include/dexbotic_amd.h"""
    if not temperature > 0:
        raise ValueError(f"sample_rows: temperature {temperature!r} must be positive")
    if not 0 < top_p <= 1:
        raise ValueError(f"sample_rows: top_p {top_p!r} outside (0, 1]")
    rows, V = logits.shape
    assert logits.stride(1) == 1
    assert u.dtype == torch.float32 and u.is_contiguous() and u.numel() == rows and u.device == logits.device
    token = torch.empty(rows, device=logits.device, dtype=torch.int64)
    kept = thresh = prob = None
    if return_info:
        kept = torch.empty(rows, device=logits.device, dtype=torch.int32)
        thresh = torch.empty(rows, device=logits.device, dtype=torch.float32)
        prob = torch.empty(rows, device=logits.device, dtype=torch.float32)
    L.check(lib.dxa_sample_rows(_ptr(logits), logits.stride(0), rows, V, dt(logits), float(temperature), int(top_k), float(top_p),
                                _ptr(u), _ptr(token), _ptr(kept), _ptr(thresh), _ptr(prob), _stream()), "dxa_sample_rows")
    return (token, kept, thresh, prob) if return_info else token


# ------------------------------------------------------------------------------------------------ image preprocessing
_RESAMPLE_TABLES: dict = {}


def resample_tables(in_size: int, out_size: int, device) -> Tuple[int, "torch.Tensor", "torch.Tensor", "torch.Tensor"]:
    """Pillow bicubic tap tables of one axis: (ksize, bounds host int32 [out,2], bounds device, taps device [out,ksize]);
    built once per (in_size, out_size, device) by the library's host routine and kept on the device"""
    key = (int(in_size), int(out_size), str(device))
    hit = _RESAMPLE_TABLES.get(key)
    if hit is None:
        ks = lib.dxa_resample_ksize(int(in_size), int(out_size))
        bounds = torch.empty(out_size, 2, dtype=torch.int32)
        taps = torch.empty(out_size, ks, dtype=torch.int32)
        L.check(lib.dxa_resample_coeffs(int(in_size), int(out_size), L.FILTER_BICUBIC, bounds.data_ptr(), taps.data_ptr()),
                "dxa_resample_coeffs")
        hit = (ks, bounds, bounds.to(device), taps.to(device))
        _RESAMPLE_TABLES[key] = hit
    return hit


def resize_output_size(h: int, w: int, shortest_edge: int) -> Tuple[int, int]:
    """(out_h, out_w) of the processor's shortest-edge resize: long side = int(shortest_edge * long / short)"""
    if w <= h:
        return int(shortest_edge * h / w), shortest_edge
    return shortest_edge, int(shortest_edge * w / h)


def image_preprocess(frames: torch.Tensor, *, pad: bool, bg: Sequence[int], size: int, crop: Tuple[int, int],
                     mean: Sequence[float], std: Sequence[float], rescale: float = 1 / 255,
                     out_dtype: torch.dtype = torch.float32, want_u8: bool = False):
    """uint8 RGB frames [n, h, w, 3] on the device -> [n, 3, crop_h, crop_w] (expand2square, Pillow-exact bicubic
    shortest-edge resize, center crop, rescale, normalise).  With want_u8 also returns the uint8 resized frame."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise L.DxaError(f"image_preprocess: expected contiguous uint8 [n,h,w,3], got {frames.dtype} {tuple(frames.shape)}")
    n, h, w, _ = frames.shape
    ph, pw = (max(h, w), max(h, w)) if pad else (h, w)
    res_h, res_w = resize_output_size(ph, pw, size)
    ch, cw = crop
    if ch > res_h or cw > res_w:
        raise L.DxaError(f"image_preprocess: crop {crop} larger than the resized frame {(res_h, res_w)}")
    top, left = (res_h - ch) // 2, (res_w - cw) // 2
    dev = frames.device
    d = L.ImageDesc()
    d.src, d.n, d.h, d.w, d.pad = _ptr(frames), n, h, w, int(bool(pad))
    for i in range(3):
        d.bg[i] = int(bg[i])
        d.mean[i] = float(mean[i])
        d.std[i] = float(std[i])
    d.res_h, d.res_w, d.crop_top, d.crop_left, d.out_h, d.out_w = res_h, res_w, top, left, ch, cw
    keep = []
    if res_w != pw:
        d.hks, _, hb, hk = resample_tables(pw, res_w, dev)
        d.hb, d.hk = _ptr(hb), _ptr(hk)
        keep += [hb, hk]
    row0, rows = top, ch
    if res_h != ph:
        d.vks, vb_host, vb, vk = resample_tables(ph, res_h, dev)
        d.vb, d.vk = _ptr(vb), _ptr(vk)
        keep += [vb, vk]
        win = vb_host[top:top + ch]
        row0 = int(win[:, 0].min())
        rows = int((win[:, 0] + win[:, 1]).max()) - row0
    d.row0, d.rows = row0, rows
    tmp = torch.empty(n * rows * cw * 3, device=dev, dtype=torch.uint8)
    out = torch.empty(n, 3, ch, cw, device=dev, dtype=out_dtype)
    u8 = torch.empty(n, ch, cw, 3, device=dev, dtype=torch.uint8) if want_u8 else None
    d.tmp, d.out, d.out_dtype, d.out_u8, d.rescale = _ptr(tmp), _ptr(out), dt(out), _ptr(u8), float(rescale)
    L.check(lib.dxa_image_preprocess(C.byref(d), _stream()), "dxa_image_preprocess")
    return (out, u8) if want_u8 else out


# ------------------------------------------------------------------------------------------------ training augmentations
_BILINEAR_TABLES: dict = {}


def bilinear_tables(in_size: int, out_size: int):
    """Pillow bilinear tap tables of one axis on the host: (ksize, bounds int32 [out,2], taps int32 [out,ksize])"""
    key = (int(in_size), int(out_size))
    hit = _BILINEAR_TABLES.get(key)
    if hit is None:
        ks = lib.dxa_resample_ksize_filter(key[0], key[1], L.FILTER_BILINEAR)
        bounds = np.zeros((out_size, 2), np.int32)
        taps = np.zeros((out_size, ks), np.int32)
        L.check(lib.dxa_resample_coeffs(key[0], key[1], L.FILTER_BILINEAR, bounds.ctypes.data, taps.ctypes.data), "dxa_resample_coeffs")
        hit = _BILINEAR_TABLES[key] = (ks, bounds, taps)
    return hit


def _check_u8_frames(frames, who):
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 \
            or not frames.is_contiguous():
        raise L.DxaError(f"{who}: expected contiguous uint8 [n,h,w,3], got {getattr(frames, 'dtype', type(frames))} "
                         f"{tuple(getattr(frames, 'shape', ()))}")


def image_crop_resize(frames: torch.Tensor, boxes, size: int, *, pad: bool = False, bg: Sequence[int] = (0, 0, 0)) -> torch.Tensor:
    """uint8 frames [n, h, w, 3] on the device -> uint8 [n, size, size, 3]: frame i's square box boxes[i] = (x0, y0, c) of
    the (expand2square-padded when `pad`) frame, cropped and resized as Pillow's crop().resize(BILINEAR)"""
    _check_u8_frames(frames, "image_crop_resize")
    n, h, w, _ = frames.shape
    boxes = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 3))
    if boxes.shape[0] != n:
        raise L.DxaError(f"image_crop_resize: {n} frames but {boxes.shape[0]} boxes")
    size = int(size)
    dev = frames.device
    out = torch.empty(n, size, size, 3, device=dev, dtype=torch.uint8)
    if n == 0:
        return out
    if size <= 0 or int(boxes[:, 2].min()) <= 0:
        raise L.DxaError(f"image_crop_resize: sides must be positive (size {size}, smallest box {int(boxes[:, 2].min())})")
    sides, which = np.unique(boxes[:, 2], return_inverse=True)          # one table per distinct crop side
    tabs = [bilinear_tables(int(c), size) for c in sides]
    ks = max(t[0] for t in tabs)
    bounds = np.stack([t[1] for t in tabs])
    taps = np.zeros((len(tabs), size, ks), np.int32)
    for j, t in enumerate(tabs):
        taps[j, :, :t[0]] = t[2]
    boxes4 = np.ascontiguousarray(np.concatenate([boxes, which.reshape(-1, 1).astype(np.int32)], 1))
    sides = np.ascontiguousarray(sides.astype(np.int32))
    cmax = int(sides.max())
    d_boxes, d_bounds, d_taps = (torch.from_numpy(a).to(dev) for a in (boxes4, bounds, taps))
    tmp = torch.empty(n * cmax * size * 3, device=dev, dtype=torch.uint8)
    bg_rgb = int(bg[0]) | (int(bg[1]) << 8) | (int(bg[2]) << 16)
    L.check(lib.dxa_image_crop_resize(_ptr(frames), n, h, w, int(bool(pad)), bg_rgb, _ptr(d_boxes), boxes4.ctypes.data, size,
                                      _ptr(d_bounds), _ptr(d_taps), sides.ctypes.data, len(tabs), ks, _ptr(tmp), cmax, _ptr(out),
                                      _stream()), "dxa_image_crop_resize")
    return out


JITTER_DTYPE = np.dtype([("apply", np.int32), ("order", np.int32, 4), ("brightness", np.float32), ("contrast", np.float32),
                         ("saturation", np.float32), ("hue", np.float32)])


def image_color_jitter(frames: torch.Tensor, apply, order, factors, hue) -> torch.Tensor:
    """ColorJitter in place on uint8 frames [n, h, w, 3] on the device, one parameter row per frame: apply [n], order [n,4]
    (a permutation of brightness 0, contrast 1, saturation 2, hue 3), factors [n,3], hue [n] in turns.  Frames with
    apply == 0 are not touched.  Pillow's ImageEnhance / HSV arithmetic, bit for bit."""
    _check_u8_frames(frames, "image_color_jitter")
    n, h, w, _ = frames.shape
    tab = np.zeros(n, JITTER_DTYPE)
    tab["apply"], tab["order"], tab["hue"] = np.asarray(apply).reshape(n), np.asarray(order).reshape(n, 4), np.asarray(hue).reshape(n)
    f = np.asarray(factors, np.float32).reshape(n, 3)
    tab["brightness"], tab["contrast"], tab["saturation"] = f[:, 0], f[:, 1], f[:, 2]
    if n == 0 or not tab["apply"].any():
        return frames
    d_tab = torch.from_numpy(tab.view(np.uint8)).to(frames.device)
    sums = torch.empty(n, device=frames.device, dtype=torch.int64)
    L.check(lib.dxa_color_jitter(_ptr(frames), n, h, w, _ptr(d_tab), tab.ctypes.data, _ptr(sums), _stream()), "dxa_color_jitter")
    return frames


def image_affine(frames: torch.Tensor, mats, fill: Sequence[int] = (0, 0, 0)) -> torch.Tensor:
    """uint8 frames [n, h, w, 3] on the device -> a new tensor of the same shape: frame i warped by its INVERSE matrix mats[i]
    (6 doubles: output pixel (x, y) reads the source at m0 (x + .5) + m1 (y + .5) + m2, m3 (x + .5) + m4 (y + .5) + m5), bilinear,
    `fill` where the source lies outside the frame.  Pillow's Image.transform(size, AFFINE, m, BILINEAR, fillcolor), bit for bit."""
    _check_u8_frames(frames, "image_affine")
    n, h, w, _ = frames.shape
    mats = np.ascontiguousarray(np.asarray(mats, np.float64).reshape(-1, 6))
    if mats.shape[0] != n:
        raise L.DxaError(f"image_affine: {n} frames but {mats.shape[0]} matrices")
    out = torch.empty_like(frames)
    if n == 0:
        return out
    d_mats = torch.from_numpy(mats).to(frames.device)
    fill_rgb = (int(fill[0]) & 255) | ((int(fill[1]) & 255) << 8) | ((int(fill[2]) & 255) << 16)
    L.check(lib.dxa_image_affine(_ptr(frames), _ptr(out), n, h, w, _ptr(d_mats), mats.ctypes.data, fill_rgb, _stream()),
            "dxa_image_affine")
    return out


def rotate_matrix(angle_deg: float, h: int, w: int):
    """the inverse matrix Pillow's Image.rotate(angle) hands to transform() for a w x h image, in Python floats: the angle
    mod 360, cos and sin rounded to 15 places, the centre (w / 2, h / 2) mapped onto itself"""
    a = -math.radians(float(angle_deg) % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def image_rotate(frames: torch.Tensor, angles_deg, fill: Sequence[int] = (0, 0, 0)) -> torch.Tensor:
    """uint8 frames [n, h, w, 3] on the device -> a new tensor: frame i rotated by angles_deg[i] degrees counter-clockwise about
    its centre, as Pillow's Image.rotate(angle, BILINEAR, fillcolor=fill)"""
    _check_u8_frames(frames, "image_rotate")
    n, h, w, _ = frames.shape
    angles = np.asarray(angles_deg, np.float64).reshape(-1)
    if angles.shape[0] != n:
        raise L.DxaError(f"image_rotate: {n} frames but {angles.shape[0]} angles")
    return image_affine(frames, np.asarray([rotate_matrix(float(a), h, w) for a in angles], np.float64).reshape(n, 6), fill)


# ------------------------------------------------------------------------------------------------ fused DiT blocks
DIT_FUSED_MAX_ROWS, DIT_FUSED_MAX_TOKENS = 47, 32


def dit_blocks_supported(N: int, T1: int, H: int, heads: int, I: int) -> bool:
    return (N * T1 <= DIT_FUSED_MAX_ROWS and T1 <= DIT_FUSED_MAX_TOKENS and H == heads * 64 and H <= 1024 and I % 64 == 0)


def dit_blocks_fwd(h: torch.Tensor, weight_table: torch.Tensor, depth: int, N: int, T1: int, H: int, heads: int, I: int,
                   eps: float) -> torch.Tensor:
    """all DiT blocks of one denoising call in one launch; h [N*T1, H] fp32 is updated in place.  ``weight_table`` is an
    int64 device tensor of depth*8 raw fp32 pointers (qkv_w, qkv_b, proj_w, proj_b, fc1_w, fc1_b, fc2_w, fc2_b per block)"""
    assert h.dtype == torch.float32 and h.is_contiguous() and h.shape == (N * T1, H)
    assert weight_table.dtype == torch.int64 and weight_table.numel() == depth * 8 and weight_table.is_cuda
    nbytes = lib.dxa_dit_blocks_workspace(N * T1, H, I)
    ws = torch.empty(nbytes, device=h.device, dtype=torch.uint8)
    L.check(lib.dxa_dit_blocks_fwd(_ptr(h), _ptr(weight_table), depth, N, T1, H, heads, I, float(eps), _ptr(ws), nbytes,
                                   _stream()), "dxa_dit_blocks_fwd")
    return h


def dit_sample_fwd(x: torch.Tensor, z_emb: torch.Tensor, t_emb: torch.Tensor, pos: torch.Tensor, x_w: torch.Tensor, x_b: torch.Tensor,
                   final_w: torch.Tensor, final_b: torch.Tensor, coef: torch.Tensor, nb: int, use_cfg: bool, cfg_scale: float,
                   weight_table: torch.Tensor, depth: int, T1: int, H: int, heads: int, I: int, eps: float) -> torch.Tensor:
    """the whole DDIM sampler in one persistent launch (dxa_dit_sample_fwd); x [nb, T1-1, A] fp32 is updated in place"""
    steps, A = t_emb.shape[0], x.shape[-1]
    N = z_emb.shape[0]
    for t in (x, z_emb, t_emb, pos, x_w, x_b, final_w, final_b, coef):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
    assert x.shape == (nb, T1 - 1, A) and z_emb.shape == (N, H) and t_emb.shape == (steps, H) and coef.shape == (steps, 4)
    assert pos.shape == (T1, H) and x_w.shape == (H, A) and final_w.shape == (A, H)
    nbytes = lib.dxa_dit_sample_workspace(N * T1, H, I)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    L.check(lib.dxa_dit_sample_fwd(_ptr(x), _ptr(z_emb), _ptr(t_emb), _ptr(pos), _ptr(x_w), _ptr(x_b), _ptr(final_w), _ptr(final_b),
                                   _ptr(coef), steps, A, nb, int(use_cfg), float(cfg_scale), _ptr(weight_table), depth, N, T1, H,
                                   heads, I, float(eps), _ptr(ws), nbytes, _stream()), "dxa_dit_sample_fwd")
    return x


def dit_bf16_pack(weight_table: torch.Tensor, depth: int, H: int, I: int, out=None, per: bool = False):
    """bf16 operand copy of the DiT blocks' matrices for dit_sample_bf16_fwd (dxa_dit_bf16_pack): returns (arena, table) — keep both
    alive; `table` is the int64 device tensor of depth*10 pointers the sampler takes.  Re-pack when the fp32 weights change
    (``out=(arena, table)`` re-packs in place).  ``per``: the blocks of MemVLA's DiT with perceptual attention (dxa_dit_bf16_pack_per:
    14 source pointers and 16 table entries per block)."""
    n_src, n_tab = (14, 16) if per else (8, 10)
    assert weight_table.dtype == torch.int64 and weight_table.numel() == depth * n_src and weight_table.is_cuda
    nbytes = (lib.dxa_dit_bf16_pack_per_bytes if per else lib.dxa_dit_bf16_pack_bytes)(depth, H, I)
    if out is not None:
        arena, table = out
        assert arena.numel() == nbytes and table.numel() == depth * n_tab
    else:
        arena = torch.empty(nbytes, device=weight_table.device, dtype=torch.uint8)
        table = torch.empty(depth * n_tab, device=weight_table.device, dtype=torch.int64)
    fn = lib.dxa_dit_bf16_pack_per if per else lib.dxa_dit_bf16_pack
    L.check(fn(_ptr(weight_table), depth, H, I, _ptr(arena), nbytes, _ptr(table), _stream()), "dxa_dit_bf16_pack")
    return arena, table


def dit_sample_bf16_supported(N: int, T1: int, H: int, heads: int, I: int, P: int = 0) -> bool:
    """``P``: perceptual keys per sample (MemVLA's DiT; 0 = the plain blocks)"""
    return (N * T1 <= 48 and T1 <= DIT_FUSED_MAX_TOKENS and H == heads * 64 and H <= 1024 and H % 64 == 0 and I % 64 == 0 and
            (P == 0 or (P % 64 == 0 and 64 <= P <= 256 and T1 <= 24)))


def dit_sample_bf16_fwd(x: torch.Tensor, z_emb: torch.Tensor, t_emb: torch.Tensor, pos: torch.Tensor, x_w: torch.Tensor,
                        x_b: torch.Tensor, final_w: torch.Tensor, final_b: torch.Tensor, coef: torch.Tensor, nb: int, use_cfg: bool,
                        cfg_scale: float, packed_table: torch.Tensor, depth: int, T1: int, H: int, heads: int, I: int,
                        eps: float, per_kv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dit_sample_fwd with bf16 MFMA operands (dxa_dit_sample_bf16_fwd; `packed_table` from dit_bf16_pack): the sampler of a model
    served in bfloat16; x [nb, T1-1, A] fp32 is updated in place.  ``per_kv`` [depth, N, P, 2, H] fp32: MemVLA's perceptual attention
    (dxa_dit_sample_bf16_per_fwd; `packed_table` from dit_bf16_pack(per=True))."""
    steps, A = t_emb.shape[0], x.shape[-1]
    N = z_emb.shape[0]
    for t in (x, z_emb, t_emb, pos, x_w, x_b, final_w, final_b, coef):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
    assert x.shape == (nb, T1 - 1, A) and z_emb.shape == (N, H) and t_emb.shape == (steps, H) and coef.shape == (steps, 4)
    assert pos.shape == (T1, H) and x_w.shape == (H, A) and final_w.shape == (A, H)
    assert packed_table.dtype == torch.int64 and packed_table.numel() == depth * (10 if per_kv is None else 16) and packed_table.is_cuda
    nbytes = lib.dxa_dit_sample_bf16_workspace(N * T1, H, I)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    if per_kv is not None:
        P_ = per_kv.shape[2]
        assert per_kv.dtype == torch.float32 and per_kv.is_contiguous() and per_kv.shape == (depth, N, P_, 2, H)
        L.check(lib.dxa_dit_sample_bf16_per_fwd(_ptr(x), _ptr(z_emb), _ptr(t_emb), _ptr(pos), _ptr(x_w), _ptr(x_b), _ptr(final_w),
                                                _ptr(final_b), _ptr(coef), steps, A, nb, int(use_cfg), float(cfg_scale),
                                                _ptr(packed_table), _ptr(per_kv), P_, depth, N, T1, H, heads, I, float(eps), _ptr(ws),
                                                nbytes, _stream()), "dxa_dit_sample_bf16_per_fwd")
        return x
    L.check(lib.dxa_dit_sample_bf16_fwd(_ptr(x), _ptr(z_emb), _ptr(t_emb), _ptr(pos), _ptr(x_w), _ptr(x_b), _ptr(final_w),
                                        _ptr(final_b), _ptr(coef), steps, A, nb, int(use_cfg), float(cfg_scale), _ptr(packed_table),
                                        depth, N, T1, H, heads, I, float(eps), _ptr(ws), nbytes, _stream()), "dxa_dit_sample_bf16_fwd")
    return x


DIT_SAMPLE_MAX_GROUPS = 16          # csrc/dit_fused.hip MAXG


def dit_sample_bf16_groups_supported(G: int, Ng: int, T1: int, H: int, heads: int, I: int, P: int = 0) -> bool:
    """G requests of ``Ng`` samples each (2 with guidance: conditional, unconditional) in one launch of the bf16 sampler"""
    return 1 <= G <= DIT_SAMPLE_MAX_GROUPS and dit_sample_bf16_supported(Ng, T1, H, heads, I, P)


def dit_sample_bf16_batched_fwd(x: torch.Tensor, z_emb: torch.Tensor, t_emb: torch.Tensor, pos: torch.Tensor, x_w: torch.Tensor,
                                x_b: torch.Tensor, final_w: torch.Tensor, final_b: torch.Tensor, coef: torch.Tensor, use_cfg: bool,
                                cfg_scale: float, packed_table: torch.Tensor, depth: int, T1: int, H: int, heads: int, I: int,
                                eps: float, per_kv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dit_sample_bf16_fwd for G requests in ONE persistent launch (dxa_dit_sample_bf16_batched_fwd / _per_batched_fwd): x [G, T1-1, A]
    fp32 is updated in place, z_emb [G, Ng, H] (Ng = 2 with guidance: the request's conditional row, then its unconditional one),
    ``per_kv`` [depth, G, Ng, P, 2, H].  Request g of the result has the bits dit_sample_bf16_fwd(x[g:g+1], z_emb[g], ...,
    per_kv=per_kv[:, g]) gives."""
    steps, A = t_emb.shape[0], x.shape[-1]
    for t in (x, z_emb, t_emb, pos, x_w, x_b, final_w, final_b, coef):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
    assert x.dim() == 3 and z_emb.dim() == 3
    G, Ng = x.shape[0], z_emb.shape[1]
    if z_emb.shape[0] != G:
        raise L.DxaError(f"dit_sample_bf16_batched_fwd: x holds {G} requests but z_emb {z_emb.shape[0]}")
    assert Ng == (2 if use_cfg else 1)
    assert x.shape == (G, T1 - 1, A) and z_emb.shape == (G, Ng, H) and t_emb.shape == (steps, H) and coef.shape == (steps, 4)
    assert pos.shape == (T1, H) and x_w.shape == (H, A) and final_w.shape == (A, H)
    assert packed_table.dtype == torch.int64 and packed_table.numel() == depth * (10 if per_kv is None else 16) and packed_table.is_cuda
    P_ = 0 if per_kv is None else per_kv.shape[3]
    if not dit_sample_bf16_groups_supported(G, Ng, T1, H, heads, I, P_):
        raise L.DxaError(f"dit_sample_bf16_batched_fwd: unsupported shape (G={G}, Ng={Ng}, T1={T1}, H={H}, heads={heads}, I={I}, P={P_})")
    nbytes = lib.dxa_dit_sample_bf16_batched_workspace(G, Ng * T1, H, I)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    if per_kv is not None:
        assert per_kv.dtype == torch.float32 and per_kv.is_contiguous() and per_kv.shape == (depth, G, Ng, P_, 2, H)
        L.check(lib.dxa_dit_sample_bf16_per_batched_fwd(_ptr(x), _ptr(z_emb), _ptr(t_emb), _ptr(pos), _ptr(x_w), _ptr(x_b),
                                                        _ptr(final_w), _ptr(final_b), _ptr(coef), steps, A, G, 1, int(use_cfg),
                                                        float(cfg_scale), _ptr(packed_table), _ptr(per_kv), P_, depth, Ng, T1, H,
                                                        heads, I, float(eps), _ptr(ws), nbytes, _stream()),
                "dxa_dit_sample_bf16_per_batched_fwd")
        return x
    L.check(lib.dxa_dit_sample_bf16_batched_fwd(_ptr(x), _ptr(z_emb), _ptr(t_emb), _ptr(pos), _ptr(x_w), _ptr(x_b), _ptr(final_w),
                                                _ptr(final_b), _ptr(coef), steps, A, G, 1, int(use_cfg), float(cfg_scale),
                                                _ptr(packed_table), depth, Ng, T1, H, heads, I, float(eps), _ptr(ws), nbytes,
                                                _stream()), "dxa_dit_sample_bf16_batched_fwd")
    return x


def dit_blocks_timed_out(stream: Optional["torch.cuda.Stream"] = None) -> bool:
    """True if a fused DiT launch on `stream` (default: the current one) gave up at a device-wide barrier since the last
    call (its result is garbage and the request must be re-run unfused).  Synchronises the stream."""
    flag = C.c_int(0)
    L.check(lib.dxa_dit_blocks_status(stream.cuda_stream if stream is not None else _stream(), C.byref(flag)),
            "dxa_dit_blocks_status")
    return bool(flag.value)


# ------------------------------------------------------------------------------------------- persistent decode step
DECODE_FUSED_MAX_WIDTH = 32768      # csrc/decode_fused.hip ACT_MAX
DECODE_FUSED_MAX_KEYS = 16383       # ... T_MAX


def decode_step_supported(d: int, Hq: int, Hkv: int, D: int, F: int) -> bool:
    return (D in (64, 128, 256) and d % 8 == 0 and F % 8 == 0 and (Hq * D) % 8 == 0 and Hq % Hkv == 0 and
            max(d, F, Hq * D) <= DECODE_FUSED_MAX_WIDTH and Hq <= 256)


def decode_step(layer_table: torch.Tensor, x_in: torch.Tensor, out: torch.Tensor, final_w: torch.Tensor, cos_row: torch.Tensor,
                sin_row: torch.Tensor, ws: torch.Tensor, n_layers: int, d: int, Hq: int, Hkv: int, D: int, F: int, slot: int,
                kv_lo: int, max_len: int, eps: float, qk_norm_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """one new token of one sequence through every decoder layer + final norm in ONE persistent launch (dxa_decode_step);
    `layer_table`: int64 device tensor of n_layers * 9 pointers (see include/dexbotic_amd.h); the caches are appended in place.
    `qk_norm_table`: int64 device tensor of n_layers * 2 pointers (q_norm / k_norm weights [D]) for a Qwen3 decoder, None: no norm"""
    assert layer_table.dtype == torch.int64 and layer_table.numel() == n_layers * 9 and layer_table.is_cuda
    if qk_norm_table is not None:
        assert qk_norm_table.dtype == torch.int64 and qk_norm_table.numel() == n_layers * 2 and qk_norm_table.is_cuda
    for t in (x_in, out, final_w):
        assert t.dtype == torch.bfloat16 and t.is_contiguous() and t.numel() == d and t.is_cuda
    for t in (cos_row, sin_row):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == D // 2 and t.is_cuda
    q = L.DecodeDesc()
    q.layers, q.x_in, q.out, q.final_norm_w = _ptr(layer_table), _ptr(x_in), _ptr(out), _ptr(final_w)
    q.cos_row, q.sin_row = _ptr(cos_row), _ptr(sin_row)
    q.workspace, q.workspace_bytes = _ptr(ws), ws.numel() * ws.element_size()
    q.n_layers, q.d, q.Hq, q.Hkv, q.D, q.F = n_layers, d, Hq, Hkv, D, F
    q.slot, q.kv_lo, q.max_len, q.eps = slot, kv_lo, max_len, float(eps)
    q.qk_norm = _ptr(qk_norm_table) if qk_norm_table is not None else None
    L.check(lib.dxa_decode_step(C.byref(q), _stream()), "dxa_decode_step")
    return out


def decode_step_workspace(d: int, Hq: int, Hkv: int, D: int, F: int, device) -> torch.Tensor:
    return torch.empty(lib.dxa_decode_step_workspace(d, Hq, Hkv, D, F), device=device, dtype=torch.uint8)


def decode_timed_out(stream: Optional["torch.cuda.Stream"] = None) -> bool:
    """True if a persistent decode launch on `stream` gave up at a device-wide barrier since the last call (its tokens are
    garbage).  Synchronises the stream."""
    flag = C.c_int(0)
    L.check(lib.dxa_decode_status(stream.cuda_stream if stream is not None else _stream(), C.byref(flag)), "dxa_decode_status")
    return bool(flag.value)
