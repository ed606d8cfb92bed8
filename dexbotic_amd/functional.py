"""Block-level autograd Functions of the CogACT path.

Each Function is one transformer block (or one front-end / head stage): its forward is a fixed
sequence of libdexbotic_amd kernel launches, its backward the hand-scheduled reverse sequence.
Weight gradients are NOT returned to autograd: the dW GEMMs (TN layout, fp32 output) write — or
accumulate, for gradient accumulation — straight into the fp32 gradient arena of the ParamStore
(engine.py), which then notifies the data-parallel reducer that the block's bucket is complete.
An ``anchor`` parameter (any trainable tensor of the block) is passed through ``apply`` only so that
autograd schedules the backward even when the activations upstream do not require grad.

With 288 GB of HBM per MI355X every block keeps its activations by default; the reference's gradient
checkpointing (base_exp.py:245, trainer.py:101,120: HF checkpoints every decoder / encoder layer) is the
opt-in ``ParamStore.recompute`` (``model.gradient_checkpointing_enable()``): the transformer-layer Functions
then keep only their INPUT and re-run their forward launches at the top of their backward (same kernels, same
order: bit-identical gradients) — ~0.75 GB -> 33 MB kept per decoder layer at 16 x 287 tokens, for a 4th forward.
"""
from __future__ import annotations


from collections import namedtuple
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch.autograd import Function

from . import _lib as L
from . import kernels as K
from .engine import ParamStore


def _names(x) -> Tuple[str, ...]:
    return (x,) if isinstance(x, str) else tuple(x)


_OUTER_GRAD = [True]     # grad mode at the apply() call site (inside Function.forward it always reads False)


class _StoreFn(Function):
    """autograd Function that writes parameter gradients into the ParamStore arenas.  Its backward runs the fp32 products in the
    mode its forward ran in (kernels.F32_GEMM_MODE: exact fp32 MFMA or the split-bf16 product): a training loop this package does
    not manage calls ``loss.backward()`` long after the model's forward — and whatever scoped the mode — has returned."""

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        fwd, bwd = cls.__dict__.get("forward"), cls.__dict__.get("backward")
        if fwd is None or bwd is None:
            return
        f0 = fwd.__func__ if isinstance(fwd, staticmethod) else fwd
        b0 = bwd.__func__ if isinstance(bwd, staticmethod) else bwd

        def forward(ctx, *args, **kwargs):
            ctx._f32_mode = K.F32_GEMM_MODE
            return f0(ctx, *args, **kwargs)

        def backward(ctx, *grads):
            mode = getattr(ctx, "_f32_mode", None)
            if mode is None or mode == K.F32_GEMM_MODE:
                return b0(ctx, *grads)
            with K.f32_gemm_mode(mode):
                return b0(ctx, *grads)
        forward.__doc__, backward.__doc__ = f0.__doc__, b0.__doc__
        cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)

    @classmethod
    def apply(cls, *args, **kwargs):
        _OUTER_GRAD[0] = torch.is_grad_enabled()
        return super().apply(*args, **kwargs)


def _use(ctx, st: ParamStore, *groups) -> None:
    """forward-side half of the bucket accounting (ParamStore.note_use): this Function's backward will write each of
    these gradient slots once.  Only when a backward can actually run (grad mode on, some input requires grad)."""
    if not (_OUTER_GRAD[0] and any(ctx.needs_input_grad)):
        return
    for g in groups:
        if g is None:
            continue
        st.note_use(*[n for n in _names(g) if n is not None])


def _recompute(ctx, st: ParamStore) -> bool:
    """activation recompute for this call: opted in on the store and a backward can actually run"""
    return bool(getattr(st, "recompute", False)) and _OUTER_GRAD[0] and any(ctx.needs_input_grad)


def _f32_nt(dy2d: torch.Tensor) -> bool:
    """fp32 products of the action head (>= 128 rows): the tiled kernel's k-contiguous (NT) staging is ~1.5-2.5x faster
    than its k-strided NN / TN staging (scripts/gemm_f32_bench.py), so transposing a small operand first pays"""
    return dy2d.dtype == torch.float32 and dy2d.shape[0] >= 128 and dy2d.shape[1] >= 128


def _dx(st: ParamStore, names, wshape, dy2d: torch.Tensor, **kw) -> torch.Tensor:
    """dX = dY W for W = fused view over `names` of shape wshape = (out, in).  bf16: an NN product on the ping-pong MFMA
    kernel that stages W as it lies in memory (k-strided operand, ds_read_b64_tr_b16 fragments) — no W^T copy exists."""
    names = _names(names)
    W = st.w(*names, shape=tuple(wshape))
    if _f32_nt(dy2d):
        return K.mm_nn_f32(dy2d, W, **kw)
    return K.mm_nn(dy2d, W, **kw)


def _wgrad(st: ParamStore, names, dy2d: torch.Tensor, x2d: torch.Tensor, shape) -> None:
    """dW (+)= dy^T x into the gradient arena (fused view over `names`).  bf16: a TN product on the ping-pong MFMA kernel:
    both activations are staged as they lie ([tokens, features], the contraction runs over the rows) — no transposed
    copies, any token count.  A parameter with several consumers in this forward (``ParamStore.note_use``) collects their
    (dy, x) pairs and writes dW with ONE product over all rows when the last consumer's backward arrives
    (``ParamStore.defer_wgrad``)."""
    names = _names(names)
    if not all(st.trainable(n) for n in names):
        if any(st.trainable(n) for n in names):
            raise L.DxaError(f"fused parameters {names} must be frozen/unfrozen together")
        return
    key = tuple(names)
    pending = st._uses.get(names[0], 0)                  # consumers whose backward has not run yet, this one included
    if st.defer_wgrad and (pending > 1 or key in st._wg_stash):
        ent = st._wg_stash.get(key)
        if ent is None:
            ent = st._wg_stash[key] = {"acc0": st.accum_flag(*names), "dy": [], "x": [], "shape": shape}
        ent["dy"].append(dy2d)
        ent["x"].append(x2d)
        if pending > 1:
            st.mark_written(*names)                      # counts this consumer down; the bucket waits for the last one
            return
        _wgrad_flush(st, key)
        return
    if st.accum_merge and dy2d.dtype == torch.bfloat16 and x2d.dtype == torch.bfloat16 and dy2d.is_contiguous() and x2d.is_contiguous():
        # gradient accumulation over TWO micro-batches (the reference recipe): the first micro-batch keeps its (dY, X) and
        # writes nothing; the last one contracts both pairs in ONE product — dW is written once instead of written, read back
        # and written again (ParamStore.accum_merge; the trainer arms it for grad_accum == 2)
        if not st.last_micro and key not in st._accum_stash:
            st._accum_stash[key] = (dy2d, x2d, shape)
            return
        held = st._accum_stash.pop(key, None)
        if held is not None:
            if st.last_micro and held[0].shape[1] == dy2d.shape[1] and held[1].shape[1] == x2d.shape[1]:
                _wgrad_now(st, names, dy2d, x2d, shape, st.accum_flag(*names), seg2=held[:2])
                return
            _wgrad_now(st, names, held[0], held[1], held[2], st.accum_flag(*names))      # (no partner: written on its own)
    _wgrad_now(st, names, dy2d, x2d, shape, st.accum_flag(*names))


def flush_accum(st: ParamStore) -> None:
    """(dY, X) pairs of the first micro-batch whose parameter the last micro-batch did not use: their dW is written now"""
    for key in list(st._accum_stash):
        dy, x, shape = st._accum_stash.pop(key)
        _wgrad_now(st, key, dy, x, shape, st.accum_flag(*key))


def _wgrad_flush(st: ParamStore, key: tuple) -> None:
    ent = st._wg_stash.pop(key)
    dy = ent["dy"][0] if len(ent["dy"]) == 1 else torch.cat(ent["dy"], dim=0)
    x = ent["x"][0] if len(ent["x"]) == 1 else torch.cat(ent["x"], dim=0)
    _wgrad_now(st, key, dy.contiguous(), x.contiguous(), ent["shape"], ent["acc0"], first_write=not ent["acc0"])


def _wgrad_now(st: ParamStore, names, dy2d: torch.Tensor, x2d: torch.Tensor, shape, accumulate: bool,
               first_write: Optional[bool] = None, seg2=None) -> None:
    side = st.wgrad_stream
    if side is not None and st.wgrad_stream_f32_only and dy2d.dtype != torch.float32:
        side = None                                # (only the fp32 action head's products leave the compute stream)
    if side is None:
        _wgrad_product(st, names, dy2d, x2d, shape, accumulate, first_write, seg2)
    else:
        # the product runs on the side stream, ordered after everything enqueued on the compute stream so far (its operands);
        # all dW products share that stream, so successive writes of one slot stay ordered; readers join (ParamStore.join_wgrad)
        side.wait_stream(torch.cuda.current_stream(st.device))
        with torch.cuda.stream(side):
            _wgrad_product(st, names, dy2d, x2d, shape, accumulate, first_write, seg2)
        for t in (dy2d, x2d) + (tuple(seg2) if seg2 is not None else ()):
            t.record_stream(side)                  # the allocator must not hand the operands out again before the product has read them
        st._wgrad_pending = True
    st.mark_written(*names)


def _wgrad_product(st: ParamStore, names, dy2d: torch.Tensor, x2d: torch.Tensor, shape, accumulate: bool,
                   first_write: Optional[bool], seg2) -> None:
    kw2 = {} if seg2 is None else {"a2": seg2[0], "b2": seg2[1]}
    if st.bf16_grads and st.gradc is not None and dy2d.dtype == torch.bfloat16 and x2d.dtype == torch.bfloat16:
        # bf16 gradient arena: the product writes bf16 only (ParamStore.bf16_grads); the slots count as already copied
        out = st.gc(*names, shape=shape)
        ssq = st.sumsq_out(names, out.shape[0], out.shape[1], first_write) if out.dim() == 2 else None
        K.mm_tn(dy2d, x2d, out=out, accumulate=accumulate, sumsq=ssq, **kw2)
        st._mirrored.update(names)
        return
    out = st.g(*names, shape=shape)
    # bf16 data parallelism: the product's epilogue also writes the bf16 communication copy of this gradient
    mirror = st.mirror_out(*names, shape=shape)
    # single-GPU clip: ... and this gradient's share of sum(g^2) (bf16 gradient arena: the norm is taken over the bf16 copy
    # AdamW reads, so an fp32 product's share is read back from that copy instead)
    ssq = st.sumsq_out(names, out.shape[0], out.shape[1], first_write) if out.dim() == 2 and not st.bf16_grads else None
    if _f32_nt(dy2d) and x2d.dtype == torch.float32:
        K.mm_tn_f32(dy2d, x2d, out=out, accumulate=accumulate, mirror=mirror, sumsq=ssq)
    else:
        K.mm_tn(dy2d, x2d, out=out, accumulate=accumulate, mirror=mirror, sumsq=ssq, **kw2)


def _bgrad(st: ParamStore, names, dy2d: torch.Tensor) -> None:
    names = _names(names)
    if not all(st.trainable(n) for n in names):
        return
    n = sum(st.slots[nm].numel for nm in names)
    # a bias applied k times in one forward (MemVLA's per-sample retrieval blocks: 16 samples x 2 roles x 11 linears): the k dY are
    # collected like the weight's (dY, X) pairs (_wgrad) and ONE column sum over all their rows writes db once — k - 1 launches of the
    # backward's host-bound stretch less per bias (profiles/r06_host_uploads.txt: the bank's backward is issued at 21 us a launch)
    key = tuple(names)
    pending = st._uses.get(names[0], 0)
    acc0 = None
    if st.defer_wgrad and (pending > 1 or key in st._bg_stash):
        ent = st._bg_stash.get(key)
        if ent is None:
            ent = st._bg_stash[key] = {"acc0": st.accum_flag(*names), "dy": []}
        ent["dy"].append(dy2d)
        if pending > 1:
            st.mark_written(*names)                      # counts this consumer down; the bucket waits for the last one
            return
        ent = st._bg_stash.pop(key)
        dy2d = ent["dy"][0] if len(ent["dy"]) == 1 else torch.cat(ent["dy"], dim=0)
        acc0 = ent["acc0"]
    _bgrad_now(st, names, n, dy2d, st.accum_flag(*names) if acc0 is None else acc0)


def _bgrad_flush(st: ParamStore, key: tuple) -> None:
    ent = st._bg_stash.pop(key)
    dy = ent["dy"][0] if len(ent["dy"]) == 1 else torch.cat(ent["dy"], dim=0)
    _bgrad_now(st, key, sum(st.slots[nm].numel for nm in key), dy, ent["acc0"])


def _bgrad_now(st: ParamStore, names, n: int, dy2d: torch.Tensor, accumulate: bool) -> None:
    side = st.wgrad_stream if st.bgrad_on_side else None
    if side is None:
        K.colsum(dy2d, out=st.g(*names, shape=(n,)), accumulate=accumulate)
    else:
        side.wait_stream(torch.cuda.current_stream(st.device))
        with torch.cuda.stream(side):
            K.colsum(dy2d, out=st.g(*names, shape=(n,)), accumulate=accumulate)
        dy2d.record_stream(side)
        st._wgrad_pending = True
    st.mark_written(*names)


def _vgrad(st: ParamStore, name: str, val: torch.Tensor) -> None:
    """small fp32 gradient vector/matrix (already reduced) into the arena"""
    if not st.trainable(name):
        return
    g = st.g(name)
    flat = g.view(-1)
    v = val.reshape(-1)
    if st.accum_flag(name):
        K.add(flat, v.contiguous(), out=flat)
    else:
        K.cast(v.contiguous(), torch.float32, out=flat)
    st.mark_written(name)


# ------------------------------------------------------------------------------------------- Qwen2 layer
@dataclass
class Qwen2LayerSpec:
    ln1: str
    qkv_w: Tuple[str, str, str]
    qkv_b: Optional[Tuple[str, str, str]]      # None: projections without bias (Qwen3, attention_bias=False)
    o_w: str
    ln2: str
    gu_w: Tuple[str, str]
    down_w: str
    B: int = 0
    S: int = 0
    Hq: int = 0
    Hkv: int = 0
    D: int = 0
    d: int = 0
    F: int = 0
    eps: float = 1e-6
    grad_mode: bool = True     # grad mode of the caller of the current forward (Qwen2Backbone.forward records it)
    # Qwen3: names of self_attn.q_norm.weight / k_norm.weight [D], adjacent in the arena — the per-head RMSNorm of q and k between the
    # projection and RoPE (HF:qwen3/modeling_qwen3.py), run inside the RoPE / split pass (dxa_qknorm_rope_split / _merge)
    qk_norm: Optional[Tuple[str, str]] = None


class Qwen2LayerFn(_StoreFn):
    """HF Qwen2DecoderLayer (HF:qwen2/modeling_qwen2.py:258-300) called from cogact_arch.py:97-106:
    x + o_proj(attn(rope(qkv(rmsnorm(x))))) ; then + down(silu(gate)*up) of rmsnorm.
    With ``sp.qk_norm`` the layer is HF Qwen3DecoderLayer: rope(q_norm(q)), rope(k_norm(k)) per head, no projection bias; the
    backward then also reads the pre-norm qkv and the per-head rstd (kept, or re-run under recompute like everything else)."""

    @staticmethod
    def _run(st: ParamStore, sp: Qwen2LayerSpec, B: int, S: int, x, cos_t, sin_t, kv_start, kv_end, keep: bool = True, pos=None,
             cache=None):
        """the layer's forward launches on x [B*S, d] -> (y, what the backward reads besides x): training, serving and the
        key/value-cached path (Qwen2Backbone.forward_cached) all run this one sequence.  ``keep`` = False (no gradient will be asked
        for: serving): the gated MLP's pre-activations are not stored and SiLU * up runs in the gate / up product's epilogue.
        ``pos``: int32 rows of the rotary tables per token (None: token s of a sequence reads row s).  ``cache`` (with ``keep`` =
        False only) = (k cache [B, Hkv, max_len, D], v cache, past): the new keys / values are appended at [past, past + S) and
        attention reads the cache's first past + S positions."""
        assert cache is None or not keep, "a backward must not read keys / values out of a cache that the next step overwrites"
        Hq, Hkv, D, d, F_ = sp.Hq, sp.Hkv, sp.D, sp.d, sp.F
        M = B * S
        nq = (Hq + 2 * Hkv) * D
        h1, rstd1 = K.rmsnorm_fwd(x, st.w(sp.ln1), sp.eps)
        qkv = K.mm_nt(h1, st.w(*sp.qkv_w, shape=(nq, d)), bias=st.w(*sp.qkv_b, shape=(nq,)) if sp.qkv_b is not None else None)
        extra = ()
        if sp.qk_norm is None:
            q, k, v = K.rope_split(qkv, cos_t, sin_t, pos, B, S, Hq, Hkv, D)
        else:
            q, k, v, rstd_qk = K.qknorm_rope_split(qkv, st.w(sp.qk_norm[0]), st.w(sp.qk_norm[1]), sp.eps, cos_t, sin_t, pos,
                                                   B, S, Hq, Hkv, D, want_rstd=keep)
            extra = (qkv, rstd_qk)
        del qkv
        if cache is not None:
            k_cache, v_cache, past = cache
            k_cache[:, :, past:past + S].copy_(k)
            v_cache[:, :, past:past + S].copy_(v)
            k, v = k_cache[:, :, :past + S], v_cache[:, :, :past + S]
        o = torch.empty((B, S, Hq, D), device=x.device, dtype=x.dtype)
        lse = K.attn_fwd(q, k, v, o.permute(0, 2, 1, 3), causal=True, scale=D ** -0.5, kv_start=kv_start, kv_end=kv_end)
        x2 = K.mm_nt(o.view(M, Hq * D), st.w(sp.o_w), residual=x)
        h2, rstd2 = K.rmsnorm_fwd(x2, st.w(sp.ln2), sp.eps)
        w_gu = st.w(*sp.gu_w, shape=(2 * F_, d))
        if K.swiglu_gemm_supported(h2, w_gu, keep_pre=keep):          # SiLU(gate) * up in the product's own epilogue
            a, gu = K.mm_nt_swiglu(h2, w_gu, keep_pre=keep)
        else:
            gu = K.mm_nt(h2, w_gu)
            a = K.swiglu_fwd(gu)
        y = K.mm_nt(a, st.w(sp.down_w), residual=x2)
        return y, (rstd1, h1, q, k, v, o, lse, x2, rstd2, h2, gu, a) + extra

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, sp: Qwen2LayerSpec, cos_t, sin_t, kv_start, kv_end):
        # will a backward come?  (needs_input_grad reports requires_grad of the inputs whatever the grad mode of the caller: a served
        #  model keeps its parameters trainable, so the caller's grad mode — recorded by Qwen2Backbone.forward — decides too)
        need = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) and getattr(sp, "grad_mode", True)
        y, saved = Qwen2LayerFn._run(st, sp, sp.B, sp.S, x, cos_t, sin_t, kv_start, kv_end, keep=need)
        if not need:
            return y
        ctx.st, ctx.sp = st, sp
        _use(ctx, st, sp.ln1, sp.qkv_w, sp.qkv_b, sp.qk_norm, sp.o_w, sp.ln2, sp.gu_w, sp.down_w)
        ctx.aux = (cos_t, sin_t, kv_start, kv_end)
        ctx.recompute = _recompute(ctx, st)
        if ctx.recompute:
            ctx.save_for_backward(x)              # gradient checkpointing: the input only, the rest is re-run in backward
        else:
            ctx.save_for_backward(x, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        st, sp = ctx.st, ctx.sp
        cos_t, sin_t, kv_start, kv_end = ctx.aux
        if ctx.recompute:
            (x,) = ctx.saved_tensors
            rstd1, h1, q, k, v, o, lse, x2, rstd2, h2, gu, a, *extra = \
                Qwen2LayerFn._run(st, sp, sp.B, sp.S, x, cos_t, sin_t, kv_start, kv_end)[1]
        else:
            x, rstd1, h1, q, k, v, o, lse, x2, rstd2, h2, gu, a, *extra = ctx.saved_tensors
        B, S, Hq, Hkv, D, d, F_ = sp.B, sp.S, sp.Hq, sp.Hkv, sp.D, sp.d, sp.F
        M = B * S
        nq = (Hq + 2 * Hkv) * D
        dy = dy.contiguous()
        # ---- MLP
        da = _dx(st, sp.down_w, (d, F_), dy)
        _wgrad(st, sp.down_w, dy, a, (d, F_))
        dgu = K.swiglu_bwd(gu, da)
        del da
        dh2 = _dx(st, sp.gu_w, (2 * F_, d), dgu)
        _wgrad(st, sp.gu_w, dgu, h2, (2 * F_, d))
        del dgu
        tr2 = st.trainable(sp.ln2)
        dx2, _ = K.rmsnorm_bwd(dh2, x2, st.w(sp.ln2), rstd2, dw_out=st.g(sp.ln2) if tr2 else None,
                               accumulate=st.accum_flag(sp.ln2), want_dw=tr2, residual=dy)     # dy + norm backward
        if tr2:
            st.mark_written(sp.ln2)
        del dh2
        # ---- attention: dO written head-major by a (b, h)-batched NN GEMM so the GQA group folds into
        #      the rows of the dK/dV GEMMs (attention.hip)
        if dx2.dtype == torch.bfloat16:
            do = K.permute_bshd(_dx(st, sp.o_w, (d, Hq * D), dx2), B, S, Hq, D, True)
        else:
            wo = st.w(sp.o_w)                                    # [d, Hq*D]
            do = torch.empty((B, Hq, S, D), device=x.device, dtype=x.dtype)
            K.gemm(L.NN, dx2, wo, S, D, d, d, Hq * D, do, D, nb=(B, Hq, 1),
                   sA=(S * d, 0, 0), sB=(0, D, 0), sC=(Hq * S * D, S * D, 0))
        _wgrad(st, sp.o_w, dx2, o.view(M, Hq * D), (d, Hq * D))
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        K.attn_bwd(q, k, v, o.permute(0, 2, 1, 3), lse, do, dq, dk, dv, causal=True, scale=D ** -0.5,
                   kv_start=kv_start, kv_end=kv_end)
        if sp.qk_norm is None:
            dqkv = K.rope_merge(dq, dk, dv, cos_t, sin_t, None, B, S, Hq, Hkv, D)
        else:
            qkv, rstd_qk = extra
            tr_qk = all(st.trainable(n) for n in sp.qk_norm)
            dqkv, part = K.qknorm_rope_merge(dq, dk, dv, qkv, rstd_qk, st.w(sp.qk_norm[0]), st.w(sp.qk_norm[1]), cos_t, sin_t, None,
                                             B, S, Hq, Hkv, D, want_dw=tr_qk)
            if tr_qk:
                _bgrad(st, sp.qk_norm, part)       # rows of (dw_q | dw_k) partial sums: the column sum that folds the bias gradients
            del qkv, extra
        del dq, dk, dv, do
        dh1 = _dx(st, sp.qkv_w, (nq, d), dqkv)
        _wgrad(st, sp.qkv_w, dqkv, h1, (nq, d))
        if sp.qkv_b is not None:
            _bgrad(st, sp.qkv_b, dqkv)
        del dqkv
        tr1 = st.trainable(sp.ln1)
        dx, _ = K.rmsnorm_bwd(dh1, x, st.w(sp.ln1), rstd1, dw_out=st.g(sp.ln1) if tr1 else None,
                              accumulate=st.accum_flag(sp.ln1), want_dw=tr1, residual=dx2)
        if tr1:
            st.mark_written(sp.ln1)
        return dx, None, None, None, None, None, None, None


# ------------------------------------------------------------------- ViT-style block (CLIP layer, DiT block)
@dataclass
class VitBlockSpec:
    ln1_w: Optional[str]
    ln1_b: Optional[str]
    qkv_w: Tuple[str, ...]      # 3 adjacent tensors (CLIP) or the single fused one (timm)
    qkv_b: Tuple[str, ...]
    out_w: str
    out_b: str
    ln2_w: Optional[str]
    ln2_b: Optional[str]
    fc1_w: str
    fc1_b: str
    fc2_w: str
    fc2_b: str
    act: int
    eps: float
    N: int = 0      # sequences
    T: int = 0      # tokens per sequence
    H: int = 0
    D: int = 0
    I: int = 0      # mlp width
    ckpt: bool = True   # recomputed under ParamStore.recompute (HF checkpoints its encoder layers; the DiT head's blocks are
                        # plain nn.Modules in the reference and keep their activations: False there)


def _padded_head_dim(D: int, dtype) -> int:
    """head width the MFMA attention kernels run at for a model head_dim D (bf16 only; fp32 uses the generic kernels)"""
    # 72 (SigLIP-So400m) runs natively on the 128-wide tiles since round 5: only its 72 real columns are loaded / stored
    # (the round-3/4 zero-padded copies: profiles/r05_pi0_hd72.txt)
    if dtype != torch.bfloat16 or D in (64, 72, 128, 256) or D > 256 or D % 8 != 0:
        return D
    return 64 if D < 64 else (128 if D < 128 else 256)


class VitBlockFn(_StoreFn):
    """Pre-LN block: x + out(attn(qkv(LN(x)))) ; + fc2(act(fc1(LN(.)))).
    CLIP encoder layer (HF:clip/modeling_clip.py:259-384; affine LN eps 1e-5, quick_gelu) and DiTBlock
    (cogact/action_model/dit.py:137-162 with timm Attention/Mlp; LN without affine eps 1e-6, tanh-GELU)."""

    @staticmethod
    def _run(st: ParamStore, sp: VitBlockSpec, x):
        """the block's forward launches on x [M, C] -> (y [M, C], what the backward reads besides x)"""
        N, T, H, D, I = sp.N, sp.T, sp.H, sp.D, sp.I
        C_ = H * D
        M = N * T
        w = lambda n: st.w(n) if n is not None else None
        h1, mean1, rstd1 = K.layernorm_fwd(x, w(sp.ln1_w), w(sp.ln1_b), sp.eps)
        qkv = K.mm_nt(h1, st.w(*sp.qkv_w, shape=(3 * C_, C_)), bias=st.w(*sp.qkv_b, shape=(3 * C_,)))
        Dp = _padded_head_dim(D, x.dtype)
        if Dp != D:
            # head_dim the MFMA attention kernels do not take (SigLIP-So400m: 72): run them at the next supported
            # width on zero-padded heads — q.k is unchanged by zero columns, the padded output columns are dropped
            qkv = K.copy2d(qkv.view(M * 3 * H, D), torch.empty((M * 3 * H, Dp), device=x.device, dtype=x.dtype), D, Dp)
        q5 = qkv.view(N, T, 3, H, Dp)
        q, k, v = (q5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o = torch.empty((N, T, H, Dp), device=x.device, dtype=x.dtype)
        lse = K.attn_fwd(q, k, v, o.permute(0, 2, 1, 3), causal=False, scale=D ** -0.5)
        o_in = o if Dp == D else K.copy2d(o.view(M * H, Dp), torch.empty((M * H, D), device=x.device, dtype=x.dtype), D, D)
        x2 = K.mm_nt(o_in.view(M, C_), st.w(sp.out_w), bias=st.w(sp.out_b), residual=x)
        h2, mean2, rstd2 = K.layernorm_fwd(x2, w(sp.ln2_w), w(sp.ln2_b), sp.eps)
        pre = torch.empty((M, I), device=x.device, dtype=x.dtype)
        a = K.mm_nt(h2, st.w(sp.fc1_w), bias=st.w(sp.fc1_b), act=sp.act, aux_out=pre)
        y = K.mm_nt(a, st.w(sp.fc2_w), bias=st.w(sp.fc2_b), residual=x2)
        return y, (mean1, rstd1, h1, qkv, o, lse, x2, mean2, rstd2, h2, pre, a)

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, sp: VitBlockSpec):
        N, T, C_ = sp.N, sp.T, sp.H * sp.D
        x = x.reshape(N * T, C_)
        y, saved = VitBlockFn._run(st, sp, x)
        ctx.st, ctx.sp = st, sp
        _use(ctx, st, sp.ln1_w, sp.ln1_b, sp.qkv_w, sp.qkv_b, sp.out_w, sp.out_b, sp.ln2_w, sp.ln2_b, sp.fc1_w, sp.fc1_b,
             sp.fc2_w, sp.fc2_b)
        ctx.recompute = sp.ckpt and _recompute(ctx, st)
        if ctx.recompute:
            ctx.save_for_backward(x)
        else:
            ctx.save_for_backward(x, *saved)
        return y.view(N, T, C_)

    @staticmethod
    def backward(ctx, dy):
        st, sp = ctx.st, ctx.sp
        if ctx.recompute:
            (x,) = ctx.saved_tensors
            mean1, rstd1, h1, qkv, o, lse, x2, mean2, rstd2, h2, pre, a = VitBlockFn._run(st, sp, x)[1]
        else:
            x, mean1, rstd1, h1, qkv, o, lse, x2, mean2, rstd2, h2, pre, a = ctx.saved_tensors
        N, T, H, D, I = sp.N, sp.T, sp.H, sp.D, sp.I
        C_ = H * D
        M = N * T
        w = lambda n: st.w(n) if n is not None else None
        dy = dy.reshape(M, C_).contiguous()
        # ---- MLP (activation gradient fused into the dX GEMM epilogue)
        dpre = _dx(st, sp.fc2_w, (C_, I), dy, mulgrad=pre, act=sp.act)
        _wgrad(st, sp.fc2_w, dy, a, (C_, I))
        _bgrad(st, sp.fc2_b, dy)
        dh2 = _dx(st, sp.fc1_w, (I, C_), dpre)
        _wgrad(st, sp.fc1_w, dpre, h2, (I, C_))
        _bgrad(st, sp.fc1_b, dpre)
        del dpre
        dx2 = _ln_bwd(st, dh2, x2, sp.ln2_w, sp.ln2_b, mean2, rstd2, residual=dy.reshape(x2.shape))
        del dh2
        # ---- attention
        do = _dx(st, sp.out_w, (C_, C_), dx2)                   # [M, C] token-major
        Dp = o.shape[-1]                                          # padded head width of the forward (== D normally)
        o_in = o if Dp == D else K.copy2d(o.view(M * H, Dp), torch.empty((M * H, D), device=o.device, dtype=o.dtype), D, D)
        _wgrad(st, sp.out_w, dx2, o_in.view(M, C_), (C_, C_))
        _bgrad(st, sp.out_b, dx2)
        if Dp != D:
            do = K.copy2d(do.view(M * H, D), torch.empty((M * H, Dp), device=o.device, dtype=o.dtype), D, Dp)
        dqkv = torch.empty_like(qkv)
        q5, d5 = qkv.view(N, T, 3, H, Dp), dqkv.view(N, T, 3, H, Dp)
        q, k, v = (q5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        dq, dk, dv = (d5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        K.attn_bwd(q, k, v, o.permute(0, 2, 1, 3), lse, do.view(N, T, H, Dp).permute(0, 2, 1, 3), dq, dk, dv,
                   causal=False, scale=D ** -0.5)
        if Dp != D:
            dqkv = K.copy2d(dqkv.view(M * 3 * H, Dp), torch.empty((M * 3 * H, D), device=o.device, dtype=o.dtype), D, D)
            dqkv = dqkv.view(M, 3 * C_)
        dh1 = _dx(st, sp.qkv_w, (3 * C_, C_), dqkv)
        _wgrad(st, sp.qkv_w, dqkv, h1, (3 * C_, C_))
        _bgrad(st, sp.qkv_b, dqkv)
        del dqkv
        dx = _ln_bwd(st, dh1, x, sp.ln1_w, sp.ln1_b, mean1, rstd1, residual=dx2.reshape(x.shape))
        return dx.view(N, T, C_), None, None, None


def _ln_bwd(st: ParamStore, dy, x, wn: Optional[str], bn: Optional[str], mean, rstd, residual=None) -> torch.Tensor:
    """LayerNorm backward; `residual` (gradient of the skip connection around the sub-block) is added inside the kernel"""
    if wn is None:
        dx, _, _ = K.layernorm_bwd(dy, x, None, mean, rstd, residual=residual)
        return dx
    tr = st.trainable(wn)
    if tr and bn is not None and st.defer_wgrad and (st._uses.get(wn, 0) > 1 or (wn, bn) in st._bg_stash) and \
            st.slots[bn].offset == st.slots[wn].offset + st.slots[wn].numel:
        # an affine LayerNorm applied k times per forward (MemVLA's retrieval blocks): the kernel's per-row-block partial sums
        # [blocks, dw | db] of the k calls are folded by ONE column sum when the last one arrives (_bgrad's stash) instead of one per call
        dx, part = K.layernorm_bwd(dy, x, st.w(wn), mean, rstd, residual=residual, return_part=True)
        _bgrad(st, (wn, bn), part)
        return dx
    dx, _, _ = K.layernorm_bwd(dy, x, st.w(wn), mean, rstd, dw_out=st.g(wn) if tr else None,
                               db_out=st.g(bn) if tr else None, accumulate=st.accum_flag(wn), want_dw=tr, residual=residual)
    if tr:
        st.mark_written(wn, bn)
    return dx


# ------------------------------------------------------------------- Perception Encoder block and downsampler
@dataclass
class PeBlockSpec:
    ln1_w: str
    ln1_b: str
    qkv_w: str                  # attn.in_proj_weight [3C, C]
    qkv_b: str
    out_w: str
    out_b: str
    ln2_w: str
    ln2_b: str
    fc1_w: str
    fc1_b: str
    fc2_w: str
    fc2_b: str
    ls1: Optional[str]          # ls_1.gamma / ls_2.gamma, None without LayerScale (ls_init_value=None)
    ls2: Optional[str]
    eps: float
    N: int = 0
    T: int = 0
    H: int = 0
    D: int = 0
    I: int = 0
    cos: Optional[torch.Tensor] = None     # fp32 [T, D] angle tables of the grid in use (kernels.rope2d_tables)
    sin: Optional[torch.Tensor] = None


def _fold_gamma(st: ParamStore, name: str, part: torch.Tensor) -> None:
    """a LayerScale backward's partial sums [p, cols] into the gradient slot of its gamma"""
    if st.trainable(name):
        K.colsum(part, out=st.g(name), accumulate=st.accum_flag(name))
        st.mark_written(name)


class PeBlockFn(_StoreFn):
    """ResidualAttentionBlock of the Perception Encoder (mm_vision/pe/pe_model.py:188-313): x + ls_1(out(attn(rope2d(qkv(LN(x)))))),
    then + ls_2(c_proj(gelu(c_fc(LN(.))))).  2-D RoPE turns q and k in place in the packed projection; with LayerScale the two
    adds are dxa_layerscale_residual launches (the GEMM epilogue has no per-column scale), without it the GEMMs' residual epilogue
    as in VitBlockFn.  Recomputed under ``ParamStore.recompute``."""

    @staticmethod
    def _run(st: ParamStore, sp: PeBlockSpec, x):
        """the block's forward launches on x [M, C] -> (y [M, C], what the backward reads besides x)"""
        N, T, H, D, I = sp.N, sp.T, sp.H, sp.D, sp.I
        C_ = H * D
        M = N * T
        none = x.new_empty(0)
        h1, mean1, rstd1 = K.layernorm_fwd(x, st.w(sp.ln1_w), st.w(sp.ln1_b), sp.eps)
        qkv = K.mm_nt(h1, st.w(sp.qkv_w), bias=st.w(sp.qkv_b))
        K.rope2d_(qkv, sp.cos, sp.sin, N, T, H, D)
        Dp = _padded_head_dim(D, x.dtype)
        if Dp != D:     # (a head width the MFMA attention kernels do not take: zero-padded heads, as in VitBlockFn)
            qkv = K.copy2d(qkv.view(M * 3 * H, D), torch.empty((M * 3 * H, Dp), device=x.device, dtype=x.dtype), D, Dp)
        q5 = qkv.view(N, T, 3, H, Dp)
        q, k, v = (q5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o = torch.empty((N, T, H, Dp), device=x.device, dtype=x.dtype)
        lse = K.attn_fwd(q, k, v, o.permute(0, 2, 1, 3), causal=False, scale=D ** -0.5)
        o_in = o if Dp == D else K.copy2d(o.view(M * H, Dp), torch.empty((M * H, D), device=x.device, dtype=x.dtype), D, D)
        if sp.ls1 is not None:
            att = K.mm_nt(o_in.view(M, C_), st.w(sp.out_w), bias=st.w(sp.out_b))
            x2 = K.layerscale_residual_fwd(x, att, st.w(sp.ls1))
        else:
            att, x2 = none, K.mm_nt(o_in.view(M, C_), st.w(sp.out_w), bias=st.w(sp.out_b), residual=x)
        h2, mean2, rstd2 = K.layernorm_fwd(x2, st.w(sp.ln2_w), st.w(sp.ln2_b), sp.eps)
        pre = torch.empty((M, I), device=x.device, dtype=x.dtype)
        a = K.mm_nt(h2, st.w(sp.fc1_w), bias=st.w(sp.fc1_b), act=L.ACT_GELU_ERF, aux_out=pre)
        if sp.ls2 is not None:
            mlp = K.mm_nt(a, st.w(sp.fc2_w), bias=st.w(sp.fc2_b))
            y = K.layerscale_residual_fwd(x2, mlp, st.w(sp.ls2))
        else:
            mlp, y = none, K.mm_nt(a, st.w(sp.fc2_w), bias=st.w(sp.fc2_b), residual=x2)
        return y, (mean1, rstd1, h1, qkv, o, lse, att, x2, mean2, rstd2, h2, pre, a, mlp)

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, sp: PeBlockSpec):
        N, T, C_ = sp.N, sp.T, sp.H * sp.D
        x = x.reshape(N * T, C_).contiguous()
        y, saved = PeBlockFn._run(st, sp, x)
        ctx.st, ctx.sp = st, sp
        # the tables belong to this call: the spec's are replaced when the tower next sees another grid
        ctx.geom, ctx.tables = (N, T), (sp.cos, sp.sin)
        _use(ctx, st, sp.ln1_w, sp.ln1_b, sp.qkv_w, sp.qkv_b, sp.out_w, sp.out_b, sp.ln2_w, sp.ln2_b, sp.fc1_w, sp.fc1_b,
             sp.fc2_w, sp.fc2_b, sp.ls1, sp.ls2)
        ctx.recompute = _recompute(ctx, st)
        if ctx.recompute:
            ctx.save_for_backward(x)
        else:
            ctx.save_for_backward(x, *saved)
        return y.view(N, T, C_)

    @staticmethod
    def backward(ctx, dy):
        st, sp = ctx.st, ctx.sp
        (sp.N, sp.T), (sp.cos, sp.sin) = ctx.geom, ctx.tables
        if ctx.recompute:
            (x,) = ctx.saved_tensors
            mean1, rstd1, h1, qkv, o, lse, att, x2, mean2, rstd2, h2, pre, a, mlp = PeBlockFn._run(st, sp, x)[1]
        else:
            x, mean1, rstd1, h1, qkv, o, lse, att, x2, mean2, rstd2, h2, pre, a, mlp = ctx.saved_tensors
        N, T, H, D, I = sp.N, sp.T, sp.H, sp.D, sp.I
        C_ = H * D
        M = N * T
        dy = dy.reshape(M, C_).contiguous()
        # ---- MLP (activation gradient fused into the dX GEMM epilogue)
        dm = dy
        if sp.ls2 is not None:
            dm, part = K.layerscale_residual_bwd(dy, mlp, st.w(sp.ls2))
            _fold_gamma(st, sp.ls2, part)
        dpre = _dx(st, sp.fc2_w, (C_, I), dm, mulgrad=pre, act=L.ACT_GELU_ERF)
        _wgrad(st, sp.fc2_w, dm, a, (C_, I))
        _bgrad(st, sp.fc2_b, dm)
        dh2 = _dx(st, sp.fc1_w, (I, C_), dpre)
        _wgrad(st, sp.fc1_w, dpre, h2, (I, C_))
        _bgrad(st, sp.fc1_b, dpre)
        del dpre, dm
        dx2 = _ln_bwd(st, dh2, x2, sp.ln2_w, sp.ln2_b, mean2, rstd2, residual=dy)
        del dh2
        # ---- attention
        da = dx2
        if sp.ls1 is not None:
            da, part = K.layerscale_residual_bwd(dx2, att, st.w(sp.ls1))
            _fold_gamma(st, sp.ls1, part)
        do = _dx(st, sp.out_w, (C_, C_), da)                    # [M, C] token-major
        Dp = o.shape[-1]                                          # padded head width of the forward (== D normally)
        o_in = o if Dp == D else K.copy2d(o.view(M * H, Dp), torch.empty((M * H, D), device=o.device, dtype=o.dtype), D, D)
        _wgrad(st, sp.out_w, da, o_in.view(M, C_), (C_, C_))
        _bgrad(st, sp.out_b, da)
        if Dp != D:
            do = K.copy2d(do.view(M * H, D), torch.empty((M * H, Dp), device=o.device, dtype=o.dtype), D, Dp)
        dqkv = torch.empty_like(qkv)
        q5, d5 = qkv.view(N, T, 3, H, Dp), dqkv.view(N, T, 3, H, Dp)
        q, k, v = (q5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        dq, dk, dv = (d5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        K.attn_bwd(q, k, v, o.permute(0, 2, 1, 3), lse, do.view(N, T, H, Dp).permute(0, 2, 1, 3), dq, dk, dv,
                   causal=False, scale=D ** -0.5)
        if Dp != D:
            dqkv = K.copy2d(dqkv.view(M * 3 * H, Dp), torch.empty((M * 3 * H, D), device=o.device, dtype=o.dtype), D, D)
        dqkv = dqkv.view(M, 3 * C_)
        K.rope2d_(dqkv, sp.cos, sp.sin, N, T, H, D, backward=True)
        dh1 = _dx(st, sp.qkv_w, (3 * C_, C_), dqkv)
        _wgrad(st, sp.qkv_w, dqkv, h1, (3 * C_, C_))
        _bgrad(st, sp.qkv_b, dqkv)
        del dqkv
        dx = _ln_bwd(st, dh1, x, sp.ln1_w, sp.ln1_b, mean1, rstd1, residual=dx2)
        return dx.view(N, T, C_), None, None, None


class Conv3x3s2Fn(_StoreFn):
    """nn.Conv2d(C, C', kernel_size=3, stride=2, padding=1) over a token-major T x T grid (vit_downsampler1 / 2,
    mm_vision/pe/pe_model.py:445-458,554-565): x [B, T*T, C] -> [B, To*To, C'].  im2col rows in the weight's own (c, ky, kx) column
    order times the weight as it lies [C', 9C], bias in the GEMM epilogue; dW and db land in the parameter's layout, dX is the
    adjoint gather of dY W."""

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, wn: str, bn: str, T: int):
        x = x.contiguous()
        B, _, C_ = x.shape
        Co = st.slots[wn].shape[0]
        rows = K.conv3x3s2_im2col(x, T)
        y = K.mm_nt(rows, st.w(wn, shape=(Co, 9 * C_)), bias=st.w(bn))
        ctx.st, ctx.wn, ctx.bn, ctx.geom = st, wn, bn, (B, T, C_, Co)
        _use(ctx, st, wn, bn)
        ctx.save_for_backward(rows)
        return y.view(B, -1, Co)

    @staticmethod
    def backward(ctx, dy):
        st, wn, bn = ctx.st, ctx.wn, ctx.bn
        B, T, C_, Co = ctx.geom
        (rows,) = ctx.saved_tensors
        dy2 = dy.reshape(-1, Co).contiguous()
        _wgrad(st, wn, dy2, rows, (Co, 9 * C_))
        _bgrad(st, bn, dy2)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.conv3x3s2_col2im(_dx(st, wn, (Co, 9 * C_), dy2), B, T)
        return dx, None, None, None, None, None


class VitEmbedTensorFn(Function):
    """dxa_vit_embed on TENSORS: x[n, 0] = cls + pos[0], x[n, 1 + p] = patch[n, p] + pos[1 + p] with a position table that is itself
    a function of the parameter (the Perception Encoder's resampled embedding at a non-native input size, pe_model.py:475-500)."""

    @staticmethod
    def forward(ctx, patch, cls, pos, N: int, np_: int):
        ctx.geom = (N, np_)
        return K.vit_embed_fwd(patch.contiguous(), cls.contiguous(), pos.contiguous(), N, np_)

    @staticmethod
    def backward(ctx, dx):
        N, np_ = ctx.geom
        dx = dx.contiguous()
        C_ = dx.shape[-1]
        s = K.colsum(dx.view(N, (np_ + 1) * C_))
        if dx.dtype != torch.float32:
            s = K.cast(s, dx.dtype)
        return K.vit_embed_bwd(dx, N, np_), s[:C_], s.view(np_ + 1, C_), None, None


# --------------------------------------------------------------------------------------- generic pieces
class LinearFn(_StoreFn):
    """y = act(x W^T + b) (+ residual).  nn.Linear call sites of the path that are not inside a block:
    patch embedding (HF:clip/modeling_clip.py:149-155 as a GEMM over im2col rows), DiT embedders and final
    layer (dit.py:22-64,106-135,165-178)."""

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, wn: str, bn: Optional[str], act: int, wshape):
        x2 = x.reshape(-1, x.shape[-1])
        if not x2.is_contiguous() and not (x2.stride(1) == 1):
            x2 = x2.contiguous()
        W = st.w(wn, shape=wshape)
        pre = None
        if act != L.ACT_NONE:
            pre = torch.empty((x2.shape[0], W.shape[0]), device=x.device, dtype=x.dtype)
        y = K.mm_nt(x2[:, :W.shape[1]] if x2.shape[1] != W.shape[1] else x2, W,
                    bias=st.w(bn) if bn else None, act=act, aux_out=pre)
        ctx.st, ctx.wn, ctx.bn, ctx.act, ctx.wshape, ctx.xshape = st, wn, bn, act, wshape, x.shape
        _use(ctx, st, wn, bn)
        ctx.save_for_backward(x2, pre if pre is not None else x2.new_empty(0))
        return y.view(*x.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        st = ctx.st
        x2, pre = ctx.saved_tensors
        W = st.w(ctx.wn, shape=ctx.wshape)
        dy2 = dy.reshape(-1, W.shape[0]).contiguous()
        if ctx.act != L.ACT_NONE:
            dy2 = K.act_bwd(pre, dy2, ctx.act)
        xk = x2[:, :W.shape[1]] if x2.shape[1] != W.shape[1] else x2
        _wgrad(st, ctx.wn, dy2, xk, W.shape)
        if ctx.bn:
            _bgrad(st, ctx.bn, dy2)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _dx(st, ctx.wn, W.shape, dy2)
            if x2.shape[1] != W.shape[1]:
                raise L.DxaError("LinearFn: padded input cannot receive a gradient")
            dx = dx.view(ctx.xshape)
        return dx, None, None, None, None, None, None


class PackedInProjFn(_StoreFn):
    """nn.MultiheadAttention's packed in-projection for CROSS attention (torch F._in_projection_packed with k is v):
    q = x W[:E]^T + b[:E] from the query rows, [k | v] = y W[E:]^T + b[E:] from the key/value rows — the perceptual
    attention of the MemVLA DiT block (memvla/action_model/dit.py:158-185).  The two products use disjoint row ranges of the
    one packed parameter: its gradient is written range by range (dW[:E] = dq^T x, dW[E:] = dkv^T y) inside ONE Function, so
    the slot is announced and marked written once.  (Applying the whole 3E-row projection to both inputs and slicing, as
    round 2 did, computed a third of the key/value projection — 16384 perceptual rows per block at the MemVLA batch — for
    nothing.)"""

    @staticmethod
    def forward(ctx, x, y, anchor, st: ParamStore, wn: str, bn: str, E: int):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        y2 = y.reshape(-1, y.shape[-1]).contiguous()
        W, b = st.w(wn), st.w(bn)
        q = K.mm_nt(x2, W[:E], bias=b[:E])
        kv = K.mm_nt(y2, W[E:], bias=b[E:])
        ctx.st, ctx.wn, ctx.bn, ctx.E = st, wn, bn, E
        _use(ctx, st, wn, bn)
        ctx.save_for_backward(x2, y2)
        return q, kv

    @staticmethod
    def backward(ctx, dq, dkv):
        st, wn, bn, E = ctx.st, ctx.wn, ctx.bn, ctx.E
        x2, y2 = ctx.saved_tensors
        W = st.w(wn)
        dq, dkv = dq.contiguous(), dkv.contiguous()
        dx = dy = None
        nt = _f32_nt(dq)
        if ctx.needs_input_grad[0]:
            dx = K.mm_nn_f32(dq, W[:E]) if nt else K.mm_nn(dq, W[:E])
        if ctx.needs_input_grad[1]:
            dy = K.mm_nn_f32(dkv, W[E:]) if _f32_nt(dkv) else K.mm_nn(dkv, W[E:])
        if st.trainable(wn):
            acc = st.accum_flag(wn)
            g, gb = st.g(wn), st.g(bn)
            for lo, hi, d2, in2 in ((0, E, dq, x2), (E, W.shape[0], dkv, y2)):
                if _f32_nt(d2) and in2.dtype == torch.float32:
                    K.mm_tn_f32(d2, in2, out=g[lo:hi], accumulate=acc)
                else:
                    K.mm_tn(d2, in2, out=g[lo:hi], accumulate=acc)
                K.colsum(d2, out=gb[lo:hi], accumulate=acc)
            st.mark_written(wn, bn)
        return dx, dy, None, None, None, None, None


class MlpFn(_StoreFn):
    """y = (act(x W1^T + b1)) W2^T + b2 : mm_projector mlp2x_gelu (mm_projector/builder.py:71-79) and the
    TimestepEmbedder MLP (dit.py:27-31)."""

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, w1, b1, w2, b2, act: int):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        W1, W2 = st.w(w1), st.w(w2)
        pre = torch.empty((x2.shape[0], W1.shape[0]), device=x.device, dtype=x.dtype)
        a = K.mm_nt(x2, W1, bias=st.w(b1), act=act, aux_out=pre)
        y = K.mm_nt(a, W2, bias=st.w(b2))
        ctx.st, ctx.names, ctx.act, ctx.xshape = st, (w1, b1, w2, b2), act, x.shape
        _use(ctx, st, w1, b1, w2, b2)
        ctx.save_for_backward(x2, pre, a)
        return y.view(*x.shape[:-1], W2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        st = ctx.st
        w1, b1, w2, b2 = ctx.names
        x2, pre, a = ctx.saved_tensors
        W1, W2 = st.w(w1), st.w(w2)
        dy2 = dy.reshape(-1, W2.shape[0]).contiguous()
        dpre = _dx(st, w2, W2.shape, dy2, mulgrad=pre, act=ctx.act)
        _wgrad(st, w2, dy2, a, W2.shape)
        _bgrad(st, b2, dy2)
        _wgrad(st, w1, dpre, x2, W1.shape)
        _bgrad(st, b1, dpre)
        dx = _dx(st, w1, W1.shape, dpre).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        return dx, None, None, None, None, None, None, None


class NormFn(_StoreFn):
    """stand-alone LayerNorm / RMSNorm: CLIP pre_layrnorm, Qwen2 final norm, DiT final LayerNorm."""

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, kind: str, wn: Optional[str], bn: Optional[str], eps: float):
        if kind == "rms":
            y, rstd = K.rmsnorm_fwd(x.contiguous(), st.w(wn), eps)
            mean = rstd.new_empty(0)
        elif kind == "rms1p":                       # GemmaRMSNorm: scale by (1 + weight) in fp32
            y, rstd = K.rmsnorm_fwd(x.contiguous(), gemma_norm_w(st, wn), eps)
            mean = rstd.new_empty(0)
        else:
            y, mean, rstd = K.layernorm_fwd(x.contiguous(), st.w(wn) if wn else None, st.w(bn) if bn else None, eps)
        ctx.st, ctx.kind, ctx.wn, ctx.bn = st, kind, wn, bn
        _use(ctx, st, wn, bn if kind not in ("rms", "rms1p") else None)
        ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        st = ctx.st
        x, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.kind in ("rms", "rms1p"):
            tr = st.trainable(ctx.wn)
            w = st.w(ctx.wn) if ctx.kind == "rms" else gemma_norm_w(st, ctx.wn)      # d(1+w) = dw
            dx, _ = K.rmsnorm_bwd(dy, x.contiguous(), w, rstd, dw_out=st.g(ctx.wn) if tr else None,
                                  accumulate=st.accum_flag(ctx.wn), want_dw=tr)
            if tr:
                st.mark_written(ctx.wn)
        else:
            dx = _ln_bwd(st, dy, x.contiguous(), ctx.wn, ctx.bn, mean, rstd).view(x.shape)
        return dx, None, None, None, None, None, None


def _fold_ln_partials(st: ParamStore, wn: str, bn: str, part: torch.Tensor) -> None:
    """a LayerNorm backward's per-workgroup partial sums [blocks, dw | db] into the gradient slots of its weight and bias"""
    cols = part.shape[1] // 2
    dw, db, acc = st.g(wn), st.g(bn), st.accum_flag(wn)
    if db.data_ptr() == dw.data_ptr() + 4 * cols:      # weight and bias slots lie back to back: one column sum
        K.colsum(part, out=torch.as_strided(dw, (2 * cols,), (1,)), accumulate=acc)
    else:
        K.colsum(part[:, :cols], out=dw, accumulate=acc)
        K.colsum(part[:, cols:], out=db, accumulate=acc)
    st.mark_written(wn, bn)


class DownsampleNormFn(_StoreFn):
    """DownSampleBlock + nn.LayerNorm(4C) of the `mlp_downsample` projector (mm_projector/builder.py:9-33,62-69): x [N, G*G, C] ->
    [N, ceil(G/2)^2, 4C], 2x2 neighbouring tokens side by side (column-pair major order, odd grids zero padded), normalised.  One
    launch per direction; only the un-merged input and the row statistics are kept, so there is nothing to recompute under
    ``ParamStore.recompute``."""

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, wn: str, bn: str, eps: float):
        x = x.contiguous()
        y, mean, rstd = K.downsample_layernorm_fwd(x, st.w(wn), st.w(bn), eps)
        ctx.st, ctx.wn, ctx.bn = st, wn, bn
        _use(ctx, st, wn, bn)
        ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        st, wn, bn = ctx.st, ctx.wn, ctx.bn
        x, mean, rstd = ctx.saved_tensors
        dx, part = K.downsample_layernorm_bwd(dy.contiguous(), x, st.w(wn), mean, rstd)
        if st.trainable(wn):
            _fold_ln_partials(st, wn, bn, part)
        return dx, None, None, None, None, None


class AddNormFn(_StoreFn):
    """LayerNorm(x + res) in one launch per direction (the MuVLA fuser, dexbotic/model/muvla/muvla_arch.py:46-47): the sum is
    never written; the one dx of the backward is the gradient of both addends."""

    @staticmethod
    def forward(ctx, x, res, anchor, st: ParamStore, wn: str, bn: str, eps: float):
        x, res = x.contiguous(), res.contiguous()
        y, mean, rstd = K.add_layernorm_fwd(x, res, st.w(wn), st.w(bn), eps)
        ctx.st, ctx.wn, ctx.bn = st, wn, bn
        _use(ctx, st, wn, bn)
        ctx.save_for_backward(x, res, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        st, wn, bn = ctx.st, ctx.wn, ctx.bn
        x, res, mean, rstd = ctx.saved_tensors
        dx, part = K.add_layernorm_bwd(dy.contiguous(), x, res, st.w(wn), mean, rstd)
        if st.trainable(wn):
            _fold_ln_partials(st, wn, bn, part)
        return dx, dx, None, None, None, None, None


class VitEmbedFn(_StoreFn):
    """CLS + position embeddings (HF:clip/modeling_clip.py:206-217)."""

    @staticmethod
    def forward(ctx, patch, anchor, st: ParamStore, cls_n: str, pos_n: str, N: int, np_: int):
        x = K.vit_embed_fwd(patch.contiguous(), st.w(cls_n), st.w(pos_n), N, np_)
        ctx.st, ctx.cls_n, ctx.pos_n, ctx.N, ctx.np_ = st, cls_n, pos_n, N, np_
        _use(ctx, st, cls_n, pos_n)
        return x

    @staticmethod
    def backward(ctx, dx):
        st, N, np_ = ctx.st, ctx.N, ctx.np_
        dx = dx.contiguous()
        C_ = dx.shape[-1]
        dpatch = K.vit_embed_bwd(dx, N, np_)
        if st.trainable(ctx.pos_n) or st.trainable(ctx.cls_n):
            s = K.colsum(dx.view(N, (np_ + 1) * C_))
            _vgrad(st, ctx.pos_n, s)
            _vgrad(st, ctx.cls_n, s[:C_])
        return dpatch, None, None, None, None, None, None


class DropClsFn(Function):
    """feature_select: hidden_states[-2][:, 1:] (mm_vision/clip/clip_encoder.py:31-36)."""

    @staticmethod
    def forward(ctx, x):
        N, T, C_ = x.shape
        ctx.shape = (N, T, C_)
        return K.vit_embed_bwd(x.contiguous(), N, T - 1).view(N, T - 1, C_)

    @staticmethod
    def backward(ctx, dy):
        N, T, C_ = ctx.shape
        dx = torch.zeros((N, T * C_), device=dy.device, dtype=dy.dtype)
        K.copy2d(dy.reshape(N, (T - 1) * C_).contiguous(), dx[:, C_:], (T - 1) * C_, (T - 1) * C_)
        return dx.view(N, T, C_)


class SpliceFn(_StoreFn):
    """_prepare_inputs_labels_for_multimodal (dexbotic_arch.py:182-373): embed_tokens gather + image
    block insertion + zero padding, driven by the integer plan built on the host (splice.py)."""

    @staticmethod
    def forward(ctx, img_feats, anchor, st: ParamStore, embed_n: str, plan: torch.Tensor):
        d = img_feats.shape[-1]
        out = K.splice_fwd(plan, st.w(embed_n), img_feats.reshape(-1, d).contiguous())
        ctx.st, ctx.embed_n, ctx.ishape = st, embed_n, img_feats.shape
        _use(ctx, st, embed_n)
        ctx.save_for_backward(plan)
        return out

    @staticmethod
    def backward(ctx, dout):
        (plan,) = ctx.saved_tensors
        return _splice_backward(ctx.st, ctx.embed_n, plan, dout.contiguous(), ctx.ishape, ctx.needs_input_grad[0]), None, None, None, None


def _splice_backward(st: ParamStore, embed_n: str, plan: torch.Tensor, dout: torch.Tensor, ishape, want_img: bool,
                     extra_rows: Optional[torch.Tensor] = None, add_rows=None):
    """the splice's backward launches (SpliceFn, OftSpliceFn, OftDiscreteSpliceFn): the image rows' gradient, or None; the token
    rows' gradient is added into the embedding's slot.  Rows the plan marks as padding (PLAN_PAD) are ignored.
    ``extra_rows`` (int64 token ids on the device) / ``add_rows(d_embed)``: embedding rows that receive a gradient from outside the
    plan — they are re-zeroed with the plan's rows on the next step, and the add is enqueued before the slot is reported written."""
    d_img = None
    if want_img:
        d_img = torch.zeros(ishape, device=dout.device, dtype=dout.dtype)
    d_embed = None
    if st.trainable(embed_n):
        d_embed = st.g(embed_n)
        if not st.accum_flag(embed_n):
            # dense nn.Embedding gradient of which only <= B*S_text rows are ever non-zero: re-zero just the rows
            # the previous step touched when the store tracks them (single GPU), the whole slice otherwise
            st.zero_embed_grad(embed_n)
        st.note_embed_rows(embed_n, plan)
        if extra_rows is not None:
            st.note_embed_rows(embed_n, extra_rows)
    K.splice_bwd(plan, dout, d_embed, d_img)
    if d_embed is not None:
        if add_rows is not None:
            add_rows(d_embed)
        # AFTER the scatter-add is enqueued: embed_tokens is alone in its bucket, so this fires the reducer / the
        # grad-norm fold, which order themselves after everything enqueued so far on this stream
        st.mark_written(embed_n)
    return d_img


class OftSpliceFn(_StoreFn):
    """SpliceFn followed by ``insert_action_embedding`` (dexbotic/model/oft/oft_arch.py:105,118-123,169-201) on the SAME buffer: the
    plan (splice.build_oft_splice_plan) reserves Q rows behind each sample's rows, dxa_splice_fwd zero-fills them and
    dxa_action_put_fwd writes the sample's state row (``state`` [B, d], with proprio) and the shared ``action_query`` rows there.  No
    [B, S, d] tensor is built and copied.  Backward: the query's gradient (sum over the batch, ascending) into its slot, the state
    rows' gradient returned, then the splice's own backward, which ignores the reserved rows."""

    @staticmethod
    def forward(ctx, img_feats, state, anchor, st: ParamStore, embed_n: str, query_n: str, plan: torch.Tensor, off: torch.Tensor,
                B: int, Sq: int):
        d = img_feats.shape[-1]
        out = K.splice_fwd(plan, st.w(embed_n), img_feats.reshape(-1, d).contiguous())
        nq = st.slots[query_n].numel // d
        K.action_put_(out.view(B, Sq, d), st.w(query_n, shape=(nq, d)), off, None if state is None else state.contiguous())
        ctx.st, ctx.embed_n, ctx.query_n, ctx.ishape, ctx.geom = st, embed_n, query_n, img_feats.shape, (B, Sq, d, nq)
        ctx.has_state = state is not None
        _use(ctx, st, embed_n, query_n)
        ctx.save_for_backward(plan, off)
        return out

    @staticmethod
    def backward(ctx, dout):
        st = ctx.st
        plan, off = ctx.saved_tensors
        B, Sq, d, nq = ctx.geom
        dout = dout.contiguous()
        tr = st.trainable(ctx.query_n)
        want_state = ctx.has_state and ctx.needs_input_grad[1]
        dstate = None
        if tr or want_state:
            _, dstate = K.action_put_bwd(dout.view(B, Sq, d), off, nq, ctx.has_state,
                                         dquery=st.g(ctx.query_n, shape=(nq, d)) if tr else None,
                                         accumulate=st.accum_flag(ctx.query_n) if tr else False, want_dstate=want_state)
            if tr:
                st.mark_written(ctx.query_n)
        d_img = _splice_backward(st, ctx.embed_n, plan, dout, ctx.ishape, ctx.needs_input_grad[0])
        return d_img, dstate, None, None, None, None, None, None, None, None


class OftDiscreteSpliceFn(_StoreFn):
    """SpliceFn followed by the discrete head's ``insert_action_embedding`` (dexbotic/model/oft/oft_discrete_arch.py:125-143) on the
    SAME buffer: ``action_query`` is ``torch.ones(1, T A)`` used as token ids, so every one of the R = T A query rows of every sample
    is the embedding row of token ``token_rows[0]`` (= 1).  dxa_action_fill_fwd writes that row (and the sample's state row) into the
    rows the plan reserved.  The token is NOT put into the plan: dxa_splice_bwd would add the B R duplicate rows serially.
    Backward: the fixed-order sum of the R rows' gradients over the batch (dxa_action_fill_bwd) is added onto the token's row of the
    embedding gradient after the splice's own scatter-add and before the slot is reported written; ``token_rows`` (int64 [1] on the
    device) joins the rows that are re-zeroed on the next step."""

    @staticmethod
    def forward(ctx, img_feats, state, anchor, st: ParamStore, embed_n: str, token: int, token_rows: torch.Tensor,
                plan: torch.Tensor, off: torch.Tensor, B: int, Sq: int, n_rows: int):
        d = img_feats.shape[-1]
        embed = st.w(embed_n)
        out = K.splice_fwd(plan, embed, img_feats.reshape(-1, d).contiguous())
        K.action_fill_(out.view(B, Sq, d), embed[token], off, n_rows, None if state is None else state.contiguous())
        ctx.st, ctx.embed_n, ctx.token, ctx.ishape, ctx.geom = st, embed_n, token, img_feats.shape, (B, Sq, d, n_rows)
        ctx.has_state = state is not None
        _use(ctx, st, embed_n)
        ctx.save_for_backward(plan, off, token_rows)
        return out

    @staticmethod
    def backward(ctx, dout):
        st = ctx.st
        plan, off, token_rows = ctx.saved_tensors
        B, Sq, d, n_rows = ctx.geom
        dout = dout.contiguous()
        want_state = ctx.has_state and ctx.needs_input_grad[1]
        got = {}

        def add_rows(d_embed):
            _, got["dstate"] = K.action_fill_bwd(dout.view(B, Sq, d), off, n_rows, ctx.has_state, drow=d_embed[ctx.token],
                                                 accumulate=True, want_dstate=want_state)

        d_img = _splice_backward(st, ctx.embed_n, plan, dout, ctx.ishape, ctx.needs_input_grad[0], extra_rows=token_rows,
                                 add_rows=add_rows)
        if want_state and "dstate" not in got:            # frozen embedding: only the state rows' gradient is wanted
            _, got["dstate"] = K.action_fill_bwd(dout.view(B, Sq, d), off, n_rows, True, want_dstate=True)
        return (d_img, got.get("dstate")) + (None,) * 10


class NoisyEmbedFn(_StoreFn):
    """fc1 and the GELU of ``NoisyActionProjector`` (oft/action_model/model.py:46-53) on the R = B T A noisy-action scalars: a
    Linear(1, d) is one multiply per element, so the product, the bias and the activation are ONE pass (dxa_noisy_embed_fwd) that
    writes the [R, d] operand of fc2.  Nothing but the scalars is kept: the backward recomputes the pre-activation and writes
    dw1 | db1 as fixed-order two-stage sums into their slots.  The noisy actions are inputs: no gradient for them."""

    @staticmethod
    def forward(ctx, a, anchor, st: ParamStore, w1n: str, b1n: str):
        a = a.reshape(-1).contiguous()
        ctx.st, ctx.names = st, (w1n, b1n)
        _use(ctx, st, w1n, b1n)
        ctx.save_for_backward(a)
        return K.noisy_embed_fwd(a, st.w(w1n), st.w(b1n), st.compute_dtype)

    @staticmethod
    def backward(ctx, dh):
        st = ctx.st
        w1n, b1n = ctx.names
        (a,) = ctx.saved_tensors
        if st.trainable(w1n):
            K.noisy_embed_bwd(dh.contiguous(), a, st.w(w1n), st.w(b1n), dw1=st.g(w1n).view(-1), db1=st.g(b1n),
                              accumulate=st.accum_flag(w1n))
            st.mark_written(w1n, b1n)
        return None, None, None, None, None


class DiffusionSpliceFn(_StoreFn):
    """SpliceFn followed by the diffusion head's ``insert_action_embedding`` (oft_arch.py:106-123) on the SAME buffer: the plan
    reserves 1 + R (+ 1) rows behind each sample's rows and dxa_diffusion_put_fwd writes the sample's state row (``state`` [B, d], with
    proprio), its time row (``time`` [B, d]) and its R projected noisy-action rows (``proj`` [B R, d]) there.  Backward: the dense
    gradient of the projected rows and of the state rows (the time row has none), then the splice's own backward."""

    @staticmethod
    def forward(ctx, img_feats, proj, time, state, anchor, st: ParamStore, embed_n: str, plan: torch.Tensor, off: torch.Tensor,
                B: int, Sq: int):
        d = img_feats.shape[-1]
        out = K.splice_fwd(plan, st.w(embed_n), img_feats.reshape(-1, d).contiguous())
        K.diffusion_put_(out.view(B, Sq, d), proj.contiguous(), time.contiguous(), off, None if state is None else state.contiguous())
        ctx.st, ctx.embed_n, ctx.ishape, ctx.geom = st, embed_n, img_feats.shape, (B, Sq, d, proj.shape[0] // B)
        ctx.has_state = state is not None
        _use(ctx, st, embed_n)
        ctx.save_for_backward(plan, off)
        return out

    @staticmethod
    def backward(ctx, dout):
        st = ctx.st
        plan, off = ctx.saved_tensors
        B, Sq, d, R = ctx.geom
        dout = dout.contiguous()
        want_state = ctx.has_state and ctx.needs_input_grad[3]
        dproj = dstate = None
        if ctx.needs_input_grad[1] or want_state:
            dproj, dstate = K.diffusion_put_bwd(dout.view(B, Sq, d), off, R, ctx.has_state, want_dstate=want_state)
        d_img = _splice_backward(st, ctx.embed_n, plan, dout, ctx.ishape, ctx.needs_input_grad[0])
        return (d_img, dproj if ctx.needs_input_grad[1] else None, None, dstate) + (None,) * 7


class ActionRowsFn(Function):
    """``extract_action_hidden_states`` (+ ``[:, 1:]`` with proprio; oft_discrete_arch.py:157-162) as the dense [B R, d] operand of the
    lm_head product, one launch per direction.  The backward writes the whole gradient of h (zero off the action rows): the head is
    the only consumer of the decoder output in this policy."""

    @staticmethod
    def forward(ctx, h, off: torch.Tensor, n_rows: int, skip: bool):
        h = h.contiguous()
        ctx.geom = (h.shape[0], h.shape[1], n_rows, skip)
        ctx.save_for_backward(off)
        return K.action_rows_fwd(h, off, n_rows, skip)

    @staticmethod
    def backward(ctx, dy):
        (off,) = ctx.saved_tensors
        B, Sq, n_rows, skip = ctx.geom
        return K.action_rows_bwd(dy.contiguous(), off, B, Sq, n_rows, skip), None, None, None


class ActionNormFn(_StoreFn):
    """``extract_action_hidden_states`` + ``reshape(B, T, A d)`` + ``MLPResNet.layer_norm1`` (oft_arch.py:137-140,203-210,
    oft/action_model/model.py:119,158) in one launch per direction: h [B, Sq, d] -> [B T, A d].  The backward writes the whole
    gradient of h (zero off the action rows): the head is the only consumer of the decoder output in this policy.  Only h and the
    row statistics are kept."""

    @staticmethod
    def forward(ctx, h, anchor, st: ParamStore, wn: str, bn: str, off: torch.Tensor, T: int, A: int, skip: bool, eps: float):
        h = h.contiguous()
        y, mean, rstd = K.action_layernorm_fwd(h, off, st.w(wn), st.w(bn), T, A, skip, eps)
        ctx.st, ctx.wn, ctx.bn, ctx.geom = st, wn, bn, (T, A, skip)
        _use(ctx, st, wn, bn)
        ctx.save_for_backward(h, off, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        st, wn, bn = ctx.st, ctx.wn, ctx.bn
        h, off, mean, rstd = ctx.saved_tensors
        T, A, skip = ctx.geom
        dh, part = K.action_layernorm_bwd(dy.contiguous(), h, off, st.w(wn), mean, rstd, T, A, skip)
        if st.trainable(wn):
            _fold_ln_partials(st, wn, bn, part)
        return dh, None, None, None, None, None, None, None, None, None


class ResidualLinearFn(_StoreFn):
    """act(LN(x) W^T + b) + x: one ``MLPResNetBlock`` (oft/action_model/model.py:83-101: Pre-LN, Linear, ReLU, skip) as
    dxa_layernorm_fwd then ONE product with bias, activation and residual in its epilogue (``aux_out`` keeps the pre-activation for
    the backward); the skip's gradient is added inside the LayerNorm backward."""

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, ln_w: str, ln_b: str, wn: str, bn: str, act: int, eps: float):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        hn, mean, rstd = K.layernorm_fwd(x2, st.w(ln_w), st.w(ln_b), eps)
        W = st.w(wn)
        pre = torch.empty((x2.shape[0], W.shape[0]), device=x.device, dtype=x.dtype)
        y = K.mm_nt(hn, W, bias=st.w(bn), act=act, aux_out=pre, residual=x2)
        ctx.st, ctx.names, ctx.act, ctx.xshape = st, (ln_w, ln_b, wn, bn), act, x.shape
        _use(ctx, st, ln_w, ln_b, wn, bn)
        ctx.save_for_backward(x2, hn, mean, rstd, pre)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        st = ctx.st
        ln_w, ln_b, wn, bn = ctx.names
        x2, hn, mean, rstd, pre = ctx.saved_tensors
        W = st.w(wn)
        dy2 = dy.reshape(-1, W.shape[0]).contiguous()
        dpre = K.act_bwd(pre, dy2, ctx.act)
        _wgrad(st, wn, dpre, hn, W.shape)
        _bgrad(st, bn, dpre)
        dhn = _dx(st, wn, W.shape, dpre)
        dx = _ln_bwd(st, dhn, x2, ln_w, ln_b, mean, rstd, residual=dy2)
        return dx.view(ctx.xshape), None, None, None, None, None, None, None, None


class L1LossFn(Function):
    """loss = |pred - target|.mean() (torch.nn.L1Loss(), oft_arch.py:152); the gradient is the sign (0 at a tie) over n"""

    @staticmethod
    def forward(ctx, pred, target):
        ctx.dtype = pred.dtype
        pred = pred.contiguous()
        if pred.dtype != torch.float32:              # bf16 compute: the loss itself is taken in fp32 (oft_arch.py:149)
            pred = K.cast(pred, torch.float32)
        loss, dpred = K.l1_loss(pred, target.contiguous(), 1.0, want_grad=True)
        ctx.save_for_backward(dpred)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        d = K.scale_dev_(dpred.clone(), g.reshape(1).float().contiguous())
        return (d if ctx.dtype == torch.float32 else K.cast(d, ctx.dtype)), None


class GatherRowsFn(Function):
    """cognition feature = hidden state of the last un-padded token (cogact_arch.py:110-120); output fp32
    (the action head runs in fp32, cogact_arch.py:133)."""

    @staticmethod
    def forward(ctx, x, idx):
        ctx.R, ctx.dtype = x.shape[0], x.dtype
        ctx.save_for_backward(idx)
        return K.gather_rows(x.contiguous(), idx, torch.float32)

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        return K.scatter_rows(dout.contiguous(), idx, ctx.R, ctx.dtype), None


class TokenDropFn(_StoreFn):
    """LabelEmbedder.token_drop (dit.py:80-96)."""

    @staticmethod
    def forward(ctx, z, anchor, st: ParamStore, unc_n: str, drop: torch.Tensor):
        ctx.st, ctx.unc_n = st, unc_n
        _use(ctx, st, unc_n)
        ctx.save_for_backward(drop)
        return K.token_drop(z.contiguous(), st.w32(unc_n).view(-1), drop)

    @staticmethod
    def backward(ctx, dout):
        (drop,) = ctx.saved_tensors
        dz, dunc = K.token_drop_bwd(dout.contiguous(), drop, want_dz=ctx.needs_input_grad[0])
        _vgrad(ctx.st, ctx.unc_n, dunc)
        return dz, None, None, None, None


class DitAssembleFn(_StoreFn):
    """x = cat(t_emb + z_emb, x_emb) + positional_embedding (dit.py:281-286)."""

    @staticmethod
    def forward(ctx, xe, te, ze, anchor, st: ParamStore, pos_n: str):
        ctx.st, ctx.pos_n = st, pos_n
        _use(ctx, st, pos_n)
        return K.dit_assemble_fwd(xe.contiguous(), te.contiguous(), ze.contiguous(), st.w32(pos_n))

    @staticmethod
    def backward(ctx, dh):
        dh = dh.contiguous()
        N, T1, hd = dh.shape
        dxe, dc = K.dit_assemble_bwd(dh)
        if ctx.st.trainable(ctx.pos_n):
            _vgrad(ctx.st, ctx.pos_n, K.colsum(dh.view(N, T1 * hd)))
        return dxe, dc, dc, None, None, None


class MseLossFn(Function):
    """loss = ((eps_hat - eps)**2).mean()  (action_models.py:119-121; the OFT diffusion head, oft_arch.py:154, whose bf16 prediction
    is cast first: the loss is taken in fp32)."""

    @staticmethod
    def forward(ctx, pred, target):
        ctx.dtype = pred.dtype
        pred = pred.contiguous()
        if pred.dtype != torch.float32:
            pred = K.cast(pred, torch.float32)
        loss, dpred = K.mse_loss(pred, target.contiguous(), 1.0, want_grad=True)
        ctx.save_for_backward(dpred)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        # g is the scalar upstream gradient (1.0 for loss.backward(); 1/accum under gradient
        # accumulation): applied on the device, no host sync
        d = K.scale_dev_(dpred.clone(), g.reshape(1).float().contiguous())
        return (d if ctx.dtype == torch.float32 else K.cast(d, ctx.dtype)), None


class ExpectileLossFn(Function):
    """mean(w d^2), d = pred - target, w = tau where d < 0 and 1 - tau elsewhere: the reward head's loss
    (dexbotic/model/muvla/muvla_arch.py:584-587, expectile 0.9)."""

    @staticmethod
    def forward(ctx, pred, target, tau: float):
        loss, dpred = K.expectile_loss(pred.contiguous(), target.contiguous(), tau, 1.0, want_grad=True)
        ctx.save_for_backward(dpred)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return K.scale_dev_(dpred.clone(), g.reshape(1).float().contiguous()), None, None


LMHEAD_SLAB_BYTES = (1 << 31) - 4096        # largest output one launch of the MFMA fast path addresses (tests shrink it)


class LmHeadLossFn(_StoreFn):
    """logits = lm_head(hidden) and the HF causal-LM cross-entropy over the (already shifted) labels
    (dexbotic_arch.py:483-488; transformers/loss/loss_utils.py ForCausalLMLoss): loss = mean over the non-ignored
    rows of logsumexp(logits) - logits[label], in fp32 on the stored logits.  Returns (loss, logits).  The vocabulary
    GEMMs are the only other large contractions of the path (4592 x 152064 x 3584 at the CogACT batch): bf16 runs them
    on the ping-pong MFMA kernel — logits NT, dW = dZ^T H as a TN and dH = dZ W as an NN product, operands as they lie."""

    @staticmethod
    def forward(ctx, hidden, anchor, st: ParamStore, wn: str, labels_shifted: torch.Tensor, n_valid: int):
        return _lm_head_loss_fwd(ctx, hidden, st, wn, labels_shifted, n_valid, None)

    @staticmethod
    def backward(ctx, g, _g_logits):
        return (_lm_head_loss_bwd(ctx, g),) + (None,) * 5


class LmHeadSoftLossFn(_StoreFn):
    """LmHeadLossFn with the NaVILA soft targets (dexbotic/model/navila/loss.py soft_cross_entropy): rows labelled with one of
    ``soft``'s "time" token ids are scored against a Gaussian over those ids, the others against their label; the sum is divided
    by the number of non-ignored rows (``targets.size(0)``), and a batch without any is 0.0, not NaN."""

    @staticmethod
    def forward(ctx, hidden, anchor, st: ParamStore, wn: str, labels_shifted: torch.Tensor, n_valid: int, soft: "K.SoftTokens"):
        return _lm_head_loss_fwd(ctx, hidden, st, wn, labels_shifted, n_valid, soft)

    @staticmethod
    def backward(ctx, g, _g_logits):
        return (_lm_head_loss_bwd(ctx, g),) + (None,) * 6


class LmHeadSampleLossFn(_StoreFn):
    """LmHeadLossFn with MuVLA's reduction (dexbotic/model/muvla/muvla_arch.py:559-576): every sample's row losses are divided by
    that sample's own number of non-ignored rows (at least 1), weighted by 1 + sigmoid(reward_b) when ``reward`` ([B] fp32, on the
    device) is given, and the B results are averaged.  The per-row factor w_b / (max(n_b, 1) B) goes into the cross-entropy
    backward kernel itself (dxa_cross_entropy_rows_bwd): no second pass over the [rows, V] gradient."""

    @staticmethod
    def forward(ctx, hidden, anchor, st: ParamStore, wn: str, labels_shifted: torch.Tensor, B: int, reward):
        return _lm_head_loss_fwd(ctx, hidden, st, wn, labels_shifted, 0, None, samples=(B, reward))

    @staticmethod
    def backward(ctx, g, _g_logits):
        return (_lm_head_loss_bwd(ctx, g),) + (None,) * 6


def _lm_head_loss_fwd(ctx, hidden, st: ParamStore, wn: str, labels_shifted: torch.Tensor, n_valid: int, soft, samples=None):
    """``samples`` = (B, reward [B] fp32 on the device or None): the per-sample normalised, reward-weighted mean of
    LmHeadSampleLossFn instead of the mean over the non-ignored rows (``n_valid`` is then unused)"""
    h2 = hidden.reshape(-1, hidden.shape[-1]).contiguous()
    W = st.w(wn)
    logits = K.mm_nt(h2, W)
    if soft is None:
        row_loss, lse = K.cross_entropy_fwd(logits, labels_shifted)
    else:
        row_loss, lse = K.soft_cross_entropy_fwd(logits, labels_shifted, soft)
    row_w = None
    if samples is not None:
        loss, row_w = K.ce_sample_reduce(row_loss, labels_shifted, samples[1], samples[0], W.shape[0])
    else:
        loss = K.colsum(row_loss.view(-1, 1))
        if n_valid > 0:
            K.scale_(loss, 1.0 / n_valid)
        elif soft is None:
            loss = loss * float("nan")                          # F.cross_entropy(mean) over zero targets
    ctx.st, ctx.wn, ctx.n_valid, ctx.hshape, ctx.soft, ctx.weighted = st, wn, n_valid, hidden.shape, soft, row_w is not None
    _use(ctx, st, wn)
    ctx.save_for_backward(h2, logits, lse, labels_shifted, *(() if row_w is None else (row_w,)))
    ctx.mark_non_differentiable(logits)
    return loss.view(()), logits.view(*hidden.shape[:-1], W.shape[0])


def _lm_head_loss_bwd(ctx, g):
    st, wn = ctx.st, ctx.wn
    h2, logits, lse, labels, *row_w = ctx.saved_tensors
    W = st.w(wn)
    gs, scale = g.reshape(1).float().contiguous(), 1.0 / max(ctx.n_valid, 1)
    if ctx.weighted:
        dz = K.cross_entropy_rows_bwd(logits, labels, lse, gs, 1.0, row_w[0])     # each row's 1 / (n_b B) is inside its weight
    elif ctx.soft is None:
        dz = K.cross_entropy_bwd(logits, labels, lse, gs, scale)
    else:
        dz = K.soft_cross_entropy_bwd(logits, labels, lse, gs, scale, ctx.soft)
    if st.trainable(wn):
        # the fp32 dW of the full vocabulary (152064 x 3584 x 4 B = 2.18 GB) is past the 2 GiB the MFMA fast path addresses
        # in one output: written in row slabs of < 2 GiB (column slices of dZ), each on the fast path
        g, acc, mir = st.g(wn), st.accum_flag(wn), st.mirror_out(wn)
        V, d_ = g.shape
        slab = max(256, min(V, LMHEAD_SLAB_BYTES // (4 * d_) // 256 * 256))
        for lo in range(0, V, slab):
            hi = min(V, lo + slab)
            K.mm_tn(dz[:, lo:hi], h2, out=g[lo:hi], accumulate=acc, mirror=None if mir is None else mir[lo:hi])
        st.mark_written(wn)
    dh = None
    if ctx.needs_input_grad[0]:
        dh = K.mm_nn(dz, W).view(ctx.hshape)
    return dh


class BinPolicyLossFn(_StoreFn):
    """The clipped GRPO policy loss of the discrete policy on its action rows (dexbotic/exp/rl/rl_trainer.py:380-399, 488-506):
    bin logits = rows W_b^T with W_b the last NB = num_bins - 1 rows of ``lm_head.weight`` as their own operand, log-probability and
    entropy of the taken bins at ``temperature`` (dxa_bin_logprob_fwd), the four masked sums and d loss / d log_prob
    (dxa_ppo_clip_fwd).  Returns (loss = sums[0] / denom, logp [rows], entropy [rows], sums [4]); only the loss is differentiable.
    ``denom`` None: the mask's own count.  The reference forms the [rows, V] logits and slices them; every vocabulary row outside
    the slice gets a zero gradient there, so here the three head products run over NB columns and nothing V wide is kept: the
    backward writes dZ over Z in place, dW_b into the last NB rows of the gradient slot and exact zeros into the rows before them
    when this is the slot's first write of the step (they are left alone when accumulating)."""

    @staticmethod
    def forward(ctx, rows, anchor, st: ParamStore, wn: str, NB: int, bins, old_logp, adv, mask, temperature: float,
                clip_low: float, clip_high: float, denom: Optional[float]):
        rows = rows.contiguous()
        W = st.w(wn)
        Z = K.mm_nt(rows, W[W.shape[0] - NB:])
        logp, entropy, lse = K.bin_logprob_fwd(Z, bins, temperature)
        loss, sums, coef = K.ppo_clip_fwd(logp, old_logp, adv, mask, clip_low, clip_high, denom)
        ctx.st, ctx.wn, ctx.NB, ctx.temperature = st, wn, NB, float(temperature)
        _use(ctx, st, wn)
        ctx.save_for_backward(rows, Z, lse, bins, coef)
        ctx.mark_non_differentiable(logp, entropy, sums)
        return loss.view(()), logp, entropy, sums

    @staticmethod
    def backward(ctx, g, _g_logp, _g_entropy, _g_sums):
        st, wn, NB = ctx.st, ctx.wn, ctx.NB
        rows, Z, lse, bins, coef = ctx.saved_tensors
        W = st.w(wn)
        V = W.shape[0]
        dz = K.bin_logprob_bwd(Z, bins, lse, coef, g.reshape(1).float().contiguous(), ctx.temperature, out=Z)
        if st.trainable(wn):
            gw, acc, mir = st.g(wn), st.accum_flag(wn), st.mirror_out(wn)
            if not acc and V > NB:
                gw[:V - NB].zero_()
                st._own_grad_write()
                if mir is not None:
                    mir[:V - NB].zero_()
            K.mm_tn(dz, rows, out=gw[V - NB:], accumulate=acc, mirror=None if mir is None else mir[V - NB:])
            st.mark_written(wn)
        dh = K.mm_nn(dz, W[V - NB:]) if ctx.needs_input_grad[0] else None
        return (dh,) + (None,) * 12


class AddPosFn(_StoreFn):
    """x[N,T,C] + pos[T,C] (learned position embedding of the SigLIP tower, HF siglip/modeling_siglip.py
    SiglipVisionEmbeddings); d_pos = sum over N of dy."""

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, pos_name: str):
        N, T, C_ = x.shape
        pos = st.w(pos_name).unsqueeze(0).expand(N, T, C_).contiguous()
        ctx.st, ctx.pos_name, ctx.shape = st, pos_name, (N, T, C_)
        _use(ctx, st, pos_name)
        return K.add(x.contiguous(), pos)

    @staticmethod
    def backward(ctx, dy):
        st, (N, T, C_) = ctx.st, ctx.shape
        dy = dy.contiguous()
        if st.trainable(ctx.pos_name):
            # rows of [N, T*C]: the column sums are the per-position gradient
            K.colsum(dy.view(N, T * C_), out=st.g(ctx.pos_name).view(-1), accumulate=st.accum_flag(ctx.pos_name))
            st.mark_written(ctx.pos_name)
        return dy, None, None, None


class MseLossRowsFn(Function):
    """sample-weighted eps-MSE (hybrid_cogact_arch.py:168-173): sum_r w_r mean(d_r^2) / (sum_r w_r + 1e-6)"""

    @staticmethod
    def forward(ctx, pred, target, row_w):
        loss, dpred = K.mse_loss_rows(pred.contiguous(), target.contiguous(), row_w.float().contiguous(), 1.0, want_grad=True)
        ctx.save_for_backward(dpred)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return K.scale_dev_(dpred.clone(), g.reshape(1).float().contiguous()), None, None


class ScaleFn(Function):
    """y = x * s in the tensor's dtype (token embeddings * sqrt(hidden), pi0_arch.py:247-250)"""

    @staticmethod
    def forward(ctx, x, s: float):
        ctx.s = s
        return ScaleFn._mul(x, s)

    @staticmethod
    def _mul(x, s):
        x = x.contiguous()
        if x.dtype == torch.float32:
            return K.scale_(x.clone(), s)
        return K.cast(K.scale_(K.cast(x, torch.float32), s), x.dtype)

    @staticmethod
    def backward(ctx, dy):
        return ScaleFn._mul(dy, ctx.s), None


# ------------------------------------------------------------------- mixture-of-transformers layer (pi0, pi0.5, DM0)
@dataclass
class GemmaLayerSpec:
    """parameter names + shapes of one Gemma decoder layer of one expert (model/llm/gemma.py)"""
    ln1: str
    qkv: Tuple[str, ...]
    o: str
    ln2: str
    gu: Tuple[str, ...]
    down: str
    d: int
    F: int
    eps: float


def gemma_norm_w(st: ParamStore, name: str) -> torch.Tensor:
    """fp32 (1 + w) of a GemmaRMSNorm weight (HF multiplies the normalised fp32 activations by 1 + w.float()): the one place that
    forms it.  One tensor per name, allocated once and re-formed IN PLACE when the weights have moved since that name was last
    formed (ParamStore.weights_key): forward and backward of a step share it (the two aten launches per use were 290 launches of a
    pi0 step), and its address never changes, so nothing a captured graph holds is ever freed under it.  The refresh itself is host
    code: whoever replays a captured graph that reads these tensors calls ``gemma_norm_refresh`` first (model/mot.py's
    ``_run_sampler`` does), or the replay normalises with the 1 + w of the capture."""
    key = st.weights_key()
    cache = st.__dict__.setdefault("_gemma_norm_cache", {})
    ent = cache.get(name)
    if ent is None:
        ent = cache[name] = [None, torch.empty(st.slots[name].shape, device=st.device, dtype=torch.float32)]
    if ent[0] != key:
        torch.add(st.w(name).float(), 1.0, out=ent[1])
        ent[0] = key
    return ent[1]


def gemma_norm_refresh(st: ParamStore) -> None:
    """bring every (1 + w) formed so far up to date: before the replay of a captured graph, which runs no host code of its own"""
    for name in st.__dict__.get("_gemma_norm_cache", ()):
        gemma_norm_w(st, name)


def gemma_pre_attention(st: ParamStore, sp: GemmaLayerSpec, x, nq: int):
    """first half of one expert's Gemma layer on x [M, d]: input GemmaRMSNorm, then the fused q/k/v product
    -> (h, rstd, qkv [M, nq = (Hq + 2 Hkv) * D])"""
    h, rstd = K.rmsnorm_fwd(x, gemma_norm_w(st, sp.ln1), sp.eps)
    return h, rstd, K.mm_nt(h, st.w(*sp.qkv, shape=(nq, sp.d)))


def gemma_post_attention(st: ParamStore, sp: GemmaLayerSpec, x, a):
    """second half, a [M, Hq * D] = this expert's rows of the attention output: x + o_proj(a); then + down(gelu_tanh(gate) * up) of
    the post-attention GemmaRMSNorm -> (y, what the backward reads besides a: r, rstd2, h2, gu, act)"""
    r = K.mm_nt(a, st.w(sp.o), residual=x)
    h2, rstd2 = K.rmsnorm_fwd(r, gemma_norm_w(st, sp.ln2), sp.eps)
    gu = K.mm_nt(h2, st.w(*sp.gu, shape=(2 * sp.F, sp.d)))
    act = K.glu_fwd(gu, L.ACT_GELU_TANH)
    return K.mm_nt(act, st.w(sp.down), residual=r), (r, rstd2, h2, gu, act)


def qwen3_pre_attention(st: ParamStore, sp: Qwen2LayerSpec, x):
    """first half of one expert's Qwen3 layer on x [M, d]: input RMSNorm (plain weight), then the fused q/k/v product without bias
    -> (h, rstd, qkv [M, (Hq + 2 Hkv) * D]); the per-head q/k norm runs in the RoPE / split pass that follows"""
    h, rstd = K.rmsnorm_fwd(x, st.w(sp.ln1), sp.eps)
    return h, rstd, K.mm_nt(h, st.w(*sp.qkv_w, shape=((sp.Hq + 2 * sp.Hkv) * sp.D, sp.d)))


def qwen3_post_attention(st: ParamStore, sp: Qwen2LayerSpec, x, a, keep: bool = True):
    """second half, a [M, Hq * D] = this expert's rows of the attention output: x + o_proj(a); then + down(silu(gate) * up) of the
    post-attention RMSNorm -> (y, what the backward reads besides a: r, rstd2, h2, gu, act).  ``keep`` = False (no backward will
    come): the pre-activations gu are not stored (None) where the product's SwiGLU epilogue applies — the same bits either way
    (kernels.mm_nt_swiglu)."""
    r = K.mm_nt(a, st.w(sp.o_w), residual=x)
    h2, rstd2 = K.rmsnorm_fwd(r, st.w(sp.ln2), sp.eps)
    w_gu = st.w(*sp.gu_w, shape=(2 * sp.F, sp.d))
    if K.swiglu_gemm_supported(h2, w_gu, keep_pre=keep):
        act, gu = K.mm_nt_swiglu(h2, w_gu, keep_pre=keep)
    else:
        gu = K.mm_nt(h2, w_gu)
        act = K.swiglu_fwd(gu)
    return K.mm_nt(act, st.w(sp.down_w), residual=r), (r, rstd2, h2, gu, act)


def adarms_pre_attention(st: ParamStore, sp: GemmaLayerSpec, x, mod1, nq: int):
    """first half of the pi0.5 action expert's layer on x [M, d]: adaptive RMSNorm with mod1 [B, 3 d] = [scale | shift | gate], then
    the fused q/k/v product -> (h, rstd, qkv [M, nq])"""
    h, rstd, _ = K.adarms_fwd(x, mod1, sp.eps)
    return h, rstd, K.mm_nt(h, st.w(*sp.qkv, shape=(nq, sp.d)))


def adarms_post_attention(st: ParamStore, sp: GemmaLayerSpec, x, a, mod1, mod2):
    """second half: o_proj; r = x + o * gate1 and the post-attention adaptive norm of r in ONE launch; GeGLU; r + down * gate2
    -> (y, what the backward reads besides a: ob, r, rstd2, h2, gu, act, mb)"""
    d = sp.d
    ob = K.mm_nt(a, st.w(sp.o))
    h2, rstd2, r = K.adarms_fwd(x, mod2, sp.eps, branch=ob, gate_prev=mod1[:, 2 * d:])
    gu = K.mm_nt(h2, st.w(*sp.gu, shape=(2 * sp.F, d)))
    act = K.glu_fwd(gu, L.ACT_GELU_TANH)
    mb = K.mm_nt(act, st.w(sp.down))
    return K.gated_residual_fwd(r, mb, mod2[:, 2 * d:]), (ob, r, rstd2, h2, gu, act, mb)


# The three kinds of expert a mixture layer runs, told from the layer spec.  Each kind is four plain functions with one signature per
# role (the forward halves above, their backwards below); MotLayerFn is the sequence around them.  ``dst`` = (q, k, v, q0, kv0): the
# shared q / k / v and this expert's first slot in them; ``rope`` = (cos_t, sin_t, pos); ``tok`` = (B, S_e, Hq, Hkv, D); ``mods`` /
# ``dmods`` = (mod1, mod2) and their gradients, None for the kinds without adaptive norms.
def _mot_kind(sp) -> str:
    if isinstance(sp, Qwen2LayerSpec):
        assert sp.qk_norm is not None, "the mixture's Qwen experts are Qwen3 layers (per-head q/k norm)"
        return "qwen3"
    return "adarms" if sp.ln1 is None else "gemma"            # (AdaRMSGemmaExpert's norms own no gain: ln1 / ln2 are None)


def _mot_params(sp):
    """(what the pre-attention half's backward writes, what the post-attention half's does)"""
    if isinstance(sp, Qwen2LayerSpec):
        return (sp.ln1, sp.qkv_w, sp.qk_norm), (sp.o_w, sp.ln2, sp.gu_w, sp.down_w)
    return (sp.ln1, sp.qkv), (sp.o, sp.ln2, sp.gu, sp.down)


def _nq(tok) -> int:
    _, _, Hq, Hkv, D = tok
    return (Hq + 2 * Hkv) * D


def _rope_pre(h, rstd, qkv, dst, rope, tok):
    """RoPE of one expert's fused q/k/v into the shared tensors.  dxa_rope_split_at writes q, k and v at ONE offset"""
    q, k, v, q0, kv0 = dst
    assert q0 == kv0
    K.rope_split_into(qkv, q, k, v, kv0, *rope, *tok)
    return h, rstd


def _gemma_pre(st, sp, x, mods, dst, rope, tok, keep):
    return _rope_pre(*gemma_pre_attention(st, sp, x, _nq(tok)), dst, rope, tok)


def _adarms_pre(st, sp, x, mods, dst, rope, tok, keep):
    return _rope_pre(*adarms_pre_attention(st, sp, x, mods[0], _nq(tok)), dst, rope, tok)


def _qwen3_pre(st, sp, x, mods, dst, rope, tok, keep):
    """the per-head q/k norm + RoPE launch has offsets of its own for q and for k / v; its backward reads qkv and the heads' rstd"""
    h, rstd, qkv = qwen3_pre_attention(st, sp, x)
    rstd_qk = K.qknorm_rope_split_into(qkv, *dst, st.w(sp.qk_norm[0]), st.w(sp.qk_norm[1]), sp.eps, *rope, *tok, want_rstd=keep)
    return h, rstd, qkv if keep else None, rstd_qk


def _gemma_post(st, sp, x, a, mods, keep):
    return gemma_post_attention(st, sp, x, a)


def _adarms_post(st, sp, x, a, mods, keep):
    return adarms_post_attention(st, sp, x, a, *mods)


def _qwen3_post(st, sp, x, a, mods, keep):
    return qwen3_post_attention(st, sp, x, a, keep=keep)


def _lin_bwd(st: ParamStore, names, shape, dy, x) -> torch.Tensor:
    """backward of y = x W^T for the fused view W over ``names``: -> dX; dW goes into the arena"""
    dx = _dx(st, names, shape, dy)
    _wgrad(st, names, dy, x, shape)
    return dx


def _rms_bwd(st: ParamStore, name: str, w, dy, x, rstd, residual) -> torch.Tensor:
    """backward of an RMSNorm with gain ``w`` (parameter ``name``) on the row x it normalised: -> dx + residual; dw into the arena"""
    tr = st.trainable(name)
    dx, _ = K.rmsnorm_bwd(dy, x, w, rstd, dw_out=st.g(name) if tr else None, accumulate=st.accum_flag(name), want_dw=tr,
                          residual=residual)
    if tr:
        st.mark_written(name)
    return dx


def _gemma_post_bwd(st, sp, dy, a, kept, mods, dmods):
    """-> (da, dr): the gradient of this expert's attention rows and of the residual stream between the two halves"""
    r, rstd2, h2, gu, act = kept
    dgu = K.glu_bwd(gu, _lin_bwd(st, sp.down, (sp.d, sp.F), dy, act), L.ACT_GELU_TANH)
    dh2 = _lin_bwd(st, sp.gu, (2 * sp.F, sp.d), dgu, h2)
    del dgu
    dr = _rms_bwd(st, sp.ln2, gemma_norm_w(st, sp.ln2), dh2, r, rstd2, dy)
    return _lin_bwd(st, sp.o, (sp.d, a.shape[1]), dr, a), dr


def _qwen3_post_bwd(st, sp, dy, a, kept, mods, dmods):
    r, rstd2, h2, gu, act = kept
    dgu = K.swiglu_bwd(gu, _lin_bwd(st, sp.down_w, (sp.d, sp.F), dy, act))
    dh2 = _lin_bwd(st, sp.gu_w, (2 * sp.F, sp.d), dgu, h2)
    del dgu
    dr = _rms_bwd(st, sp.ln2, st.w(sp.ln2), dh2, r, rstd2, dy)
    return _lin_bwd(st, sp.o_w, (sp.d, a.shape[1]), dr, a), dr


def _adarms_post_bwd(st, sp, dy, a, kept, mods, dmods):
    """gated add, GeGLU, fused adaptive norm + gated add, o_proj; writes all of dmod2 and the gate third of dmod1"""
    ob, r, rstd2, h2, gu, act, mb = kept
    (mod1, mod2), (dmod1, dmod2), d = mods, dmods, sp.d
    dmb = K.gated_residual_bwd(dy, mb, mod2[:, 2 * d:], dmod2[:, 2 * d:])
    dgu = K.glu_bwd(gu, _lin_bwd(st, sp.down, (d, sp.F), dmb, act), L.ACT_GELU_TANH)
    dh2 = _lin_bwd(st, sp.gu, (2 * sp.F, d), dgu, h2)
    del dgu
    dr, dob = K.adarms_bwd(dh2, r, mod2, rstd2, dmod2, residual=dy, branch=ob, gate_prev=mod1[:, 2 * d:], dgate_prev=dmod1[:, 2 * d:])
    return _lin_bwd(st, sp.o, (d, a.shape[1]), dob, a), dr


def _gemma_pre_bwd(st, sp, x, kept, dr, dqkv3, off, rope, tok, mods, dmods):
    """-> dx: this expert's slots [off, off + S_e) of the shared dq / dk / dv back through RoPE, the q/k/v product and the norm"""
    h, rstd = kept
    dh = _lin_bwd(st, sp.qkv, (_nq(tok), sp.d), K.rope_merge_from(*dqkv3, off, *rope, *tok), h)              # (no slicing copies)
    return _rms_bwd(st, sp.ln1, gemma_norm_w(st, sp.ln1), dh, x, rstd, dr)


def _qwen3_pre_bwd(st, sp, x, kept, dr, dqkv3, off, rope, tok, mods, dmods):
    h, rstd, qkv, rstd_qk = kept
    tr_qk = all(st.trainable(n) for n in sp.qk_norm)
    dqkv, part = K.qknorm_rope_merge_from(*dqkv3, off, qkv, rstd_qk, st.w(sp.qk_norm[0]), st.w(sp.qk_norm[1]), *rope, *tok,
                                          want_dw=tr_qk)
    if tr_qk:
        _bgrad(st, sp.qk_norm, part)       # rows of (dw_q | dw_k) partial sums, folded by the column sum as Qwen2LayerFn does
    dh = _lin_bwd(st, sp.qkv_w, (_nq(tok), sp.d), dqkv, h)
    del dqkv
    return _rms_bwd(st, sp.ln1, st.w(sp.ln1), dh, x, rstd, dr)


def _adarms_pre_bwd(st, sp, x, kept, dr, dqkv3, off, rope, tok, mods, dmods):
    """writes the scale and shift thirds of dmod1"""
    h, rstd = kept
    dh = _lin_bwd(st, sp.qkv, (_nq(tok), sp.d), K.rope_merge_from(*dqkv3, off, *rope, *tok), h)
    return K.adarms_bwd(dh, x, mods[0], rstd, dmods[0], residual=dr)[0]


# q_apart: the kind's RoPE launch takes an offset for q apart from the one for k / v
_MotKind = namedtuple("_MotKind", "pre post post_bwd pre_bwd q_apart")
_MOT_KINDS = {
    "gemma": _MotKind(_gemma_pre, _gemma_post, _gemma_post_bwd, _gemma_pre_bwd, False),
    "qwen3": _MotKind(_qwen3_pre, _qwen3_post, _qwen3_post_bwd, _qwen3_pre_bwd, True),
    "adarms": _MotKind(_adarms_pre, _adarms_post, _adarms_post_bwd, _adarms_pre_bwd, False),
}


class MotLayerFn(_StoreFn):
    """One layer of a mixture of transformers for its two experts at once (pi0 pi0_arch.py:130-216, pi0.5 pi05_arch.py:134-238, DM0
    dm0_arch.py:145-268): per expert norm -> fused q/k/v -> RoPE written straight into the q / k / v both experts share; ONE
    attention over all tokens with the block mask as q_limit / key_valid; per expert o_proj + residual -> norm -> gated MLP ->
    residual.  What an expert's halves are is its kind (_mot_kind): Gemma (pi0's two experts, the pi0.5 llm), Qwen3 (DM0: plain
    gains, per-head q/k norm inside the RoPE launch, SwiGLU) or the pi0.5 action expert, whose norms are adaptive (``mod1`` /
    ``mod2`` [B, 3 d_a] = [scale | shift | gate], dense layers of the flow-time embedding evaluated OUTSIDE the layer; None for the
    other policies) and whose residual adds are gated.  The rotary tables are the llm's for both experts.  ``skip_post0``: the last
    layer's llm half after attention feeds only prefix_out, which the loss never reads — it is not computed (the reference computes
    it and its parameters get no gradient); that layer's llm q_proj (and DM0's q_norm) still get their zero gradient written."""

    @staticmethod
    def _run(st: ParamStore, sps, geom, skip_post0: bool, x0, x1, mod1, mod2, cos_t, sin_t, pos0, pos1, q_limit, key_valid,
             keep: bool = True, kv=None, kv0: int = 0):
        """the layer's forward launches -> ((y0, y1), what the backward reads besides its inputs, or None): the training forward,
        its recompute, the no-grad forward and the sampler all run this one sequence.  An expert whose x is None (its S in ``geom``
        is 0) is left out (the sampler: the prefix pass runs the llm alone, the Euler steps the action expert alone).  ``keep`` =
        False: nothing is kept for a backward (no rstd of the heads, no SwiGLU pre-activations).  ``kv`` (with ``keep`` = False
        only) = (k, v) [B, Hkv, cap, D] buffers: this call's keys / values are WRITTEN at [kv0, kv0 + S) and attention reads
        [0, kv0 + S) — the sampler's prefix pass fills [0, P), every Euler step the slots behind it; no concatenation, no copy."""
        assert kv is None or not keep, "a backward must not read keys / values out of a buffer that the next step overwrites"
        B, S0, S1, Hq, Hkv, D = geom
        S = S0 + S1
        xs, Ss, poss, mods = (x0, x1), (S0, S1), (pos0, pos1), (mod1, mod2)
        live = [i for i in range(2) if xs[i] is not None]
        assert all(Ss[i] > 0 for i in live) and sum(Ss[i] for i in live) == S
        kinds = {i: _MOT_KINDS[_mot_kind(sps[i])] for i in live}
        dev, dtype = xs[live[0]].device, xs[live[0]].dtype
        k, v = kv if kv is not None else (torch.empty((B, Hkv, S, D), device=dev, dtype=dtype) for _ in range(2))
        # the queries' offset: a kind whose RoPE launch writes q, k and v at ONE offset gets, with ``kv``, a scratch tensor of the
        # buffer's capacity for its queries, of which attention reads the window
        q0, q_cap = (0, S) if kv is None or all(kd.q_apart for kd in kinds.values()) else (kv0, k.shape[2])
        qb = torch.empty((B, Hq, q_cap, D), device=dev, dtype=dtype)
        pre, off = [None, None], 0
        for i in live:
            pre[i] = kinds[i].pre(st, sps[i], xs[i], mods, (qb, k, v, q0 + off, kv0 + off), (cos_t, sin_t, poss[i]),
                                  (B, Ss[i], Hq, Hkv, D), keep)
            off += Ss[i]
        q = qb if q_cap == S else qb[:, :, q0:q0 + S]
        ka, va = (k, v) if k.shape[2] == kv0 + S else (k[:, :, :kv0 + S], v[:, :, :kv0 + S])
        o = torch.empty((B, S, Hq, D), device=dev, dtype=dtype)
        lse = K.attn_fwd(q, ka, va, o.permute(0, 2, 1, 3), causal=False, scale=D ** -0.5, q_limit=q_limit, key_valid=key_valid)
        ys, post, off = [None, None], [None, None], 0
        for i in live:
            if not (i == 0 and skip_post0):
                a = o[:, off:off + Ss[i]].reshape(B * Ss[i], Hq * D).contiguous()
                ys[i], kept = kinds[i].post(st, sps[i], xs[i], a, mods, keep)
                post[i] = (a, *kept)
            off += Ss[i]
        return (ys[0], ys[1]), ((q, k, v, o, lse), pre[0], pre[1], post[0], post[1]) if keep else None

    @staticmethod
    def forward(ctx, x0, x1, mod1, mod2, anchor, st: ParamStore, sp0, sp1, geom, cos_t, sin_t, pos0, pos1, q_limit, key_valid,
                skip_post0: bool):
        sps = (sp0, sp1)
        ys, kept = MotLayerFn._run(st, sps, geom, skip_post0, x0, x1, mod1, mod2, cos_t, sin_t, pos0, pos1, q_limit, key_valid)
        ctx.st, ctx.sps, ctx.geom, ctx.skip_post0 = st, sps, geom, skip_post0
        for i, sp in enumerate(sps):
            before, after = _mot_params(sp)
            _use(ctx, st, *before)
            if not (i == 0 and skip_post0):
                _use(ctx, st, *after)
        ctx.aux = (cos_t, sin_t, pos0, pos1, q_limit, key_valid)
        ctx.recompute = _recompute(ctx, st)
        if ctx.recompute:
            ctx.save_for_backward(x0, x1, mod1, mod2)
        else:
            ctx.counts = [len(g or ()) for g in kept]           # the layout of what is saved: each group's length, by kind
            ctx.save_for_backward(x0, x1, mod1, mod2, *[t for g in kept for t in g or ()])
        if skip_post0:
            return x0.new_zeros((0,)), ys[1]                   # placeholder, never read downstream
        return ys

    @staticmethod
    def backward(ctx, dy0, dy1):
        """post-attention backward for expert 0 then 1, the attention backward, pre-attention backward for expert 0 then 1: the
        weight-gradient coalescing (_wgrad, _bgrad) goes by this order"""
        st, sps, skip_post0 = ctx.st, ctx.sps, ctx.skip_post0
        B, S0, S1, Hq, Hkv, D = ctx.geom
        cos_t, sin_t, pos0, pos1, q_limit, key_valid = ctx.aux
        x0, x1, mod1, mod2, *flat = ctx.saved_tensors
        if ctx.recompute:
            kept = MotLayerFn._run(st, sps, ctx.geom, skip_post0, x0, x1, mod1, mod2, cos_t, sin_t, pos0, pos1, q_limit, key_valid)[1]
        else:
            it = iter(flat)
            kept = [tuple(next(it) for _ in range(n)) for n in ctx.counts]
        (q, k, v, o, lse), pre, post = kept[0], kept[1:3], kept[3:5]
        del flat, kept
        kinds = [_MOT_KINDS[_mot_kind(sp)] for sp in sps]
        xs, Ss, poss, dys, mods = (x0, x1), (S0, S1), (pos0, pos1), (dy0, dy1), (mod1, mod2)
        dmods = (None, None) if mod1 is None else (torch.empty_like(mod1), torch.empty_like(mod2))
        S = S0 + S1
        do = torch.zeros((B, S, Hq, D), device=q.device, dtype=q.dtype)
        drs, off = [None, None], 0
        for i in range(2):
            if not (i == 0 and skip_post0):
                a, *kept_i = post[i]
                da, drs[i] = kinds[i].post_bwd(st, sps[i], dys[i].contiguous(), a, kept_i, mods, dmods)
                do[:, off:off + Ss[i]].copy_(da.view(B, Ss[i], Hq, D))
                del a, kept_i, da
            off += Ss[i]
        del post
        do_h = K.permute_bshd(do, B, S, Hq, D, True)                       # head-major dO for the GQA fold
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        K.attn_bwd(q, k, v, o.permute(0, 2, 1, 3), lse, do_h, dq, dk, dv, causal=False, scale=D ** -0.5,
                   q_limit=q_limit, key_valid=key_valid)
        dxs, off = [], 0
        for i in range(2):
            dxs.append(kinds[i].pre_bwd(st, sps[i], xs[i], pre[i], drs[i], (dq, dk, dv), off, (cos_t, sin_t, poss[i]),
                                   (B, Ss[i], Hq, Hkv, D), mods, dmods))
            off += Ss[i]
        return (dxs[0], dxs[1], *dmods) + (None,) * 12


def mot_layer(st: ParamStore, sps, geom, skip_post0: bool, x0, x1, mod1, mod2, cos_t, sin_t, pos0, pos1, q_limit, key_valid,
              kv=None, kv0: int = 0):
    """one mixture layer as the policies call it -> (y0, y1): through autograd when gradients are on, MotLayerFn._run alone
    otherwise (the same launches: the same bits) — and then with the sampler's ``kv`` / ``kv0``"""
    if torch.is_grad_enabled():
        assert kv is None
        anchor = st.params[_mot_params(sps[1])[1][-1]]                     # the action expert's down_proj
        return MotLayerFn.apply(x0, x1, mod1, mod2, anchor, st, sps[0], sps[1], geom, cos_t, sin_t, pos0, pos1, q_limit, key_valid,
                                skip_post0)
    return MotLayerFn._run(st, sps, geom, skip_post0, x0, x1, mod1, mod2, cos_t, sin_t, pos0, pos1, q_limit, key_valid, keep=False,
                           kv=kv, kv0=kv0)[0]


class AdaRMSNormFn(Function):
    """adaptive RMSNorm on its own (the action expert's final norm, whose gate nothing reads: that third of dmod is zero)"""

    @staticmethod
    def forward(ctx, x, mod, eps: float):
        y, rstd, _ = K.adarms_fwd(x, mod, eps)
        ctx.save_for_backward(x, mod, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mod, rstd = ctx.saved_tensors
        dmod = torch.zeros_like(mod)
        dx, _ = K.adarms_bwd(dy.contiguous(), x, mod, rstd, dmod)
        return dx, dmod, None


class FusedLinearFn(_StoreFn):
    """y = x W^T + b for W / b the fused views over ADJACENT parameters (``wn`` / ``bn``: tuples of names registered as one group
    each): the 2 L + 1 ``dense`` layers of the pi0.5 action expert's adaptive norms as ONE product, one dW product, one column sum"""

    @staticmethod
    def forward(ctx, x, anchor, st: ParamStore, wn: Tuple[str, ...], bn: Tuple[str, ...], wshape):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        y = K.mm_nt(x2, st.w(*wn, shape=wshape), bias=st.w(*bn, shape=(wshape[0],)))
        ctx.st, ctx.wn, ctx.bn, ctx.wshape, ctx.xshape = st, wn, bn, tuple(wshape), x.shape
        _use(ctx, st, wn, bn)
        ctx.save_for_backward(x2)
        return y.view(*x.shape[:-1], wshape[0])

    @staticmethod
    def backward(ctx, dy):
        st = ctx.st
        x2, = ctx.saved_tensors
        dy2 = dy.reshape(-1, ctx.wshape[0]).contiguous()
        _wgrad(st, ctx.wn, dy2, x2, ctx.wshape)
        _bgrad(st, ctx.bn, dy2)
        dx = _dx(st, ctx.wn, ctx.wshape, dy2).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        return dx, None, None, None, None, None


# ------------------------------------------------------------------ small differentiable pieces (MemVLA memory modules)
class AddFn(Function):
    """a + b (same shape): residual connections outside the fused blocks"""

    @staticmethod
    def forward(ctx, a, b):
        return K.add(a.contiguous(), b.contiguous())

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


class ForkFn(Function):
    """x -> n aliases of x, one per consumer: the sum of the consumers' gradients is then library launches (dxa_add) instead of
    the autograd engine's own at::add on a tensor that fans out (the MemVLA retrieval path is built from small Functions)"""

    @staticmethod
    def forward(ctx, x, n=2):
        ctx.n = n
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g for g in gs if g is not None]
        if not gs:
            return None, None
        acc = gs[0].contiguous()
        for g in gs[1:]:
            acc = K.add(acc, g.contiguous())
        return acc, None


class CatLastFn(Function):
    """[R, Da] , [R, Db] -> [R, Da + Db] (torch.cat(dim=-1) of the gate-fusion input, memvla_arch.py:176-180) with the
    library's 2-D copy; the backward hands the two column blocks back as contiguous tensors"""

    @staticmethod
    def forward(ctx, a, b):
        R, Da = a.shape
        Db = b.shape[1]
        ctx.dims = (Da, Db)
        out = torch.empty((R, Da + Db), device=a.device, dtype=a.dtype)
        K.copy2d(a.contiguous(), out[:, :Da], Da, Da)
        K.copy2d(b.contiguous(), out[:, Da:], Db, Db)
        return out

    @staticmethod
    def backward(ctx, dy):
        Da, Db = ctx.dims
        R = dy.shape[0]
        da = torch.empty((R, Da), device=dy.device, dtype=dy.dtype)
        db = torch.empty((R, Db), device=dy.device, dtype=dy.dtype)
        K.copy2d(dy[:, :Da], da, Da, Da)
        K.copy2d(dy[:, Da:], db, Db, Db)
        return da, db


class AttnFn(Function):
    """softmax(q k^T / sqrt(D)) v for [B,S,H,D] VIEWS (any strides with D contiguous) -> [B,Sq,H*D]: the cross
    attention of CrossTransformerBlock (memvla_arch.py:84-127) and of the DiT per-attention (nn.MultiheadAttention,
    memvla/action_model/dit.py:158-185).  ``drop_mask`` ([B,H,Sq,Sk], entries 0 or 1/(1-p)): SDPA's dropout_p on the
    attention weights (memvla_arch.py:120-123), the mask drawn by the caller.  ``kv_end`` ([B] int32): sample b attends to its
    keys [0, kv_end[b]) only (the padded banks of the 'parallel_stream' memory); dk = dv = 0 behind them."""

    @staticmethod
    def forward(ctx, q, k, v, drop_mask=None, kv_end=None):
        B, Sq, H, D = q.shape
        o = torch.empty((B, Sq, H, D), device=q.device, dtype=q.dtype)
        lse = K.attn_fwd(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), o.permute(0, 2, 1, 3),
                         causal=False, scale=D ** -0.5, kv_end=kv_end, drop_mask=drop_mask)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.drop_mask, ctx.kv_end = drop_mask, kv_end
        return o.view(B, Sq, H * D)

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        B, Sq, H, D = q.shape
        do = do.contiguous().view(B, Sq, H, D)
        dq, dk, dv = torch.empty(q.shape, device=q.device, dtype=q.dtype), torch.empty(k.shape, device=q.device, dtype=q.dtype), \
            torch.empty(v.shape, device=q.device, dtype=q.dtype)
        P = lambda t: t.permute(0, 2, 1, 3)
        K.attn_bwd(P(q), P(k), P(v), P(o), lse, P(do), P(dq), P(dk), P(dv), causal=False, scale=D ** -0.5, kv_end=ctx.kv_end,
                   drop_mask=ctx.drop_mask)
        return dq, dk, dv, None, None


class AttnPackedFn(Function):
    """AttnFn on PACKED projections: ``qkv`` [B,S,3,H,D] (self attention, q = None) or ``q`` [B,Sq,H,D] + ``kv`` [B,Sk,2,H,D]
    (nn.MultiheadAttention's packed in_proj of the DiT's perceptual cross attention, memvla/action_model/dit.py:158-185).  The
    backward writes dq / dk / dv straight into ONE packed gradient buffer (the attention kernels take strided views), so
    autograd sees a single tensor with a single consumer: no select_backward zero-fills, no gradient adds."""

    @staticmethod
    def forward(ctx, q, packed):
        self_attn = q is None
        ctx.self_attn = self_attn
        if self_attn:
            q, k, v = packed[:, :, 0], packed[:, :, 1], packed[:, :, 2]
        else:
            k, v = packed[:, :, 0], packed[:, :, 1]
        B, Sq, H, D = q.shape
        o = torch.empty((B, Sq, H, D), device=q.device, dtype=q.dtype)
        P = lambda t: t.permute(0, 2, 1, 3)
        lse = K.attn_fwd(P(q), P(k), P(v), P(o), causal=False, scale=D ** -0.5)
        ctx.save_for_backward(q if not self_attn else packed, packed, o, lse)
        return o.view(B, Sq, H * D)

    @staticmethod
    def backward(ctx, do):
        qs, packed, o, lse = ctx.saved_tensors
        dpk = torch.empty(packed.shape, device=packed.device, dtype=packed.dtype)
        if ctx.self_attn:
            q, k, v = packed[:, :, 0], packed[:, :, 1], packed[:, :, 2]
            dq, dk, dv = dpk[:, :, 0], dpk[:, :, 1], dpk[:, :, 2]
        else:
            q, k, v = qs, packed[:, :, 0], packed[:, :, 1]
            dq, dk, dv = torch.empty(q.shape, device=q.device, dtype=q.dtype), dpk[:, :, 0], dpk[:, :, 1]
        B, Sq, H, D = q.shape
        do = do.contiguous().view(B, Sq, H, D)
        P = lambda t: t.permute(0, 2, 1, 3)
        K.attn_bwd(P(q), P(k), P(v), P(o), lse, P(do), P(dq), P(dk), P(dv), causal=False, scale=D ** -0.5)
        return (None, dpk) if ctx.self_attn else (dq, dpk)


class DropFn(Function):
    """x * mask with mask entries 0 or 1/(1-p): nn.Dropout with the mask drawn by the caller (the FFN of the retrieval
    blocks, memvla_arch.py:99-105)"""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return K.mul(x.contiguous(), mask)

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        return K.mul(dy.contiguous(), mask), None


class GateFuseFn(Function):
    """scale * x1 + (1 - scale) * x2 (GateFusion, memvla_arch.py:170-187; scale = sigmoid(proj(cat)) comes in)"""

    @staticmethod
    def forward(ctx, scale, x1, x2):
        scale, x1, x2 = scale.contiguous(), x1.contiguous(), x2.contiguous()
        d = K.axpby(x1, x2, 1.0, -1.0)
        ctx.save_for_backward(scale, d)
        return K.add(K.mul(scale, d), x2)

    @staticmethod
    def backward(ctx, dy):
        scale, d = ctx.saved_tensors
        dy = dy.contiguous()
        dd = K.mul(dy, scale)
        return K.mul(dy, d), dd, K.axpby(dy, dd, 1.0, -1.0)


class TokenMeanFn(Function):
    """mean over the token axis: [B,N,C] -> [B,C] (AdaptiveAvgPool2d(1) of BottleneckSE, memvla_arch.py:139-141)"""

    @staticmethod
    def forward(ctx, x):
        B, N, C_ = x.shape
        ctx.shape = (B, N, C_)
        return K.token_sum(x.contiguous(), 1.0 / N)          # one launch: fp32 sums in token order, scaled, rounded once

    @staticmethod
    def backward(ctx, dm):
        B, N, C_ = ctx.shape
        return K.add_rows(None, dm.contiguous(), N, 1.0 / N)  # dm / N broadcast over the tokens


class AddRowsFn(Function):
    """x [R, N, C] + g [R, C] broadcast over the tokens: the timestep positional embedding on every token of a memory entry
    (memvla_arch.py:352-360: pe.unsqueeze(1).expand(-1, N, -1) added to the bank)"""

    @staticmethod
    def forward(ctx, x, g):
        ctx.n = x.shape[1]
        ctx.needs = (x.requires_grad, g.requires_grad)
        return K.add_rows(x.contiguous(), g.contiguous(), x.shape[1])

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        return (dy if ctx.needs[0] else None), (K.token_sum(dy) if ctx.needs[1] else None)


class BankStageFn(Function):
    """what one 'parallel_stream' step of the memory bank retrieves from, for all B slots (K.bank_stage_fwd): (mem [B, cap, N, D],
    ts_eff [B, cap], kv_len [B]).  The bank's entries are detached copies; only a slot WITHOUT history — its own tokens stand as
    entry 0, memvla_arch.py:378-387 — hands a gradient back to ``tokens``."""

    @staticmethod
    def forward(ctx, tokens, feat, ts, counts, timesteps):
        mem, ts_eff, kv_len = K.bank_stage_fwd(feat, ts, counts, tokens.contiguous(), timesteps)
        ctx.counts = counts
        ctx.mark_non_differentiable(ts_eff, kv_len)
        return mem, ts_eff, kv_len

    @staticmethod
    def backward(ctx, dmem, _dts, _dkv):
        return K.bank_stage_bwd(dmem.contiguous(), ctx.counts), None, None, None, None


class UnbindRowsFn(Function):
    """[B, ...] -> B tensors [1, ...] (the per-sample walk of the memory bank); the backward writes the B gradients side by
    side with library copies instead of autograd's zero-fill + add per slice"""

    @staticmethod
    def forward(ctx, x):
        ctx.shape, ctx.dt = tuple(x.shape), x.dtype
        x = x.contiguous()
        return tuple(x[i:i + 1] for i in range(x.shape[0]))

    @staticmethod
    def backward(ctx, *gs):
        out = torch.empty(ctx.shape, device=next(g for g in gs if g is not None).device, dtype=ctx.dt)
        for i, g in enumerate(gs):
            if g is None:
                out[i].zero_()                                   # (a sample whose output nobody used: not on the training path)
            else:
                K.cast(g.contiguous(), ctx.dt, out=out[i:i + 1])
        return out


class CatRowsFn(Function):
    """B tensors [1, ...] -> [B, ...] with library copies (torch.cat of the per-sample outputs)"""

    @staticmethod
    def forward(ctx, *xs):
        out = torch.empty((len(xs),) + tuple(xs[0].shape[1:]), device=xs[0].device, dtype=xs[0].dtype)
        for i, x in enumerate(xs):
            K.cast(x.contiguous(), out.dtype, out=out[i:i + 1])
        return out

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        return tuple(dy[i:i + 1] for i in range(dy.shape[0]))


class RowGateFn(Function):
    """x[B,N,C] * g[B,C] (SE channel gate, memvla_arch.py:160-161)"""

    @staticmethod
    def forward(ctx, x, g):
        x, g = x.contiguous(), g.contiguous()
        ctx.save_for_backward(x, g)
        return K.mul_rows(x, g)

    @staticmethod
    def backward(ctx, dy):
        x, g = ctx.saved_tensors
        dy = dy.contiguous()
        B = x.shape[0]
        return K.mul_rows(dy, g), K.token_sum(K.mul(dy, x))



class ParamFn(_StoreFn):
    """a parameter used as an ACTIVATION (the Q-former's learned queries, dexbotic/model/muvla/muvla_arch.py:53,61): its
    compute-dtype value going in, its gradient written to the arena coming back"""

    @staticmethod
    def forward(ctx, anchor, st: ParamStore, name: str):
        ctx.st, ctx.name = st, name
        _use(ctx, st, name)
        w = st.w(name)
        return w.view(w.shape)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        _vgrad(ctx.st, ctx.name, dy if dy.dtype == torch.float32 else K.cast(dy, torch.float32))
        return None, None, None


class BroadcastBatchFn(Function):
    """x [S, ...] -> a stride-0 view [B, S, ...] (one projection of the shared queries serves every sample); the backward sums the B
    gradients with the library's token sum, in batch order"""

    @staticmethod
    def forward(ctx, x, B: int):
        ctx.B = B
        return x.unsqueeze(0).expand(B, *x.shape)

    @staticmethod
    def backward(ctx, dy):
        B = ctx.B
        dy = dy.contiguous()
        if B == 1:
            return dy[0], None
        return K.token_sum(dy.view(1, B, -1)).view(dy.shape[1:]), None


class SplitRowsFn(Function):
    """[R, ...] -> ([n, ...], [R - n, ...]) views; the backward writes the two gradients side by side with library copies"""

    @staticmethod
    def forward(ctx, x, n: int):
        ctx.shape, ctx.dt, ctx.n = tuple(x.shape), x.dtype, n
        x = x.contiguous()
        return x[:n], x[n:]

    @staticmethod
    def backward(ctx, ga, gb):
        n = ctx.n
        out = torch.empty(ctx.shape, device=(ga if ga is not None else gb).device, dtype=ctx.dt)
        for g, dst in ((ga, out[:n]), (gb, out[n:])):
            if g is None:
                dst.zero_()
            else:
                K.cast(g.contiguous(), ctx.dt, out=dst)
        return out, None
