"""The elementwise route cases: every kernel instantiation csrc/elementwise.hip can launch, written down as data with the host
condition that selects it, and one deterministic table of small calls of its entry points that together reach all of them.
Used on the CPU by tests/test_elementwise_cases.py (the table is complete and each case's route is the one the host conditions
give) and tests/test_elementwise_ref.py (the reference and the slack constants below), and on the MI355X by
tests/test_elementwise_routes_gpu.py.  Nothing here needs a GPU.

A case is ``dict(id, entry, dtype, kernel, off, values, trip2, p)``:
  * ``entry``: the C entry point without its ``dxa_`` prefix (``rope_split`` is dxa_rope_split_at, ``rope_merge`` dxa_rope_merge_at,
    ``qknorm_split`` dxa_qknorm_rope_split_at, ``qknorm_merge`` dxa_qknorm_rope_merge_from);
  * ``dtype`` (and ``p["dst"]`` / ``p["w"]`` where an entry point takes a second dtype): "bf16" or "f32";
  * ``p``: sizes, leading dimensions and flags of the call (see ``operands`` for the tensors each entry point takes);
  * ``off``: operand -> offset in elements from a 256-byte-aligned base (default 0).  Misalignment is what selects the narrow and
    scalar routes; RoPE operands are never misaligned (the host does not check them: include/dexbotic_amd.h);
  * ``values``: "randn", or "special" (|x| in {20, 88, 89, 100}, +-0, products in the subnormal range; NaN and +-inf only through
    the cast and data-movement routes);
  * ``kernel``: the instantiation the case is there to reach, as a key of INSTANTIATIONS;
  * ``trip2``: the case claims a second grid-stride trip: more than 4096 * 256 work items (dxa_grid1d caps the grid at 4096
    workgroups) with a partial last trip.

Value criterion (tests/test_elementwise_routes_gpu.py), against the fp64 reference of tests/elementwise_ref.py: EXACT outputs
(data movement, single correctly rounded operations, sums in a fixed order, the RoPE rotation) bit for bit, NaN as NaN; every
other element
    |got - ref| <= ulp_T(ref) + k * 2^-24 * mag + 2^-126       (the ulp term only for a bf16 output)
with ``mag`` per output kind from elementwise_ref.py, and for GELU-tanh an absolute term GELU_TANH_ABS * (its factor).  Where the
formula rounds an intermediate to bf16 (rnd<T>), the reference also offers the neighbour that intermediate rounds to when its
exact value lies within k * 2^-24 * mag of a rounding boundary.  K_SLACK holds k per output kind: 4 x the largest error, in units
of 2^-24 * mag and beyond the ulp, of two stand-ins measured against the fp64 reference over this table: the same formulas and
rounding points in fp32 on the CPU (elementwise_ref.emulate, re-measured by tests/test_elementwise_ref.py) and in fp32 torch ops on
the MI355X (elementwise_ref.emulate on the device, re-measured by tests/test_elementwise_routes_gpu.py).  SHARE_CAP: per entry
point and dtype, GELU-tanh excluded, at most 0.5 % of the bf16 output elements may differ from the reference rounded to bf16; the
same per kernel instantiation over the cases with ordinary values (elementwise_ref.share_keys)."""
import torch

F32, BF16 = 0, 1
DT = {"f32": F32, "bf16": BF16}
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ES = {"f32": 4, "bf16": 2}
ACT = dict(none=0, gelu_erf=1, gelu_tanh=2, quick_gelu=3, silu=4, relu=5, sigmoid=6)
GRID_CAP = 4096 * 256              # work items of one grid-stride trip at the grid cap
LAUNCH_SITES = 82                  # hipLaunchKernelGGL sites in csrc/elementwise.hip

# k per output kind: 4 x the worst stand-in error over this table, in units of 2^-24 * mag beyond the ulp (CPU fp32 / GPU torch fp32):
#   act 1.767 / 1.767, act_grad 4.154 / 4.309, glu 3.229 / 3.142, glu_grad 4.630 / 4.630, two_term 1.952 / 1.952,
#   diffusion 1.264 / 1.346, trig 0.990 / 0.990, mse 1.871 / 1.181   ->  x 4, rounded up
K_SLACK = {"act": 7.1, "act_grad": 17.3, "glu": 13.0, "glu_grad": 18.6, "two_term": 7.9, "diffusion": 5.4, "trig": 4.0, "mse": 7.5}
# GELU-tanh's absolute term: 4 x the largest |1 - 2 / (1 + e^2u) in fp32 - tanh u| over the arguments of the GELU-tanh cases (CPU),
# measured 1.774e-07
GELU_TANH_ABS = 7.1e-07
SHARE_CAP = 0.005

# ---------------------------------------------------------------------------------------------------------- instantiations
# key -> (entry points that launch it, kernel, template arguments, host condition that selects it)
_I = []


def _inst(entries, kernel, targs, cond):
    _I.append((entries, kernel, tuple(targs), cond))


for m, tag in ((False, "rope_split"), (True, "rope_merge")):
    _inst((tag,), "rope_k", ("bf16", m, 8), "bf16, D % 16 == 0, qkv/q/k/v 16-byte aligned")
    _inst((tag,), "rope_k", ("bf16", m, 4), "bf16 otherwise")
    _inst((tag,), "rope_k", ("f32", m, 4), "fp32")
_inst(("qknorm_split",), "qknorm_rope_split_k", ("bf16", 8), "bf16")
_inst(("qknorm_split",), "qknorm_rope_split_k", ("f32", 4), "fp32")
_inst(("qknorm_merge",), "qknorm_rope_merge_k", ("bf16", 8), "bf16")
_inst(("qknorm_merge",), "qknorm_rope_merge_k", ("f32", 4), "fp32")
for k in ("swiglu_fwd_k", "swiglu_bwd_k", "glu_fwd_k", "glu_bwd_k"):
    e = k[:-2]
    _inst((e,), k, ("bf16", 8), "bf16, F % 8 == 0, operands 16-byte aligned")
    _inst((e,), k, ("bf16", 4), "bf16, F % 4 == 0 (not % 8), operands 16-byte aligned")
    _inst((e,), k, ("bf16", 1), "bf16, F % 4 != 0 or an operand not 16-byte aligned")
    _inst((e,), k, ("f32", 4), "fp32, F % 4 == 0, operands 16-byte aligned")
    _inst((e,), k, ("f32", 1), "fp32 otherwise")
for k, es in (("act_fwd_k", ("act_fwd",)), ("act_bwd_k", ("act_bwd",)), ("add_k", ("add",))):
    for t in ("bf16", "f32"):
        _inst(es, k, (t, 4), f"{t}, n % 4 == 0, operands 16-byte aligned")
        _inst(es, k, (t, 1), f"{t} otherwise")
for op, e in ((0, "axpby"), (1, "mul")):
    for t in ("bf16", "f32"):
        _inst((e,), "binary_k", (t, 4, op), f"{t}, n % 4 == 0, operands 16-byte aligned")
        _inst((e,), "binary_k", (t, 1, op), f"{t} otherwise")
for t in ("bf16", "f32"):
    _inst(("mul_rows",), "mul_rows_k", (t,), t)
_PAIRS = (("f32", "bf16"), ("bf16", "f32"), ("f32", "f32"), ("bf16", "bf16"))
for s, d in _PAIRS:
    _inst(("cast",), "cast_k", (s, d, 4), f"{s} -> {d}, n % 4 == 0, operands 16-byte aligned")
    _inst(("cast",), "cast_k", (s, d, 1), f"{s} -> {d} otherwise")
    _inst(("copy2d",), "copy2d_k", (s, d), f"{s} -> {d}")
    _inst(("gather",), "gather_rows_k", (s, d), f"{s} -> {d}")
    _inst(("scatter",), "scatter_rows_k", (s, d), f"{s} -> {d}")
    _inst(("im2col",), "im2col_k", (s, d), f"images {s}, rows {d}")
for k, e in (("splice_fwd_k", "splice_fwd"), ("splice_bwd_k", "splice_bwd")):
    for t in ("bf16", "f32"):
        _inst((e,), k, (t, 4), f"{t}, d % 4 == 0, the row operands 16-byte aligned")
        _inst((e,), k, (t, 1), f"{t} otherwise")
_inst(("zero_rows",), "zero_rows_k", (), "always")
_inst(("vit_embed_fwd",), "vit_embed_fwd_k", ("bf16", "bf16"), "activations bf16, weights bf16")
_inst(("vit_embed_fwd",), "vit_embed_fwd_k", ("bf16", "f32"), "activations bf16, weights fp32")
_inst(("vit_embed_fwd",), "vit_embed_fwd_k", ("f32", "f32"), "fp32")
for t in ("bf16", "f32"):
    _inst(("vit_embed_bwd",), "vit_embed_bwd_k", (t,), t)
for k, e in (("qsample_k", "qsample"), ("timestep_embedding_k", "timestep"), ("dit_assemble_fwd_k", "dit_fwd"),
             ("dit_assemble_bwd_k", "dit_bwd"), ("token_drop_k", "token_drop"), ("token_drop_bwd_k", "token_drop_bwd"),
             ("mse_loss_k", "mse"), ("mse_loss_rows_k", "mse_rows"), ("ddim_step_k", "ddim")):
    _inst((e,), k, (), "always")
_inst(("transpose",), "transpose8_bf16_k", (), "bf16, vec, C % 8 == 0, R_padded % 8 == 0")
_inst(("transpose",), "transpose_k", ("bf16",), "bf16 otherwise")
_inst(("transpose",), "transpose_k", ("f32",), "fp32")
for t in ("bf16", "f32"):
    _inst(("permute",), "permute_bshd_k", (t,), t)


def _targ(a, mangled):
    if isinstance(a, bool):
        return ("Lb1E" if a else "Lb0E") if mangled else ("true" if a else "false")
    if isinstance(a, int):
        return f"Li{a}E" if mangled else str(a)
    return {"bf16": "t", "f32": "f"}[a] if mangled else {"bf16": "unsigned short", "f32": "float"}[a]


def key(kernel, targs):
    return f"{kernel}<{','.join(str(a).lower() if isinstance(a, bool) else str(a) for a in targs)}>" if targs else kernel


def mangled(kernel, targs):
    """fragment of the Itanium-mangled name (anonymous namespace): '6rope_kItLb0ELi8EE' for rope_k<bf16_t, false, 8>"""
    return f"{len(kernel)}{kernel}" + ("I" + "".join(_targ(a, True) for a in targs) + "EE" if targs else "E")


def demangled(kernel, targs):
    return f"{kernel}<{', '.join(_targ(a, False) for a in targs)}>(" if targs else f"{kernel}("


INSTANTIATIONS = {key(k, t): dict(entries=e, kernel=k, targs=t, cond=c, mangled=mangled(k, t), demangled=demangled(k, t))
                  for e, k, t, c in _I}

# ------------------------------------------------------------------------------------------------------------------ cases
CASES = []


def _c(entry, dtype, kernel, off=None, values="randn", trip2=False, tag="", **p):
    off = dict(off or {})
    pid = "-".join(f"{k}{v}" for k, v in p.items() if not isinstance(v, (list, tuple)))
    cid = f"{entry}-{dtype}-{kernel}-{pid}" + "".join(f"-off_{k}{v}" for k, v in off.items()) + \
        ("" if values == "randn" else f"-{values}") + ("-trip2" if trip2 else "") + (f"-{tag}" if tag else "")
    assert kernel in INSTANTIATIONS, kernel
    CASES.append(dict(id=cid, entry=entry, dtype=dtype, kernel=kernel, off=off, values=values, trip2=trip2, p=p))


N2 = GRID_CAP + 37                 # a second trip with 37 live items in it

# RoPE.  D in {24, 72 (bf16 narrow: D % 16 != 0), 64, 128, 256}; GQA 7:1 and 2:2; pos tables that are not monotonic and reach
# past S; the _at form with S_cap > S and s0 > 0 (the other rows keep their sentinels).
for e, m in (("rope_split", "false"), ("rope_merge", "true")):
    W, N_, F = f"rope_k<bf16,{m},8>", f"rope_k<bf16,{m},4>", f"rope_k<f32,{m},4>"
    _c(e, "bf16", W, B=2, S=5, Hq=7, Hkv=1, D=64, S_cap=5, s0=0, pos=0)
    _c(e, "bf16", W, B=1, S=3, Hq=2, Hkv=2, D=128, S_cap=7, s0=3, pos=1)
    _c(e, "bf16", W, B=2, S=3, Hq=2, Hkv=2, D=256, S_cap=3, s0=0, pos=1)
    _c(e, "bf16", N_, B=2, S=5, Hq=7, Hkv=1, D=24, S_cap=5, s0=0, pos=1)
    _c(e, "bf16", N_, B=1, S=3, Hq=2, Hkv=2, D=72, S_cap=6, s0=2, pos=0)
    _c(e, "bf16", N_, B=1, S=3, Hq=2, Hkv=2, D=64, S_cap=3, s0=0, pos=1, off={"qkv" if m == "false" else "dqkv": 4})   # 8-byte aligned
    _c(e, "f32", F, B=2, S=5, Hq=7, Hkv=1, D=64, S_cap=5, s0=0, pos=0)
    _c(e, "f32", F, B=1, S=3, Hq=2, Hkv=2, D=128, S_cap=7, s0=3, pos=1)
    _c(e, "f32", F, B=1, S=3, Hq=2, Hkv=2, D=256, S_cap=4, s0=1, pos=0)
    _c(e, "f32", F, B=2, S=5, Hq=7, Hkv=1, D=24, S_cap=5, s0=0, pos=1)
    _c(e, "f32", F, B=1, S=3, Hq=2, Hkv=2, D=72, S_cap=3, s0=0, pos=1)
    # second trips: D = 8, one work item per (token, head slot)
    _c(e, "bf16", N_, B=1, S=349539, Hq=1, Hkv=1, D=8, S_cap=349539, s0=0, pos=0, trip2=True)
    _c(e, "f32", F, B=1, S=349539, Hq=1, Hkv=1, D=8, S_cap=349539, s0=0, pos=1, trip2=True)
    _c(e, "bf16", W, B=1, S=349539, Hq=1, Hkv=1, D=16, S_cap=349539, s0=0, pos=0, trip2=True)

# Qwen3 per-head RMSNorm + RoPE: the routes (the values are held by tests/test_qknorm_rope_gpu.py; here the v third and, in the
# "unit" cases, q and k bit for bit as rope_k rotates them: the split with unit weights on unit-RMS rows whose products with the
# full-precision tables are inexact (rstd must come out 1.0), the merge with unit weights, rstd = 1 and pre-norm rows of zeros,
# which make the RMSNorm backward the identity)
_c("qknorm_split", "bf16", "qknorm_rope_split_k<bf16,8>", B=1, S=3, Hq=2, Hkv=1, D=64, pos=1)
_c("qknorm_split", "f32", "qknorm_rope_split_k<f32,4>", B=2, S=3, Hq=7, Hkv=1, D=128, pos=1, tag="unit")
_c("qknorm_split", "f32", "qknorm_rope_split_k<f32,4>", B=1, S=5, Hq=2, Hkv=2, D=32, pos=0, tag="unit")
_c("qknorm_split", "bf16", "qknorm_rope_split_k<bf16,8>", B=1, S=174763, Hq=1, Hkv=1, D=32, pos=0, trip2=True)
_c("qknorm_split", "f32", "qknorm_rope_split_k<f32,4>", B=1, S=87382, Hq=1, Hkv=1, D=32, pos=0, trip2=True, tag="unit")
_c("qknorm_merge", "bf16", "qknorm_rope_merge_k<bf16,8>", B=1, S=3, Hq=2, Hkv=1, D=64, pos=1)
_c("qknorm_merge", "f32", "qknorm_rope_merge_k<f32,4>", B=1, S=3, Hq=2, Hkv=2, D=32, pos=0)
_c("qknorm_merge", "f32", "qknorm_rope_merge_k<f32,4>", B=2, S=3, Hq=7, Hkv=1, D=128, pos=1, tag="unit")
_c("qknorm_merge", "f32", "qknorm_rope_merge_k<f32,4>", B=1, S=5, Hq=2, Hkv=2, D=32, pos=0, tag="unit")
_c("qknorm_merge", "bf16", "qknorm_rope_merge_k<bf16,8>", B=1, S=3, Hq=2, Hkv=1, D=64, pos=1, tag="unit")
_c("qknorm_merge", "bf16", "qknorm_rope_merge_k<bf16,8>", B=1, S=43691, Hq=1, Hkv=1, D=32, pos=0, trip2=True)   # grid cap 1024
_c("qknorm_merge", "f32", "qknorm_rope_merge_k<f32,4>", B=1, S=21846, Hq=1, Hkv=1, D=32, pos=1, trip2=True)

# gated MLPs: F % 8 (x8), F % 4 only (x4), odd F and misaligned operands (x1); special values through every bf16 route
for e, k in (("swiglu_fwd", "swiglu_fwd_k"), ("swiglu_bwd", "swiglu_bwd_k"), ("glu_fwd", "glu_fwd_k"), ("glu_bwd", "glu_bwd_k")):
    act = {} if e.startswith("swiglu") else dict(act=ACT["gelu_tanh"])
    act2 = {} if e.startswith("swiglu") else dict(act=ACT["gelu_erf"])
    act3 = {} if e.startswith("swiglu") else dict(act=ACT["quick_gelu"])
    first = "gu"
    _c(e, "bf16", f"{k}<bf16,8>", rows=3, F=264, **act)
    _c(e, "bf16", f"{k}<bf16,8>", rows=24, F=264, **act2)        # ordinary values enough for a share of the route's own
    _c(e, "bf16", f"{k}<bf16,4>", rows=24, F=268, **act3)
    _c(e, "bf16", f"{k}<bf16,8>", rows=128, F=64, values="special", **act2)
    _c(e, "bf16", f"{k}<bf16,4>", rows=3, F=68, **act3)
    _c(e, "bf16", f"{k}<bf16,4>", rows=128, F=68, values="special", **act2)
    _c(e, "bf16", f"{k}<bf16,1>", rows=3, F=67, **act)
    _c(e, "bf16", f"{k}<bf16,1>", rows=128, F=64, off={first: 1}, values="special", **act2)
    _c(e, "bf16", f"{k}<bf16,1>", rows=3, F=64, off={"out" if e.endswith("fwd") else "dgu": 4}, **act3)
    _c(e, "f32", f"{k}<f32,4>", rows=3, F=68, **act)
    _c(e, "f32", f"{k}<f32,1>", rows=3, F=67, **act2)
    _c(e, "f32", f"{k}<f32,1>", rows=3, F=64, off={first: 1}, **act3)
    _c(e, "bf16", f"{k}<bf16,1>", rows=1, F=N2, trip2=True, **act2)
    _c(e, "f32", f"{k}<f32,4>", rows=4, F=GRID_CAP + 36, trip2=True, **act3)
    if e == "swiglu_bwd":
        _c(e, "bf16", f"{k}<bf16,1>", rows=3, F=64, off={"dout": 2})

# activations: every act on some route; special values through every bf16 route
for e, k in (("act_fwd", "act_fwd_k"), ("act_bwd", "act_bwd_k")):
    for i, (a, av) in enumerate(ACT.items()):
        t = "bf16" if i % 2 == 0 else "f32"
        _c(e, t, f"{k}<{t},4>", n=260, act=av)
        _c(e, t, f"{k}<{t},1>", n=259, act=av)
    for a in ("silu", "gelu_erf", "quick_gelu", "sigmoid"):
        _c(e, "bf16", f"{k}<bf16,4>", n=4096, act=ACT[a], values="special")
        _c(e, "bf16", f"{k}<bf16,1>", n=4096, act=ACT[a], values="special", off={"x": 1})
    _c(e, "bf16", f"{k}<bf16,1>", n=260, act=ACT["silu"], off={"dx" if e == "act_bwd" else "y": 2})
    _c(e, "f32", f"{k}<f32,1>", n=260, act=ACT["gelu_erf"], off={"x": 2})
    _c(e, "f32", f"{k}<f32,4>", n=4 * N2, act=ACT["silu"], trip2=True)
    _c(e, "f32", f"{k}<f32,1>", n=N2, act=ACT["gelu_tanh"], trip2=True)
    _c(e, "bf16", f"{k}<bf16,4>", n=4 * N2, act=ACT["quick_gelu"], trip2=True)
    _c(e, "bf16", f"{k}<bf16,1>", n=N2, act=ACT["sigmoid"], trip2=True)

# add / axpby / mul: n % 4 (x4), odd n and misaligned operands (x1)
for e, k, extra in (("add", "add_k", ""), ("axpby", "binary_k", ",0"), ("mul", "binary_k", ",1")):
    ab = dict(alpha=0.75, beta=-1.25) if e == "axpby" else {}
    for t in ("bf16", "f32"):
        _c(e, t, f"{k}<{t},4{extra}>", n=352, **ab)
        _c(e, t, f"{k}<{t},1{extra}>", n=350, **ab)
        _c(e, t, f"{k}<{t},1{extra}>", n=352, off={"b": 1}, **ab)
        _c(e, t, f"{k}<{t},1{extra}>", n=352, off={"out": 2}, **ab)
        _c(e, t, f"{k}<{t},4{extra}>", n=4 * N2, trip2=True, **ab)
        _c(e, t, f"{k}<{t},1{extra}>", n=N2, trip2=True, **ab)
    _c(e, "bf16", f"{k}<bf16,4{extra}>", n=4096, values="special", **ab)
    _c(e, "bf16", f"{k}<bf16,1{extra}>", n=4096, values="special", off={"a": 1}, **ab)
for t in ("bf16", "f32"):
    _c("mul_rows", t, f"mul_rows_k<{t}>", R=3, Nn=5, C=7)
    _c("mul_rows", t, f"mul_rows_k<{t}>", R=2, Nn=3, C=174763, trip2=True)

# cast / copy2d / gather / scatter / im2col: all four dtype pairs
for s, d in _PAIRS:
    _c("cast", s, f"cast_k<{s},{d},4>", n=260, dst=d)
    _c("cast", s, f"cast_k<{s},{d},4>", n=4096, dst=d, values="special")
    _c("cast", s, f"cast_k<{s},{d},1>", n=4096, dst=d, values="special", off={"dst": 1})
    _c("cast", s, f"cast_k<{s},{d},1>", n=259, dst=d)
    _c("cast", s, f"cast_k<{s},{d},1>", n=N2, dst=d, trip2=True)
    _c("copy2d", s, f"copy2d_k<{s},{d}>", rows=5, cols=13, cols_padded=16, lds=17, ldd=20, dst=d)
    _c("copy2d", s, f"copy2d_k<{s},{d}>", rows=3, cols=64, cols_padded=64, lds=64, ldd=64, dst=d, values="special")
    _c("copy2d", s, f"copy2d_k<{s},{d}>", rows=1, cols=GRID_CAP + 30, cols_padded=N2, lds=N2, ldd=N2 + 3, dst=d, trip2=True)
    _c("gather", s, f"gather_rows_k<{s},{d}>", n=9, R=5, d=13, dst=d, values="special")
    _c("gather", s, f"gather_rows_k<{s},{d}>", n=N2, R=3, d=1, dst=d, trip2=True)
    _c("scatter", s, f"scatter_rows_k<{s},{d}>", n=9, R=6, d=13, dst=d)
    _c("scatter", s, f"scatter_rows_k<{s},{d}>", n=4, R=N2, d=1, dst=d, trip2=True)
    _c("im2col", s, f"im2col_k<{s},{d}>", N=2, H=12, W=8, P=4, ld=52, dst=d)
    _c("im2col", s, f"im2col_k<{s},{d}>", N=1, H=18726, W=16, P=2, ld=14, dst=d, trip2=True)

# splice: d % 4 (x4), odd d / misaligned (x1); backward: >= 3 ballot windows, a token id repeated across windows, an id first
# seen at r & 255 != 0, > 64 duplicates inside one wave, d = 1028 (x4 with a tail chunk), d = 1030 (scalar, 5 y-chunks), PAD rows,
# d_img / d_embed NULL
for t in ("bf16", "f32"):
    _c("splice_fwd", t, f"splice_fwd_k<{t},4>", n_rows=40, V=11, n_img=9, d=12)
    _c("splice_fwd", t, f"splice_fwd_k<{t},1>", n_rows=40, V=11, n_img=9, d=13)
    _c("splice_fwd", t, f"splice_fwd_k<{t},1>", n_rows=40, V=11, n_img=9, d=12, off={"img": 1})
    _c("splice_fwd", t, f"splice_fwd_k<{t},1>", n_rows=16, V=11, n_img=9, d=64, values="special", off={"out": 2})
    _c("splice_fwd", t, f"splice_fwd_k<{t},4>", n_rows=16, V=11, n_img=9, d=64, values="special")
    _c("splice_fwd", t, f"splice_fwd_k<{t},1>", n_rows=N2, V=3, n_img=2, d=1, trip2=True)
    _c("splice_bwd", t, f"splice_bwd_k<{t},4>", n_rows=600, V=7, n_img=40, d=8)
    _c("splice_bwd", t, f"splice_bwd_k<{t},4>", n_rows=300, V=20, n_img=30, d=1028)
    _c("splice_bwd", t, f"splice_bwd_k<{t},1>", n_rows=600, V=7, n_img=40, d=13)
    _c("splice_bwd", t, f"splice_bwd_k<{t},1>", n_rows=300, V=20, n_img=30, d=1030)
    _c("splice_bwd", t, f"splice_bwd_k<{t},1>", n_rows=600, V=7, n_img=40, d=8, off={"dout": 1})
    _c("splice_bwd", t, f"splice_bwd_k<{t},4>", n_rows=600, V=7, n_img=40, d=8, no_img=1)
    _c("splice_bwd", t, f"splice_bwd_k<{t},4>", n_rows=600, V=7, n_img=40, d=8, no_embed=1)
_c("zero_rows", "f32", "zero_rows_k", n_rows=300, V=20, n_img=30, d=1030)

# ViT front-end
_c("vit_embed_fwd", "bf16", "vit_embed_fwd_k<bf16,bf16>", N=2, np=5, C=13, w="bf16")
_c("vit_embed_fwd", "bf16", "vit_embed_fwd_k<bf16,f32>", N=2, np=5, C=13, w="f32")
_c("vit_embed_fwd", "f32", "vit_embed_fwd_k<f32,f32>", N=2, np=5, C=13, w="f32")
_c("vit_embed_fwd", "bf16", "vit_embed_fwd_k<bf16,bf16>", N=1, np=8, C=116509, w="bf16", trip2=True)
_c("vit_embed_fwd", "bf16", "vit_embed_fwd_k<bf16,f32>", N=1, np=8, C=116509, w="f32", trip2=True)
_c("vit_embed_fwd", "f32", "vit_embed_fwd_k<f32,f32>", N=1, np=8, C=116509, w="f32", trip2=True)
for t in ("bf16", "f32"):
    _c("vit_embed_bwd", t, f"vit_embed_bwd_k<{t}>", N=2, np=5, C=13, values="special")
    _c("vit_embed_bwd", t, f"vit_embed_bwd_k<{t}>", N=1, np=9, C=116509, trip2=True)

# diffusion glue (fp32)
_c("qsample", "f32", "qsample_k", N=3, per=37)
_c("qsample", "f32", "qsample_k", N=3, per=349538, trip2=True)
_c("timestep", "f32", "timestep_embedding_k", N=5, half=33)
_c("timestep", "f32", "timestep_embedding_k", N=31, half=33826, trip2=True)
_c("dit_fwd", "f32", "dit_assemble_fwd_k", N=2, T=5, hd=13)
_c("dit_fwd", "f32", "dit_assemble_fwd_k", N=1, T=8, hd=116509, trip2=True)
_c("dit_bwd", "f32", "dit_assemble_bwd_k", N=2, T=5, hd=13, values="special")
_c("dit_bwd", "f32", "dit_assemble_bwd_k", N=1, T=8, hd=116509, trip2=True)
_c("token_drop", "f32", "token_drop_k", N=6, d=37, values="special")
_c("token_drop", "f32", "token_drop_k", N=3, d=349538, trip2=True)
_c("token_drop_bwd", "f32", "token_drop_bwd_k", N=6, d=300, accumulate=0)
_c("token_drop_bwd", "f32", "token_drop_bwd_k", N=6, d=300, accumulate=1)
_c("token_drop_bwd", "f32", "token_drop_bwd_k", N=6, d=300, accumulate=1, no_dz=1)
_c("mse", "f32", "mse_loss_k", n=2500, gscale=0.5)
_c("mse_rows", "f32", "mse_loss_rows_k", rows=7, cols=301, gscale=0.5)
_c("ddim", "f32", "ddim_step_k", B=2, per=37, use_cfg=0)
_c("ddim", "f32", "ddim_step_k", B=2, per=37, use_cfg=1)
_c("ddim", "f32", "ddim_step_k", B=1, per=N2, use_cfg=1, trip2=True)

# transpose: the bf16 fast path with R % 8 != 0 and whole zero tiles (R_padded - R >= 64), ld_dst > R_padded (the columns beyond
# keep their sentinels); the LDS path for C % 8 != 0, R_padded % 8 != 0 and vec = 0
_c("transpose", "bf16", "transpose8_bf16_k", R=37, C=40, Rp=136, lds=40, ldd=144, values="special")
_c("transpose", "bf16", "transpose8_bf16_k", R=130, C=136, Rp=136, lds=136, ldd=136)
_c("transpose", "bf16", "transpose_k<bf16>", R=37, C=42, Rp=104, lds=48, ldd=112)                 # C % 8 != 0, vec
_c("transpose", "bf16", "transpose_k<bf16>", R=37, C=40, Rp=100, lds=40, ldd=104)                 # Rp % 8 != 0, vec
_c("transpose", "bf16", "transpose_k<bf16>", R=70, C=40, Rp=136, lds=43, ldd=136, values="special")  # ld % 8: vec = 0
_c("transpose", "bf16", "transpose_k<bf16>", R=70, C=40, Rp=136, lds=40, ldd=136, off={"src": 1})  # misaligned: vec = 0
_c("transpose", "f32", "transpose_k<f32>", R=37, C=42, Rp=104, lds=44, ldd=108)
_c("transpose", "f32", "transpose_k<f32>", R=70, C=67, Rp=135, lds=67, ldd=137)                   # vec = 0
_c("transpose", "f32", "transpose_k<f32>", R=5, C=9, Rp=72, lds=12, ldd=76, values="special")
for t in ("bf16", "f32"):
    for th in (1, 0):
        _c("permute", t, f"permute_bshd_k<{t}>", B=2, S=3, H=5, D=16, to_head=th, values="special")
    _c("permute", t, f"permute_bshd_k<{t}>", B=1, S=65541, H=2, D=64 if t == "bf16" else 32, to_head=1, trip2=True)

# every bf16 route of a family on the same special inputs: their outputs must agree bit for bit
ROUTE_GROUPS = {}
for c in CASES:
    if c["values"] == "special" and c["dtype"] == "bf16" and c["entry"] in ("swiglu_fwd", "swiglu_bwd", "glu_fwd", "glu_bwd",
                                                                              "act_fwd", "act_bwd", "add", "axpby", "mul"):
        g = (c["entry"], tuple(sorted((k, v) for k, v in c["p"].items() if k not in ("rows", "F"))))      # x4 needs another F
        ROUTE_GROUPS.setdefault(g, []).append(c["id"])


# ---------------------------------------------------------------------------------------------------------------- routing
def _al(case, name, a=16):
    es = ES[case["dtype"]]
    return (case["off"].get(name, 0) * es) % a == 0


def _al_t(case, name, dt, a=16):
    return (case["off"].get(name, 0) * ES[dt]) % a == 0


def route(case):
    """the instantiation the host launcher picks for ``case`` (mirrors the conditions in csrc/elementwise.hip)"""
    e, t, p = case["entry"], case["dtype"], case["p"]
    if e in ("rope_split", "rope_merge"):
        m = "true" if e == "rope_merge" else "false"
        ops = ("qkv", "q", "k", "v") if e == "rope_split" else ("dqkv", "dq", "dk", "dv")
        if t == "bf16" and p["D"] % 16 == 0 and all(_al(case, n) for n in ops):
            return f"rope_k<bf16,{m},8>"
        return f"rope_k<{t},{m},4>"
    if e.startswith("qknorm"):
        return f"qknorm_rope_{e.split('_')[1]}_k<{t},{8 if t == 'bf16' else 4}>"
    if e in ("swiglu_fwd", "swiglu_bwd", "glu_fwd", "glu_bwd"):
        ops = ("gu", "out") if e.endswith("fwd") else ("gu", "dout", "dgu")
        vec = p["F"] % 4 == 0 and all(_al(case, n) for n in ops)
        v = (8 if vec and p["F"] % 8 == 0 else 4 if vec else 1) if t == "bf16" else (4 if vec else 1)
        return f"{e}_k<{t},{v}>"
    if e in ("act_fwd", "act_bwd", "add", "axpby", "mul"):
        ops = {"act_fwd": ("x", "y"), "act_bwd": ("x", "dy", "dx")}.get(e, ("a", "b", "out"))
        v = 4 if p["n"] % 4 == 0 and all(_al(case, n) for n in ops) else 1
        if e in ("axpby", "mul"):
            return f"binary_k<{t},{v},{0 if e == 'axpby' else 1}>"
        return f"{e}_k<{t},{v}>"
    if e == "mul_rows":
        return f"mul_rows_k<{t}>"
    if e == "cast":
        v = 4 if p["n"] % 4 == 0 and _al_t(case, "src", t) and _al_t(case, "dst", p["dst"]) else 1
        return f"cast_k<{t},{p['dst']},{v}>"
    if e in ("copy2d", "gather", "scatter", "im2col"):
        k = {"copy2d": "copy2d_k", "gather": "gather_rows_k", "scatter": "scatter_rows_k", "im2col": "im2col_k"}[e]
        return f"{k}<{t},{p['dst']}>"
    if e == "splice_fwd":
        v = 4 if p["d"] % 4 == 0 and all(_al(case, n) for n in ("embed", "out", "img")) else 1
        return f"splice_fwd_k<{t},{v}>"
    if e == "splice_bwd":
        v = 4 if p["d"] % 4 == 0 and _al(case, "dout") and (p.get("no_img") or _al(case, "d_img")) else 1
        return f"splice_bwd_k<{t},{v}>"
    if e == "vit_embed_fwd":
        return f"vit_embed_fwd_k<{t},{p['w']}>"
    if e == "vit_embed_bwd":
        return f"vit_embed_bwd_k<{t}>"
    if e == "transpose":
        epv = 16 // ES[t]
        vec = _al(case, "src") and _al(case, "dst") and p["lds"] % epv == 0 and p["ldd"] % epv == 0
        if t == "bf16" and vec and p["C"] % 8 == 0 and p["Rp"] % 8 == 0:
            return "transpose8_bf16_k"
        return f"transpose_k<{t}>"
    if e == "permute":
        return f"permute_bshd_k<{t}>"
    return {"zero_rows": "zero_rows_k", "qsample": "qsample_k", "timestep": "timestep_embedding_k", "dit_fwd": "dit_assemble_fwd_k",
            "dit_bwd": "dit_assemble_bwd_k", "token_drop": "token_drop_k", "token_drop_bwd": "token_drop_bwd_k", "mse": "mse_loss_k",
            "mse_rows": "mse_loss_rows_k", "ddim": "ddim_step_k"}[e]


def transpose_vec(case):
    """the ``vec`` flag dxa_transpose hands transpose_k"""
    t, p = case["dtype"], case["p"]
    epv = 16 // ES[t]
    return int(_al(case, "src") and _al(case, "dst") and p["lds"] % epv == 0 and p["ldd"] % epv == 0)


def work_items(case):
    """work items of the grid-stride loop of the launch the case makes (None: the kernel has no grid-stride loop)"""
    e, p = case["entry"], case["p"]
    v = int(route(case).split(",")[-1].rstrip(">")) if e in ("swiglu_fwd", "swiglu_bwd", "glu_fwd", "glu_bwd", "act_fwd", "act_bwd",
                                                              "add", "cast", "splice_fwd") else 1
    if e in ("axpby", "mul"):
        v = int(route(case).split(",")[1])
    if e in ("rope_split", "rope_merge", "qknorm_split", "qknorm_merge"):
        rv = int(route(case).split(",")[-1].rstrip(">"))
        return p["B"] * p["S"] * (p["Hq"] + 2 * p["Hkv"]) * (p["D"] // 2 // rv)
    if e in ("swiglu_fwd", "swiglu_bwd", "glu_fwd", "glu_bwd"):
        return p["rows"] * p["F"] // v
    if e in ("act_fwd", "act_bwd", "add", "axpby", "mul", "cast"):
        return p["n"] // v
    if e == "mul_rows":
        return p["R"] * p["Nn"] * p["C"]
    if e == "copy2d":
        return p["rows"] * p["cols_padded"]
    if e == "gather":
        return p["n"] * p["d"]
    if e == "scatter":
        return p["R"] * p["d"]
    if e == "im2col":
        return p["N"] * (p["H"] // p["P"]) * (p["W"] // p["P"]) * p["ld"]
    if e == "splice_fwd":
        return p["n_rows"] * p["d"] // v
    if e == "vit_embed_fwd":
        return p["N"] * (p["np"] + 1) * p["C"]
    if e == "vit_embed_bwd":
        return p["N"] * p["np"] * p["C"]
    if e in ("qsample", "token_drop"):
        return p["N"] * (p["per"] if e == "qsample" else p["d"])
    if e == "timestep":
        return p["N"] * p["half"]
    if e in ("dit_fwd", "dit_bwd"):
        return p["N"] * (p["T"] + 1) * p["hd"]
    if e == "ddim":
        return p["B"] * p["per"]
    if e == "permute":
        return p["B"] * p["S"] * p["H"] * (p["D"] // (16 // ES[case["dtype"]]))
    return None


def grid_cap(case):
    """the grid cap of the case's launch: 1024 workgroups for the qknorm backward, 4096 otherwise"""
    return 1024 * 256 if case["entry"] == "qknorm_merge" else GRID_CAP
