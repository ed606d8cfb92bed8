"""The norm route cases: one deterministic table of small calls of the norm entry points of csrc/norm.hip (RMSNorm, LayerNorm,
add-LayerNorm, 2x2-downsample LayerNorm, adaptive RMSNorm and gated residual forward and backward, dxa_colsum) that together reach every instantiation their launchers can launch, each with
the kernel it is there to reach, written down as data.  Used on the CPU by tests/test_norm_cases.py (the table is complete and
its kernels are the planner's) and tests/test_norm_ref.py (the reference and the slack constants below), and on the MI355X by
tests/test_norm_routes_gpu.py.  Nothing here needs a GPU.

A norm case is ``dict(id, entry, rows, cols, dtype, w_dtype, w, b, res, mis, kernel, trips)``:
  * ``entry``: rmsnorm_fwd / rmsnorm_bwd / layernorm_fwd / layernorm_bwd / add_layernorm_fwd / add_layernorm_bwd, and
    downsample_layernorm_* (rows = N, cols = C, and G: x [N, G*G, C]) and adarms_* / gated_residual_* (rows = B * rps, B, rps,
    ``gated``: with a branch and the gate third of another [B, 3 cols] modulation) — see _ds and _ar;
  * ``w`` / ``b``: the gain / bias is given; ``res``: the backward's residual (dx += res); add-LayerNorm always has its second
    addend (``x2``);
  * ``mis``: the operand carved one element into a larger buffer (16-byte alignment broken), or None;
  * ``trips``: the row-loop trips the plan must report, where a case is there for them (2049 rows: a second trip with one live
    row; 4100 rows: a third trip, which reuses the parity-indexed LDS slots of rmsnorm_bwd_split_k).
A column-sum case is ``dict(id, entry="colsum", rows, cols, dtype, view, accumulate, kernel, capture_kernel)``: ``view`` is how
the input is laid out (``contig``; ``ld4``: ld > cols, ld % 4 == 0; ``ldodd``: ld % 4 != 0; ``coloff``: the right half
``part[:, cols:]`` of a [rows, 2 cols] slab, as dxa_layernorm_bwd's db half is folded); ``capture_kernel`` is what the same call
launches on a capturing stream whose counters do not exist yet (the two-launch form).

Value criterion (tests/test_norm_routes_gpu.py), every output element against tests/norm_ref.py:
    |got - ref| <= U * ulp_T(ref) + k * 2^-24 * mag,        U = 1 for a bf16 output, 0 for fp32,
with ``mag`` the sum of the absolute values of the terms that made the element (norm_ref.py).  ``K_SLACK`` holds k per output
kind: 4 x the largest error, in units of 2^-24 * mag and beyond the U ulp, of a plain fp32 torch evaluation of the same
formulas on the CPU (norm_ref.emulate) against the fp64 reference, over the whole table (tests/test_norm_ref.py measures it
again and requires it to stay within K_SLACK / 4).  Measured over this table:
    y 4.08, dx 3.61, dw / db / per-sample sums 2.80, column sums 0.99, mean / rstd 2.72  ->  k = 16.4, 14.5, 11.3, 4.0, 10.9
(x 4, rounded up)
The factor 4 covers the kernels' wave-shuffle summation order and v_rsq_f32 against torch's order and 1 / sqrt.
Share condition: over the bf16 cases of one entry point, at most SHARE_CAP = 0.5 % of the elements may differ from the
reference rounded to bf16 (the emulation: 0.009 % at worst, add-LayerNorm backward)."""
import torch

F32, BF16 = 0, 1
DT = {"f32": F32, "bf16": BF16}
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
EPS = 1e-5

K_SLACK = {"y": 16.4, "dx": 14.5, "dw": 11.3, "colsum": 4.0, "stat": 10.9}
SHARE_CAP = 0.005

# the operands of each entry point (dxa_norm_desc roles), in the order the test allocates them
OPERANDS = {
    "rmsnorm_fwd": ("x", "w", "y", "rstd"),
    "rmsnorm_bwd": ("dy", "x", "w", "rstd", "dx", "residual", "partial"),
    "layernorm_fwd": ("x", "w", "b", "y", "mean", "rstd"),
    "layernorm_bwd": ("dy", "x", "w", "mean", "rstd", "dx", "residual", "partial"),
    "add_layernorm_fwd": ("x", "x2", "w", "b", "y", "mean", "rstd"),
    "add_layernorm_bwd": ("dy", "x", "x2", "w", "mean", "rstd", "dx", "partial"),
    "colsum": ("x", "y", "partial"),
    "downsample_layernorm_fwd": ("x", "w", "b", "y", "mean", "rstd"),
    "downsample_layernorm_bwd": ("dy", "x", "w", "mean", "rstd", "dx", "partial"),
    # adarms / gated residual: x2 = branch, gate = the gate third of a [B, 3 cols] modulation (row stride 3 cols), aux = r_out
    # (forward) / dbranch (backward), dx = dr (adarms) / dbranch (gated residual), dgate = the gate third of another [B, 3 cols]
    "adarms_fwd": ("x", "x2", "gate", "mod", "aux", "y", "rstd"),
    "adarms_bwd": ("dy", "x", "mod", "rstd", "residual", "x2", "gate", "dx", "dmod", "aux", "dgate", "partial"),
    "gated_residual_fwd": ("x", "x2", "gate", "y"),
    "gated_residual_bwd": ("dy", "x2", "gate", "dx", "dgate", "partial"),
}
# fake addresses for the planner: 256-byte aligned, far apart
FAKE = {n: (0x10 + i) << 36 for i, n in enumerate(("x", "x2", "w", "b", "y", "dy", "dx", "residual", "partial", "mean", "rstd", "gate",
                                                   "mod", "aux", "dgate", "dmod"))}
SAMPLE_ENTRIES = ("adarms_fwd", "adarms_bwd", "gated_residual_fwd", "gated_residual_bwd")


def _c(entry, rows, cols, kernel, dtype="bf16", w_dtype=None, w=True, b=True, res=None, mis=None, trips=None):
    bwd = entry.endswith("_bwd")
    if w_dtype is None:
        w_dtype = dtype
    if res is None:
        res = bwd and not entry.startswith("add_")
    tag = f"{entry}-{rows}x{cols}-{dtype}-{w_dtype}" + ("" if w else "-now") + ("" if (b or not entry.startswith(("layer", "add"))) else "-nob") + \
          ("-res" if res else "") + (f"-mis_{mis}" if mis else "")
    return dict(id=tag, entry=entry, rows=rows, cols=cols, dtype=dtype, w_dtype=w_dtype, w=w, b=b and w, res=res, mis=mis,
                kernel=kernel, trips=trips)


NORM_CASES = [
    # ---------------------------------------------------------------------------------------------- RMSNorm forward
    _c("rmsnorm_fwd", 3, 8, "rmsnorm_fwd_fast_k<bf16>"),                        # one live lane of the register-resident kernel
    _c("rmsnorm_fwd", 5, 8192, "rmsnorm_fwd_fast_k<float>", w_dtype="f32"),     # its last chunk
    _c("rmsnorm_fwd", 2049, 16, "rmsnorm_fwd_fast_k<bf16>"),
    _c("rmsnorm_fwd", 3, 520, "rmsnorm_fwd_fast_k<bf16>", w=False),
    _c("rmsnorm_fwd", 3, 8200, "rmsnorm_fwd_k<bf16,bf16,4>"),                   # generic above 8192
    _c("rmsnorm_fwd", 3, 4, "rmsnorm_fwd_k<bf16,bf16,4>"),
    _c("rmsnorm_fwd", 5, 7, "rmsnorm_fwd_k<bf16,bf16,1>"),
    _c("rmsnorm_fwd", 3, 512, "rmsnorm_fwd_k<bf16,bf16,1>", mis="x"),
    _c("rmsnorm_fwd", 3, 504, "rmsnorm_fwd_k<bf16,bf16,1>", mis="y"),
    _c("rmsnorm_fwd", 3, 132, "rmsnorm_fwd_k<bf16,float,4>", w_dtype="f32"),
    _c("rmsnorm_fwd", 2, 8208, "rmsnorm_fwd_k<bf16,float,4>", w_dtype="f32"),
    _c("rmsnorm_fwd", 1, 130, "rmsnorm_fwd_k<bf16,float,1>", w_dtype="f32"),
    _c("rmsnorm_fwd", 3, 72, "rmsnorm_fwd_k<bf16,float,1>", w_dtype="f32", mis="w"),
    _c("rmsnorm_fwd", 3, 512, "rmsnorm_fwd_k<float,float,4>", dtype="f32"),
    _c("rmsnorm_fwd", 3, 4100, "rmsnorm_fwd_k<float,float,4>", dtype="f32", w=False),
    _c("rmsnorm_fwd", 5, 1, "rmsnorm_fwd_k<float,float,1>", dtype="f32"),
    _c("rmsnorm_fwd", 3, 504, "rmsnorm_fwd_k<float,float,1>", dtype="f32", mis="y"),
    # --------------------------------------------------------------------------------------------- RMSNorm backward
    _c("rmsnorm_bwd", 5, 4096, "rmsnorm_bwd_split_k<bf16,4,4>"),                # last size of split NIT = 4
    _c("rmsnorm_bwd", 3, 512, "rmsnorm_bwd_split_k<bf16,4,4>", res=False),
    _c("rmsnorm_bwd", 4100, 16, "rmsnorm_bwd_split_k<bf16,4,4>", trips=3),      # third trip: parity slots reused
    _c("rmsnorm_bwd", 5, 512, "rmsnorm_bwd_split_k<bf16,4,4>", w=False),
    _c("rmsnorm_bwd", 3, 4112, "rmsnorm_bwd_split_k<bf16,8,4>"),                # first size of split NIT = 8
    _c("rmsnorm_bwd", 5, 8192, "rmsnorm_bwd_split_k<bf16,8,4>"),                # its last chunk
    _c("rmsnorm_bwd", 2049, 16, "rmsnorm_bwd_split_k<float,4,4>", w_dtype="f32", trips=2),
    _c("rmsnorm_bwd", 3, 8192, "rmsnorm_bwd_split_k<float,8,4>", w_dtype="f32", res=False),
    _c("rmsnorm_bwd", 3, 72, "norm_bwd_fast8_k<bf16,false>"),                   # % 8 but not % 16
    _c("rmsnorm_bwd", 4100, 8, "norm_bwd_fast8_k<bf16,false>", trips=3),        # one live lane, third trip
    _c("rmsnorm_bwd", 5, 520, "norm_bwd_fast8_k<float,false>", w_dtype="f32"),
    _c("rmsnorm_bwd", 3, 132, "norm_bwd_fast_k<bf16,bf16,false>"),              # % 4 but not % 8
    _c("rmsnorm_bwd", 4100, 4, "norm_bwd_fast_k<bf16,bf16,false>", trips=3),
    _c("rmsnorm_bwd", 1, 132, "norm_bwd_fast_k<bf16,float,false>", w_dtype="f32"),
    _c("rmsnorm_bwd", 3, 512, "norm_bwd_fast_k<float,float,false>", dtype="f32"),
    _c("rmsnorm_bwd", 3, 4096, "norm_bwd_fast_k<float,float,false>", dtype="f32", res=False),
    _c("rmsnorm_bwd", 2049, 4, "norm_bwd_fast_k<float,float,false>", dtype="f32", trips=2),
    _c("rmsnorm_bwd", 3, 4100, "rmsnorm_bwd_k<bf16,bf16,4>"),                   # generic 4-wide backward
    _c("rmsnorm_bwd", 3, 8200, "rmsnorm_bwd_k<bf16,bf16,4>"),
    _c("rmsnorm_bwd", 2, 8208, "rmsnorm_bwd_k<bf16,bf16,4>", res=False),
    _c("rmsnorm_bwd", 5, 7, "rmsnorm_bwd_k<bf16,bf16,1>"),
    _c("rmsnorm_bwd", 3, 130, "rmsnorm_bwd_k<bf16,bf16,1>"),
    _c("rmsnorm_bwd", 4100, 3, "rmsnorm_bwd_k<bf16,bf16,1>", trips=3),
    _c("rmsnorm_bwd", 1, 1, "rmsnorm_bwd_k<bf16,bf16,1>"),
    _c("rmsnorm_bwd", 3, 512, "rmsnorm_bwd_k<bf16,bf16,1>", mis="x"),           # aligned sizes, misaligned pointer
    _c("rmsnorm_bwd", 3, 512, "rmsnorm_bwd_k<bf16,bf16,1>", mis="dy"),
    _c("rmsnorm_bwd", 3, 512, "rmsnorm_bwd_k<bf16,bf16,1>", mis="dx"),
    _c("rmsnorm_bwd", 3, 512, "rmsnorm_bwd_k<bf16,bf16,1>", mis="w"),
    _c("rmsnorm_bwd", 3, 512, "rmsnorm_bwd_k<bf16,bf16,1>", mis="partial"),
    _c("rmsnorm_bwd", 3, 512, "rmsnorm_bwd_k<bf16,bf16,1>", mis="residual"),
    _c("rmsnorm_bwd", 3, 4104, "rmsnorm_bwd_k<bf16,float,4>", w_dtype="f32"),
    _c("rmsnorm_bwd", 3, 130, "rmsnorm_bwd_k<bf16,float,1>", w_dtype="f32"),
    _c("rmsnorm_bwd", 3, 72, "rmsnorm_bwd_k<bf16,float,1>", w_dtype="f32", mis="w"),
    _c("rmsnorm_bwd", 3, 4100, "rmsnorm_bwd_k<float,float,4>", dtype="f32"),
    _c("rmsnorm_bwd", 2, 8200, "rmsnorm_bwd_k<float,float,4>", dtype="f32", w=False),
    _c("rmsnorm_bwd", 5, 7, "rmsnorm_bwd_k<float,float,1>", dtype="f32"),
    _c("rmsnorm_bwd", 3, 130, "rmsnorm_bwd_k<float,float,1>", dtype="f32", w=False),
    _c("rmsnorm_bwd", 3, 512, "rmsnorm_bwd_k<float,float,1>", dtype="f32", mis="residual"),
    # -------------------------------------------------------------------------------------------- LayerNorm forward
    _c("layernorm_fwd", 3, 512, "layernorm_fwd_k<bf16,bf16,4>"),
    _c("layernorm_fwd", 3, 72, "layernorm_fwd_k<bf16,bf16,4>", w=False),
    _c("layernorm_fwd", 5, 7, "layernorm_fwd_k<bf16,bf16,1>"),
    _c("layernorm_fwd", 3, 512, "layernorm_fwd_k<bf16,bf16,1>", mis="b"),
    _c("layernorm_fwd", 3, 4104, "layernorm_fwd_k<bf16,float,4>", w_dtype="f32"),
    _c("layernorm_fwd", 3, 130, "layernorm_fwd_k<bf16,float,1>", w_dtype="f32"),
    _c("layernorm_fwd", 3, 512, "layernorm_fwd_k<bf16,float,1>", w_dtype="f32", mis="x"),
    _c("layernorm_fwd", 3, 512, "layernorm_fwd_k<bf16,float,1>", w_dtype="f32", mis="w"),
    _c("layernorm_fwd", 2, 8192, "layernorm_fwd_k<float,float,4>", dtype="f32"),
    _c("layernorm_fwd", 1, 1, "layernorm_fwd_k<float,float,1>", dtype="f32"),
    _c("layernorm_fwd", 3, 132, "layernorm_fwd_k<float,float,1>", dtype="f32", mis="y"),
    # ------------------------------------------------------------------------------------------- LayerNorm backward
    _c("layernorm_bwd", 5, 512, "norm_bwd_fast_k<bf16,bf16,true>"),
    _c("layernorm_bwd", 4100, 4, "norm_bwd_fast_k<bf16,bf16,true>", trips=3),
    _c("layernorm_bwd", 3, 520, "norm_bwd_fast_k<bf16,bf16,true>", w=False),
    _c("layernorm_bwd", 3, 72, "norm_bwd_fast_k<bf16,float,true>", w_dtype="f32", res=False),
    _c("layernorm_bwd", 2049, 8, "norm_bwd_fast_k<bf16,float,true>", w_dtype="f32", trips=2),
    _c("layernorm_bwd", 3, 4096, "norm_bwd_fast_k<float,float,true>", dtype="f32"),
    _c("layernorm_bwd", 4100, 16, "norm_bwd_fast_k<float,float,true>", dtype="f32", trips=3),
    _c("layernorm_bwd", 3, 4100, "layernorm_bwd_k<bf16,bf16,4>"),               # cols > 4096
    _c("layernorm_bwd", 4100, 3, "layernorm_bwd_k<bf16,bf16,1>", trips=3),
    _c("layernorm_bwd", 3, 512, "layernorm_bwd_k<bf16,bf16,1>", mis="partial"),
    _c("layernorm_bwd", 2, 8208, "layernorm_bwd_k<bf16,float,4>", w_dtype="f32"),
    _c("layernorm_bwd", 3, 130, "layernorm_bwd_k<bf16,float,1>", w_dtype="f32"),
    _c("layernorm_bwd", 3, 512, "layernorm_bwd_k<bf16,float,1>", w_dtype="f32", mis="x"),
    _c("layernorm_bwd", 3, 512, "layernorm_bwd_k<bf16,float,1>", w_dtype="f32", mis="dy"),
    _c("layernorm_bwd", 3, 512, "layernorm_bwd_k<bf16,float,1>", w_dtype="f32", mis="dx"),
    _c("layernorm_bwd", 3, 512, "layernorm_bwd_k<bf16,float,1>", w_dtype="f32", mis="w"),
    _c("layernorm_bwd", 3, 512, "layernorm_bwd_k<bf16,float,1>", w_dtype="f32", mis="residual"),
    _c("layernorm_bwd", 2, 4104, "layernorm_bwd_k<float,float,4>", dtype="f32"),
    _c("layernorm_bwd", 5, 7, "layernorm_bwd_k<float,float,1>", dtype="f32"),
    _c("layernorm_bwd", 3, 130, "layernorm_bwd_k<float,float,1>", dtype="f32", w=False),
    # ---------------------------------------------------------------------------------------- add-LayerNorm forward
    _c("add_layernorm_fwd", 3, 512, "layernorm_fwd_k<bf16,bf16,4,true>"),
    _c("add_layernorm_fwd", 3, 72, "layernorm_fwd_k<bf16,bf16,4,true>", w=False),
    _c("add_layernorm_fwd", 5, 130, "layernorm_fwd_k<bf16,bf16,1,true>"),
    _c("add_layernorm_fwd", 2, 4104, "layernorm_fwd_k<bf16,float,4,true>", w_dtype="f32"),
    _c("add_layernorm_fwd", 3, 512, "layernorm_fwd_k<bf16,float,1,true>", w_dtype="f32", mis="x2"),
    _c("add_layernorm_fwd", 3, 512, "layernorm_fwd_k<bf16,bf16,1,true>", mis="x"),
    _c("add_layernorm_fwd", 3, 512, "layernorm_fwd_k<bf16,float,1,true>", w_dtype="f32", mis="y"),
    _c("add_layernorm_fwd", 3, 512, "layernorm_fwd_k<float,float,1,true>", dtype="f32", mis="w"),
    _c("add_layernorm_fwd", 3, 512, "layernorm_fwd_k<bf16,bf16,1,true>", mis="b"),
    _c("add_layernorm_fwd", 3, 8, "layernorm_fwd_k<float,float,4,true>", dtype="f32"),
    _c("add_layernorm_fwd", 5, 7, "layernorm_fwd_k<float,float,1,true>", dtype="f32"),
    # --------------------------------------------------------------------------------------- add-LayerNorm backward
    _c("add_layernorm_bwd", 5, 512, "layernorm_bwd_k<bf16,bf16,4,true>"),
    _c("add_layernorm_bwd", 4100, 4, "layernorm_bwd_k<bf16,bf16,4,true>", trips=3),
    _c("add_layernorm_bwd", 3, 72, "layernorm_bwd_k<bf16,bf16,4,true>", w=False),
    _c("add_layernorm_bwd", 3, 130, "layernorm_bwd_k<bf16,bf16,1,true>"),
    _c("add_layernorm_bwd", 2, 8208, "layernorm_bwd_k<bf16,float,4,true>", w_dtype="f32"),
    _c("add_layernorm_bwd", 2049, 3, "layernorm_bwd_k<bf16,float,1,true>", w_dtype="f32", trips=2),
    _c("add_layernorm_bwd", 2, 4100, "layernorm_bwd_k<float,float,4,true>", dtype="f32"),
    _c("add_layernorm_bwd", 3, 512, "layernorm_bwd_k<float,float,1,true>", dtype="f32", mis="x2"),
    _c("add_layernorm_bwd", 3, 512, "layernorm_bwd_k<bf16,bf16,1,true>", mis="x"),
    _c("add_layernorm_bwd", 3, 512, "layernorm_bwd_k<bf16,float,1,true>", w_dtype="f32", mis="dy"),
    _c("add_layernorm_bwd", 3, 512, "layernorm_bwd_k<float,float,1,true>", dtype="f32", mis="dx"),
    _c("add_layernorm_bwd", 3, 512, "layernorm_bwd_k<bf16,float,1,true>", w_dtype="f32", mis="w"),
]


def _ds(entry, N, G, C, kernel, dtype="bf16", w_dtype=None, w=True, mis=None, trips=None):
    """a 2x2 token merge + LayerNorm(4C) case: x [N, G*G, C] -> [N * h * h, 4C], h = ceil(G / 2)"""
    w_dtype = w_dtype or dtype
    tag = f"{entry}-{N}x{G}x{G}x{C}-{dtype}-{w_dtype}" + ("" if w else "-now") + (f"-mis_{mis}" if mis else "")
    return dict(id=tag, entry=entry, rows=N, G=G, cols=C, dtype=dtype, w_dtype=w_dtype, w=w, b=w, res=False, mis=mis, kernel=kernel,
                trips=trips)


def _ar(entry, B, rps, C, kernel, dtype="bf16", gated=True, res=False, mis=None, trips=None):
    """an adarms / gated-residual case: B samples of rps rows of C columns"""
    gated = gated or entry.startswith("gated")
    tag = f"{entry}-{B}x{rps}x{C}-{dtype}" + ("-gated" if gated and entry.startswith("adarms") else "") + ("-res" if res else "") + \
          (f"-mis_{mis}" if mis else "")
    return dict(id=tag, entry=entry, rows=B * rps, B=B, rps=rps, cols=C, dtype=dtype, w_dtype=dtype, w=False, b=False, gated=gated, res=res,
                mis=mis, kernel=kernel, trips=trips)


DS_CASES = [
    _ds("downsample_layernorm_fwd", 1, 3, 8, "ds_layernorm_fwd_k<bf16,bf16,8>"),            # odd grid: padded quarters
    _ds("downsample_layernorm_fwd", 1, 3, 8, "ds_layernorm_fwd_k<bf16,bf16,8>", w=False),
    _ds("downsample_layernorm_fwd", 2, 3, 6, "ds_layernorm_fwd_k<bf16,bf16,1>"),
    _ds("downsample_layernorm_fwd", 1, 4, 8, "ds_layernorm_fwd_k<bf16,bf16,1>", mis="y"),
    _ds("downsample_layernorm_fwd", 1, 4, 16, "ds_layernorm_fwd_k<bf16,float,8>", w_dtype="f32"),
    _ds("downsample_layernorm_fwd", 1, 3, 12, "ds_layernorm_fwd_k<bf16,float,1>", w_dtype="f32"),
    _ds("downsample_layernorm_fwd", 1, 3, 4, "ds_layernorm_fwd_k<float,float,4>", dtype="f32"),
    _ds("downsample_layernorm_fwd", 1, 3, 6, "ds_layernorm_fwd_k<float,float,1>", dtype="f32"),
    _ds("downsample_layernorm_bwd", 1, 3, 8, "ds_layernorm_bwd_k<bf16,bf16,8>"),
    _ds("downsample_layernorm_bwd", 1, 3, 8, "ds_layernorm_bwd_k<bf16,bf16,8>", w=False),
    _ds("downsample_layernorm_bwd", 1, 2, 1928, "ds_layernorm_bwd_k<bf16,bf16,8>"),       # sums too wide for LDS: in the slab
    _ds("downsample_layernorm_bwd", 2, 3, 6, "ds_layernorm_bwd_k<bf16,bf16,1>"),
    _ds("downsample_layernorm_bwd", 1, 4, 8, "ds_layernorm_bwd_k<bf16,bf16,1>", mis="dy"),
    _ds("downsample_layernorm_bwd", 1, 4, 16, "ds_layernorm_bwd_k<bf16,float,8>", w_dtype="f32"),
    _ds("downsample_layernorm_bwd", 1, 3, 12, "ds_layernorm_bwd_k<bf16,float,1>", w_dtype="f32"),
    _ds("downsample_layernorm_bwd", 2049, 2, 4, "ds_layernorm_bwd_k<float,float,4>", dtype="f32", trips=2),
    _ds("downsample_layernorm_bwd", 1, 3, 6, "ds_layernorm_bwd_k<float,float,1>", dtype="f32"),
]

AR_CASES = [
    # a 4-row workgroup spans samples (rps 3); widths: 64 / 8200 (16-byte bf16, register-resident up to 8192), 20 (8-byte bf16,
    # 16-byte fp32), 21 (scalar)
    _ar("adarms_fwd", 2, 3, 64, "adarms_fwd_fast_k<false>", gated=False),
    _ar("adarms_fwd", 2, 3, 64, "adarms_fwd_fast_k<true>"),
    _ar("adarms_fwd", 1, 2, 8200, "adarms_fwd_k<bf16,8,false>", gated=False),
    _ar("adarms_fwd", 1, 2, 8200, "adarms_fwd_k<bf16,8,true>"),
    _ar("adarms_fwd", 2, 3, 20, "adarms_fwd_k<bf16,4,false>", gated=False),
    _ar("adarms_fwd", 2, 3, 20, "adarms_fwd_k<bf16,4,true>"),
    _ar("adarms_fwd", 2, 3, 21, "adarms_fwd_k<bf16,1,false>", gated=False),
    _ar("adarms_fwd", 2, 3, 21, "adarms_fwd_k<bf16,1,true>"),
    _ar("adarms_fwd", 2, 3, 64, "adarms_fwd_k<bf16,1,true>", mis="aux"),
    _ar("adarms_fwd", 2, 3, 20, "adarms_fwd_k<float,4,false>", dtype="f32", gated=False),
    _ar("adarms_fwd", 2, 3, 20, "adarms_fwd_k<float,4,true>", dtype="f32"),
    _ar("adarms_fwd", 2, 3, 21, "adarms_fwd_k<float,1,false>", dtype="f32", gated=False),
    _ar("adarms_fwd", 2, 3, 21, "adarms_fwd_k<float,1,true>", dtype="f32"),
    _ar("adarms_fwd", 2, 3, 64, "adarms_fwd_k<float,1,false>", dtype="f32", gated=False, mis="x"),
    _ar("adarms_bwd", 2, 3, 64, "adarms_bwd_k<bf16,8,false>", gated=False, res=True),
    _ar("adarms_bwd", 2, 3, 64, "adarms_bwd_k<bf16,8,true>"),
    _ar("adarms_bwd", 2, 3, 20, "adarms_bwd_k<bf16,4,false>", gated=False),
    _ar("adarms_bwd", 2, 3, 20, "adarms_bwd_k<bf16,4,true>", res=True),
    _ar("adarms_bwd", 2, 3, 21, "adarms_bwd_k<bf16,1,false>", gated=False, res=True),
    _ar("adarms_bwd", 2, 3, 21, "adarms_bwd_k<bf16,1,true>"),
    _ar("adarms_bwd", 2, 3, 64, "adarms_bwd_k<bf16,1,false>", gated=False, res=True, mis="residual"),
    _ar("adarms_bwd", 2, 3, 20, "adarms_bwd_k<float,4,false>", dtype="f32", gated=False),
    _ar("adarms_bwd", 2, 3, 20, "adarms_bwd_k<float,4,true>", dtype="f32", res=True),
    _ar("adarms_bwd", 1, 1030, 4, "adarms_bwd_k<float,4,false>", dtype="f32", gated=False, trips=3),   # third trip of the row loop
    _ar("adarms_bwd", 2, 3, 21, "adarms_bwd_k<float,1,false>", dtype="f32", gated=False),
    _ar("adarms_bwd", 2, 3, 21, "adarms_bwd_k<float,1,true>", dtype="f32", res=True),
    _ar("gated_residual_fwd", 2, 3, 64, "gated_residual_fwd_k<bf16,8>"),
    _ar("gated_residual_fwd", 2, 3, 20, "gated_residual_fwd_k<bf16,4>"),
    _ar("gated_residual_fwd", 2, 3, 21, "gated_residual_fwd_k<bf16,1>"),
    _ar("gated_residual_fwd", 2, 3, 64, "gated_residual_fwd_k<bf16,1>", mis="y"),
    _ar("gated_residual_fwd", 2, 3, 20, "gated_residual_fwd_k<float,4>", dtype="f32"),
    _ar("gated_residual_fwd", 2, 3, 21, "gated_residual_fwd_k<float,1>", dtype="f32"),
    _ar("gated_residual_bwd", 2, 3, 64, "gated_residual_bwd_k<bf16,8>"),
    _ar("gated_residual_bwd", 1, 1030, 8, "gated_residual_bwd_k<bf16,8>", trips=3),
    _ar("gated_residual_bwd", 2, 3, 20, "gated_residual_bwd_k<bf16,4>"),
    _ar("gated_residual_bwd", 2, 3, 21, "gated_residual_bwd_k<bf16,1>"),
    _ar("gated_residual_bwd", 2, 3, 64, "gated_residual_bwd_k<bf16,1>", mis="dx"),
    _ar("gated_residual_bwd", 2, 3, 20, "gated_residual_bwd_k<float,4>", dtype="f32"),
    _ar("gated_residual_bwd", 2, 3, 21, "gated_residual_bwd_k<float,1>", dtype="f32"),
]

NORM_CASES = NORM_CASES + DS_CASES + AR_CASES


def _cs(rows, cols, dtype, view, accumulate, kernel, capture_kernel=None):
    return dict(id=f"colsum-{rows}x{cols}-{dtype}-{view}" + ("-acc" if accumulate else ""), entry="colsum", rows=rows, cols=cols,
                dtype=dtype, view=view, accumulate=accumulate, kernel=kernel, capture_kernel=capture_kernel)


_F, _FF = "colsum_fused_k<bf16>", "colsum_fused_k<float>"
_S, _SF = "colsum_stage1_k<bf16,false>", "colsum_stage1_k<float,false>"
COLSUM_CASES = [
    _cs(1, 1, "f32", "contig", False, "colsum_stage1_k<float,true>"),
    _cs(1, 260, "f32", "coloff", True, "colsum_stage1_k<float,true>"),
    _cs(32, 257, "bf16", "contig", True, "colsum_stage1_k<bf16,true>"),        # last row count of the direct kernel
    _cs(32, 4, "bf16", "ld4", False, "colsum_stage1_k<bf16,true>"),
    _cs(33, 256, "f32", "contig", False, _FF, _SF),                             # first of the fused one
    _cs(33, 3, "bf16", "ldodd", True, _F, _S),
    _cs(64, 4, "f32", "ld4", True, _FF, _SF),
    _cs(65, 255, "bf16", "coloff", False, _F, _S),
    _cs(65, 257, "f32", "coloff", True, _FF, _SF),
    _cs(2048, 260, "f32", "contig", False, _FF, _SF),                           # 64 splits of 32 rows
    _cs(2049, 257, "bf16", "ld4", False, _F, _S),                               # nsplit capped at 64
    _cs(2081, 1, "f32", "ldodd", True, _FF, _SF),
    _cs(2081, 3, "bf16", "coloff", True, _F, _S),
]

ALL_CASES = NORM_CASES + COLSUM_CASES


def ld_of(case):
    """row stride (elements) and element offset of a column-sum input inside its buffer"""
    c = case["cols"]
    v = case["view"]
    if v == "contig":
        return c, 0
    if v == "ld4":
        return (c // 4 + 2) * 4, 0
    if v == "ldodd":
        return c + (1 if (c + 1) % 4 else 2), 0
    return 2 * c, c                     # coloff: part[:, cols:] of a [rows, 2 cols] slab


def ds_rows(case):
    """output rows of a downsample case: N * h * h"""
    h = (case["G"] + 1) // 2
    return case["rows"] * h * h


def adarms_groups(rps):
    return max(1, min(128, (rps + 3) // 4))


def partial_rows(case):
    """rows of the partial slab a backward case writes: one per workgroup (dxa_norm_bwd_blocks); adarms / gated residual: one per
    wave of each sample's row groups"""
    if case["entry"] in SAMPLE_ENTRIES:
        return case["B"] * adarms_groups(case["rps"]) * 4
    r = ds_rows(case) if case["entry"].startswith("downsample") else case["rows"]
    return max(1, min(512, (r + 3) // 4))


def partial_cols(case):
    e, C = case["entry"], case["cols"]
    if e in SAMPLE_ENTRIES:
        return (1 if e.startswith("gated") else 3 if case["gated"] else 2) * C
    if e.startswith("downsample"):
        return 8 * C
    return (1 if e == "rmsnorm_bwd" else 2) * C


def colsum_nsplit(rows):
    return max(1, min(64, (rows + 31) // 32))


def present(case):
    """the operands a case passes (others are NULL)"""
    ops = []
    sample = case["entry"] in SAMPLE_ENTRIES
    for n in OPERANDS[case["entry"]]:
        if sample and n in ("x2", "gate", "aux", "dgate") and not case["gated"]:
            continue
        if not sample and n in ("w", "partial") and not case.get("w", True):
            continue
        if n == "b" and not case.get("b", True):
            continue
        if n == "residual" and not case.get("res"):
            continue
        ops.append(n)
    return ops


def plan_fields(case, addr):
    """dxa_norm_desc fields of a case; ``addr(name)`` gives the address of a present operand"""
    e = case["entry"]
    f = dict(dtype=DT[case["dtype"]], rows=case["rows"], cols=case["cols"])
    if e == "colsum":
        f.update(ld=ld_of(case)[0], accumulate=int(case["accumulate"]),
                 partial_bytes=colsum_nsplit(case["rows"]) * case["cols"] * 4)
    else:
        f["w_dtype"] = DT[case["w_dtype"]]
    if e.startswith("downsample"):
        f["G"] = case["G"]
    if e in SAMPLE_ENTRIES:
        f.update(rows_per_sample=case["rps"], gate_ld=3 * case["cols"], dgate_ld=3 * case["cols"],
                 partial_bytes=partial_rows(case) * partial_cols(case) * 4)
    for n in present(case):
        f[n] = addr(n)
    return f


def fake_addr(case):
    """the planner's addresses: 256-byte aligned, the ``mis`` operand one element in; a column-sum input at its view's offset"""
    es = {"f32": 4, "bf16": 2}

    def addr(n):
        a = FAKE[n]
        if case["entry"] == "colsum" and n == "x":
            return a + ld_of(case)[1] * es[case["dtype"]]
        if n in ("gate", "dgate"):                # the gate third of a [B, 3 cols] modulation
            a += 2 * case["cols"] * es[case["dtype"]]
        if n == case.get("mis"):
            wide = n in ("w", "b") and case["w_dtype"] == "f32" or n == "partial" or case["dtype"] == "f32" and n not in ("w", "b")
            return a + (4 if wide else 2)
        return a
    return addr


def inputs(case):
    """the case's inputs on the CPU, in their stored dtypes (seeded by the case's id)"""
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"])) & 0x7FFFFFFF)
    R, C = case["rows"], case["cols"]
    T = TORCH_DT[case["dtype"]]
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    if case["entry"] == "colsum":
        out = dict(x=rn(R, C).to(T))
        if case["accumulate"]:
            out["y0"] = rn(C).float()
        return out
    e = case["entry"]
    if e.startswith("downsample"):
        G, h = case["G"], (case["G"] + 1) // 2
        TW = TORCH_DT[case["w_dtype"]]
        out = dict(x=(rn(R, G * G, C) + 0.5).to(T))
        if case["w"]:
            out["w"] = (1 + 0.1 * rn(4 * C)).to(TW)
            out["b"] = (0.1 * rn(4 * C)).to(TW)
        if e.endswith("_bwd"):
            out["dy"] = rn(R * h * h, 4 * C).to(T)
        return out
    if e in SAMPLE_ENTRIES:
        B = case["B"]
        out = dict(x=rn(R, C).to(T))
        # every sample has a modulation of its own; the gate is the last third of another one
        out["mod"] = (0.5 * rn(B, 3 * C) + 0.25 * torch.arange(B, dtype=torch.float64)[:, None]).to(T)
        out["modp"] = (0.5 * rn(B, 3 * C) - 0.25 * torch.arange(B, dtype=torch.float64)[:, None]).to(T)
        out["x2"] = rn(R, C).to(T)
        if e.endswith("_bwd"):
            out["dy"] = rn(R, C).to(T)
            if case["res"]:
                out["residual"] = rn(R, C).to(T)
        if not case["gated"]:
            del out["x2"]
        return out
    TW = TORCH_DT[case["w_dtype"]]
    ln = not case["entry"].startswith("rms")
    out = dict(x=(rn(R, C) + (0.5 if ln else 0.0)).to(T))
    if case["entry"].startswith("add_"):
        out["x2"] = rn(R, C).to(T)
    if case["w"]:
        out["w"] = (1 + 0.1 * rn(C)).to(TW)
        if ln and case["b"]:
            out["b"] = (0.1 * rn(C)).to(TW)
    if case["entry"].endswith("_bwd"):
        out["dy"] = rn(R, C).to(T)
        if case["res"]:
            out["residual"] = rn(R, C).to(T)
    return out
