"""The loss-head route cases: one deterministic table of small calls of the entry points of csrc/loss.hip other than
dxa_sample_rows (cross-entropy forward and backward with hard, soft and row-weighted targets, dxa_argmax_rows,
dxa_ce_sample_reduce, dxa_expectile_loss) that together reach every kernel instantiation their launchers can launch, each with
the kernel it is there to reach, written down as data.  Used on the CPU by tests/test_loss_cases.py (the table is complete and
``route`` — the launch predicates of ce_fwd_launch, ce_bwd_launch and dxa_argmax_rows in plain Python — agrees with it) and
tests/test_loss_ref.py (the reference and the slack constants below), and on the MI355X by tests/test_loss_routes_gpu.py.
Nothing here needs a GPU.

A case is a dict with ``id``, ``entry``, ``dtype``, ``kernel`` (a key of INSTANTIATIONS), ``reason`` (why it leaves the 4-wide /
wide route, or None), ``off`` (operand name -> elements between a 256-byte-aligned address and the operand's first element) and
  * cross-entropy (``ce_fwd``, ``soft_fwd``, ``ce_bwd``, ``soft_bwd``, ``rows_bwd``): ``rows``, ``V``; ``layout`` of the logits
    (``contig``; ``ld4``: ld = V + 8; ``ldodd``: ld = V + 9); ``dlayout`` of the backward's dlogits (``same``: its own buffer with
    ldd = ld; ``contig``: ldd = V; ``ld12``: ldd = V + 12; ``ldodd``: ldd = V + 9; ``inplace``: dlogits is logits); ``vals`` (the
    value family, see ``ce_values``); ``labels`` (per-row tokens, cycled: ``r`` a random id, ``0``, ``last`` = V - 1, ``tail`` = V - 2
    (in the row's last vector), ``ign`` = the ignore index, ``V``, ``-1``, ``-7``, ``soft`` = one of the soft ids); ``ignore_index``;
    ``K`` soft ids; ``gscale`` (None: NULL) and ``row_w`` (None: NULL, else per-row tokens); ``trips``: the row-loop trips of one
    thread the case is there for;
  * ``argmax``: ``rows``, ``cols``, ``layout`` (``contig``, ``ld4`` = cols + 4, ``ld8`` = cols + 8, ``ldodd`` = cols + 9), ``maxcols``
    (columns that hold the row's largest value, the lowest must win) or ``special`` (see ``argmax_values``);
  * ``sample_reduce``: ``B``, ``L``, ``reward`` (None, ``gauss``, ``big`` = +-30), ``empty`` (sample 0 has no valid label);
  * ``expectile``: ``n``, ``tau``, ``dpred``.

Value criterion (tests/test_loss_routes_gpu.py), every output element against tests/loss_ref.py:
    |got - ref| <= U * ulp_T(ref) + k * 2^-24 * mag,        U = 1 for a bf16 output, 0 for fp32,
a non-finite reference element must be matched exactly (NaN by NaN, an infinity by the same one), argmax indices must be equal.
``mag`` is the sum of the absolute values of the terms that made the element (loss_ref.py).  ``K_SLACK`` holds k per output kind:
4 x the largest error, in units of 2^-24 * mag and beyond the U ulp, of a plain fp32 torch evaluation of the same formulas on the
CPU (loss_ref.emulate) against the fp64 reference over the whole table (tests/test_loss_ref.py measures it again and requires
it to stay within K_SLACK / 4).  Measured over this table:
    lse 0.85, row_loss 1.20, dlogits 1.29, sample loss 0.96, row_w 0.80, expectile loss 1.79, dpred 2.28
    ->  k = 3.4, 4.8, 5.2, 3.9, 3.2, 7.2, 9.2                                                    (x 4, rounded up)
The factor 4 covers the kernels' butterfly summation order and expf / logf against torch's.
Share condition: over the bf16 dlogits of one entry point at most SHARE_CAP = 0.5 % of the elements may differ from the
reference rounded to bf16 (the emulation: 0.014 % at worst, the soft backward; none over the hard and row-weighted ones)."""
import math

import torch

from tests.elementwise_cases import demangled, key, mangled

F32, BF16 = 0, 1
DT = {"f32": F32, "bf16": BF16}
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ES = {"f32": 4, "bf16": 2}

K_SLACK = {"lse": 3.4, "row_loss": 4.8, "dlogits": 5.2, "sample_loss": 3.9, "row_w": 3.2, "expectile_loss": 7.2, "dpred": 9.2}
SHARE_CAP = 0.005

INV2S2 = 1.0 / 18.0                                  # soft targets: std 3 ids
SCALE = 1.0 / 7.0                                    # the backward's 1 / #rows factor
GSCALE = 0.37
SAMPLE_V = 1000                                      # vocabulary of the per-sample reduction's labels
FWD, BWD = ("ce_fwd", "soft_fwd"), ("ce_bwd", "soft_bwd", "rows_bwd")

# ------------------------------------------------------------------------------------------------------- instantiations
_I = [("soft_ce_fwd_k", (t, v)) for t in ("f32", "bf16") for v in (4, 1)]
_I += [("soft_ce_bwd_k", (t, v, s, w)) for t in ("f32", "bf16") for v in (4, 1) for s, w in ((False, False), (True, False), (False, True))]
_I += [("argmax_rows_k", (t, v)) for t in ("f32", "bf16") for v in (4, 1)]
_I += [("argmax_rows_wide_k", ()), ("ce_sample_reduce_k", ()), ("expectile_loss_k", ())]
INSTANTIATIONS = {key(k, t): dict(kernel=k, targs=t, mangled=mangled(k, t), demangled=demangled(k, t)) for k, t in _I}

FALL_OFF_CE = ("V%4", "ld%4", "ldd%4", "mis_logits", "mis_dlogits", "off4")
FALL_OFF_WIDE = ("rows65", "cols16376", "cols16388", "ld+4", "off4", "f32")


def fk(t, v):
    return key("soft_ce_fwd_k", (t, v))


def bk(t, v, soft=False, roww=False):
    return key("soft_ce_bwd_k", (t, v, soft, roww))


def ak(t, v):
    return key("argmax_rows_k", (t, v))


WIDE = "argmax_rows_wide_k"


# ------------------------------------------------------------------------------------------------------- geometry and route
def ld_of(case):
    n = case["V"] if "V" in case else case["cols"]
    return n + {"contig": 0, "ld4": 8 if "V" in case else 4, "ld8": 8, "ldodd": 9}[case["layout"]]


def ldd_of(case):
    d = case["dlayout"]
    return ld_of(case) if d in ("same", "inplace") else case["V"] + {"contig": 0, "ld12": 12, "ldodd": 9}[d]


def _al(case, name, a):
    return (case["off"].get(name, 0) * ES[case["dtype"]]) % a == 0


def route(case):
    """the instantiation the launcher chooses for the case (ce_fwd_launch, ce_bwd_launch, dxa_argmax_rows)"""
    e, t = case["entry"], case["dtype"]
    if e == "sample_reduce":
        return "ce_sample_reduce_k"
    if e == "expectile":
        return "expectile_loss_k"
    es = ES[t]
    if e == "argmax":
        rows, cols, ld = case["rows"], case["cols"], ld_of(case)
        if t == "bf16" and rows <= 64 and 16384 <= cols < 2 ** 31 and cols % 8 == 0 and ld % 8 == 0 and _al(case, "x", 16):
            return WIDE
        vec = cols % 4 == 0 and ld % 4 == 0 and _al(case, "x", 4 * es)
        return ak(t, 4 if vec else 1)
    V, ld = case["V"], ld_of(case)
    vec = V % 4 == 0 and ld % 4 == 0 and _al(case, "logits", 4 * es)
    if e in FWD:
        return fk(t, 4 if vec else 1)
    vec = vec and ldd_of(case) % 4 == 0 and _al(case, "dlogits", 4 * es)
    soft = case["K"] > 0
    return bk(t, 4 if vec else 1, soft, (not soft) and case["row_w"] is not None)


def vec_width(case):
    k = route(case)
    return 8 if k == WIDE else INSTANTIATIONS[k]["targs"][1]


def trips_of(case):
    """row-loop trips of the busiest thread: 256 threads x VEC columns a trip (1024 x 8 in the wide argmax, a pair of them a trip
    and an unpaired tail one more)"""
    e = case["entry"]
    if e in ("sample_reduce", "expectile"):                  # one 1024-thread workgroup striding by 1024
        return -(-(case["L"] if e == "sample_reduce" else case["n"]) // 1024)
    n = case["cols"] if e == "argmax" else case["V"]
    if route(case) == WIDE:
        paired = max(0, -(-(n - 8192) // 16384))            # thread 0's trips of `for (i = 0; i + 8192 < cols; i += 16384)`
        return paired + (1 if n > 16384 * paired else 0)
    return -(-n // (256 * vec_width(case)))


# ------------------------------------------------------------------------------------------------------------------ table
CASES = []


def _add(c):
    CASES.append(c)
    return c


def _ce(entry, rows, V, dtype, kernel, layout="contig", dlayout="same", vals="gauss", labels=("r",), ignore_index=-100, K=0,
        gscale=GSCALE, row_w=None, off=None, reason=None, trips=None, tag=""):
    off = dict(off or {})
    bwd = entry in BWD
    if bwd and dlayout == "inplace":
        off["dlogits"] = off.get("logits", 0)
    parts = [entry, f"{rows}x{V}", dtype, layout] + ([f"d_{dlayout}"] if bwd else []) + [vals] + ([f"K{K}"] if K else []) + \
        (["lab_" + "_".join(labels)] if labels != ("r",) else []) + ([f"ign{ignore_index}"] if ignore_index != -100 else []) + \
        (["nogscale"] if bwd and gscale is None else []) + ([f"off_{n}{o}" for n, o in sorted(off.items()) if not (n == "dlogits" and dlayout == "inplace")]) + \
        ([tag] if tag else [])
    return _add(dict(id="-".join(parts), entry=entry, rows=rows, V=V, dtype=dtype, kernel=kernel, layout=layout,
                     dlayout=dlayout if bwd else None, vals=vals, labels=tuple(labels), ignore_index=ignore_index, K=K,
                     gscale=gscale if bwd else None, row_w=row_w if entry == "rows_bwd" else None, off=off, reason=reason, trips=trips))


ROW_W = ("zero", "neg", "r")                    # a zero weight, a negative weight, random ones
SOFT_LABELS = ("soft", "r", "ign")              # a soft row, a hard row and an ignored row in one call

for t in ("bf16", "f32"):
    # ---- sizes: the 4-wide route at V = 4 (one live thread), 1024 (exactly one trip), 1028 (a second trip for one thread), 2052 (a
    # third); the scalar route at V = 1, 7, 257, 513; rows 1, 3, 9 — forward and the three backward forms
    for rows, V, v, trips, reason in ((1, 4, 4, 1, None), (3, 1024, 4, 1, None), (9, 1028, 4, 2, None), (3, 2052, 4, 3, None),
                                      (3, 1, 1, 1, "V%4"), (1, 7, 1, 1, "V%4"), (9, 257, 1, 2, "V%4"), (3, 513, 1, 3, "V%4")):
        _ce("ce_fwd", rows, V, t, fk(t, v), reason=reason, trips=trips)
        _ce("ce_bwd", rows, V, t, bk(t, v), reason=reason, trips=trips)
        _ce("rows_bwd", rows, V, t, bk(t, v, False, True), row_w=ROW_W, reason=reason, trips=trips)
    _ce("rows_bwd", 3, 1028, t, bk(t, 4), row_w=None, tag="noroww")
    _ce("rows_bwd", 3, 1028, t, bk(t, 4, False, True), row_w=ROW_W, gscale=None)
    _ce("ce_bwd", 3, 1028, t, bk(t, 4), gscale=None)
    # ---- layouts and the reasons for leaving the 4-wide route
    _ce("ce_fwd", 3, 1028, t, fk(t, 4), layout="ld4")
    _ce("ce_fwd", 3, 1028, t, fk(t, 1), layout="ldodd", reason="ld%4")
    _ce("ce_fwd", 3, 1028, t, fk(t, 1), off={"logits": 1}, reason="mis_logits")
    _ce("ce_fwd", 3, 1028, t, fk(t, 1), layout="ld4", off={"logits": 3}, reason="mis_logits")
    _ce("ce_bwd", 3, 1028, t, bk(t, 4), layout="ld4", dlayout="same")
    _ce("ce_bwd", 3, 1028, t, bk(t, 4), layout="ld4", dlayout="ld12")
    _ce("ce_bwd", 3, 1028, t, bk(t, 4), layout="ld4", dlayout="contig")
    _ce("ce_bwd", 3, 1028, t, bk(t, 4), layout="ld4", dlayout="inplace")
    _ce("ce_bwd", 3, 1028, t, bk(t, 4), layout="contig", dlayout="inplace")
    _ce("ce_bwd", 3, 1028, t, bk(t, 1), layout="ldodd", dlayout="inplace", reason="ld%4")
    _ce("ce_bwd", 3, 1028, t, bk(t, 1), layout="ldodd", dlayout="ld12", reason="ld%4")
    _ce("ce_bwd", 3, 1028, t, bk(t, 1), layout="ld4", dlayout="ldodd", reason="ldd%4")
    _ce("ce_bwd", 3, 1028, t, bk(t, 1), off={"logits": 1}, reason="mis_logits")
    _ce("ce_bwd", 3, 1028, t, bk(t, 1), layout="ld4", dlayout="ld12", off={"dlogits": 1}, reason="mis_dlogits")
    _ce("rows_bwd", 3, 1028, t, bk(t, 1, False, True), row_w=ROW_W, layout="ld4", dlayout="ldodd", reason="ldd%4")
    _ce("rows_bwd", 3, 1028, t, bk(t, 4, False, True), row_w=ROW_W, layout="ld4", dlayout="inplace")
    # ---- value families, forward and backward, on the 4-wide route with ld > V and on the scalar route with an odd ld
    for vals in ("offset+90", "offset-90", "ramp_up", "ramp_down", "peaked", "flat", "masked_head", "masked_sparse", "masked_label",
                 "one_nan", "all_masked", "nan_in_masked"):
        lab = ("r", "ign", "r") if vals in ("all_masked", "nan_in_masked") else ("r", "last", "0") if vals == "masked_label" else ("r",)
        _ce("ce_fwd", 3, 2052, t, fk(t, 4), layout="ld4", vals=vals, labels=lab, trips=3)
        _ce("ce_fwd", 3, 513, t, fk(t, 1), layout="ldodd", vals=vals, labels=lab, reason="V%4", trips=3)
        _ce("ce_bwd", 3, 2052, t, bk(t, 4), layout="ld4", dlayout="ld12", vals=vals, labels=lab, trips=3)
        _ce("ce_bwd", 3, 513, t, bk(t, 1), layout="ldodd", dlayout="contig", vals=vals, labels=lab, reason="V%4", trips=3)
    # ---- labels: column 0, V - 1, the last vector, -100, out-of-range ids (ignored by the kernels' rule), an ignore index that is
    # a valid id, every row ignored
    edge = ("0", "last", "tail", "ign", "r", "V", "-1", "-7", "last")
    for V, v, reason in ((1028, 4, None), (257, 1, "V%4")):
        _ce("ce_fwd", 9, V, t, fk(t, v), labels=edge, reason=reason)
        _ce("ce_bwd", 9, V, t, bk(t, v), labels=edge, reason=reason)
        _ce("rows_bwd", 9, V, t, bk(t, v, False, True), row_w=ROW_W, labels=edge, reason=reason)
        _ce("ce_fwd", 3, V, t, fk(t, v), labels=("ign", "r", "ign"), ignore_index=3, reason=reason)
        _ce("ce_bwd", 3, V, t, bk(t, v), labels=("ign", "r", "ign"), ignore_index=3, reason=reason)
        _ce("ce_fwd", 3, V, t, fk(t, v), labels=("ign",), reason=reason)
        _ce("ce_bwd", 3, V, t, bk(t, v), labels=("ign",), reason=reason)
    # ---- soft rows: K = 1, 8, 64; ids out of order, at both ends of the row and in its last vector
    for K in (1, 8, 64):
        for V, v, layout, reason in ((1028, 4, "ld4", None), (257, 1, "contig", "V%4")):
            rows = 9 if K == 8 else 3
            _ce("soft_fwd", rows, V, t, fk(t, v), layout=layout, K=K, labels=SOFT_LABELS, reason=reason)
            _ce("soft_bwd", rows, V, t, bk(t, v, True), layout=layout, K=K, labels=SOFT_LABELS, reason=reason)
    _ce("soft_bwd", 3, 1028, t, bk(t, 4, True), layout="ld4", dlayout="inplace", K=8, labels=SOFT_LABELS)
    _ce("soft_bwd", 3, 1028, t, bk(t, 1, True), layout="ld4", dlayout="ldodd", K=8, labels=SOFT_LABELS, reason="ldd%4")
    _ce("soft_bwd", 3, 257, t, bk(t, 1, True), dlayout="inplace", K=64, labels=SOFT_LABELS, reason="V%4")

# bf16 operands 4 elements in: 8-byte but not 16-byte aligned, still the 4-wide route
_ce("ce_fwd", 3, 1028, "bf16", fk("bf16", 4), off={"logits": 4}, reason="off4")
_ce("ce_bwd", 3, 1028, "bf16", bk("bf16", 4), off={"logits": 4, "dlogits": 4}, reason="off4")
_ce("ce_bwd", 3, 1028, "bf16", bk("bf16", 4), layout="ld4", dlayout="inplace", off={"logits": 4}, reason="off4")
_ce("soft_fwd", 3, 1028, "bf16", fk("bf16", 4), K=8, labels=SOFT_LABELS, off={"logits": 4}, reason="off4")
_ce("soft_bwd", 3, 1028, "bf16", bk("bf16", 4, True), K=8, labels=SOFT_LABELS, off={"dlogits": 4}, reason="off4")
_ce("rows_bwd", 3, 1028, "bf16", bk("bf16", 4, False, True), row_w=ROW_W, off={"logits": 4, "dlogits": 4}, reason="off4")


# ---- argmax
def _am(rows, cols, dtype, kernel, layout="contig", off=0, maxcols=None, special=None, reason=None, trips=None, tag=""):
    what = special or ("gauss" if maxcols is None else "max_" + "_".join(str(c) for c in maxcols))
    parts = ["argmax", f"{rows}x{cols}", dtype, layout, what] + ([f"off{off}"] if off else []) + ([tag] if tag else [])
    return _add(dict(id="-".join(parts), entry="argmax", rows=rows, cols=cols, dtype=dtype, kernel=kernel, layout=layout,
                     off={"x": off} if off else {}, maxcols=tuple(maxcols) if maxcols else None, special=special, reason=reason,
                     trips=trips))


for t in ("bf16", "f32"):
    # narrow kernels: cols 1, 7, 255 (scalar), 4, 1024, 1028 (4-wide), each scalar-route reason
    for rows, cols, v in ((3, 1, 1), (1, 7, 1), (9, 255, 1), (3, 4, 4), (3, 1024, 4), (9, 1028, 4)):
        _am(rows, cols, t, ak(t, v), reason=None if v == 4 else "V%4", trips=-(-cols // (256 * v)))
    _am(3, 1028, t, ak(t, 4), layout="ld4")
    _am(3, 1028, t, ak(t, 1), layout="ldodd", reason="ld%4")
    _am(3, 1028, t, ak(t, 1), off=1, reason="mis_logits")
    # a unique maximum at column 0, at the last column; equal maxima: two elements of one vector, two lanes of one wave, two
    # waves (the lower index in the LATER wave's earlier trip and the other way round), two trips of one thread
    for cols, v in ((2052, 4), (513, 1)):
        T = 256 * v
        for mc in ((0,), (cols - 1,), (2 * v + 1, 2 * v + 2) if v == 4 else (5, 6), (3 * v, 7 * v), (10 * v, 70 * v), (200 * v, T + 2 * v),
                   (5 * v, T + 5 * v), (cols - 3, T + 5 * v), (T + 65 * v, 2 * T)):
            _am(3, cols, t, ak(t, v), maxcols=mc, reason=None if v == 4 else "V%4", trips=3)
        for sp in ("negzero", "all_ninf", "all_nan", "one_nan", "two_nan"):
            _am(3, cols, t, ak(t, v), special=sp, reason=None if v == 4 else "V%4", trips=3)
_am(3, 1028, "bf16", ak("bf16", 4), off=4, reason="off4")

# the wide kernel: a paired trip only; plus one thread's tail; a paired trip plus a full tail; two paired trips; two plus a tail
for rows, cols, trips in ((1, 16384, 1), (64, 16392, 2), (1, 24576, 2), (64, 32768, 2), (1, 32776, 3), (64, 16384, 1), (1, 16392, 2)):
    _am(rows, cols, "bf16", WIDE, trips=trips)
_am(3, 16384, "bf16", WIDE, layout="ld8")
# each way of falling off it, with the narrow kernel it lands on
_am(65, 16384, "bf16", ak("bf16", 4), reason="rows65")
_am(3, 16376, "bf16", ak("bf16", 4), reason="cols16376")
_am(3, 16388, "bf16", ak("bf16", 4), reason="cols16388")
_am(3, 16384, "bf16", ak("bf16", 4), layout="ld4", reason="ld+4")
_am(3, 16384, "bf16", ak("bf16", 4), off=4, reason="off4")
_am(3, 16384, "f32", ak("f32", 4), reason="f32")
# placement in the wide kernel at 32776 columns (thread t loads columns 8t.., 8192 + 8t.. as a pair, 16384 + 8t.., 24576 + 8t..
# as a pair, and thread 0 the unpaired tail 32768..): unique maxima at column 0, at the last column (the tail), in the second
# load of a pair; equal maxima in one vector, two lanes, two waves, the two loads in flight (the lower index in a HIGHER thread's
# first load against a lower thread's second load), two trips
for mc in ((0,), (32775,), (8192 + 8 * 700 + 3,), (24576 + 5,), (8 * 5 + 1, 8 * 5 + 6), (8 * 3, 8 * 40 + 7), (8 * 20 + 2, 8 * 900),
           (8 * 1000, 8192 + 8 * 3), (8192 + 8 * 1000 + 1, 16384 + 8 * 2), (8 * 77 + 4, 16384 + 8 * 77 + 4), (24576 + 8 * 1023 + 7, 32768)):
    _am(2, 32776, "bf16", WIDE, maxcols=mc, trips=3)
for sp in ("negzero", "all_ninf", "all_nan", "one_nan", "two_nan"):
    _am(2, 32776, "bf16", WIDE, special=sp, trips=3)
    _am(2, 16384, "bf16", WIDE, special=sp, trips=1, tag="paired_only")


# ---- per-sample reduction and expectile loss: one kernel each, the 1024-thread stride taken once, exactly once, twice, three times
def _sr(B, L, reward, empty=False):
    return _add(dict(id=f"sample_reduce-{B}x{L}-{reward}" + ("-empty" if empty else ""), entry="sample_reduce", B=B, L=L, dtype="f32",
                     kernel="ce_sample_reduce_k", reward=reward, empty=empty, off={}, reason=None, trips=-(-L // 1024)))


for B, L, reward, empty in ((1, 1, "gauss", False), (3, 5, "gauss", True), (3, 1024, None, False), (1, 1025, "big", False),
                            (3, 1025, "gauss", True), (3, 2049, "big", True), (1, 2049, None, False), (1, 5, "big", True)):
    _sr(B, L, reward, empty)


def _ex(n, tau, dpred):
    return _add(dict(id=f"expectile-{n}-tau{tau}" + ("-dpred" if dpred else ""), entry="expectile", n=n, tau=tau, dpred=dpred, dtype="f32",
                     kernel="expectile_loss_k", off={}, reason=None, trips=-(-n // 1024)))


for n in (1, 1023, 1024, 1025, 2049):
    for tau, dpred in ((0.1, True), (0.9, True), (0.9 if n % 2 else 0.1, False)):
        _ex(n, tau, dpred)


# ----------------------------------------------------------------------------------------------------------------- inputs
def _gen(case):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"])) & 0x7FFFFFFF)


def soft_ids(K, V):
    """K distinct ids, out of order: the row's last column, column 0, the last vector, and a cluster around the middle"""
    if K == 0:
        return []
    if K == 1:
        return [V - 2]
    c = V // 2
    cluster = [c + ((7 * i) % (K - 3)) - (K - 3) // 2 for i in range(K - 3)]          # 7 is coprime to 5 and 61: a permutation
    ids = [V - 1, 0, V - 2] + cluster
    assert len(set(ids)) == K and all(0 <= i < V for i in ids)
    return ids


def _labels(case, g):
    V, ign, ids = case["V"], case["ignore_index"], soft_ids(case["K"], case["V"])
    hard = [i for i in range(V) if i not in ids and i != ign]
    out = []
    for r in range(case["rows"]):
        tok = case["labels"][r % len(case["labels"])]
        pick = int(torch.randint(0, 1 << 30, (1,), generator=g))
        if tok == "r":
            out.append(hard[pick % len(hard)] if hard else 0)
        elif tok == "soft":
            out.append(ids[2 + pick % (len(ids) - 2)] if len(ids) > 2 else ids[0])   # the last vector or the cluster (close neighbours)
        else:
            out.append({"0": 0, "last": V - 1, "tail": max(V - 2, 0), "ign": ign, "V": V, "-1": -1, "-7": -7}[tok])
    return torch.tensor(out, dtype=torch.int64)


def ignored(labels, V, ignore_index):
    """the kernels' rule (soft_ce_fwd_k, soft_ce_bwd_k and ce_sample_reduce_k share it)"""
    return (labels == ignore_index) | (labels < 0) | (labels >= V)


def ce_values(case, labels, g):
    """the logits [rows, V] of a cross-entropy case, fp32 before the rounding to the case's dtype:
    gauss N(0, 3^2); offset+-90: the same around +-90 (expf overflows or vanishes without the shift by the maximum);
    ramp_up / ramp_down: N(0, 1) on a slope of +-12 a trip of the case's kernel — the running maximum of a thread moves on every
    trip (each rescale factor about e^-12) or never after the first; peaked: the label's logit 40 above the rest (lse - x[label]
    cancels to about 0); flat: all 1.5 (lse = 1.5 + log V); masked_head: the first 1024 columns (4-wide route: the whole first
    trip of every thread) or 256 (scalar route) -inf; masked_sparse: 30 % of the entries -inf, the label's finite; masked_label:
    the label's own logit -inf; one_nan: one NaN in one row; all_masked: the first row with an ignored label all -inf;
    nan_in_masked: that row all -inf but for one NaN"""
    rows, V, fam = case["rows"], case["V"], case["vals"]
    x = torch.randn(rows, V, generator=g) * 3.0
    valid = ~ignored(labels, V, case["ignore_index"])
    trip = 256 * vec_width(case)
    j = torch.arange(V, dtype=torch.float32)
    if fam.startswith("offset"):
        x = x + float(fam[6:])
    elif fam.startswith("ramp"):
        x = x / 3.0 + (12.0 if fam == "ramp_up" else -12.0) * (j / trip)[None, :]
    elif fam == "flat":
        x = torch.full_like(x, 1.5)
    elif fam == "masked_head":
        x[:, :trip] = -math.inf
    elif fam == "masked_sparse":
        x[torch.rand(rows, V, generator=g) < 0.3] = -math.inf
        x[:, 0] = 1.0
    for r in range(rows):
        lab = int(labels[r])
        if not valid[r]:
            continue
        if fam == "peaked":
            x[r, lab] = x[r].max() + 40.0
        elif fam == "masked_sparse":
            x[r, lab] = 0.5
        elif fam == "masked_label":
            x[r, lab] = -math.inf
    if fam == "one_nan":
        x[min(1, rows - 1), V // 3] = math.nan
    if fam in ("all_masked", "nan_in_masked"):
        r0 = int((~valid).nonzero()[0])
        x[r0] = -math.inf
        if fam == "nan_in_masked":
            x[r0, V - 2] = math.nan
    return x


def argmax_values(case, g):
    """rows of N(0, 3^2) (below 20) with 50.0 at ``maxcols``, or a special row: negzero: all below -1 but a -0.0 and, later, a
    +0.0 (equal: the first wins); all_ninf; all_nan; one_nan: a NaN after the largest finite entry, in another thread's part;
    two_nan: two NaNs, the later one in an earlier thread's later trip"""
    rows, cols, sp = case["rows"], case["cols"], case["special"]
    x = torch.randn(rows, cols, generator=g) * 3.0
    w = vec_width(case)
    T = (1024 if w == 8 else 256) * w
    if case["maxcols"]:
        for c in case["maxcols"]:
            x[:, c] = 50.0
    elif sp == "negzero":
        x = -x.abs() - 1.0
        x[:, 3 * w + 1] = -0.0
        x[:, min(cols - 1, T + 2 * w)] = 0.0
    elif sp == "all_ninf":
        x[:] = -math.inf
    elif sp == "all_nan":
        x[:] = math.nan
    elif sp == "one_nan":
        x[:, 2 * w] = 50.0
        x[0, min(cols - 1, 100 * w + 1)] = math.nan           # the other rows have none
    elif sp == "two_nan":
        x[:, 2 * w] = 50.0
        x[:, 90 * w + 1] = math.nan
        x[:, min(cols - 1, T + 3 * w)] = math.nan
    return x


def inputs(case):
    """the case's inputs on the CPU in their stored dtypes (seeded by the case's id); bf16 inputs are rounded here, so the
    reference sees what the kernel sees"""
    g = _gen(case)
    e = case["entry"]
    if e == "argmax":
        return dict(x=argmax_values(case, g).to(TORCH_DT[case["dtype"]]))
    if e == "expectile":
        n = case["n"]
        pred, target = torch.randn(n, generator=g), torch.randn(n, generator=g)
        target[::5] = pred[::5]                              # exact zeros of pred - target
        if n > 1:
            target[1] = pred[1] - 0.75                       # both signs whatever the draw
        if n > 2:
            target[2] = pred[2] + 0.75
        return dict(pred=pred, target=target, gscale=0.5)
    if e == "sample_reduce":
        B, L = case["B"], case["L"]
        labels = torch.randint(0, SAMPLE_V, (B, L), generator=g)
        kind = torch.rand(B, L, generator=g)
        labels[kind < 0.3] = -100
        labels[(kind >= 0.3) & (kind < 0.35)] = SAMPLE_V
        labels[(kind >= 0.35) & (kind < 0.4)] = -1
        if case["empty"]:
            labels[0] = -100
        out = dict(row_loss=torch.rand(B * L, generator=g) * 12.0, labels=labels.reshape(-1))
        if case["reward"] == "gauss":
            out["reward"] = torch.randn(B, generator=g)
        elif case["reward"] == "big":
            out["reward"] = torch.tensor([30.0, -30.0, 29.5][:B])
        return out
    labels = _labels(case, g)
    out = dict(logits=ce_values(case, labels, g).to(TORCH_DT[case["dtype"]]), labels=labels)
    if case["K"]:
        out["soft_ids"] = torch.tensor(soft_ids(case["K"], case["V"]), dtype=torch.int64)
    if case["gscale"] is not None:
        out["gscale"] = torch.tensor([case["gscale"]], dtype=torch.float32)
    if case["row_w"] is not None:
        rw = torch.rand(case["rows"], generator=g) + 0.25
        for r in range(case["rows"]):
            tok = case["row_w"][r % len(case["row_w"])]
            if tok == "zero" and case["rows"] > 1:
                rw[r] = 0.0
            elif tok == "neg" or (tok == "zero" and case["rows"] == 1):
                rw[r] = -0.75
        out["row_w"] = rw
    return out
