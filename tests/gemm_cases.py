"""The GEMM route cases: one deterministic table of descriptors that together run every row of dxa_gemm's launcher table in
every mode gemm_plan can put it in, with the route each descriptor must get.  Used on the CPU by tests/test_gemm_cases.py
(the table is complete and its routes are the planner's) and on the MI355X by tests/test_gemm_routes_gpu.py (each case is run
against an exact reference inside guarded buffers).  Nothing here needs a GPU.

A case is ``dict(id, kernels, fields)``:
  * ``fields`` is the descriptor in the form tests/test_gemm_plan.py::desc produces, except that an operand is SYMBOLIC: the
    field of a buffer that is present holds its byte offset from a 256-byte aligned base (0: aligned), a buffer that is absent
    has no field.  ``with_pointers`` turns the offsets into addresses: fake ones for the planner alone, real ones on the GPU.
  * ``kernels`` is the launcher row of each step, written down by whoever added the case: the target it was chosen for.
  * the whole route (``route_of``: the mode fields of every step) is pinned by tests/golden/gemm_case_routes.json, which
    ``python -m tests.gemm_cases --record`` writes from dxa_gemm_plan after a deliberate change of the table or of a route.

Shapes were chosen by asking dxa_gemm_plan (never by repeating its arithmetic here): the smallest descriptor found that
reaches the target, M, N <= 512 and K <= 4608 wherever the route allows, so that sums of small integers stay exact in fp32.
Leading dimensions exceed the extents (rounded up to 8 elements, plus 8) unless a case is about an odd one.

Operands are small integers (|x| <= 3), bias / residual within +-40, a C that is accumulated into within +-100: every fp32
sum is exact, so the fp64 reference rounded ONCE to the output type is what a correct kernel stores, bit for bit.  bf16 outputs
default to alpha = 33/32, which leaves the exact sums with fraction bits the single rounding has to remove."""
import json
import os
import sys

import torch

NT, NN, TN = 0, 1, 2
F32, BF16 = 0, 1
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_QUICK_GELU, ACT_SILU, ACT_RELU, ACT_SIGMOID = range(7)
DTYPES = {"bb": (BF16, BF16), "bf": (BF16, F32), "ff": (F32, F32)}
LAYOUTS = {"nt": NT, "nn": NN, "tn": TN}
BUFFERS = ("A", "B", "C", "bias", "residual", "aux_out", "mulgrad", "mirror", "sumsq", "A2", "B2")
# fake operand addresses for the planner: 256-byte aligned, far apart
FAKE = {n: (0x10 + i) << 36 for i, n in enumerate(BUFFERS)}
STEP_MODE_FIELDS = ("kernel", "K", "K2", "seg2", "accumulate", "bias", "residual", "tm", "tn", "full", "tail_r", "split_s", "vecA", "vecB",
                    "vecC", "vecR", "vecG", "vecBias", "ksplit", "kper", "mirror", "sumsq")
ROUTES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_case_routes.json")
ALPHA_BF16 = 33.0 / 32.0
ALPHA_ACT = 1.0 / 32.0      # activation cases: integer sums scaled into the range where the activations bend


def up8(n):
    return -(-n // 8) * 8


def desc(layout, dt, M, N, K, **kw):
    """a product with padded leading dimensions; ``kw`` overrides and adds buffers (name=byte offset)"""
    ind, outd = DTYPES[dt]
    d = dict(layout=layout, in_dtype=ind, out_dtype=outd, act=ACT_NONE, M=M, N=N, K=K, A=0, B=0, C=0,
             lda=up8(M if layout == TN else K) + 8, ldb=up8(K if layout == NT else N) + 8, ldc=up8(N) + 8,
             ldr=up8(N) + 16, ldg=up8(N) + 24, alpha=ALPHA_BF16 if outd == BF16 else 1.0, nb=(1, 1, 1))
    d.update(kw)
    return d


def with_pointers(fields, base=None):
    """the descriptor fields with addresses in place of offsets: ``base[name]`` + offset (default: the fake addresses)"""
    base = FAKE if base is None else base
    out = dict(fields)
    for n in BUFFERS:
        if n in fields:
            out[n] = base[n] + fields[n]
    return out


def make_desc(L, fields):
    d = L.GemmDesc()
    for k, v in fields.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(d, k)[i] = x
        else:
            setattr(d, k, v)
    return d


def route_of(L, fields):
    """what dxa_gemm_plan answers for a descriptor with addresses, as the table states routes"""
    import ctypes as C
    info = L.GemmPlanInfo()
    rc = L.lib.dxa_gemm_plan(make_desc(L, fields), C.byref(info))
    if rc != 0:
        return {"rc": rc, "error": L.last_error()}
    steps = []
    for i in range(info.nsteps):
        s = info.step[i]
        steps.append({f: (s.kernel.decode() if f == "kernel" else getattr(s, f)) for f in STEP_MODE_FIELDS})
    return {"rc": 0, "nsteps": info.nsteps, "mirror_pass": info.mirror_pass, "sumsq_pass": info.sumsq_pass, "steps": steps}


def kernel_names(L):
    names = []
    while L.lib.dxa_gemm_kernel_name(len(names)) is not None:
        names.append(L.lib.dxa_gemm_kernel_name(len(names)).decode())
    return names


def desc_from_tensors(layout, a, b, out, *, bias=None, residual=None, aux_out=None, mulgrad=None, accumulate=False, act=ACT_NONE,
                      mirror=None, sumsq=None, a2=None, b2=None, epi_f32=False):
    """the descriptor kernels.mm_nt / mm_nn / mm_tn build for 2-D row-major tensors (real addresses): for a GPU test to ask
    dxa_gemm_plan which kernel its shapes reach"""
    code = {torch.float32: F32, torch.bfloat16: BF16}
    lay = LAYOUTS[layout] if isinstance(layout, str) else layout
    M = a.shape[1] if lay == TN else a.shape[0]
    K = a.shape[0] if lay == TN else a.shape[1]
    N = b.shape[0] if lay == NT else b.shape[1]
    d = dict(layout=lay, in_dtype=code[a.dtype], out_dtype=code[out.dtype], act=act, M=M, N=N, K=K, A=a.data_ptr(), lda=a.stride(0),
             B=b.data_ptr(), ldb=b.stride(0), C=out.data_ptr(), ldc=out.stride(0), alpha=1.0, accumulate=int(accumulate), nb=(1, 1, 1),
             epi_f32=int(epi_f32))
    for n, t in (("bias", bias), ("residual", residual), ("aux_out", aux_out), ("mulgrad", mulgrad), ("mirror", mirror), ("sumsq", sumsq)):
        if t is not None:
            d[n] = t.data_ptr()
    if residual is not None:
        d["ldr"] = residual.stride(0)
    if mulgrad is not None:
        d["ldg"] = mulgrad.stride(0)
    if a2 is not None:
        d.update(A2=a2.data_ptr(), B2=b2.data_ptr(), K2=a2.shape[0])
    return d


def tensor_route(L, layout, a, b, out_dtype, **kw):
    """the route dxa_gemm_plan gives kernels.mm_nt / mm_nn / mm_tn(a, b, **kw) with a fresh output of ``out_dtype``"""
    lay = LAYOUTS[layout]
    M, N = (a.shape[1] if lay == TN else a.shape[0]), (b.shape[0] if lay == NT else b.shape[1])
    r = route_of(L, desc_from_tensors(lay, a, b, torch.empty((M, N), dtype=out_dtype, device=a.device), **kw))
    assert r["rc"] == 0, r
    return r


# ------------------------------------------------------------------------------------------------ the table
def family(kernel):
    return kernel.split("<")[0].replace("gemv_nn_stage1", "gemv").replace("gemv_nn_stage2", "gemv")


# What each family's kernels can be asked to do (gemm_plan's modes), as data: tests/test_gemm_cases.py requires every one of
# them to be reached by a case.  ``modes_of`` below says how a mode is read off a case.
REQUIRED_MODES = {
    "generic": {"tile64", "tile128", "batched", "broadcast_stride", "sR", "sG", "vecA=0", "vecB=0", "vecC=0", "vecR=0", "vecG=0",
                "vecBias=0", "bias+residual", "accumulate", "act", "mulgrad", "aux_out", "alpha", "mirror_pass", "sumsq_pass",
                "seg2_step", "ktail_step"},
    "t128": {"split_s=1", "split_s=2", "split_s=3", "split_s=4", "vecC=0", "vecR=0", "vecG=0", "vecBias=0", "bias+residual",
             "accumulate", "act", "mulgrad", "aux_out", "alpha", "mirror_pass", "sumsq_pass"},
    "gemv": {"ksplit>1", "kper=512", "column_blocks>1", "alpha"},
    "skinny_f32": {"split_s=1", "split_s=2", "split_s=8", "vecC=0", "vecR=0", "vecG=0", "vecBias=0", "bias+residual", "accumulate",
                   "act", "mulgrad", "aux_out", "alpha"},
    "skinny_bf16": {"split_s=1", "split_s=2", "split_s=8", "vecC=0", "vecR=0", "vecG=0", "vecBias=0", "bias+residual", "accumulate",
                    "act", "mulgrad", "aux_out", "alpha"},
    "ring": {"unsplit", "tail_only", "full+tail", "vecC=0", "vecR=0", "vecG=0", "vecBias=0", "bias+residual", "accumulate", "act",
             "mulgrad", "aux_out", "alpha", "mirror_pass", "sumsq_pass", "ktail_step", "tm%4"},
    "pp": {"unsplit", "tail_only", "full+tail", "lean", "full", "vecC=0", "vecR=0", "vecG=0", "vecBias=0", "bias+residual",
           "accumulate", "act", "mulgrad", "aux_out", "alpha", "mirror_epilogue", "sumsq_epilogue", "mirror_pass", "sumsq_pass",
           "seg2_fused", "ktail_head", "swiglu", "swiglu+aux", "tm%4"},
    "pp3": {"unsplit", "tail_only", "full+tail", "lean", "full", "vecC=0", "vecR=0", "vecG=0", "vecBias=0", "bias+residual",
            "accumulate", "act", "mulgrad", "aux_out", "alpha", "mirror_pass", "sumsq_pass", "ktail_head", "swiglu", "swiglu+aux", "tm%4"},
}
SPLIT_FAMILIES = ("t128", "skinny_f32", "skinny_bf16", "ring", "pp", "pp3")


def modes_of(fields, route, i):
    """the modes step ``i`` of a case's route runs its kernel in"""
    s = route["steps"][i]
    fam = family(s["kernel"])
    last = i == route["nsteps"] - 1
    m = set()
    if fam == "generic":
        m.add("tile128" if s["kernel"].endswith(",128>") else "tile64")
        nb = fields["nb"]
        if nb != (1, 1, 1):
            m.add("batched")
            if any(n > 1 and fields[k][j] == 0 for k in ("sA", "sB") for j, n in enumerate(nb)):
                m.add("broadcast_stride")
            if "residual" in fields and any(fields["sR"]):
                m.add("sR")
            if "mulgrad" in fields and any(fields["sG"]):
                m.add("sG")
        if i == 1 and s["seg2"]:
            m.add("seg2_step")
    if fam == "gemv":
        if s["ksplit"] > 1:
            m.add("ksplit>1")
        if s["kper"] == 512 and s["ksplit"] * 512 >= fields["K"] > 64 * 512:
            m.add("kper=512")
        if fields["N"] > 2048:
            m.add("column_blocks>1")
        if fields["alpha"] not in (1.0, ALPHA_BF16):
            m.add("alpha")
        return m
    if fam in ("generic", "ring") and i == 1 and not s["seg2"]:
        m.add("ktail_step")
    if fam in ("t128", "skinny_f32", "skinny_bf16"):
        m.add("split_s=%d" % s["split_s"])
    if fam in ("ring", "pp", "pp3"):
        m.add("unsplit" if s["tail_r"] == 0 else "tail_only" if s["full"] == 0 else "full+tail")
        if s["tm"] % 4:
            m.add("tm%4")
    if fam in ("pp", "pp3"):
        if "swiglu" in s["kernel"]:
            m.add("swiglu+aux" if "aux_out" in fields else "swiglu")
        else:
            m.add("lean" if "lean" in s["kernel"] else "full")
        if s["K2"] > 0:
            m.add("seg2_fused")
        if route["nsteps"] == 2 and i == 0 and not route["steps"][1]["seg2"]:
            m.add("ktail_head")
        if s["mirror"]:
            m.add("mirror_epilogue")
        if s["sumsq"]:
            m.add("sumsq_epilogue")
    if last and route["mirror_pass"]:
        m.add("mirror_pass")
    if last and route["sumsq_pass"]:
        m.add("sumsq_pass")
    if not s["vecA"]:
        m.add("vecA=0")
    if not s["vecB"]:
        m.add("vecB=0")
    if not s["vecC"]:
        m.add("vecC=0")
    if s["residual"] and not s["vecR"]:
        m.add("vecR=0")
    if "mulgrad" in fields and not s["vecG"]:
        m.add("vecG=0")
    if s["bias"] and not s["vecBias"]:
        m.add("vecBias=0")
    if s["bias"] and s["residual"] and fields["ldr"] != fields["ldc"]:
        m.add("bias+residual")
    if fields.get("accumulate") and i == 0:
        m.add("accumulate")
    if fields["act"] != ACT_NONE and "mulgrad" not in fields:
        m.add("act")
    if "mulgrad" in fields and fields["ldg"] != fields["ldc"]:
        m.add("mulgrad")
    if "aux_out" in fields and not fields.get("fuse"):
        m.add("aux_out")
    if fields["alpha"] in (0.5, 2.0):
        m.add("alpha")
    return m


def is_ragged(fields, route):
    """M and N are no multiples of the step's tile and C's rows are longer than N"""
    s = route["steps"][0]
    if family(s["kernel"]) == "gemv":
        return fields["ldc"] > fields["N"] and fields["N"] % 2048 != 0
    if family(s["kernel"]).startswith("skinny"):
        return fields["M"] % 16 != 0 and fields["N"] % 16 != 0 and fields["ldc"] > fields["N"]
    n_cols = fields["N"] // 2 if fields.get("fuse") else fields["N"]
    return fields["M"] % 64 != 0 and fields["N"] % 64 != 0 and fields["ldc"] > n_cols


def _br(**kw):
    return dict(bias=0, residual=0, **kw)


def _batched(lay, dt, M, N, K, nb, **kw):
    d = desc(lay, dt, M, N, K, nb=nb, **kw)
    ra, rb = (K if lay == TN else M), (N if lay == NT else K)
    n1, n2 = nb[1], nb[2]
    d.setdefault("sA", (n1 * n2 * ra * d["lda"], n2 * ra * d["lda"], ra * d["lda"]))
    d.setdefault("sB", (n1 * n2 * rb * d["ldb"], n2 * rb * d["ldb"], rb * d["ldb"]))
    d.setdefault("sC", (n1 * n2 * M * d["ldc"], n2 * M * d["ldc"], M * d["ldc"]))
    d.setdefault("sR", (n1 * n2 * M * d["ldr"], n2 * M * d["ldr"], M * d["ldr"]))
    d.setdefault("sG", (n1 * n2 * M * d["ldg"], n2 * M * d["ldg"], M * d["ldg"]))
    return d


def cases():
    """[dict(id, kernels, fields)], deterministic"""
    out = []

    def add(cid, kernels, fields):
        if isinstance(kernels, str):
            kernels = (kernels,)
        out.append(dict(id=cid, kernels=tuple(kernels), fields=fields))

    io_name = {"bb": "bf16,bf16", "bf": "bf16,f32", "ff": "f32,f32"}
    ty_name = {"bb": "bf16,bf16", "bf": "f32,bf16", "ef": "f32,f32"}          # <output, epilogue operands>
    lay_name = {NT: "nt", NN: "nn", TN: "tn"}
    es_of = {"bb": 2, "bf": 2, "ff": 4}

    def ty(t, **kw):
        """dtype key and descriptor extras of a 256-column-tile kernel's TY"""
        return ("bf", dict(epi_f32=1, **kw)) if t == "ef" else (t, kw)

    # ---- the generic kernel: every <in, out>, layout and tile size.  64-row tiles: a product too small or too odd for any fast
    #      path; 128-row tiles: 192 tiles, reached cheaply by 48 batches of 200 x 200 x 40
    for dt in ("bb", "bf", "ff"):
        for lay in (NT, NN, TN):
            k64, k128 = (f"generic<{io_name[dt]},{lay_name[lay]},{t}>" for t in (64, 128))
            tag = f"generic/{dt}/{lay_name[lay]}"
            add(f"{tag}/64/ragged", k64, desc(lay, dt, 130, 70, 40))
            add(f"{tag}/64/bias_res", k64, desc(lay, dt, 130, 70, 40, **_br()))
            add(f"{tag}/64/acc", k64, desc(lay, dt, 130, 70, 40, accumulate=1))
            add(f"{tag}/128/ragged", k128, _batched(lay, dt, 200, 200, 40, (48, 1, 1)))
            add(f"{tag}/128/bias_res", k128, _batched(lay, dt, 200, 200, 40, (48, 1, 1), **_br()))
            add(f"{tag}/128/acc", k128, _batched(lay, dt, 200, 200, 40, (6, 4, 2), accumulate=1))
    # each vector flag off on its own, on both tile sizes: an operand one element off 16 bytes, or an odd leading dimension
    for dt in ("bb", "ff"):
        es = es_of[dt]
        for t, mk in ((64, lambda **kw: desc(NT, dt, 130, 70, 40, **kw)), (128, lambda **kw: _batched(NT, dt, 200, 200, 40, (48, 1, 1), **kw))):
            k = f"generic<{io_name[dt]},nt,{t}>"
            tag = f"generic/{dt}/nt/{t}"
            add(f"{tag}/A+1", k, mk(A=es))
            add(f"{tag}/lda_odd", k, mk(lda=49))
            add(f"{tag}/B+1", k, mk(B=es))
            add(f"{tag}/ldb_odd", k, mk(ldb=51))
            add(f"{tag}/C+1", k, mk(C=es, **_br()))
            add(f"{tag}/ldc_odd", k, mk(ldc=up8(200 if t == 128 else 70) + 9, accumulate=1))
            add(f"{tag}/R+1", k, mk(bias=0, residual=es))
            add(f"{tag}/ldr_odd", k, mk(bias=0, residual=0, ldr=up8(200 if t == 128 else 70) + 11))
            add(f"{tag}/G+1", k, mk(mulgrad=es, act=ACT_RELU))
            add(f"{tag}/ldg_odd", k, mk(mulgrad=0, act=ACT_RELU, ldg=up8(200 if t == 128 else 70) + 13))
            add(f"{tag}/bias+1", k, mk(bias=es, residual=0))
            add(f"{tag}/aux+1", k, mk(bias=0, aux_out=es))
    # k-strided operands off their 4-element vector path
    for lay in (NN, TN):
        k = f"generic<bf16,bf16,{lay_name[lay]},64>"
        add(f"generic/bb/{lay_name[lay]}/64/B+1", k, desc(lay, "bb", 130, 70, 40, B=2))
        add(f"generic/bb/{lay_name[lay]}/64/ldb_odd", k, desc(lay, "bb", 130, 70, 40, ldb=81))
    add("generic/bb/tn/64/A+1", "generic<bf16,bf16,tn,64>", desc(TN, "bb", 130, 70, 40, A=2))
    add("generic/bb/tn/64/lda_odd", "generic<bf16,bf16,tn,64>", desc(TN, "bb", 130, 70, 40, lda=145))
    # batched: a broadcast (zero) stride on B and on the residual, sR / sG of their own, alpha
    for dt in ("bb", "ff"):
        k = f"generic<{io_name[dt]},nt,64>"
        g = _batched(NT, dt, 70, 70, 1000, (2, 2, 3), alpha=0.5)
        g["sB"] = (g["sB"][1], g["sB"][2], 0)
        add(f"generic/{dt}/nt/64/gqa_alpha0.5", k, g)
        r = dict(g, alpha=2.0, bias=0, residual=0)
        r["sR"] = (0, 70 * r["ldr"], 0)
        add(f"generic/{dt}/nt/64/gqa_sR_alpha2", k, r)
        m = dict(g, alpha=1.0, mulgrad=0, act=ACT_RELU)
        m["sG"] = (3 * 70 * m["ldg"], 0, 70 * m["ldg"])
        add(f"generic/{dt}/nt/64/gqa_sG", k, m)

    # ---- few-row NT on 128 x 128 tiles: 33 tiles, K cut in 1 .. 4
    for dt in ("bb", "bf"):
        k = f"t128<{'bf16' if dt == 'bb' else 'f32'}>"
        tag = f"t128/{dt}"
        for sp, Kd in ((1, 512), (2, 1024), (3, 1536), (4, 2048)):
            add(f"{tag}/split{sp}", k, desc(NT, dt, 300, 1400, Kd))
        add(f"{tag}/bias_res", k, desc(NT, dt, 300, 1400, 64, **_br()))
        add(f"{tag}/split3/bias_res", k, desc(NT, dt, 300, 1400, 1536, **_br()))
        add(f"{tag}/acc", k, desc(NT, dt, 300, 1400, 192, accumulate=1))
        add(f"{tag}/split2/acc", k, desc(NT, dt, 300, 1400, 1024, accumulate=1, alpha=2.0))

    # ---- few-row NN: every stage-1 row count with both stage-2 outputs; column blocks; the k-per-slice cap
    for dt in ("bb", "bf"):
        k2 = f"gemv_nn_stage2<{'bf16' if dt == 'bb' else 'f32'}>"
        for M, mh in ((1, 1), (2, 2), (3, 4), (7, 8)):
            add(f"gemv/{dt}/{M}/ragged", (f"gemv_nn_stage1<{mh}>", k2), desc(NN, dt, M, 72, 100))
        add(f"gemv/{dt}/2/blocks", ("gemv_nn_stage1<2>", k2), desc(NN, dt, 2, 2120, 64))
        add(f"gemv/{dt}/8/deep", ("gemv_nn_stage1<8>", k2), desc(NN, dt, 8, 264, 4608, alpha=2.0))
    add("gemv/bb/1/kper_cap", ("gemv_nn_stage1<1>", "gemv_nn_stage2<bf16>"), desc(NN, "bb", 1, 64, 40000, alpha=1.0))

    # ---- skinny NT (M <= 64): every 16-row block count, K cut in 1, 2 and 8
    for dt in ("ff", "bb", "bf"):
        for mb, M in ((1, 5), (2, 17), (3, 40), (4, 63)):
            k = f"skinny_f32<{mb}>" if dt == "ff" else f"skinny_bf16<{mb},{'bf16' if dt == 'bb' else 'f32'}>"
            tag = f"skinny/{dt}/{mb}"
            add(f"{tag}/ragged", k, desc(NT, dt, M, 100, 64))
            add(f"{tag}/split2", k, desc(NT, dt, M, 500, 1024))
            add(f"{tag}/split8/bias_res", k, desc(NT, dt, M, 500, 4096, **_br()))
            add(f"{tag}/bias_res", k, desc(NT, dt, M, 100, 192, **_br()))
            add(f"{tag}/acc", k, desc(NT, dt, M, 100, 128, accumulate=1))
            add(f"{tag}/split2/acc", k, desc(NT, dt, M, 100, 1024, accumulate=1, alpha=0.5))

    # ---- the 256-column-tile kernels (bf16 operands): ring (K % 64 == 32), ping-pong on 256 rows (pp) and on 192 rows (pp3).
    #      500 rows take 256-row tiles, 300 rows 192-row tiles; N = 264 keeps the lean epilogue, N = 270 needs the full one.
    #      A single round of tiles is cut along K from 2048 on (tail_only); K >= 1024 with K % 64 != 0 and M, N >= 256 is cut in
    #      two steps first, so the deep ring cases keep N below 256 or carry an operand the two-step cut refuses
    for t in ("bb", "bf", "ef"):
        dt, x = ty(t)
        for rows, M in (("256", 500), ("192", 300)):
            k = f"ring<{ty_name[t]},{rows}>"
            tag = f"ring/{t}/{rows}"
            add(f"{tag}/ragged", k, desc(NT, dt, M, 270, 96, **x))
            add(f"{tag}/bias_res", k, desc(NT, dt, M, 270, 160, **_br(**x)))
            add(f"{tag}/acc", k, desc(NT, dt, M, 264, 32, accumulate=1, **x))
            add(f"{tag}/tail", k, desc(NT, dt, M, 200, 2080, **x))
            add(f"{tag}/tail/bias_res", k, desc(NT, dt, M, 200, 2080, **_br(**x)))
            add(f"{tag}/tail/acc", k, desc(NT, dt, M, 248, 4128, accumulate=1, alpha=2.0, **x))
        for lean, N in (("lean", 264), ("full", 270)):
            for fam, M in (("pp", 500), ("pp3", 300)):
                k = f"pp<{ty_name[t]},{lean},nt>" if fam == "pp" else f"pp3<{ty_name[t]},{lean}>"
                tag = f"{fam}/{t}/{lean}"
                add(f"{tag}/ragged", k, desc(NT, dt, M, N, 128, **x))
                add(f"{tag}/k64", k, desc(NT, dt, M, N, 64, **x))
                add(f"{tag}/bias_res", k, desc(NT, dt, M, N, 192, **_br(**x)))
                add(f"{tag}/acc", k, desc(NT, dt, M, N, 320, accumulate=1, **x))
                add(f"{tag}/tail", k, desc(NT, dt, M, N, 2048, **x))
                add(f"{tag}/tail/bias_res", k, desc(NT, dt, M, N, 2112, **_br(**x)))
                add(f"{tag}/tail/acc", k, desc(NT, dt, M, N, 4608, accumulate=1, alpha=0.5, **x))
    # NN (dX) and TN (dW) on the ping-pong kernel; TN takes any K
    for k, lay, dt, N in (("pp<bf16,bf16,lean,nn>", NN, "bb", 264), ("pp<bf16,bf16,full,nn>", NN, "bb", 270), ("pp<f32,bf16,lean,nn>", NN, "bf", 264),
                          ("pp<bf16,bf16,lean,tn>", TN, "bb", 264), ("pp<f32,bf16,lean,tn>", TN, "bf", 264)):
        tag = k[:-1].replace("<", "/")
        odd = 100 if lay == TN else 128
        add(f"{tag}/ragged", k, desc(lay, dt, 500, N, odd))
        add(f"{tag}/bias_res", k, desc(lay, dt, 500, N, 192, **_br()))
        add(f"{tag}/acc", k, desc(lay, dt, 500, N, 64 if lay == NN else 70, accumulate=1))
        add(f"{tag}/tail", k, desc(lay, dt, 500, N, 2048 if lay == NN else 2075))
        add(f"{tag}/tail/bias_res", k, desc(lay, dt, 500, N, 2112, **_br(alpha=2.0)))
        add(f"{tag}/tail/acc", k, desc(lay, dt, 500, N, 4608 if lay == NN else 4600, accumulate=1))
    # full rounds of 256 tiles and then a cut tail: the three cases with more than 256 tiles
    add("pp/bb/lean/full+tail", "pp<bf16,bf16,lean,nt>", desc(NT, "bb", 1160, 13064, 2048, **_br()))
    add("ring/bf/256/full+tail", "ring<f32,bf16,256>", desc(NT, "bf", 1160, 13064, 2080, accumulate=1, mirror=0, sumsq=0))
    add("pp3/bf/lean/full+tail", "pp3<f32,bf16,lean>", desc(NT, "bf", 1100, 10760, 2048, accumulate=1))

    # ---- the epilogue implementations: generic, t128, skinny f32, skinny bf16, and the full epilogue of pp, pp3 and ring.
    #      Each activation once per implementation (with the pre-activation copy), the activation gradient with its own
    #      leading dimension, and each epilogue vector flag off where the route survives it
    impls = (("generic", "generic<bf16,bf16,nt,64>", lambda **kw: desc(NT, "bb", 130, 70, 40, **kw), 2),
             ("generic_f32", "generic<f32,f32,nn,64>", lambda **kw: desc(NN, "ff", 130, 70, 40, **kw), 4),
             ("t128", "t128<bf16>", lambda **kw: desc(NT, "bb", 300, 1400, 128, **kw), 2),
             ("t128_split", "t128<f32>", lambda **kw: desc(NT, "bf", 300, 1400, 1024, **kw), 2),
             ("skinny_f32", "skinny_f32<2>", lambda **kw: desc(NT, "ff", 17, 100, 128, **kw), 4),
             ("skinny_f32_split", "skinny_f32<3>", lambda **kw: desc(NT, "ff", 40, 100, 1024, **kw), 4),
             ("skinny_bf16", "skinny_bf16<2,bf16>", lambda **kw: desc(NT, "bb", 17, 100, 128, **kw), 2),
             ("skinny_bf16_split", "skinny_bf16<3,f32>", lambda **kw: desc(NT, "bf", 40, 100, 1024, **kw), 2),
             ("pp", "pp<bf16,bf16,full,nt>", lambda **kw: desc(NT, "bb", 500, 264, 128, **kw), 2),
             ("pp_tail", "pp<f32,bf16,full,nt>", lambda **kw: desc(NT, "bf", 500, 264, 2048, **kw), 2),
             ("pp_nn", "pp<bf16,bf16,full,nn>", lambda **kw: desc(NN, "bb", 500, 264, 128, **kw), 2),
             ("pp3", "pp3<bf16,bf16,full>", lambda **kw: desc(NT, "bb", 300, 264, 128, **kw), 2),
             ("pp3_tail", "pp3<f32,bf16,full>", lambda **kw: desc(NT, "bf", 300, 264, 2048, **kw), 2),
             ("ring", "ring<bf16,bf16,256>", lambda **kw: desc(NT, "bb", 500, 264, 96, **kw), 2),
             ("ring_tail", "ring<f32,bf16,192>", lambda **kw: desc(NT, "bf", 300, 200, 2080, **kw), 2),
             ("pp_f32epi", "pp<f32,f32,full,nt>", lambda **kw: desc(NT, "bf", 500, 264, 128, epi_f32=1, **kw), 4),
             ("ring_f32epi", "ring<f32,f32,256>", lambda **kw: desc(NT, "bf", 500, 264, 96, epi_f32=1, **kw), 4))
    for name, k, mk, ees in impls:
        main = name in ("generic", "generic_f32", "t128", "skinny_f32", "skinny_bf16", "pp", "pp3", "ring")
        for act in range(1, 7) if main else (ACT_GELU_TANH,):
            add(f"epi/{name}/act{act}", k, mk(act=act, bias=0, aux_out=0, alpha=ALPHA_ACT))
        add(f"epi/{name}/aux", k, mk(bias=0, residual=0, aux_out=0))
        add(f"epi/{name}/mulgrad_relu", k, mk(mulgrad=0, act=ACT_RELU))
        add(f"epi/{name}/mulgrad_silu", k, mk(mulgrad=0, act=ACT_SILU, alpha=ALPHA_ACT))
        if name.startswith("generic"):
            continue
        ldc = mk()["ldc"]
        add(f"epi/{name}/C+1", k, mk(C=2 if mk()["out_dtype"] == BF16 else 4, **_br()))
        add(f"epi/{name}/ldc_odd", k, mk(ldc=ldc + 1, accumulate=1))
        add(f"epi/{name}/R+1", k, mk(bias=0, residual=ees))
        add(f"epi/{name}/ldr_odd", k, mk(bias=0, residual=0, ldr=ldc + 3))
        add(f"epi/{name}/G+1", k, mk(mulgrad=ees, act=ACT_RELU))
        add(f"epi/{name}/ldg_odd", k, mk(mulgrad=0, act=ACT_RELU, ldg=ldc + 5))
        add(f"epi/{name}/bias+1", k, mk(bias=ees, residual=0, aux_out=0))

    # ---- mirror (bf16 copy of an fp32 C) and sumsq: written by the lean epilogue, or by the separate passes
    add("norm/pp_tn/epilogue", "pp<f32,bf16,lean,tn>", desc(TN, "bf", 500, 264, 100, accumulate=1, mirror=0, sumsq=0))
    add("norm/pp_tn/epilogue/tail", "pp<f32,bf16,lean,tn>", desc(TN, "bf", 500, 264, 2075, mirror=0, sumsq=0))
    add("norm/pp_tn_bf16/epilogue", "pp<bf16,bf16,lean,tn>", desc(TN, "bb", 500, 264, 100, sumsq=0))
    add("norm/pp_nt/epilogue", "pp<f32,bf16,lean,nt>", desc(NT, "bf", 500, 264, 128, accumulate=1, mirror=0, sumsq=0))
    add("norm/pp_nn/epilogue", "pp<f32,bf16,lean,nn>", desc(NN, "bf", 500, 264, 128, mirror=0, sumsq=0))
    add("norm/pp3/lean_has_no_epilogue", "pp3<f32,bf16,lean>", desc(NT, "bf", 300, 264, 128, accumulate=1, mirror=0, sumsq=0))
    add("norm/pp_full/passes", "pp<f32,bf16,full,nt>", desc(NT, "bf", 500, 270, 128, accumulate=1, mirror=0, sumsq=0))
    add("norm/generic/passes", "generic<bf16,f32,tn,64>", desc(TN, "bf", 130, 70, 40, accumulate=1, mirror=0, sumsq=0))
    add("norm/generic_f32/passes", "generic<f32,f32,tn,64>", desc(TN, "ff", 300, 270, 40, mirror=0, sumsq=0))
    add("norm/generic_bf16/sumsq_pass", "generic<bf16,bf16,tn,64>", desc(TN, "bb", 130, 70, 40, sumsq=0))
    add("norm/t128/passes", "t128<f32>", desc(NT, "bf", 300, 1400, 1024, mirror=0, sumsq=0))
    add("norm/ring/passes", "ring<f32,bf16,192>", desc(NT, "bf", 300, 270, 2080, mirror=0, sumsq=0))

    # ---- a second (A2, B2) segment of a TN product: contracted by the ping-pong kernel, or two steps
    for dt in ("bb", "bf"):
        k = f"pp<{ty_name[dt]},lean,tn>"
        add(f"seg2/{dt}/fused", k, desc(TN, dt, 500, 264, 100, A2=0, B2=0, K2=70))
        add(f"seg2/{dt}/fused/acc_tail", k, desc(TN, dt, 500, 264, 1100, A2=0, B2=0, K2=1000, accumulate=1))
        add(f"seg2/{dt}/fused/bias_res", k, desc(TN, dt, 500, 264, 100, A2=0, B2=0, K2=200, **_br()))
        g = f"generic<{io_name[dt]},tn,64>"
        add(f"seg2/{dt}/two_steps", (g, g), desc(TN, dt, 130, 70, 40, A2=0, B2=0, K2=24))
        add(f"seg2/{dt}/two_steps/bias_res", (g, g), desc(TN, dt, 130, 70, 40, A2=0, B2=0, K2=24, **_br()))
        add(f"seg2/{dt}/two_steps/A2+8", (k, g), desc(TN, dt, 500, 264, 100, A2=8, B2=0, K2=70, accumulate=1))
    add("seg2/ff/two_steps", ("generic<f32,f32,tn,64>",) * 2, desc(TN, "ff", 130, 70, 40, A2=0, B2=0, K2=24, accumulate=1))
    add("seg2/bf/two_steps/norm", ("generic<bf16,f32,tn,64>",) * 2, desc(TN, "bf", 130, 70, 40, A2=0, B2=0, K2=24, mirror=0, sumsq=0))

    # ---- K % 64 != 0 from 1024 on, M, N >= 256: the MFMA-deep part, then the tail accumulated by the generic kernel.  A bf16 C
    #      is rounded after each step (documented at the cut in gemm_plan): the reference rounds the partial result too
    for dt in ("bb", "bf"):
        add(f"ktail/{dt}/nt", (f"pp<{ty_name[dt]},lean,nt>", f"generic<{io_name[dt]},nt,64>"), desc(NT, dt, 256, 264, 1048, **_br()))
        add(f"ktail/{dt}/nt/acc", (f"pp3<{ty_name[dt]},full>", f"ring<{ty_name[dt]},192>"), desc(NT, dt, 300, 270, 1056, accumulate=1))
        add(f"ktail/{dt}/nn", (f"pp<{ty_name[dt]},lean,nn>", f"generic<{io_name[dt]},nn,64>"), desc(NN, dt, 500, 264, 1030))
        add(f"ktail/{dt}/nt/tail", (f"pp<{ty_name[dt]},lean,nt>", f"generic<{io_name[dt]},nt,64>"), desc(NT, dt, 500, 264, 2070, **_br()))

    # ---- the gated-MLP epilogue on both ping-pong kernels, with and without the pre-activations
    for fam, k, M in (("pp", "pp<bf16,bf16,swiglu,nt>", 500), ("pp3", "pp3<bf16,bf16,swiglu>", 300)):
        for Kd, t in ((128, ""), (2048, "/tail")):
            f = desc(NT, "bb", M, 528, Kd, fuse=1, ldc=272, ld_aux=536, alpha=1.0)
            add(f"swiglu/{fam}{t}", k, f)
            add(f"swiglu/{fam}{t}/aux", k, dict(f, aux_out=0))
    return out


# ------------------------------------------------------------------------------------------------ routes on file
def load_routes():
    with open(ROUTES) as f:
        return json.load(f)


def _record():
    from dexbotic_amd import _lib as L
    routes = {c["id"]: route_of(L, with_pointers(c["fields"])) for c in cases()}
    with open(ROUTES, "w") as f:
        json.dump(routes, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(routes)} routes written to {ROUTES}")


# ------------------------------------------------------------------------------------------------ operands and reference
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}
GUARD_BYTES = 4096          # in front of every operand; a multiple of 256 so the offsets keep their meaning
SENTINEL = -24832.0         # exact in bf16; no kernel result of the table comes near it


def geometry(fields):
    """{buffer: (rows, cols, ld, batch strides, dtype code)} of the buffers the case has"""
    lay, M, N, K = fields["layout"], fields["M"], fields["N"], fields["K"]
    ind, outd = fields["in_dtype"], fields["out_dtype"]
    epi = F32 if fields.get("epi_f32") else ind
    z = (0, 0, 0)
    sA, sB, sC = fields.get("sA", z), fields.get("sB", z), fields.get("sC", z)
    fuse = fields.get("fuse", 0)
    g = {"A": ((K, M) if lay == TN else (M, K), fields["lda"], sA, ind),
         "B": ((N, K) if lay == NT else (K, N), fields["ldb"], sB, ind),
         "C": ((M, N // 2 if fuse else N), fields["ldc"], sC, outd)}
    if "A2" in fields:
        g["A2"] = ((fields["K2"], M), fields["lda"], z, ind)
        g["B2"] = ((fields["K2"], N), fields["ldb"], z, ind)
    if "bias" in fields:
        g["bias"] = ((1, N), N, z, epi)
    if "residual" in fields:
        g["residual"] = ((M, N), fields["ldr"], fields.get("sR", z), epi)
    if "mulgrad" in fields:
        g["mulgrad"] = ((M, N), fields["ldg"], fields.get("sG", z), epi)
    if "aux_out" in fields:
        g["aux_out"] = ((M, N), fields["ld_aux"] if fuse else fields["ldc"], sC, outd)
    if "mirror" in fields:
        g["mirror"] = ((M, N), fields["ldc"], z, BF16)
    if "sumsq" in fields:
        slots = ((M + 255) // 256) * ((N + 255) // 256)
        g["sumsq"] = ((1, slots), slots, z, F32)
    return g


class Buffer:
    """one operand inside a larger guarded allocation: ``view`` [nb0, nb1, nb2, rows, cols] is the operand, everything else of
    ``raw`` is guard"""

    def __init__(self, name, fields, geo, device, fill):
        (rows, cols), ld, st, code = geo
        self.name, self.dtype = name, TORCH_DT[code]
        es = 2 if code == BF16 else 4
        off = fields[name]
        assert off % es == 0
        nb = fields["nb"]
        self.start = GUARD_BYTES // es + off // es
        span = sum((n - 1) * s for n, s in zip(nb, st)) + (rows - 1) * ld + cols
        self.raw = torch.full((self.start + span + 2 * ld + 256,), fill, dtype=self.dtype, device=device)
        self.size, self.stride = (*nb, rows, cols), (*st, ld, 1)
        self.view = self.raw.as_strided(self.size, self.stride, self.start)
        # the part of the view that is distinct memory: batch extents with a zero stride collapse
        self.own = self.raw.as_strided(tuple(1 if s == 0 else n for n, s in zip(nb, st)) + (rows, cols), self.stride, self.start)

    def ptr(self):
        return self.raw.data_ptr() + self.start * self.raw.element_size()

    def inside(self):
        """bool mask over ``raw``: the operand's own elements"""
        m = torch.zeros(self.raw.numel(), dtype=torch.bool, device=self.raw.device)
        m.as_strided(self.own.shape, self.stride, self.start).fill_(True)
        return m


def _ints(shape, lo, hi, seed, dtype, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(dtype).to(device)


INPUT_RANGE = {"A": 3, "B": 3, "A2": 3, "B2": 3, "bias": 40, "residual": 40, "mulgrad": 2}


def make_buffers(fields, device="cpu"):
    """{name: Buffer}: inputs hold small integers inside NaN, outputs the sentinel (C the values to accumulate into, when the
    case accumulates; sumsq NaN)"""
    bufs = {}
    for i, (name, geo) in enumerate(sorted(geometry(fields).items())):
        if name in INPUT_RANGE:
            b = Buffer(name, fields, geo, device, float("nan"))
            r = INPUT_RANGE[name]
            b.own.copy_(_ints(b.own.shape, -r, r, 1000 + i, b.dtype, device))
        elif name == "sumsq":
            b = Buffer(name, fields, geo, device, SENTINEL)
            b.own.fill_(float("nan"))
        else:
            b = Buffer(name, fields, geo, device, SENTINEL)
            if name == "C" and fields.get("accumulate"):
                b.own.copy_(_ints(b.own.shape, -100, 100, 1000 + i, b.dtype, device))
        bufs[name] = b
    return bufs


def _act(act, x):
    import torch.nn.functional as F_
    return {ACT_GELU_ERF: F_.gelu, ACT_GELU_TANH: lambda v: F_.gelu(v, approximate="tanh"),
            ACT_QUICK_GELU: lambda v: v * torch.sigmoid(1.702 * v), ACT_SILU: F_.silu, ACT_RELU: F_.relu, ACT_SIGMOID: torch.sigmoid}[act](x)


def _act_grad(act, g):
    x = g.clone().requires_grad_(True)
    _act(act, x).backward(torch.ones_like(x))
    return x.grad


def is_exact(fields):
    """the case's C is held with torch.equal: no activation, or one that is exact on integers (ReLU and its 0 / 1 gradient)"""
    return fields["act"] in (ACT_NONE, ACT_RELU) and not fields.get("fuse")


def reference(fields, route, bufs):
    """fp64 -> {"acc": the largest exact sum in magnitude, "C": [nb.., M, N] in the output dtype, "C64": before that rounding,
    "aux_out": ...}.  The epilogue in the order include/dexbotic_amd.h states it, rounded once to the output dtype; a bf16 C that
    a two-step route rounds after its first step is rounded there as well (the step's K range is the table's)."""
    lay = fields["layout"]
    outdt = TORCH_DT[fields["out_dtype"]]

    def product(a, b):
        a, b = a.double(), b.double()
        a = a.transpose(-1, -2) if lay == TN else a
        b = b.transpose(-1, -2) if lay == NT else b
        return a @ b

    def rnd(x):
        return x.float().to(outdt)

    A, B = bufs["A"].view, bufs["B"].view
    steps = route["steps"]
    two = route["nsteps"] == 2 and family(steps[0]["kernel"]) != "gemv"
    if two and steps[1]["seg2"]:
        parts = [product(A, B), product(bufs["A2"].view, bufs["B2"].view)]
    elif two:                                       # the K tail: the head on the fast path, the rest on top
        K0 = steps[0]["K"]
        ka, kb = (-2 if lay == TN else -1), (-1 if lay == NT else -2)
        parts = [product(A.narrow(ka, 0, K0), B.narrow(kb, 0, K0)),
                 product(A.narrow(ka, K0, fields["K"] - K0), B.narrow(kb, K0, fields["K"] - K0))]
    else:
        parts = [product(A, B)]
        if "A2" in fields:
            parts[0] = parts[0] + product(bufs["A2"].view, bufs["B2"].view)
    ref = {"acc": max(float(p.abs().max()) for p in parts)}
    alpha = float(torch.tensor(fields["alpha"], dtype=torch.float32))
    pre = alpha * parts[0]
    if "bias" in fields:
        pre = pre + bufs["bias"].view.double()
    if fields.get("fuse"):
        pre = rnd(pre)
        ref["aux_out"] = pre
        F_ = fields["N"] // 2
        gate, up = pre[..., :F_].double(), pre[..., F_:].double()
        ref["C64"] = _act(ACT_SILU, gate) * up
        ref["C"] = rnd(ref["C64"])
        return ref
    if "aux_out" in fields:
        ref["aux_out"] = rnd(pre)
    if "mulgrad" in fields:
        v = pre * _act_grad(fields["act"], bufs["mulgrad"].view.double())
    elif fields["act"] != ACT_NONE:
        v = _act(fields["act"], pre)
    else:
        v = pre
    if "residual" in fields:
        v = v + bufs["residual"].view.double()
    if fields.get("accumulate"):
        v = v + bufs["C"].view.double()
    for p in parts[1:]:
        if fields["out_dtype"] == BF16:
            v = rnd(v).double()                     # the extra rounding of a bf16 C between the two steps
        v = v + alpha * p
    ref["C64"] = v
    ref["C"] = rnd(v)
    return ref


def _table():
    """the "GEMM route coverage" table of DESIGN.md: launcher row -> cases -> modes, from the routes on file"""
    routes, rows = load_routes(), {}
    for c in cases():
        r = routes[c["id"]]
        for i, s in enumerate(r["steps"]):
            n, modes = rows.setdefault(s["kernel"], [0, set()])
            rows[s["kernel"]][0] = n + 1
            modes |= modes_of(c["fields"], r, i) & REQUIRED_MODES[family(s["kernel"])]
    print("| launcher row | cases | modes reached |\n|---|---|---|")
    for k, (n, modes) in rows.items():
        print(f"| `{k}` | {n} | {', '.join(sorted(modes))} |")


if __name__ == "__main__":
    if "--record" in sys.argv:
        _record()
    if "--table" in sys.argv:
        _table()
