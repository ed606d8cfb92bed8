"""Which kernel a product gets: dxa_gemm_plan against the routes recorded from the commit before the dispatch was split
into a planner and a launcher (tests/golden/gemm_plan_parent.json.gz: one record per descriptor of ``corpus()``, written
by that commit's own dispatch with its launch sites turned into recorders).  The planner only does host arithmetic on the
descriptor, so the pointers are fake and never dereferenced and no GPU is needed.

A deliberate route change re-records the fixture from the commit that makes it; an accidental one fails here instead of
showing up only in the benchmark."""
import ctypes as C
import gzip
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_parent.json.gz")

NT, NN, TN = 0, 1, 2
F32, BF16 = 0, 1
ACT_GELU_TANH = 2
# fake operand addresses: 16-byte aligned, far apart
PTR = {"A": 0x10 << 36, "B": 0x11 << 36, "C": 0x12 << 36, "bias": 0x13 << 36, "residual": 0x14 << 36, "aux_out": 0x15 << 36,
       "mulgrad": 0x16 << 36, "mirror": 0x17 << 36, "sumsq": 0x18 << 36, "A2": 0x19 << 36, "B2": 0x1A << 36}
DTYPES = {"bb": (BF16, BF16), "bf": (BF16, F32), "ff": (F32, F32)}
STEP_FIELDS = ("grid", "block", "lds", "K", "K2", "a_off", "b_off", "seg2", "accumulate", "bias", "residual", "tm", "tn", "full",
               "tail_r", "split_s", "group_m", "vecA", "vecB", "vecC", "vecR", "vecG", "vecBias", "ksplit", "kper", "split_ws",
               "mirror", "sumsq")


def desc(layout, dt, M, N, K, **kw):
    """a plain product of contiguous operands as a dict of dxa_gemm_desc fields; ``kw`` overrides"""
    ind, outd = DTYPES[dt]
    d = dict(layout=layout, in_dtype=ind, out_dtype=outd, act=0, M=M, N=N, K=K, A=PTR["A"], B=PTR["B"], C=PTR["C"],
             lda=M if layout == TN else K, ldb=K if layout == NT else N, ldc=N, ldr=N, ldg=N, alpha=1.0, nb=(1, 1, 1))
    d.update(kw)
    return d


def _epilogues(d):
    """the epilogue families of one product: (tag, descriptor)"""
    f32_out = d["out_dtype"] == F32
    yield "none", d
    yield "bias_res", dict(d, bias=PTR["bias"], residual=PTR["residual"])
    yield "aux", dict(d, bias=PTR["bias"], aux_out=PTR["aux_out"])
    yield "act", dict(d, act=ACT_GELU_TANH, bias=PTR["bias"])
    yield "mulgrad", dict(d, act=ACT_GELU_TANH, mulgrad=PTR["mulgrad"])
    yield "acc_norm", dict(d, accumulate=1, sumsq=PTR["sumsq"], **({"mirror": PTR["mirror"]} if f32_out else {}))
    if d["in_dtype"] == BF16 and f32_out:
        yield "epi_f32", dict(d, epi_f32=1, bias=PTR["bias"], residual=PTR["residual"])
        yield "epi_f32_act", dict(d, epi_f32=1, bias=PTR["bias"], act=ACT_GELU_TANH)


def _misalign(d):
    yield "", d
    yield "A+8", dict(d, A=d["A"] + 8)
    yield "B+8", dict(d, B=d["B"] + 8)
    yield "C+4", dict(d, C=d["C"] + 4)
    yield "ldc_odd", dict(d, ldc=d["ldc"] + 1)
    if d.get("residual"):
        yield "ldr+4", dict(d, ldr=d["ldr"] + 4)
        yield "bias+4", dict(d, bias=d["bias"] + 4)


def corpus():
    """[(id, descriptor fields or None)]: a descriptor on each side of every threshold of the planner, the project's real
    shapes, every epilogue family, a few misalignments, and what every check rejects.  Deterministic."""
    out = []

    def add(tag, d):
        out.append((f"{len(out):05d}:{tag}", d))

    def tag(d, extra=""):
        return f"{'nt nn tn'.split()[d['layout']]}/{d['in_dtype']}{d['out_dtype']}/{d['M']}x{d['N']}x{d['K']}{'/' if extra else ''}{extra}"

    def plain(layouts, dts, Ms, Ns, Ks, extra="", **kw):
        for lay in layouts:
            for dt in dts:
                for M in Ms:
                    for N in Ns:
                        for K in Ks:
                            d = desc(lay, dt, M, N, K, **kw)
                            add(tag(d, extra), d)

    ALL, DT = (NT, NN, TN), ("bb", "bf", "ff")
    rows = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 287, 384, 385, 512, 513,
            543, 576, 577, 768, 769, 1024, 1025, 4592)
    cols = (1, 63, 64, 72, 100, 101, 128, 256, 264, 1152, 2048, 2052, 4304, 4608)
    deep = (1, 31, 32, 33, 63, 64, 96, 100, 960, 1023, 1024, 1056, 1088, 1100, 1984, 2016, 2048, 2080, 2112, 4032, 4096, 4160, 4304)
    # rows, columns and contraction lengths on each side of the thresholds
    plain(ALL, DT, rows, (256, 1152), (64, 1024, 3584))
    plain(ALL, DT, (1, 8, 16, 64, 287, 1024, 4592), cols, (256,))
    plain(ALL, DT, (1, 8, 64, 65, 256, 287, 543, 1025, 4592), (256, 4608), deep)
    # 128x128 tiles: tile counts around 32, NUM_CU / 4, NUM_CU / 2 and NUM_CU; K around 1024, 2048 and 4096
    for M, tn in ((128, (31, 32, 33, 64, 65, 128, 129, 256, 257)), (1024, (3, 4, 5, 8, 9, 16, 17, 32, 33)), (287, (10, 11, 21, 22, 36, 43, 85, 86))):
        plain((NT,), ("bb", "bf"), (M,), [128 * t for t in tn], (512, 960, 1024, 1984, 2048, 4096, 4160))
    # the 256-row kernels: a last round of tiles cut along K, nk_tot around 64; the project's real shapes
    plain(ALL, ("bb", "bf"), (4592,), (4608, 3584, 37888, 18944), (3584, 18944, 1984, 2016, 2048, 2080))
    plain((TN,), ("bb", "bf"), (3584, 4608, 18944), (3584, 18944), (4592, 287))
    plain((NT, NN), ("bb", "bf"), (287, 543), (4608, 3584, 37888, 18944, 151936), (3584, 18944))
    # SigLIP's 4304-wide MLP (K % 64 == 16: the K tail) and tails of 32
    plain(ALL, ("bb", "bf"), (729, 5832), (4304, 1152), (1152, 4304, 1056))
    # DiT head widths, fp32 and as bf16x3 products (K' = 3 K, fp32 epilogue operands)
    for h in (384, 768, 1024):
        plain(ALL, ("ff",), (17, 34, 68, 1088), (h, 3 * h, 4 * h, 6 * h, 7), (h, 4 * h, 17))
        plain((NT,), ("bf",), (17, 32, 68, 136, 272, 1088), (h, 3 * h, 4 * h, 6 * h), (3 * h, 12 * h, 3 * 32, 3 * 1088), epi_f32=1, bias=PTR["bias"])
    # skinny kernels: N / 16 tiles around NUM_CU / 2, K cut 1 .. 8
    plain((NT,), DT, (1, 16, 17, 32, 33, 48, 49, 64), (64, 2048, 2064, 4096), (512, 1024, 4096, 8192))
    # few-row NN: rows 1 .. 9, column blocks, the K slices, the scratch limit, what the route refuses
    plain((NN,), ("bb", "bf"), range(1, 10), (64, 100, 2048, 2056, 14336, 37888), (64, 96, 3584, 14336, 40000))
    for M in (1, 8):
        d = desc(NN, "bb", M, 4096, 4096)
        for t, dd in (("bias", dict(d, bias=PTR["bias"])), ("acc", dict(d, accumulate=1)), ("ldb", dict(d, ldb=4100)), ("B+8", dict(d, B=d["B"] + 8))):
            add(tag(dd, t), dd)
    # every epilogue family and misalignment on a moderate set of shapes
    for M, N, K in ((1, 256, 256), (16, 1152, 1152), (64, 1152, 4304), (129, 512, 256), (287, 4608, 3584), (543, 1152, 1152),
                    (1025, 1152, 4304), (4592, 3584, 3584), (1088, 768, 2304), (300, 300, 300), (512, 512, 1056)):
        for lay in ALL:
            for dt in DT:
                for et, e in _epilogues(desc(lay, dt, M, N, K)):
                    for mt, m in _misalign(e):
                        add(tag(m, et + (":" + mt if mt else "")), m)
    # the gated-MLP epilogue, with and without the pre-activations
    for M in (128, 129, 192, 193, 287, 4592):
        for N in (256, 260, 272, 37888):
            for K in (64, 100, 3584):
                d = desc(NT, "bb", M, N, K, fuse=1, ldc=N // 2, ld_aux=N)
                add(tag(d, "swiglu"), d)
                add(tag(d, "swiglu+aux"), dict(d, aux_out=PTR["aux_out"]))
    d = desc(NT, "bb", 287, 37888, 3584, fuse=1, ldc=18944, ld_aux=37888, aux_out=PTR["aux_out"])
    for t, dd in (("A+8", dict(d, A=d["A"] + 8)), ("C+4", dict(d, C=d["C"] + 4)), ("aux+4", dict(d, aux_out=d["aux_out"] + 4)), ("ldc", dict(d, ldc=18000)),
                  ("bias", dict(d, bias=PTR["bias"])), ("f32", dict(d, out_dtype=F32)), ("nn", dict(d, layout=NN)), ("mode7", dict(d, fuse=7)),
                  ("K2", dict(d, K2=64)), ("big", dict(d, M=40000))):
        add(tag(dd, "swiglu:" + t), dd)
    # a second (A2, B2) segment: contracted by the ping-pong kernel, or two products
    for M, N in ((64, 256), (63, 256), (127, 128), (3584, 4608), (300, 304), (300, 301)):
        for dt in DT:
            for K, K2 in ((4592, 4592), (100, 37), (32, 4592)):
                d = desc(TN, dt, M, N, K, A2=PTR["A2"], B2=PTR["B2"], K2=K2)
                add(tag(d, "seg"), d)
                add(tag(d, "seg:A2+8"), dict(d, A2=d["A2"] + 8))
                add(tag(d, "seg:bias_res"), dict(d, bias=PTR["bias"], residual=PTR["residual"]))
                e = dict(d, accumulate=1, sumsq=PTR["sumsq"], **({"mirror": PTR["mirror"]} if d["out_dtype"] == F32 else {}))
                add(tag(e, "seg:acc_norm"), e)
                add(tag(e, "seg:acc_norm:C+4"), dict(e, C=e["C"] + 4))
    for lay in (NT, NN):
        for M in (287, 4592):
            d = desc(lay, "bb", M, 1152, 1024, A2=PTR["A2"], B2=PTR["B2"], K2=64)
            add(tag(d, "seg"), d)
    d = desc(TN, "bb", 512, 512, 512, A2=PTR["A2"], B2=PTR["B2"], K2=64)
    add(tag(d, "seg:noA2"), dict(d, A2=0))
    add(tag(d, "seg:batched"), dict(d, nb=(2, 1, 1)))
    # batched products
    for nb in ((2, 1, 1), (1, 3, 2), (16, 12, 1), (255, 257, 1), (256, 256, 1)):
        for M, N, K in ((64, 64, 64), (197, 197, 64), (1024, 1024, 128), (4592, 4608, 3584)):
            for lay in ALL:
                for dt in DT:
                    d = desc(lay, dt, M, N, K, nb=nb, sA=(M * K, 0, 0), sB=(N * K, 0, 0), sC=(M * N, 0, 0))
                    add(tag(d, "nb%dx%dx%d" % nb), d)
                    add(tag(d, "nb%dx%dx%d:sA+1" % nb), dict(d, sA=(M * K + 1, 0, 0)))
    # what the checks reject, and what is no work
    g = desc(NT, "bb", 512, 512, 512)
    add("null", None)
    for t, dd in (("M<0", dict(g, M=-1)), ("K<0", dict(g, K=-1)), ("layout3", dict(g, layout=3)), ("layout-1", dict(g, layout=-1)),
                  ("in2", dict(g, in_dtype=2)), ("f32->bf16", dict(g, in_dtype=F32, out_dtype=BF16)), ("nb0", dict(g, nb=(1, 0, 1))),
                  ("M0", dict(g, M=0)), ("N0", dict(g, N=0, A=0)), ("K0", dict(g, K=0)), ("A0", dict(g, A=0)), ("B0", dict(g, B=0)), ("C0", dict(g, C=0)),
                  ("mirror_bf16", dict(g, mirror=PTR["mirror"])), ("mirror_nb", dict(g, out_dtype=F32, mirror=PTR["mirror"], nb=(2, 1, 1))),
                  ("sumsq_nb", dict(g, sumsq=PTR["sumsq"], nb=(2, 1, 1))), ("epi_f32_bb", dict(g, epi_f32=1)),
                  ("epi_f32_ff", dict(g, in_dtype=F32, out_dtype=F32, epi_f32=1)), ("epi_f32_slow", dict(g, out_dtype=F32, epi_f32=1, M=32)),
                  ("epi_f32_K", dict(g, out_dtype=F32, epi_f32=1, K=100)), ("fuse_slow", dict(g, fuse=1, M=64, ldc=256, ld_aux=512))):
        add(t, dd)
    return out


def _load_lib():
    from dexbotic_amd import _lib as L
    return L


def _make(L, fields):
    d = L.GemmDesc()
    for k, v in fields.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(d, k)[i] = x
        else:
            setattr(d, k, v)
    return d


def plan_record(L, fields):
    """one fixture record from dxa_gemm_plan: the status and message of a rejected descriptor, or the plan"""
    info = L.GemmPlanInfo()
    rc = L.lib.dxa_gemm_plan(_make(L, fields) if fields is not None else None, C.byref(info))
    if rc != 0:
        return {"rc": rc, "error": L.last_error()}
    steps = []
    for i in range(info.nsteps):
        s = info.step[i]
        r = {"kernel": s.kernel.decode()}
        for f in STEP_FIELDS:
            v = getattr(s, f)
            r[f] = list(v) if f == "grid" else v
        steps.append(r)
    return {"rc": 0, "mirror_pass": info.mirror_pass, "sumsq_pass": info.sumsq_pass, "steps": steps}


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def test_corpus_is_the_recorded_one(golden):
    ids = [i for i, _ in corpus()]
    assert ids == [r["id"] for r in golden["records"]]
    assert len(set(ids)) == len(ids)


def test_every_descriptor_gets_the_route_the_parent_commit_gave_it(golden):
    L = _load_lib()
    wrong = []
    for (cid, fields), want in zip(corpus(), golden["records"]):
        got = dict(plan_record(L, fields), id=cid)
        if got != want:
            wrong.append((cid, {k: (want.get(k), got.get(k)) for k in set(want) | set(got) if want.get(k) != got.get(k)}))
    assert not wrong, f"{len(wrong)} of {len(golden['records'])} routes differ (expected, got); the first: {wrong[:3]}"


def test_the_corpus_reaches_every_row_of_the_launcher_table(golden):
    """every kernel the library can launch is pinned by a descriptor, and the table has no row nothing selects"""
    L = _load_lib()
    names = []
    while L.lib.dxa_gemm_kernel_name(len(names)) is not None:
        names.append(L.lib.dxa_gemm_kernel_name(len(names)).decode())
    assert len(names) >= 60 and len(set(names)) == len(names) and L.lib.dxa_gemm_kernel_name(-1) is None
    recorded = {s["kernel"] for r in golden["records"] for s in r.get("steps", ())}
    assert recorded == set(names), (sorted(set(names) - recorded), sorted(recorded - set(names)))
