"""Every case of tests/loss_cases.py on the MI355X: the entry points of csrc/loss.hip other than dxa_sample_rows (cross-entropy
forward and backward with hard, soft and row-weighted targets, dxa_argmax_rows, dxa_ce_sample_reduce, dxa_expectile_loss) called
through the C ABI on the test's own buffers, against the fp64 reference of tests/loss_ref.py.

Inputs are carved out of NaN-filled buffers — the columns [V, ld) of every row and the guards in front and behind included — and
outputs out of sentinel-filled ones, each at the case's offset from a 256-byte-aligned address; the argmax cases run a second
time with the largest finite value as the fill.  Per case: the guards are intact, the columns [V, ldd) of dlogits keep their
sentinel (in place: the logits' NaN), the inputs are unchanged; the call, captured once into a graph that is never replayed,
holds one kernel node that the runtime names with the case's instantiation; every output element holds
    |got - ref| <= U * ulp_T(ref) + k * 2^-24 * mag          (loss_cases.py: U, k = K_SLACK per output kind; mag: loss_ref.py)
with a non-finite reference element matched exactly, and argmax indices are equal to torch.argmax's.  The backward takes the lse
the kernel's own forward returned.  Each backward case and each per-sample reduction runs twice with another case in between:
the same bits.  Over the bf16 dlogits of one entry point at most SHARE_CAP of the elements differ from the reference rounded to
bf16.  Bit identities: in place equals out of place; dxa_soft_cross_entropy_* with K = 0 equals dxa_cross_entropy_*;
dxa_cross_entropy_rows_bwd with row_w = NULL equals dxa_cross_entropy_bwd; the wide and the narrow argmax kernel agree on the
same rows (presented once aligned, once 4 elements in), and with dxa_sample_rows(top_k = 1, u = 0) on NaN-free rows."""
import time

import pytest
import torch

from tests import loss_cases as LC
from tests import loss_ref as R
from tests.helpers import _captured_kernel

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import graphs
    from dexbotic_amd import kernels as K

DEV = "cuda"
G = 256                                        # guard elements on each side (a multiple of 256 bytes for every dtype used)
F32, I64 = torch.float32, torch.int64
SENT = {torch.float32: -7777.0, torch.bfloat16: -7776.0, torch.int64: -12345}
IV = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int64: torch.int64}
NAN = float("nan")


class Carved:
    """``n`` elements carved out of a larger buffer filled with ``fill``: ``G + off`` guard elements in front, G behind"""

    def __init__(self, n, dtype, fill, off=0, value=None):
        self.buf = torch.full((2 * G + off + n,), fill, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.lo, self.hi = G + off, G + off + n
        self.t = self.buf[self.lo:self.hi]
        if value is not None:
            self.t.copy_(value.to(DEV).reshape(-1))
        self.mark()

    def mark(self):
        self.before = self.buf.clone()

    def rows(self, rows, ld, cols):
        """the [rows, cols] operand of row stride ld"""
        return self.t.view(rows, ld)[:, :cols]

    def _iv(self, t):
        return t.view(IV[self.buf.dtype])

    def guards_ok(self):
        b, a = self._iv(self.buf), self._iv(self.before)
        return torch.equal(b[:self.lo], a[:self.lo]) and torch.equal(b[self.hi:], a[self.hi:])

    def pad_ok(self, rows, ld, cols):
        """the columns [cols, ld) of every row are what they were"""
        b, a = self._iv(self.t).view(rows, ld), self._iv(self.before[self.lo:self.hi]).view(rows, ld)
        return torch.equal(b[:, cols:], a[:, cols:])

    def unchanged(self):
        return torch.equal(self._iv(self.buf), self._iv(self.before))


def _ptr(c):
    return c.t.data_ptr() if c is not None else None


class Call:
    """the operands of one case on the device and its C call.  ``variant``: ``soft_k0`` (a hard case through the soft entry point
    without soft ids), ``rows_null`` (a dxa_cross_entropy_bwd case through dxa_cross_entropy_rows_bwd without row weights),
    ``out_of_place`` (an in-place case with a dlogits buffer of its own), ``off4`` (an argmax case 4 elements in);
    ``fill``: what surrounds the input rows"""

    def __init__(self, case, inp, stats=None, variant=None, fill=NAN):
        self.case, self.variant, e = case, variant, case["entry"]
        self.ins, self.outs, self.keep = {}, {}, []
        T = LC.TORCH_DT[case["dtype"]]
        off = dict(case["off"])
        if e == "argmax":
            rows, cols, ld = case["rows"], case["cols"], LC.ld_of(case)
            x = Carved(rows * ld, T, fill, 4 if variant == "off4" else off.get("x", 0))
            x.rows(rows, ld, cols).copy_(inp["x"].to(DEV))
            x.mark()
            self.ins["x"] = x
            self.outs["out"] = Carved(rows, I64, SENT[I64])
            return
        if e == "expectile":
            n = case["n"]
            self.ins.update(pred=Carved(n, F32, NAN, value=inp["pred"]), target=Carved(n, F32, NAN, value=inp["target"]))
            self.outs["loss"] = Carved(1, F32, SENT[F32])
            if case["dpred"]:
                self.outs["dpred"] = Carved(n, F32, SENT[F32])
            return
        if e == "sample_reduce":
            n = case["B"] * case["L"]
            self.ins.update(row_loss=Carved(n, F32, NAN, value=inp["row_loss"]), labels=Carved(n, I64, 7, value=inp["labels"]))
            if "reward" in inp:
                self.ins["reward"] = Carved(case["B"], F32, NAN, value=inp["reward"])
            self.outs.update(row_w=Carved(n, F32, SENT[F32]), loss=Carved(1, F32, SENT[F32]))
            return
        rows, V, ld = case["rows"], case["V"], LC.ld_of(case)
        self.inplace = e in LC.BWD and case["dlayout"] == "inplace" and variant != "out_of_place"
        lg = Carved(rows * ld, T, NAN, off.get("logits", 0))
        lg.rows(rows, ld, V).copy_(inp["logits"].to(DEV))
        lg.mark()
        (self.outs if self.inplace else self.ins)["logits"] = lg
        self.ins["labels"] = Carved(rows, I64, 7, value=inp["labels"])
        if case["K"]:
            self.ins["soft_ids"] = Carved(case["K"], I64, 7, value=inp["soft_ids"])
            self.keep.append(inp["soft_ids"].contiguous())                 # the host copy the call checks
        if e in LC.FWD:
            self.outs.update(row_loss=Carved(rows, F32, SENT[F32]), lse=Carved(rows, F32, SENT[F32]))
            return
        self.ins["lse"] = Carved(rows, F32, NAN, value=stats["lse"])
        if "gscale" in inp:
            self.ins["gscale"] = Carved(1, F32, NAN, value=inp["gscale"])
        if "row_w" in inp:
            self.ins["row_w"] = Carved(rows, F32, NAN, value=inp["row_w"])
        if not self.inplace:
            self.outs["dlogits"] = Carved(rows * LC.ldd_of(case), T, SENT[T], off.get("dlogits", 0))

    def __call__(self, stream):
        c, e, lib = self.case, self.case["entry"], L.lib
        p = lambda n: _ptr(self.ins.get(n) or self.outs.get(n))
        dt = LC.DT[c["dtype"]]
        if e == "argmax":
            return lib.dxa_argmax_rows(p("x"), LC.ld_of(c), p("out"), c["rows"], c["cols"], dt, stream)
        if e == "expectile":
            return lib.dxa_expectile_loss(p("pred"), p("target"), p("loss"), p("dpred"), c["n"], c["tau"], 0.5, stream)
        if e == "sample_reduce":
            return lib.dxa_ce_sample_reduce(p("row_loss"), p("labels"), p("reward"), p("row_w"), p("loss"), c["B"], c["L"], LC.SAMPLE_V, -100,
                                            stream)
        rows, V, ld, ign = c["rows"], c["V"], LC.ld_of(c), c["ignore_index"]
        host = self.keep[0].data_ptr() if self.keep else None
        if e in LC.FWD:
            if e == "soft_fwd" or self.variant == "soft_k0":
                return lib.dxa_soft_cross_entropy_fwd(p("logits"), ld, p("labels"), p("row_loss"), p("lse"), rows, V, ign, p("soft_ids"), host,
                                                      c["K"], LC.INV2S2, dt, stream)
            return lib.dxa_cross_entropy_fwd(p("logits"), ld, p("labels"), p("row_loss"), p("lse"), rows, V, ign, dt, stream)
        d = p("logits") if self.inplace else p("dlogits")
        ldd = LC.ldd_of(c)
        if e == "soft_bwd" or self.variant == "soft_k0":
            return lib.dxa_soft_cross_entropy_bwd(p("logits"), ld, p("labels"), p("lse"), p("gscale"), LC.SCALE, d, ldd, rows, V, ign,
                                                  p("soft_ids"), host, c["K"], LC.INV2S2, dt, stream)
        if e == "rows_bwd" or self.variant == "rows_null":
            return lib.dxa_cross_entropy_rows_bwd(p("logits"), ld, p("labels"), p("lse"), p("gscale"), LC.SCALE, p("row_w"), d, ldd, rows, V,
                                                  ign, dt, stream)
        return lib.dxa_cross_entropy_bwd(p("logits"), ld, p("labels"), p("lse"), p("gscale"), LC.SCALE, d, ldd, rows, V, ign, dt, stream)

    def collect(self):
        """(outputs on the CPU, problems)"""
        c, e = self.case, self.case["entry"]
        problems = [f"{n}: guard damaged" for n, o in self.outs.items() if not o.guards_ok()]
        problems += [f"{n}: input changed" for n, o in self.ins.items() if not o.unchanged()]
        got = {}
        for n, o in self.outs.items():
            if n in ("logits", "dlogits"):
                rows, V, ld = c["rows"], c["V"], LC.ld_of(c) if n == "logits" else LC.ldd_of(c)
                if not o.pad_ok(rows, ld, V):
                    problems.append(f"{n}: columns [V, ld) written")
                got["dlogits"] = o.rows(rows, ld, V).cpu()
            else:
                got[n] = o.t.cpu()
        return got, problems


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(case, inp, stats=None, side=None, variant=None, fill=NAN):
    """one guarded call -> (outputs on the CPU, problems, (kernel name, grid.x) of the captured call or None)"""
    call = Call(case, inp, stats, variant, fill)
    cap = None
    if side is not None:
        g = torch.cuda.CUDAGraph(keep_graph=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            with graphs.capture(g, side):
                rc = call(side.cuda_stream)
        assert rc == 0, L.last_error()
        cap = _captured_kernel(g.raw_cuda_graph(), side.cuda_stream)
    L.check(call(_stream()), case["entry"])
    torch.cuda.synchronize()
    got, problems = call.collect()
    return got, problems, cap


def _forward_lse(case, inp):
    """the lse the kernel's own forward returns for a backward case's inputs"""
    got, problems, _ = _run(R.forward_case(case), inp)
    assert not problems, problems
    return {"lse": got["lse"]}


def _bits_equal(a, b):
    return all(torch.equal(a[n].contiguous().view(IV[a[n].dtype]), b[n].contiguous().view(IV[b[n].dtype])) for n in a)


def _case(cid):
    return next(c for c in LC.CASES if c["id"] == cid)


_OTHER = next(c for c in LC.CASES if c["entry"] == "ce_bwd" and c["rows"] == 9 and c["V"] == 1028 and c["dtype"] == "bf16")


class _Results(dict):
    """id -> record of the case run once (a backward case and a per-sample reduction twice, another case in between; an argmax case
    a second time inside the largest finite value), computed on first use"""

    def __init__(self):
        super().__init__()
        self.side = torch.cuda.Stream()

    def __missing__(self, cid):
        case = _case(cid)
        e = case["entry"]
        inp = LC.inputs(case)
        stats = _forward_lse(case, inp) if e in LC.BWD else None
        got, problems, cap = _run(case, inp, stats, self.side)
        rec = dict(got=got, problems=problems, cap=cap, stats=stats, inp=inp)
        if e in LC.BWD or e == "sample_reduce":
            oi = LC.inputs(_OTHER)
            _run(_OTHER, oi, _forward_lse(_OTHER, oi))
            got2, problems2, _ = _run(case, inp, stats)
            problems += problems2
            if not _bits_equal(got, got2):
                problems.append("second run not bit-identical")
        if e == "argmax":
            got2, problems2, _ = _run(case, inp, fill=torch.finfo(LC.TORCH_DT[case["dtype"]]).max)
            problems += problems2
            rec["got_maxfill"] = got2
        else:
            rec["ref"] = R.reference(case, inp, stats)
        self[cid] = rec
        return rec


@pytest.fixture(scope="module")
def results():
    t0 = time.time()
    res = _Results()
    yield res
    torch.cuda.synchronize()
    print(f"\n{len(res)} cases in {time.time() - t0:.1f} s")


def _bad_values(case, got, ref):
    bad = []
    for n, (v, kind, U, mag) in ref.items():
        ex = R.excess(got[n].reshape(v.shape), v, U, mag)
        k = LC.K_SLACK[kind]
        print(f"{case['id']} {n}: worst {float(ex.max()):.3g} x 2^-24 mag (k {k})")
        if not (ex <= k).all():
            i = int(torch.argmax(ex))
            bad.append(f"{n}: {int((ex > k).sum())}/{ex.numel()} over the bound, worst {float(ex.flatten()[i]):.3g} x 2^-24 mag (k {k}) "
                       f"at flat {i}: got {float(got[n].flatten()[i]):.9g} want {float(v.flatten()[i]):.9g}")
    return bad


@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c["id"])
def test_loss_route(case, results):
    rec = results[case["id"]]
    name, _ = rec["cap"]
    inst = LC.INSTANTIATIONS[case["kernel"]]
    assert name is not None, "the runtime did not name the captured kernel"
    assert inst["mangled"] in name or inst["demangled"] in name, (name, case["kernel"])
    assert not rec["problems"], rec["problems"]
    if case["entry"] == "argmax":
        want = R.argmax_ref(rec["inp"]["x"])
        assert torch.equal(rec["got"]["out"], want), (rec["got"]["out"].tolist(), want.tolist())
        assert torch.equal(rec["got_maxfill"]["out"], want), ("inside the largest finite value", rec["got_maxfill"]["out"].tolist(), want.tolist())
        return
    bad = _bad_values(case, rec["got"], rec["ref"])
    assert not bad, bad


def test_loss_share_not_bit_equal(results):
    neq, tot = {}, {}
    for case in LC.CASES:
        if case["entry"] not in LC.BWD or case["dtype"] != "bf16":
            continue
        rec = results[case["id"]]
        v = rec["ref"]["dlogits"][0]
        neq[case["entry"]] = neq.get(case["entry"], 0) + R.not_bit_equal(rec["got"]["dlogits"], v)
        tot[case["entry"]] = tot.get(case["entry"], 0) + v.numel()
    share = {e: neq[e] / tot[e] for e in tot}
    print("share of bf16 dlogits not bit-equal:", {e: f"{neq[e]}/{tot[e]} = {100 * s:.4f}%" for e, s in share.items()})
    assert set(share) == set(LC.BWD) and all(s <= LC.SHARE_CAP for s in share.values()), share


_INPLACE = [c for c in LC.CASES if c["entry"] in LC.BWD and c["dlayout"] == "inplace"]
_HARD = [c for c in LC.CASES if c["entry"] in ("ce_fwd", "ce_bwd")]
_WIDE = [c for c in LC.CASES if c["kernel"] == LC.WIDE and c["layout"] == "contig"]


@pytest.mark.parametrize("case", _INPLACE, ids=lambda c: c["id"])
def test_in_place_equals_out_of_place(case, results):
    rec = results[case["id"]]
    got, problems, _ = _run(case, rec["inp"], rec["stats"], variant="out_of_place")
    assert not problems, problems
    assert _bits_equal(rec["got"], got)


@pytest.mark.parametrize("case", _HARD, ids=lambda c: c["id"])
def test_soft_entry_without_soft_ids_equals_plain(case, results):
    rec = results[case["id"]]
    got, problems, cap = _run(case, rec["inp"], rec["stats"], results.side, variant="soft_k0")
    assert not problems, problems
    assert cap == rec["cap"]
    assert _bits_equal(rec["got"], got)


@pytest.mark.parametrize("case", [c for c in _HARD if c["entry"] == "ce_bwd"], ids=lambda c: c["id"])
def test_rows_backward_without_weights_equals_plain(case, results):
    rec = results[case["id"]]
    got, problems, cap = _run(case, rec["inp"], rec["stats"], results.side, variant="rows_null")
    assert not problems, problems
    assert cap == rec["cap"]
    assert _bits_equal(rec["got"], got)


@pytest.mark.parametrize("case", _WIDE, ids=lambda c: c["id"])
def test_wide_and_narrow_argmax_agree(case, results):
    rec = results[case["id"]]
    got, problems, cap = _run(case, rec["inp"], None, results.side, variant="off4")
    assert not problems, problems
    assert LC.INSTANTIATIONS[LC.ak("bf16", 4)]["mangled"] in cap[0] or LC.INSTANTIATIONS[LC.ak("bf16", 4)]["demangled"] in cap[0], cap
    assert torch.equal(got["out"], rec["got"]["out"])
    x = rec["inp"]["x"]
    clean = ~torch.isnan(x).any(1)
    if clean.any():
        tok = K.sample_rows(x.to(DEV), torch.zeros(x.shape[0], dtype=torch.float32, device=DEV), top_k=1).cpu()
        assert torch.equal(tok[clean], rec["got"]["out"][clean])
