"""CPU checks of the loss-head reference (tests/loss_ref.py): it is F.cross_entropy and its autograd gradient, torch.logsumexp
and torch.argmax in float64 wherever torch defines the case, and the slack constants and the share cap of tests/loss_cases.py hold
for a plain fp32 evaluation of the same formulas over the whole case table (what they were measured from)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import loss_cases as LC
from tests import loss_ref as R

_CE = [c for c in LC.CASES if c["entry"] in LC.FWD + LC.BWD]
_HARD_FWD = [c for c in _CE if c["entry"] == "ce_fwd"]


def _same(a, b, tol=1e-12):
    """equal non-finite values, and finite ones within ``tol`` of the larger magnitude (absolute below 1)"""
    fin = torch.isfinite(b)
    if not torch.equal(torch.isnan(a), torch.isnan(b)) or not torch.equal(a[~fin & ~torch.isnan(b)], b[~fin & ~torch.isnan(b)]):
        return False
    return bool(((a[fin] - b[fin]).abs() <= tol * torch.clamp(b[fin].abs(), min=1.0)).all())


def _torch_labels(case, labels):
    """the kernels' rule as F.cross_entropy states it: every ignored label becomes ignore_index = -100"""
    return torch.where(LC.ignored(labels, case["V"], case["ignore_index"]), torch.full_like(labels, -100), labels)


@pytest.mark.parametrize("case", _HARD_FWD, ids=lambda c: c["id"])
def test_forward_reference_is_torch(case):
    inp = LC.inputs(case)
    x = inp["logits"].double()
    ref = R.reference(case, inp)
    assert _same(ref["lse"][0], torch.logsumexp(x, 1))
    want = F.cross_entropy(x, _torch_labels(case, inp["labels"]), reduction="none", ignore_index=-100)
    assert _same(ref["row_loss"][0], want)
    assert (ref["lse"][3][torch.isfinite(ref["lse"][0])] >= 1.0).all()         # mag: at least the relative error of the sum


def _unrounded(case):
    """the case without the rounding of dlogits to bf16 (its inputs are the bf16 case's, already rounded)"""
    return dict(case, dtype="f32")


@pytest.mark.parametrize("case", [c for c in _CE if c["entry"] in ("ce_bwd", "rows_bwd")], ids=lambda c: c["id"])
def test_backward_reference_is_torch_autograd(case):
    inp = LC.inputs(case)
    x = inp["logits"].double().requires_grad_(True)
    loss = F.cross_entropy(x, _torch_labels(case, inp["labels"]), reduction="none", ignore_index=-100)
    g = (inp["gscale"].double()[0] if "gscale" in inp else 1.0) * float(torch.tensor(LC.SCALE, dtype=torch.float32))
    w = g * (inp["row_w"].double() if "row_w" in inp else torch.ones(case["rows"], dtype=torch.float64))
    fin = torch.isfinite(loss.detach())
    if not fin.all():                                 # torch's gradient through an infinite or NaN loss is NaN: those rows by formula only
        w = torch.where(fin, w, torch.zeros_like(w))
    (torch.where(fin, loss, torch.zeros_like(loss)) * w).sum().backward()
    fwd = R.reference(R.forward_case(case), inp)
    ref = R.reference(_unrounded(case), inp, {"lse": fwd["lse"][0]})["dlogits"][0]
    soft = torch.isfinite(fwd["lse"][0])              # rows that have a softmax (torch: 0 * NaN = NaN through an ignored all -inf row)
    assert _same(ref[fin & soft], x.grad[fin & soft], 1e-11)
    assert torch.isfinite(ref[soft]).all()            # a label on a -inf logit: finite gradient, -g at the label
    ign = LC.ignored(inp["labels"], case["V"], case["ignore_index"])
    assert (ref[ign] == 0).all()                      # an ignored row is zeros whatever it holds


@pytest.mark.parametrize("case", [c for c in _CE if c["entry"] in ("soft_fwd", "soft_bwd")], ids=lambda c: c["id"])
def test_soft_reference_is_torch_autograd(case):
    """navila's soft_cross_entropy written with torch: the cross-entropy against a Gaussian over the soft ids centred on the label"""
    inp = LC.inputs(case)
    x = inp["logits"].double().requires_grad_(True)
    labels, ids = inp["labels"], inp["soft_ids"]
    ign = LC.ignored(labels, case["V"], case["ignore_index"])
    tgt = torch.zeros(case["rows"], case["V"], dtype=torch.float64)
    for r in range(case["rows"]):
        if ign[r]:
            continue
        if int(labels[r]) in ids.tolist():
            d = (labels[r] - ids).double()
            tgt[r, ids] = torch.softmax(-(d * d) * float(torch.tensor(LC.INV2S2, dtype=torch.float32)), 0)
        else:
            tgt[r, labels[r]] = 1.0
    loss = -(tgt * torch.log_softmax(x, 1)).sum(1)
    fwd = R.reference(R.forward_case(case), inp)
    assert _same(fwd["row_loss"][0], loss.detach(), 1e-11) and _same(fwd["lse"][0], torch.logsumexp(x.detach(), 1))
    assert any(int(l) in ids.tolist() for l in labels[~ign])
    if case["entry"] == "soft_bwd":
        g = inp["gscale"].double()[0] * float(torch.tensor(LC.SCALE, dtype=torch.float32))
        (loss.sum() * g).backward()
        assert _same(R.reference(_unrounded(case), inp, {"lse": fwd["lse"][0]})["dlogits"][0], x.grad, 1e-11)


@pytest.mark.parametrize("case", [c for c in LC.CASES if c["entry"] == "argmax"], ids=lambda c: c["id"])
def test_argmax_reference_is_torch(case):
    x = LC.inputs(case)["x"]
    want = R.argmax_ref(x)
    assert torch.equal(want, torch.argmax(x.double(), 1))
    if case["maxcols"]:
        assert (want == min(case["maxcols"])).all()
    if case["special"] in ("one_nan", "two_nan"):
        assert torch.isnan(x[0, want[0]]) and not torch.isnan(x[0, :want[0]]).any()
    if case["special"] == "negzero":
        assert (x[torch.arange(case["rows"]), want].view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32) < 0).all()   # the -0.0


def test_sample_reduce_and_expectile_reference():
    for case in (c for c in LC.CASES if c["entry"] == "sample_reduce"):
        inp = LC.inputs(case)
        B, L = case["B"], case["L"]
        ref = R.reference(case, inp)
        total = 0.0
        for b in range(B):
            lab = inp["labels"].view(B, L)[b]
            keep = (lab != -100) & (lab >= 0) & (lab < LC.SAMPLE_V)
            w = 1.0 + (torch.sigmoid(inp["reward"].double()[b]) if "reward" in inp else 0.0)
            total = total + w * inp["row_loss"].double().view(B, L)[b][keep].sum() / max(int(keep.sum()), 1) / B
            assert _same(ref["row_w"][0].view(B, L)[b], torch.full((L,), float(w / max(int(keep.sum()), 1) / B), dtype=torch.float64))
            if case["empty"] and b == 0:
                assert int(keep.sum()) == 0
        assert _same(ref["loss"][0], torch.as_tensor(total, dtype=torch.float64).view(1))
    for case in (c for c in LC.CASES if c["entry"] == "expectile" and c["dpred"]):
        inp = LC.inputs(case)
        p = inp["pred"].double().requires_grad_(True)
        d = p - inp["target"].double()
        tau = torch.tensor(case["tau"], dtype=torch.float32).double()
        loss = (torch.where(d < 0, tau, 1.0 - tau) * d * d).mean()
        (loss * 0.5).backward()
        ref = R.reference(case, inp)
        assert _same(ref["loss"][0], loss.detach().view(1)) and _same(ref["dpred"][0], p.grad)


_MEASURED = {}


def measure():
    """largest excess (units of 2^-24 mag beyond the U ulp) of the fp32 emulation per output kind, and per backward entry point
    the share of bf16 dlogits not bit-equal to the reference rounded to bf16"""
    if _MEASURED:
        return _MEASURED
    worst = {k: 0.0 for k in LC.K_SLACK}
    neq, tot = {}, {}
    for case in LC.CASES:
        if case["entry"] == "argmax":
            continue
        inp = LC.inputs(case)
        stats = {"lse": R.emulate(R.forward_case(case), inp)["lse"]} if case["entry"] in LC.BWD else None
        ref, emu = R.reference(case, inp, stats), R.emulate(case, inp, stats)
        for n, (v, kind, U, mag) in ref.items():
            worst[kind] = max(worst[kind], float(R.excess(emu[n], v, U, mag).max()))
            if U:
                neq[case["entry"]] = neq.get(case["entry"], 0) + R.not_bit_equal(emu[n], v)
                tot[case["entry"]] = tot.get(case["entry"], 0) + v.numel()
    _MEASURED.update(worst=worst, share={e: neq[e] / tot[e] for e in tot})
    return _MEASURED


def test_slack_constants_cover_the_fp32_emulation():
    m = measure()
    print("fp32 emulation, largest excess per kind (2^-24 mag):", {k: round(v, 3) for k, v in m["worst"].items()})
    for kind, v in m["worst"].items():
        assert math.isfinite(v) and v > 0 and 4 * v <= LC.K_SLACK[kind], (kind, v)


def test_share_cap_holds_for_the_fp32_emulation():
    m = measure()
    print("fp32 emulation, share of bf16 dlogits not bit-equal per entry point:", {k: f"{100 * v:.4f}%" for k, v in m["share"].items()})
    assert set(m["share"]) == set(LC.BWD)
    for e, s in m["share"].items():
        assert s <= LC.SHARE_CAP / 10, (e, s)
