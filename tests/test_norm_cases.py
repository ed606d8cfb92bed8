"""CPU checks of the norm route table (tests/norm_cases.py) against dxa_norm_plan: every case gets the kernel it names (and the
row-loop trips, where it names them), the column sums take the direct / fused / two-launch form their row count and stream
state call for, every instantiation the launchers of the norm entry points can reach (dxa_norm_kernel_name: RMSNorm, LayerNorm,
add-LayerNorm, dxa_colsum, downsample LayerNorm, adarms, gated residual) is reached by a case, and the planner refuses what the entry points refuse, with the same status and message.  dxa_norm_plan is host
arithmetic: fake addresses, no GPU."""
import ctypes as C

import pytest

from dexbotic_amd import _lib as L
from dexbotic_amd import kernels as K
from tests import norm_cases as NC


def plan(case, **extra):
    return K.norm_plan(case["entry"], **NC.plan_fields(case, NC.fake_addr(case)), **extra)


@pytest.mark.parametrize("case", NC.NORM_CASES, ids=lambda c: c["id"])
def test_norm_case_route(case):
    p = plan(case)
    e = case["entry"]
    assert p["kernel"] == case["kernel"], p
    assert p["mode"] is None
    if case["trips"] is not None:
        assert p["trips"] == case["trips"], p
    elif e not in NC.SAMPLE_ENTRIES:
        assert p["trips"] == 1, p
    fwd = e.endswith("_fwd")
    k = p["kernel"]
    if e in NC.SAMPLE_ENTRIES:
        T = "bf16" if case["dtype"] == "bf16" else "float"
        if fwd:
            assert p["kernel2"] is None and p["grid"] == ((case["rows"] + 3) // 4, 1, 1)
        else:
            assert p["kernel2"] == f"adarms_fold_k<{T}>" and p["grid"] == (NC.adarms_groups(case["rps"]), case["B"], 1)
        assert p["vec"] == int(k.split(",")[1].rstrip(">")) if "fast" not in k else p["vec"] == 8
        return
    assert p["kernel2"] is None
    rows = NC.ds_rows(case) if e.startswith("downsample") else case["rows"]
    assert p["grid"] == (((rows + 3) // 4) if fwd else NC.partial_rows(case), 1, 1)
    assert p["block"] == (512 if "split" in k else 256)
    if e.startswith("downsample"):
        assert p["vec"] == int(k.rstrip(">").split(",")[-1])
        sums = 8 * case["cols"] * 4
        assert p["lds"] == (sums if (not fwd and case["w"] and sums <= 60 * 1024) else 0), p
        return
    assert p["vec"] == (8 if ("fast8" in k or "fwd_fast" in k or "split" in k) else
                        1 if k.rstrip(">").endswith((",1", ",1,true")) else 4)


@pytest.mark.parametrize("case", NC.COLSUM_CASES, ids=lambda c: c["id"])
def test_colsum_case_route(case):
    rows = case["rows"]
    p = plan(case, have_counters=1)
    assert p["kernel"] == case["kernel"], p
    assert p["nsplit"] == (1 if rows <= 32 else NC.colsum_nsplit(rows))
    assert p["mode"] == ("direct" if rows <= 32 else "fused") and p["kernel2"] is None
    assert p["grid"] == ((case["cols"] + 255) // 256, p["nsplit"], 1)
    # counters not there yet: fused all the same when they can be made, two launches under capture
    assert plan(case, have_counters=0, capturing=0)["kernel"] == case["kernel"]
    q = plan(case, have_counters=0, capturing=1)
    if rows <= 32:
        assert q == p
    else:
        assert q["kernel"] == case["capture_kernel"] and q["mode"] == "two_launch" and q["kernel2"] == "colsum_stage2_k", q
        assert q["nsplit"] == p["nsplit"]
    # a stream that captures with its counters made keeps the fused form
    assert plan(case, have_counters=1, capturing=1) == p
    vec = NC.ld_of(case)[0] % 4 == 0 and NC.ld_of(case)[1] % 4 == 0
    assert p["vec"] == (4 if vec else 1)


def test_every_reachable_kernel_is_named_by_a_case():
    names = K.norm_kernel_names()
    assert len(names) == len(set(names)) and L.lib.dxa_norm_kernel_name(-1) is None
    reached = {c["kernel"] for c in NC.ALL_CASES} | {c["capture_kernel"] for c in NC.COLSUM_CASES if c["capture_kernel"]}
    reached |= {"colsum_stage2_k", "adarms_fold_k<bf16>", "adarms_fold_k<float>"}   # second launches (checked per case above)
    assert set(names) - reached == set()
    assert reached - set(names) == set()
    # the table is the planner's, not a copy of it: every case's kernel comes back from dxa_norm_plan (test_*_route above)
    assert len(names) == 103


def _vp(a):
    return C.c_void_p(a) if a else None


def test_plan_refuses_what_the_entry_points_refuse():
    """status and dxa_last_error text of dxa_norm_plan and of the entry point itself, on calls refused before any launch"""
    a = 1 << 40
    lib = L.lib
    calls = [
        (dict(entry="rmsnorm_fwd", dtype=1, w_dtype=1, rows=3, cols=0, x=a, y=a),
         lambda: lib.dxa_rmsnorm_fwd(_vp(a), None, _vp(a), None, 3, 0, 1e-5, 1, 1, None)),
        (dict(entry="rmsnorm_fwd", dtype=0, w_dtype=1, rows=3, cols=8, x=a, y=a),
         lambda: lib.dxa_rmsnorm_fwd(_vp(a), None, _vp(a), None, 3, 8, 1e-5, 0, 1, None)),
        (dict(entry="rmsnorm_bwd", dtype=1, w_dtype=1, rows=3, cols=8, x=a, dy=a, dx=a, rstd=a, w=a),
         lambda: lib.dxa_rmsnorm_bwd(_vp(a), _vp(a), _vp(a), _vp(a), _vp(a), None, None, 3, 8, 1, 1, None)),
        (dict(entry="layernorm_bwd", dtype=1, w_dtype=0, rows=3, cols=8, x=a, dy=a, dx=a, rstd=a),
         lambda: lib.dxa_layernorm_bwd(_vp(a), _vp(a), None, None, _vp(a), _vp(a), None, None, 3, 8, 1, 0, None)),
        (dict(entry="add_layernorm_fwd", dtype=1, w_dtype=1, rows=3, cols=8, x=a, y=a),
         lambda: lib.dxa_add_layernorm_fwd(_vp(a), None, None, None, _vp(a), None, None, 3, 8, 1e-5, 1, 1, None)),
        (dict(entry="add_layernorm_bwd", dtype=1, w_dtype=1, rows=-1, cols=8, x=a, x2=a, dy=a, dx=a, mean=a, rstd=a),
         lambda: lib.dxa_add_layernorm_bwd(_vp(a), _vp(a), _vp(a), None, _vp(a), _vp(a), _vp(a), None, -1, 8, 1, 1, None)),
        (dict(entry="colsum", dtype=0, rows=100, cols=8, ld=8, x=a, y=a, partial=a, partial_bytes=4 * 8 * 3),
         lambda: lib.dxa_colsum(_vp(a), 8, _vp(a), 100, 8, 0, 0, _vp(a), 4 * 8 * 3, None)),
        (dict(entry="colsum", dtype=0, rows=10, cols=8, ld=7, x=a, y=a, partial=a, partial_bytes=1 << 20),
         lambda: lib.dxa_colsum(_vp(a), 7, _vp(a), 10, 8, 0, 0, _vp(a), 1 << 20, None)),
        (dict(entry="colsum", dtype=5, rows=10, cols=8, ld=8, x=a, y=a, partial=a, partial_bytes=1 << 20),
         lambda: lib.dxa_colsum(_vp(a), 8, _vp(a), 10, 8, 5, 0, _vp(a), 1 << 20, None)),
    ]
    for fields, call in calls:
        entry = fields.pop("entry")
        d = L.NormDesc()
        d.entry = L.NORM_ENTRIES.index(entry)
        for k, v in fields.items():
            setattr(d, k, v)
        info = L.NormPlanInfo()
        rc_plan = lib.dxa_norm_plan(C.byref(d), C.byref(info))
        msg_plan = L.last_error()
        rc_call = call()
        msg_call = L.last_error()
        assert rc_plan != 0 and (rc_plan, msg_plan) == (rc_call, msg_call), (entry, msg_plan, msg_call)
    assert lib.dxa_norm_plan(None, C.byref(L.NormPlanInfo())) == -1 and "null desc" in L.last_error()
    d = L.NormDesc()
    d.entry = 99
    assert lib.dxa_norm_plan(C.byref(d), C.byref(L.NormPlanInfo())) == -1 and "unknown entry" in L.last_error()
    assert lib.dxa_norm_plan(C.byref(d), None) == -1 and "null output" in L.last_error()


def test_zero_rows_plan_no_launch():
    for e in ("rmsnorm_fwd", "layernorm_bwd"):
        p = K.norm_plan(e, dtype=1, w_dtype=1, rows=0, cols=8, x=1 << 40, y=1 << 40, dy=1 << 40, dx=1 << 40, mean=1 << 40,
                        rstd=1 << 40)
        assert p["kernel"] is None and p["trips"] == 0
