"""tests/attn_ref.py pinned down without a GPU: the fp64 reference against torch's own attention, its dead-row convention and
its gradient; the condition that makes the mask-edge inputs worth running (a bound moved by one key moves o far beyond the bf16
tolerance, which N(0,1) inputs do not); and the route dxa_attn_plan gives every case of the GPU sweep."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from . import attn_ref as R

IDS = [c.name for c in R.CASES]


@pytest.fixture(scope="module")
def edge():
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = R.edge_inputs(case)
        return cache[case.name]
    return get


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[3], R.CASES[4], R.CASES[6], R.CASES[9]], ids=lambda c: c.name)
def test_reference_matches_torch_sdpa_on_live_rows(case, edge):
    q, k, v, _ = (t.double() for t in edge(case))
    vis = case.vis()
    o, lse = R.attention_ref(q, k, v, vis, case.scale)
    G = case.Hq // case.Hkv
    live = vis.any(-1)
    mask = vis | ~live[..., None]                    # torch gives NaN on a row without keys: open those rows, compare the others
    want = F.scaled_dot_product_attention(q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), attn_mask=mask[:, None],
                                          scale=case.scale)
    rows = live[:, None].expand(-1, case.Hq, -1)
    assert rows.any() and torch.allclose(o[rows], want[rows], rtol=1e-12, atol=1e-12)
    s = (q @ k.repeat_interleave(G, 1).transpose(-1, -2) * case.scale).masked_fill(~mask[:, None], float("-inf"))
    assert torch.allclose(lse[rows], torch.logsumexp(s, -1)[rows], rtol=1e-12, atol=1e-12)


def test_visibility_is_the_written_rule():
    """every clause by brute force at a shape small enough to loop over"""
    B, Sq, Sk = 2, 5, 7
    kv_start, kv_end = [0, 2], [7, 6]
    q_limit = torch.tensor([[1, 2, 7, 7, 0], [7, 7, 3, 5, 6]])
    key_valid = torch.ones(B, Sk, dtype=torch.uint8)
    key_valid[1, 4] = 0
    for causal in (False, True):
        vis = R.visibility(B, Sq, Sk, causal, kv_start, kv_end, q_limit, key_valid)
        for b in range(B):
            for i in range(Sq):
                for j in range(Sk):
                    want = kv_start[b] <= j < min(kv_end[b], int(q_limit[b, i])) and bool(key_valid[b, j]) and \
                        (not causal or j <= i + (Sk - Sq))
                    assert bool(vis[b, i, j]) == want, (causal, b, i, j)


def test_dead_rows_give_zero_output_zero_lse_and_no_gradient():
    case = R.CASES[5]                                # causal with Sq > Sk: the first 130 queries see nothing
    q, k, v, do = (t.double() for t in R.edge_inputs(case))
    q.requires_grad_(True)
    vis = case.vis()
    dead = ~vis.any(-1)
    assert int(dead.sum()) == 130
    o, lse = R.attention_ref(q, k, v, vis, case.scale)
    rows = dead[:, None].expand(-1, case.Hq, -1)
    assert torch.all(o[rows] == 0) and torch.all(lse[rows] == 0)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    o.backward(do)
    assert torch.isfinite(q.grad).all() and torch.all(q.grad[rows] == 0)


def test_reference_gradcheck():
    torch.manual_seed(3)
    B, Hq, Hkv, Sq, Sk, D = 2, 4, 2, 3, 5, 4
    q, k, v = (torch.randn(*s, dtype=torch.float64, requires_grad=True) for s in ((B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D)))
    key_valid = torch.ones(B, Sk, dtype=torch.uint8)
    key_valid[0, 1] = 0
    vis = R.visibility(B, Sq, Sk, True, [0, 1], [5, 4], torch.tensor([[5, 5, 5], [0, 5, 5]]), key_valid)
    assert (~vis.any(-1)).any() and vis.any()
    assert torch.autograd.gradcheck(lambda a, b, c: R.attention_ref(a, b, c, vis, 0.5), (q, k, v))


def test_bf16_emulation_is_the_reference_plus_bf16_rounding():
    """attention_ref_bf16 on a small case: off the fp64 reference by bf16 rounding (not zero, not more than the project's bf16
    bounds, which this case holds with room), zero where the reference is zero"""
    case = R.CASES[3]
    q, k, v, do = R.edge_inputs(case)
    vis = case.vis()
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o, _ = R.attention_ref(qr, kr, vr, vis, case.scale)
    o.backward(do.double())
    emu = R.attention_ref_bf16(q, k, v, do, vis, case.scale)
    for name, ref, rtol, atol in (("o", o.detach(), 1 / 64, 2e-2), ("dq", qr.grad, 1 / 32, 6e-2), ("dk", kr.grad, 1 / 32, 1.2e-1),
                                  ("dv", vr.grad, 1 / 32, 1.2e-1)):
        err = (emu[name] - ref).abs()
        assert 0 < float(err.max()) and bool((err <= 0.5 * (atol + rtol * ref.abs())).all()), name
        assert torch.all(emu[name][ref == 0] == 0), name
    unseen = ~vis.any(1)
    assert unseen.any() and torch.all(emu["dk"][unseen[:, None].expand(-1, case.Hkv, -1)] == 0)


@pytest.mark.parametrize("case", [c for c in R.CASES if c.emulated], ids=lambda c: c.name)
def test_emulated_bounds_are_needed_where_a_case_takes_them(case, edge):
    """Case.emulated names an output only where bf16 rounding alone (attention_ref_bf16, no kernel) misses the project's bound"""
    q, k, v, do = edge(case)
    vis = case.vis()
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o, _ = R.attention_ref(qr, kr, vr, vis, case.scale)
    o.backward(do.double())
    emu = R.attention_ref_bf16(q, k, v, do, vis, case.scale)
    for name, ref, rtol, atol in (("o", o.detach(), 1 / 64, 2e-2), ("dq", qr.grad, 1 / 32, 6e-2), ("dk", kr.grad, 1 / 32, 1.2e-1),
                                  ("dv", vr.grad, 1 / 32, 1.2e-1)):
        ratio = float(((emu[name] - ref).abs() / (atol + rtol * ref.abs())).max())
        print(f"{case.name}: {name}: emulation max err {float((emu[name] - ref).abs().max()):.4f}, {ratio:.3f} x the bound")
        assert (ratio > 1) == (name in case.emulated), (name, ratio)


# ------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_edge_inputs_make_every_moved_bound_visible(case, edge):
    """The sensitivity condition: for every bound of the case's mask moved by one key, at least half of the (b, i) rows whose
    mask changed move in o, reference against reference, by more than 0.08 (4 x the bf16 atol) in some column.  A condition on
    the inputs: with it, a kernel that is off by one at that bound cannot stay inside the tolerance of the GPU sweep."""
    inputs = edge(case)
    assert max(float(t.abs().max()) for t in inputs) < 16
    seen = 0
    for name, vis_p in R.perturbations(case):
        affected, moved = R.sensitivity(case, inputs, vis_p)
        print(f"{case.name}: {name}: {moved}/{affected}")
        assert affected > 0, f"{name} changes no row of this case's mask"
        assert 2 * moved >= affected, f"{name}: only {moved} of {affected} affected rows move by 0.08"
        seen += 1
    assert seen >= 2


def test_normal_inputs_do_not_make_a_moved_bound_visible():
    """why the edge inputs exist: on N(0,1) inputs (what tests/test_kernels_gpu.py draws) the same condition fails at case 1"""
    case = R.CASES[0]
    inputs = R.normal_inputs(case)
    failed = []
    for name, vis_p in R.perturbations(case):
        affected, moved = R.sensitivity(case, inputs, vis_p)
        if 2 * moved < affected:
            failed.append(name)
    assert "kv_end-1" in failed and "kv_end+1" in failed, failed


# ------------------------------------------------------------------------------------------------ the routes
def _lib():
    try:
        from dexbotic_amd import _lib as L
    except ImportError:
        pytest.skip("libdexbotic_amd.so is not built")
    return L


def plan_desc(L, case, dtype="bf16", force_generic=0, base=1 << 20, v_off=0):
    """descriptor of the case in head-major contiguous tensors at made-up aligned addresses (dxa_attn_plan dereferences nothing)"""
    c = case
    d = L.AttnDesc()
    d.dtype = L.BF16 if dtype == "bf16" else L.F32
    d.B, d.Hq, d.Hkv, d.Sq, d.Sk, d.D, d.causal, d.scale = c.B, c.Hq, c.Hkv, c.Sq, c.Sk, c.D, int(c.causal), c.scale
    d.force_generic = force_generic
    for i, (name, H, S) in enumerate((("q", c.Hq, c.Sq), ("k", c.Hkv, c.Sk), ("v", c.Hkv, c.Sk), ("o", c.Hq, c.Sq), ("d_o", c.Hq, c.Sq),
                                      ("dq", c.Hq, c.Sq), ("dk", c.Hkv, c.Sk), ("dv", c.Hkv, c.Sk))):
        setattr(d, name, base * (i + 1) * 64 + (v_off if name == "v" else 0))
        pre = "do" if name == "d_o" else name
        setattr(d, pre + "_sb", H * S * c.D)
        setattr(d, pre + "_sh", S * c.D)
        setattr(d, pre + "_ss", c.D)
    d.lse = base * 1024
    m = case.masks()
    for i, key in enumerate(("kv_start", "kv_end", "q_limit", "key_valid")):
        setattr(d, key, base * (2048 + i) if m[key] is not None else None)
    return d


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_case_plans_the_route_it_names(case):
    L = _lib()
    R.check_route(L, case, plan_desc(L, case))
    # a V that is 8-byte but not 16-byte aligned: the forward with V transposed through registers, everything else the same
    d8 = plan_desc(L, case, v_off=8)
    R.check_route(L, case, d8, fwd_family="flash", backward=False)
    assert R.plan(L, d8, True).family.decode() == "composed"            # (the fused backward loads V rows 16 bytes at a time)
    if case.fp32_generic:
        R.check_route_fp32_generic(L, case, plan_desc(L, case, dtype="f32", force_generic=1))


def test_the_sweep_reaches_every_flash_route():
    """the routes the issue lists, each named by at least one case: a threshold moved in the library changes a case's plan and
    fails the test above; a case dropped from the list fails here"""
    routes = {(c.tile or c.D, c.D, c.nw, c.nw_dkv, c.pf, c.nsplit > 1) for c in R.CASES}
    for want in ((128, 128, 4, 8, 1, False), (256, 256, 4, 8, 0, False), (256, 256, 8, 8, 0, False), (64, 64, 4, 4, 1, False),
                 (128, 72, 8, 4, 1, False), (128, 72, 4, 4, 1, False), (256, 256, 4, 8, 0, True)):
        assert want in routes, want
    assert sum(c.fp32_generic for c in R.CASES) == 5


def test_plan_checks_its_arguments_like_the_entry_points():
    L = _lib()
    info = L.AttnPlanInfo()
    assert L.lib.dxa_attn_plan(None, 0, C.byref(info)) == -1 and "null desc" in L.last_error()
    d = plan_desc(L, R.CASES[0])
    assert L.lib.dxa_attn_plan(C.byref(d), 0, None) == -1 and "null output" in L.last_error()
    d.dq = None
    assert L.lib.dxa_attn_plan(C.byref(d), 0, C.byref(info)) == 0
    assert L.lib.dxa_attn_plan(C.byref(d), 1, C.byref(info)) == -1 and "null gradient" in L.last_error()
    d = plan_desc(L, R.CASES[0])
    d.Hkv = 3
    assert L.lib.dxa_attn_plan(C.byref(d), 0, C.byref(info)) == -1 and "bad shape" in L.last_error()
