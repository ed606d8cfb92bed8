"""Every row of dxa_gemm's launcher table, in every mode gemm_plan has for it, on the MI355X against an exact reference: the
cases of tests/gemm_cases.py (test_gemm_cases.py pins their routes and their completeness on the CPU).

Per case: dxa_gemm_plan must give the real descriptor (real addresses, same alignment as the table's symbolic ones) the route
the table states; then dxa_gemm runs it.  Operands are small integers inside NaN-filled allocations (leading dimensions longer
than the extents, guard rows in front and behind, an offset where the case has one), so a load past K, M, N or a leading
dimension that reaches a sum turns it into NaN; outputs (C, aux_out, mirror) lie in sentinel-filled allocations, so a store past
column N, past row M or into the ldc padding damages a sentinel.  Every fp32 sum of the integers is exact, so cases without an
activation (ReLU and its 0 / 1 gradient count as none) are held with torch.equal against the fp64 epilogue rounded once to the
output type; the others with test_kernels_gpu.tol_for(dtype, K), unchanged.  The pre-activation copy is exact in every case.
Extra roundings the reference models because the code documents them: a bf16 C is rounded after the first step of a two-step
route (gemm_plan's K-tail cut says so; the two-step second segment is the same mechanism) — nothing else needed one: a bf16 C
that is accumulated into is read, added in fp32 and rounded once.

A second run into freshly filled buffers, after two differently shaped split-K products on the same stream, must repeat the
first bit for bit: the split-K arrival counters and scratch are left clean."""
import ctypes as C

import pytest
import torch

from tests import gemm_cases as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K
    from tests.test_kernels_gpu import assert_close, tol_for

DEV = "cuda"
CASES = G.cases()
OUTPUTS = ("C", "aux_out", "mirror", "sumsq")


@pytest.fixture(scope="module")
def routes():
    return G.load_routes()


@pytest.fixture(scope="module")
def other_split_products():
    """two split-K products of other shapes (t128 cut in two, skinny bf16 cut in two) to run between a case's two runs"""
    g = torch.Generator(device="cpu").manual_seed(5)
    ops = [tuple(torch.randint(-3, 4, s, generator=g).to(torch.bfloat16).to(DEV) for s in ((M, Kd), (N, Kd)))
           for M, N, Kd in ((300, 1400, 1024), (17, 500, 1024))]
    for (a, b), want in zip(ops, ("t128<bf16>", "skinny_bf16<2,bf16>")):
        out = torch.empty(a.shape[0], b.shape[0], device=DEV, dtype=torch.bfloat16)
        r = G.route_of(L, G.desc_from_tensors("nt", a, b, out))
        assert r["steps"][0]["kernel"] == want and r["steps"][0]["split_s"] == 2, r

    def run():
        for a, b in ops:
            K.mm_nt(a, b)
    return run


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def run_case(f, want_route):
    """build the guarded buffers, check the route of the real descriptor, run dxa_gemm -> (buffers, reference)"""
    bufs = G.make_buffers(f, DEV)
    base = {n: b.ptr() - f[n] for n, b in bufs.items()}
    assert all(p % 256 == 0 for p in base.values())
    real = G.with_pointers(f, base)
    assert G.route_of(L, real) == want_route, "the real descriptor does not get the table's route"
    ref = G.reference(f, want_route, bufs)           # (before the run: an accumulating case overwrites its C)
    before = {n: bufs[n].raw.clone() for n in OUTPUTS if n in bufs}
    d = G.make_desc(L, real)
    L.check(L.lib.dxa_gemm(C.byref(d), K._stream()), "dxa_gemm")
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                        # a faulted device runs nothing more: end the session, keep the evidence
        pytest.exit(f"GPU error in dxa_gemm of {G.route_of(L, real)['steps']}: {e}", returncode=3)
    return bufs, before, ref


def damaged_guards(b, before):
    """'' or where elements of ``b.raw`` outside the operand changed (row, column relative to the operand, in units of its ld)"""
    chk = b.raw.clone()
    chk.as_strided(b.own.shape, b.stride, b.start).copy_(before.as_strided(b.own.shape, b.stride, b.start))
    bad = torch.nonzero(bits(chk) != bits(before)).flatten()
    if bad.numel() == 0:
        return ""
    ld = b.stride[3]
    where = [divmod(int(i) - b.start, ld) for i in bad[:6].tolist()]
    return f"{b.name}: {bad.numel()} guard elements changed, first at (row, col) {where} (ld {ld}, operand {tuple(b.size)})"


def mismatch(what, got, want):
    if torch.equal(got, want):
        return ""
    ne = torch.nonzero(got != want)
    i = tuple(ne[0].tolist())
    rows, cols = sorted(set(ne[:, -2].tolist())), sorted(set(ne[:, -1].tolist()))
    return (f"{what}: {ne.shape[0]} of {got.numel()} elements differ, first at {i}: got {got[i].item()} want {want[i].item()}; "
            f"rows {rows[0]}..{rows[-1]} ({len(rows)}), columns {cols[0]}..{cols[-1]} ({len(cols)})")


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_route_computes_the_exact_product_inside_its_buffers(case, routes, other_split_products):
    f, route = case["fields"], routes[case["id"]]
    bufs, before, ref = run_case(f, route)
    problems = []
    c = bufs["C"].view
    if torch.isnan(c.float()).any():
        problems.append(f"C: {int(torch.isnan(c.float()).sum())} NaN")
    if G.is_exact(f):
        problems.append(mismatch("C", c, ref["C"]))
    else:
        rtol, atol = tol_for(c.dtype, f["K"])
        try:
            assert_close(c, ref["C64"], rtol, atol, "C")
        except AssertionError as e:
            problems.append(str(e))
    if "aux_out" in f:
        problems.append(mismatch("aux_out", bufs["aux_out"].view, ref["aux_out"]))
    if "mirror" in f:
        problems.append(mismatch("mirror", bufs["mirror"].view, c.to(torch.bfloat16)))
    if "sumsq" in f:
        part = bufs["sumsq"].view.flatten()
        if not torch.isfinite(part).all():
            problems.append(f"sumsq: {int((~torch.isfinite(part)).sum())} of {part.numel()} slots not written")
        exact = c.double().pow(2).sum().item()
        if not abs(part.double().sum().item() - exact) <= 1e-5 * exact:
            problems.append(f"sumsq: total {part.double().sum().item()} against {exact}")
    for n in before:
        problems.append(damaged_guards(bufs[n], before[n]))
    problems = [p for p in problems if p]
    assert not problems, f"{case['id']} {route['steps']}: " + " | ".join(problems)
    # the second run, after other split-K products on the stream, into fresh buffers
    other_split_products()
    again, _, _ = run_case(f, route)
    for n in before:
        assert torch.equal(bits(again[n].raw), bits(bufs[n].raw)), f"{case['id']}: {n} differs between two runs"
