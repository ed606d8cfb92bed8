"""The GEMM route table (tests/gemm_cases.py) on the CPU: every case gets exactly the route the table states, the table reaches
every launcher row in every mode gemm_plan has for it, and the operands and references the GPU test (test_gemm_routes_gpu.py)
will use are sane.  dxa_gemm_plan is host arithmetic, so the addresses are fake and no GPU is needed; a route change that
orphans a row or a mode fails here instead of silently losing GPU coverage."""
import collections

import pytest
import torch

from tests import gemm_cases as G

CASES = G.cases()


@pytest.fixture(scope="module")
def L():
    from dexbotic_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def routes():
    return G.load_routes()


def test_ids_are_unique_and_the_routes_on_file_are_the_table_s(routes):
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids)
    assert sorted(routes) == sorted(ids)


def test_every_case_gets_exactly_the_route_the_table_states(L, routes):
    wrong = []
    for c in CASES:
        got = G.route_of(L, G.with_pointers(c["fields"]))
        assert got["rc"] == 0, f"{c['id']}: the planner rejects it ({got}): a table error"
        kernels = tuple(s["kernel"] for s in got["steps"])
        if kernels != c["kernels"] or got != routes[c["id"]]:
            wrong.append((c["id"], c["kernels"], kernels, [(k, routes[c["id"]].get(k), got.get(k)) for k in got if got[k] != routes[c["id"]].get(k)]))
    assert not wrong, f"{len(wrong)} of {len(CASES)} routes differ (id, kernels wanted, got, fields): the first: {wrong[:3]}"


def test_every_launcher_row_is_the_kernel_of_some_case_and_no_case_names_another(L, routes):
    names = G.kernel_names(L)
    assert len(names) == 63 and len(set(names)) == 63
    used = {k for c in CASES for k in c["kernels"]}
    assert used == set(names), (sorted(set(names) - used), sorted(used - set(names)))


def test_every_row_has_its_ragged_split_bias_residual_and_accumulate_cases(L, routes):
    """per launcher row: a ragged case (M, N no multiples of the tile, ldc > N); for kernels that cut K a cut and an uncut case;
    for kernels with the epilogue menu bias + residual with ldr != ldc, and an accumulate case"""
    have = collections.defaultdict(set)
    for c in CASES:
        f, r = c["fields"], routes[c["id"]]
        for i, st in enumerate(r["steps"]):
            if G.family(st["kernel"]) == "gemv" or i == 0:
                k = st["kernel"]
                if G.is_ragged(f, r):
                    have[k].add("ragged")
                have[k].add("cut" if max(st["split_s"], st["ksplit"]) > 1 else "uncut")
                if st["bias"] and st["residual"] and f["ldr"] != f["ldc"]:
                    have[k].add("bias+residual")
                if st["accumulate"]:
                    have[k].add("accumulate")
    missing = {}
    for k in G.kernel_names(L):
        fam = G.family(k)
        need = {"ragged"}
        if fam in G.SPLIT_FAMILIES:
            need |= {"cut", "uncut"}
        if fam == "gemv":
            need |= {"cut"}
        if fam != "gemv" and "swiglu" not in k:
            need |= {"bias+residual", "accumulate"}
        if need - have[k]:
            missing[k] = sorted(need - have[k])
    assert not missing, missing


def test_every_mode_of_every_family_is_reached(L, routes):
    reached = collections.defaultdict(set)
    for c in CASES:
        r = routes[c["id"]]
        for i, s in enumerate(r["steps"]):
            reached[G.family(s["kernel"])] |= G.modes_of(c["fields"], r, i)
    assert set(G.REQUIRED_MODES) == {G.family(k) for k in G.kernel_names(L)}
    missing = {f: sorted(req - reached[f]) for f, req in G.REQUIRED_MODES.items() if req - reached[f]}
    assert not missing, missing
    unlisted = {f: sorted(reached[f] - req) for f, req in G.REQUIRED_MODES.items() if reached[f] - req}
    assert not unlisted, f"modes the table reaches that REQUIRED_MODES does not list: {unlisted}"


def test_the_table_keeps_to_its_size_limits(routes):
    big = [c["id"] for c in CASES if routes[c["id"]]["steps"][0]["full"] + routes[c["id"]]["steps"][0]["tail_r"] > 256]
    assert len(big) <= 3, big
    assert all(routes[i]["steps"][0]["full"] > 0 and routes[i]["steps"][0]["tail_r"] > 0 for i in big)
    deep = [c["id"] for c in CASES if c["fields"]["K"] + c["fields"].get("K2", 0) > 4608]
    assert deep == ["gemv/bb/1/kper_cap"]
    for c in CASES:
        f = c["fields"]
        assert f["alpha"] in (0.5, 1.0, 2.0, G.ALPHA_BF16, G.ALPHA_ACT)
        assert f["ldc"] >= (f["N"] // 2 if f.get("fuse") else f["N"])


def test_inputs_and_references_are_sane(routes):
    """on the CPU, per exact case: the integer reference stays below 2^24 (every fp32 partial sum is exact), no NaN of the padding
    reaches it, and for a bf16 output the rounding point is tested: a nonzero share of elements changes when rounded"""
    unrounded = []
    for c in CASES:
        f, r = c["fields"], routes[c["id"]]
        bufs = G.make_buffers(f, "cpu")
        ref = G.reference(f, r, bufs)
        assert ref["acc"] * max(1.0, f["alpha"]) + 40 + 40 + 100 < 2 ** 24, c["id"]
        assert torch.isfinite(ref["C64"]).all(), c["id"]
        if not G.is_exact(f):
            continue
        assert float(ref["C64"].abs().max()) < 2 ** 24, c["id"]
        assert ref["C64"].abs().max() > 0, c["id"]
        if f["out_dtype"] == G.BF16:
            if not (ref["C"].double() != ref["C64"]).any():
                unrounded.append(c["id"])
        else:
            assert torch.equal(ref["C"].double(), ref["C64"]), c["id"]      # fp32 holds the exact value
    assert not unrounded, f"the bf16 rounding changes no element of {unrounded}"
