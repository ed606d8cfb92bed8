"""CPU checks of the loss-head route table (tests/loss_cases.py): ids are unique, every instantiation the launchers of
csrc/loss.hip can choose (dxa_sample_rows aside) and every reason for leaving the vector routes is named by a case, ``route`` —
the launch predicates in plain Python — gives every case the kernel it names, and the sizes that claim a second or third trip
take one."""
import collections

import pytest

from tests import loss_cases as LC


def test_ids_are_unique():
    n = collections.Counter(c["id"] for c in LC.CASES)
    assert not [i for i, k in n.items() if k > 1]


def test_every_instantiation_is_named():
    assert len(LC.INSTANTIATIONS) == 23
    named = {c["kernel"] for c in LC.CASES}
    assert named == set(LC.INSTANTIATIONS), set(LC.INSTANTIATIONS) ^ named
    # the forward kernels with and without soft ids
    for t in ("f32", "bf16"):
        for v in (4, 1):
            ks = {c["K"] > 0 for c in LC.CASES if c["kernel"] == LC.fk(t, v)}
            assert ks == {False, True}, (t, v, ks)


@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c["id"])
def test_route_gives_the_named_kernel(case):
    assert LC.route(case) == case["kernel"]


def _has(pred):
    return any(pred(c) for c in LC.CASES)


def test_every_fall_off_reason_is_present():
    scalar = lambda c: LC.INSTANTIATIONS[c["kernel"]]["targs"][1] == 1
    for t in ("f32", "bf16"):
        for entries in (LC.FWD, LC.BWD):
            of = lambda c: c["entry"] in entries and c["dtype"] == t
            assert _has(lambda c: of(c) and scalar(c) and c["reason"] == "V%4" and c["V"] % 4)
            assert _has(lambda c: of(c) and scalar(c) and c["reason"] == "ld%4" and c["V"] % 4 == 0 and LC.ld_of(c) % 4)
            assert _has(lambda c: of(c) and scalar(c) and c["reason"] == "mis_logits" and c["V"] % 4 == 0 and LC.ld_of(c) % 4 == 0
                        and c["off"].get("logits", 0) % 4)
        bw = lambda c: c["entry"] in LC.BWD and c["dtype"] == t
        assert _has(lambda c: bw(c) and scalar(c) and c["reason"] == "ldd%4" and c["V"] % 4 == 0 and LC.ld_of(c) % 4 == 0 and LC.ldd_of(c) % 4)
        assert _has(lambda c: bw(c) and scalar(c) and c["reason"] == "mis_dlogits" and not c["off"].get("logits") and c["off"]["dlogits"] % 4)
        assert _has(lambda c: bw(c) and not scalar(c) and LC.ldd_of(c) != LC.ld_of(c))
        assert _has(lambda c: bw(c) and c["dlayout"] == "inplace" and LC.ld_of(c) > c["V"] and not scalar(c))
        assert _has(lambda c: bw(c) and c["dlayout"] == "inplace" and LC.ld_of(c) > c["V"] and scalar(c))
        am = lambda c: c["entry"] == "argmax" and c["dtype"] == t
        for reason in ("V%4", "ld%4", "mis_logits"):
            assert _has(lambda c: am(c) and c["reason"] == reason and c["kernel"] == LC.ak(t, 1)), (t, reason)
        assert _has(lambda c: am(c) and c["layout"] == "ld4" and c["kernel"] == LC.ak(t, 4))
    # bf16 operands 4 elements in stay on the 4-wide route
    for e in ("ce_fwd", "ce_bwd", "soft_fwd", "soft_bwd", "rows_bwd", "argmax"):
        assert _has(lambda c: c["entry"] == e and c["reason"] == "off4" and c["dtype"] == "bf16" and 4 in c["off"].values()
                    and LC.INSTANTIATIONS[c["kernel"]]["targs"][1] == 4), e
    # each way of falling off the wide argmax names the narrow kernel it lands on
    want = {"rows65": lambda c: c["rows"] == 65, "cols16376": lambda c: c["cols"] == 16376, "cols16388": lambda c: c["cols"] == 16388,
            "ld+4": lambda c: LC.ld_of(c) == c["cols"] + 4, "off4": lambda c: c["off"] == {"x": 4} and c["cols"] >= 16384,
            "f32": lambda c: c["dtype"] == "f32" and c["cols"] >= 16384}
    assert set(want) == set(LC.FALL_OFF_WIDE)
    for reason, pred in want.items():
        hit = [c for c in LC.CASES if c["entry"] == "argmax" and c["reason"] == reason and pred(c)]
        assert hit and all(c["kernel"].startswith("argmax_rows_k<") for c in hit), reason
    wide = [c for c in LC.CASES if c["kernel"] == LC.WIDE]
    assert {c["cols"] for c in wide} == {16384, 16392, 24576, 32768, 32776} and {1, 64} <= {c["rows"] for c in wide}


def test_sizes_layouts_values_and_labels_are_present():
    ce = [c for c in LC.CASES if c["entry"] in LC.FWD + LC.BWD]
    vec = lambda c: LC.INSTANTIATIONS[c["kernel"]]["targs"][1] == 4
    assert {c["V"] for c in ce if vec(c)} == {4, 1024, 1028, 2052}
    assert {1, 7, 257, 513} <= {c["V"] for c in ce if not vec(c)}
    assert {c["rows"] for c in ce} == {1, 3, 9} and max(c["V"] for c in ce) == 2052
    fams = {"gauss", "offset+90", "offset-90", "ramp_up", "ramp_down", "peaked", "flat", "masked_head", "masked_sparse", "masked_label",
            "one_nan", "all_masked"}
    for entries in (LC.FWD, LC.BWD):
        for v in (True, False):
            assert fams <= {c["vals"] for c in ce if c["entry"] in entries and vec(c) == v}
    assert all(c["V"] >= (1028 if vec(c) else 257) for c in ce if c["vals"] == "masked_head")
    toks = set().union(*(c["labels"] for c in ce))
    assert {"r", "0", "last", "tail", "ign", "V", "-1", "-7", "soft"} <= toks
    assert _has(lambda c: c["entry"] in LC.FWD and c["ignore_index"] == 3 and "ign" in c["labels"])
    assert _has(lambda c: c["entry"] in LC.BWD and c["labels"] == ("ign",))
    assert {c["K"] for c in ce if c["entry"].startswith("soft")} == {1, 8, 64}
    assert all(set(c["labels"]) >= {"soft", "r", "ign"} for c in ce if c["entry"].startswith("soft"))
    for K in (8, 64):
        ids = LC.soft_ids(K, 1028)
        assert ids != sorted(ids) and {0, 1027, 1026} <= set(ids)
    rw = [c for c in ce if c["row_w"]]
    assert rw and all({"zero", "neg"} <= set(c["row_w"]) for c in rw)
    assert {c["gscale"] is None for c in rw} == {True, False} == {c["gscale"] is None for c in ce if c["entry"] == "ce_bwd"}
    sr = [c for c in LC.CASES if c["entry"] == "sample_reduce"]
    assert {c["L"] for c in sr} == {1, 5, 1024, 1025, 2049} and {c["B"] for c in sr} == {1, 3}
    assert {c["reward"] for c in sr} == {None, "gauss", "big"} and any(c["empty"] for c in sr)
    ex = [c for c in LC.CASES if c["entry"] == "expectile"]
    assert {c["n"] for c in ex} == {1, 1023, 1024, 1025, 2049} and {c["tau"] for c in ex} == {0.1, 0.9} and {c["dpred"] for c in ex} == {True, False}
    d = LC.inputs(next(c for c in ex if c["n"] == 1025))
    diff = d["pred"] - d["target"]
    assert (diff == 0).any() and (diff > 0).any() and (diff < 0).any()
    am = [c for c in LC.CASES if c["entry"] == "argmax" and c["kernel"] != LC.WIDE]
    assert {1, 7, 255, 1024, 1028} <= {c["cols"] for c in am}
    for k in (LC.WIDE, LC.ak("bf16", 4), LC.ak("bf16", 1), LC.ak("f32", 4), LC.ak("f32", 1)):
        assert {"negzero", "all_ninf", "all_nan", "one_nan", "two_nan"} <= {c["special"] for c in LC.CASES if c["kernel"] == k}, k


def test_claimed_trips_are_taken():
    claimed = [c for c in LC.CASES if c["trips"] is not None]
    assert {1, 2, 3} <= {c["trips"] for c in claimed if c["entry"] in LC.FWD} and {1, 2, 3} <= {c["trips"] for c in claimed if c["kernel"] == LC.WIDE}
    for c in claimed:
        assert LC.trips_of(c) == c["trips"], (c["id"], LC.trips_of(c))
    # the wide kernel's placements: a maximum in the unpaired tail, in the second load of a pair, and the pair of equal maxima whose
    # lower index sits in a HIGHER thread's first load against a lower thread's second load
    wide = [c["maxcols"] for c in LC.CASES if c["kernel"] == LC.WIDE and c["maxcols"]]
    assert any(m == (32775,) for m in wide) and any(len(m) == 1 and 8192 <= m[0] < 16384 for m in wide)
    assert any(len(m) == 2 and m[0] < 8192 <= m[1] < 16384 and m[0] // 8 > (m[1] - 8192) // 8 for m in wide)
    assert all(max(c["maxcols"]) < c["cols"] for c in LC.CASES if c.get("maxcols"))
