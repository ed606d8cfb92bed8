"""The cases of the flow-serving fixture (tests/golden/flow_serve_t1.npz), stated once: ``make_inputs`` draws the inputs,
``run_transforms`` / ``run_tokenizers`` drive a namespace of transform / tokeniser classes over them and return every result as a
flat {name: array} dict.  scripts/gen_golden_flow_serve.py runs them over the REFERENCE's classes and stores inputs and results;
tests/test_flow_serve_ref.py runs them over the native classes on the stored inputs and compares name by name, values and dtypes.

Transform cases, for mean / std ("ms") and quantile ("q") statistics alike: a state of 8 numbers (2-D, 1-D, and the float32 zeros of
a request without states) padded to 32 and normalised with 32-wide statistics; a 32-wide chunk de-normalised with action statistics
of 7 entries, twice with the same mapping (the padding the first call leaves in the mapping serves the second; the mapping after
both is recorded), each followed by AbsoluteAction with non_delta_mask [6]; an action of the state's rank; periodic components with
the default range and a given one; PadAction; ToNumpy on nested lists."""
from __future__ import annotations

import numpy as np

from .flow_serve_tokenizers import dm0_tokenizer, pi0_tokenizer

SEED = 61
WIDTH, STATE_DIM, ACTION_STATS, CHUNK = 32, 8, 7, 6
PI0_MAX_LEN, DM0_MAX_LEN, DM0_SHORT_LEN = 12, 48, 20
PROMPTS = ("pick up the red_block\nand place it",
           "   open the drawer  ",
           "put_the_cup_on_the_plate then push the plate to the left side of the table and come back to the start now please",
           "stack")
STAT_KEYS = {"ms": ("mean", "std"), "q": ("min", "max")}


def make_inputs(seed: int = SEED) -> dict:
    rs = np.random.RandomState(seed)
    u = rs.uniform
    d = {"stats/ms/state/mean": u(-0.5, 0.5, WIDTH), "stats/ms/state/std": u(0.2, 1.5, WIDTH),
         "stats/ms/action/mean": u(-0.5, 0.5, ACTION_STATS), "stats/ms/action/std": u(0.2, 1.5, ACTION_STATS),
         "stats/q/state/min": -u(0.5, 2.0, WIDTH), "stats/q/state/max": u(0.5, 2.0, WIDTH),
         "stats/q/action/min": -u(0.5, 2.0, ACTION_STATS), "stats/q/action/max": u(0.5, 2.0, ACTION_STATS),
         "state2d": u(-1, 1, (2, STATE_DIM)), "state1d": u(-1, 1, STATE_DIM),
         "chunk1": rs.standard_normal((2, CHUNK, WIDTH)).astype(np.float32),
         "chunk2": rs.standard_normal((2, CHUNK, WIDTH)).astype(np.float32),
         "flat": rs.standard_normal((2, WIDTH)).astype(np.float32),
         "periodic_state": u(-3, 3, (2, WIDTH)), "periodic_action": u(-3, 3, (2, CHUNK, WIDTH)),
         "act7": u(-1, 1, (3, ACTION_STATS))}
    return d


def statistics(d: dict, mode: str) -> dict:
    """a fresh mapping {"state": {...}, "action": {...}} of float64 arrays (the transforms pad it in place)"""
    return {key: {n: np.array(d[f"stats/{mode}/{key}/{n}"], dtype=np.float64) for n in STAT_KEYS[mode]} for key in ("state", "action")}


def run_transforms(T, d: dict) -> dict:
    """``T``: anything with PadState, PadAction, ActionNorm, ActionDenorm, AbsoluteAction, ToNumpy, ToTensor, Pipeline"""
    out = {}
    meta = lambda **kw: {"meta_data": dict(non_delta_mask=np.array([6]), **kw)}
    for mode, uq in (("ms", False), ("q", True)):
        st = statistics(d, mode)
        inp = T.Pipeline([T.PadState(ndim=WIDTH, axis=-1), T.ActionNorm(statistic_mapping=st, strict=False, use_quantiles=uq),
                          T.ToTensor()])
        outp = T.Pipeline([T.ToNumpy(), T.ActionDenorm(statistic_mapping=st, strict=False, use_quantiles=uq), T.AbsoluteAction()])
        assert inp.statistic_mapping is st and outp.statistic_mapping is st
        for name, s in (("2d", d["state2d"]), ("1d", d["state1d"]), ("absent", np.zeros((2, WIDTH), dtype=np.float32))):
            r = inp({"state": np.array(s), **meta()})
            out[f"{mode}/in_{name}/state"] = r["state"].numpy()
            out[f"{mode}/in_{name}/non_delta_mask"] = r["meta_data"]["non_delta_mask"].numpy()
        normed = out[f"{mode}/in_2d/state"]
        for i in (1, 2):
            r = outp({"state": normed.copy(), "action": d[f"chunk{i}"].copy(), **meta()})
            out[f"{mode}/out{i}/action"], out[f"{mode}/out{i}/state"] = r["action"], r["state"]
            assert r["abs_action"] is r["action"]
        r = outp({"state": normed.copy(), "action": d["flat"].copy(), **meta()})
        out[f"{mode}/out_same_rank/action"] = r["action"]
        for key in st:
            for n in STAT_KEYS[mode]:
                out[f"{mode}/stats_after/{key}/{n}"] = st[key][n]
    for name, kw in (("default", {}), ("range2", {"periodic_range": 2.0})):
        r = T.AbsoluteAction()({"state": d["periodic_state"].copy(), "action": d["periodic_action"].copy(),
                                **meta(periodic_mask=[3, 4, 5], **kw)})
        out[f"periodic/{name}/action"] = r["action"]
    r = T.AbsoluteAction()({"state": d["periodic_state"].copy(), "action": d["periodic_action"].copy(), "meta_data": {}})
    out["no_mask_given/action"] = r["action"]
    out["pad_action/action"] = T.PadAction(ndim=WIDTH, axis=-1)({"action": d["act7"].copy()})["action"]
    out["pad_action/wide"] = T.PadAction(ndim=4, axis=-1)({"action": d["act7"].copy()})["action"]
    r = T.ToNumpy()({"a": [1, 2, 3], "b": [[1.5, 2.0], [3.0, 4.0]], "c": "text", "d": 5, "e": {"f": [0.25]}, "g": ["x", 1]})
    assert r["c"] == "text" and isinstance(r["g"], list)
    out.update({"tonumpy/a": r["a"], "tonumpy/b": r["b"], "tonumpy/d": r["d"], "tonumpy/e_f": r["e"]["f"]})
    return out


def run_tokenizers(P) -> dict:
    """``P``: anything with Pi0Tokenization and DM0Tokenization"""
    out = {}
    pi0 = P.Pi0Tokenization(pi0_tokenizer(PI0_MAX_LEN))
    for i, p in enumerate(PROMPTS):
        for k, v in pi0([{"value": p}]).items():
            out[f"tok/pi0/{i}/{k}"] = v
    dm0 = P.DM0Tokenization(dm0_tokenizer(DM0_MAX_LEN))
    short = P.DM0Tokenization(dm0_tokenizer(DM0_SHORT_LEN))
    turns = {f"{i}": [{"from": "human", "value": p}] for i, p in enumerate(PROMPTS)}
    turns["empty_gpt"] = [{"from": "human", "value": PROMPTS[0]}, {"from": "gpt", "value": ""}]
    turns["answered"] = [{"from": "human", "value": PROMPTS[1]}, {"from": "gpt", "value": "done\nnow"}]
    turns["unknown_role"] = [{"from": "system", "value": "ignored"}, {"value": PROMPTS[3]}, {"from": "gpt", "value": None}]
    for name, conv in turns.items():
        for tag, tok in (("dm0", dm0), ("dm0_short", short)):
            for k, v in tok([dict(t) for t in conv]).items():
                out[f"tok/{tag}/{name}/{k}"] = v
    return out
