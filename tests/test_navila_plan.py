"""NaVILA's per-sample splice rule on the host (no GPU): ``build_navila_splice_plan`` against the reference's spliced labels /
mask (tests/golden/navila_t1.npz) and against the rule as dexbotic/model/navila/navila_arch.py states it."""
import os

import numpy as np

from dexbotic_amd.constants import IGNORE_INDEX, IMAGE_TOKEN_INDEX
from dexbotic_amd.splice import PLAN_PAD, PlanCache, build_navila_splice_plan, build_splice_plan

IMG = IMAGE_TOKEN_INDEX


def feature_rows(plan_row):
    """feature-row indices a plan row reads, in order"""
    return [int(-1 - v) for v in plan_row if v != PLAN_PAD and v < 0]


def test_planner_reproduces_reference_labels_and_mask(golden_dir):
    g = np.load(os.path.join(golden_dir, "navila_t1.npz"), allow_pickle=False)
    R = 3 * 4                                              # 3 frames x (3x3 grid -> 2x2 merged) tokens
    p = build_navila_splice_plan(g["input_ids"], g["attention_mask"], g["labels"], R, 2)
    assert np.array_equal(p.labels, g["spliced_labels"])
    assert np.array_equal(p.attention_mask, g["spliced_mask"])
    # sample 0: three placeholders, 4 rows each, in order; sample 1: ONE placeholder, its whole 12-row block
    assert feature_rows(p.plan[0]) == list(range(0, 12))
    assert feature_rows(p.plan[1]) == list(range(12, 24))
    pos0 = np.flatnonzero(g["input_ids"][0] == IMG)
    assert list(pos0) == [1, 3, 5]
    assert [int(-1 - v) for v in p.plan[0, 1:5]] == [0, 1, 2, 3] and p.plan[0, 5] == g["input_ids"][0, 2]
    assert [int(-1 - v) for v in p.plan[0, 6:10]] == [4, 5, 6, 7]
    assert list(p.kv_start) == [0, 0] and list(p.kv_end) == [int(m.sum()) for m in g["spliced_mask"]]
    assert list(p.last_index) == [int(m.sum()) - 1 for m in g["spliced_mask"]]


def test_placeholder_to_feature_rows():
    R = 12
    ids = np.array([[5, IMG, 6, IMG, 7, 8, 9],            # two placeholders: 6 rows each
                    [5, 6, 7, 8, 9, 10, 11],              # none: no rows
                    [IMG, 5, 6, 7, 0, 0, 0],              # one: all 12 (three padded ids masked out)
                    [5, IMG, IMG, IMG, IMG, IMG, 6]])     # five: 12 // 5 = 2 rows each, the last two rows unused
    mask = np.ones_like(ids, dtype=bool)
    mask[2, 4:] = False
    labels = np.where(ids == IMG, IGNORE_INDEX, ids)
    p = build_navila_splice_plan(ids, mask, labels, R, 4)
    assert feature_rows(p.plan[0]) == list(range(0, 12)) and list(p.plan[0, :2]) == [5, -1]
    assert int(p.plan[0, 7]) == 6 and int(p.plan[0, 8]) == -1 - 6
    assert feature_rows(p.plan[1]) == [] and list(p.plan[1, :7]) == list(ids[1])
    assert feature_rows(p.plan[2]) == list(range(24, 36))
    assert feature_rows(p.plan[3]) == list(range(36, 46))
    assert list(p.lengths) == [5 + 12, 7, 3 + 12, 2 + 10]
    # labels: IGNORE_INDEX on image rows and padding, the text labels elsewhere
    assert all(p.labels[0][p.plan[0] < 0] == IGNORE_INDEX) and p.labels[0, 0] == 5 and p.labels[0, 7] == 6
    assert not p.attention_mask[1, 7:].any() and p.attention_mask[1, :7].all()
    # the batch index is clamped to the last feature sample (navila_arch.py:161)
    q = build_navila_splice_plan(ids, mask, labels, R, 3)
    assert feature_rows(q.plan[2]) == list(range(24, 36)) and feature_rows(q.plan[3]) == list(range(24, 34))


def test_left_padding_and_truncation_through_an_image_block():
    R = 8
    ids = np.array([[5, IMG, 6, 7], [5, 6, 7, 8]])
    p = build_navila_splice_plan(ids, None, ids.copy(), R, 2, max_length=6, padding_side="left")
    # sample 0 = [5, r0..r7, 6, 7] cut to 6 positions: the token and the first five rows of the block
    assert list(p.plan[0]) == [5, -1, -2, -3, -4, -5]
    assert list(p.plan[1]) == [PLAN_PAD, PLAN_PAD, 5, 6, 7, 8]
    assert list(p.kv_start) == [0, 2] and list(p.kv_end) == [6, 6]
    assert list(p.attention_mask[1]) == [False, False, True, True, True, True]
    assert list(p.labels[1]) == [IGNORE_INDEX, IGNORE_INDEX, 5, 6, 7, 8] and list(p.labels[0]) == [5] + [IGNORE_INDEX] * 5
    assert list(p.last_index) == [5, 5]
    r = build_navila_splice_plan(ids, None, None, R, 2, padding_side="right")
    assert list(r.plan[1]) == [5, 6, 7, 8] + [PLAN_PAD] * 7 and list(r.last_index) == [10, 3]


def test_plan_cache_keys_on_the_rule():
    ids = np.array([[5, IMG, 6, IMG, 7]])
    cache = PlanCache()
    base = cache.get(ids, None, None, 4, None, "right")
    nav = cache.get(ids, None, None, 4, None, "right", rule="navila", n_feature_samples=1)
    assert base is not nav
    assert np.array_equal(base.plan, build_splice_plan(ids, None, None, 4).plan)
    assert np.array_equal(nav.plan, build_navila_splice_plan(ids, None, None, 4, 1).plan)
    assert feature_rows(base.plan[0]) == list(range(8)) and feature_rows(nav.plan[0]) == list(range(4))
    assert cache.get(ids, None, None, 4, None, "right") is base
    assert cache.get(ids, None, None, 4, None, "right", rule="navila", n_feature_samples=1) is nav
