"""build_parallel_stream_batches (dexbotic_amd/exp/mem_trainer.py): the schedule the 'parallel_stream' memory bank expects —
batch slot i is one running episode, one frame per slot per step."""
import random

import pytest

from dexbotic_amd.exp.mem_trainer import build_parallel_stream_batches


def make_index(n_eps=23, seed=5, datasets=2):
    """global_index rows (dataset, file, frame): episodes of 1 .. 9 frames, the rows shuffled so that sample order is no help"""
    rng = random.Random(seed)
    rows = []
    for e in range(n_eps):
        for f in range(rng.randint(1, 9)):
            rows.append((e % datasets, e // datasets, f))
    rng.shuffle(rows)
    return rows


@pytest.mark.parametrize("B", [1, 3, 4])
def test_slots_walk_their_episodes_frame_by_frame(B):
    gi = make_index()
    length = {}
    for d, f, k in gi:
        length[(d, f)] = max(length.get((d, f), 0), k + 1)
    batches = build_parallel_stream_batches(gi, B, seed=42, epoch=0, rank=0, world=1)
    assert batches and all(len(b) == B for b in batches)
    started = set()
    for i in range(B):
        cur, last = None, None
        for b in batches:
            d, f, k = gi[b[i]]
            if (d, f) == cur:
                assert k == last + 1, "frames of a slot are consecutive and never go backwards"
            else:
                # a slot moves on only after the LAST frame of its episode, starts the next at frame 0, and no episode is
                # ever started twice (in this slot or another)
                assert cur is None or last == length[cur] - 1, (cur, last)
                assert k == 0 and (d, f) not in started
                started.add((d, f))
                cur = (d, f)
            last = k
    flat = [g for b in batches for g in b]
    assert len(flat) == len(set(flat))


def test_no_frame_appears_on_two_ranks_and_every_rank_has_work():
    gi = make_index(n_eps=40)
    frame_rank, episode_rank = {}, {}
    for rank in range(4):
        batches = build_parallel_stream_batches(gi, 2, seed=7, epoch=3, rank=rank, world=4)
        assert batches
        for b in batches:
            for g in b:
                assert frame_rank.setdefault(g, rank) == rank, f"sample {g} on ranks {frame_rank[g]} and {rank}"
                assert episode_rank.setdefault(gi[g][:2], rank) == rank, f"episode {gi[g][:2]} on two ranks"


def test_same_seed_and_epoch_give_the_same_batches():
    gi = make_index()
    a = build_parallel_stream_batches(gi, 3, seed=11, epoch=2, rank=1, world=2)
    b = build_parallel_stream_batches(gi, 3, seed=11, epoch=2, rank=1, world=2)
    c = build_parallel_stream_batches(gi, 3, seed=11, epoch=3, rank=1, world=2)
    d = build_parallel_stream_batches(gi, 3, seed=10, epoch=3, rank=1, world=2)      # seed + epoch is what is drawn from
    assert a == b and a != c and a == d


def test_only_full_steps_are_kept():
    gi = [(0, 0, 0), (0, 0, 1), (0, 1, 0)]                       # two episodes, three slots: no step can be filled
    assert build_parallel_stream_batches(gi, 3, seed=0, epoch=0, rank=0, world=1) == []
    assert len(build_parallel_stream_batches(gi, 2, seed=0, epoch=0, rank=0, world=1)) == 1
    with pytest.raises(ValueError):
        build_parallel_stream_batches(gi, 0, seed=0, epoch=0, rank=0, world=1)


def test_sampler_still_refuses_the_mode():
    from dexbotic_amd.exp.mem_trainer import EpisodeBatchSampler

    class DS:
        global_index = make_index()
    with pytest.raises(NotImplementedError):
        EpisodeBatchSampler(DS(), "parallel_stream", 4, 2)
