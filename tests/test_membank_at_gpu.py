"""The slot-indexed memory-bank kernels on the GPU (csrc/memvla.hip: dxa_bank_stage_fwd_at, dxa_bank_append_at,
dxa_bank_consolidate_batched_at): a call on rows ``slot_ids`` of a bank of S slots is bit-equal to the existing kernel run on the
gathered [R, cap, N, D] copy of those slots, with the result scattered back; the slots it does not name are not touched."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(5, 4, 1, 64), (5, 4, 16, 48), (3, 3, 64, 256)]          # (S, cap, N, D)
SENTINEL_F, SENTINEL_T = -77.5, -3.25                              # exactly representable in bf16


def _row_sets(S):
    """a strict subset, a permuted set, a single row, all slots"""
    if S == 5:
        return {"subset": [1, 3], "permuted": [3, 0, 4], "single": [2], "all": [0, 1, 2, 3, 4]}
    return {"subset": [0, 2], "permuted": [2, 0], "single": [1], "all": [0, 1, 2], "all-permuted": [1, 2, 0]}


def _bank(S, cap, N, D, dtype, rows, seed):
    """random content in the named slots, the sentinel pattern in the others"""
    gen = torch.Generator().manual_seed(seed)
    feat = torch.randn((S, cap, N, D), generator=gen).to(DEV, dtype)
    ts = (torch.rand((S, cap), generator=gen) * 50).to(DEV)
    idle = [s for s in range(S) if s not in rows]
    feat[idle], ts[idle] = SENTINEL_F, SENTINEL_T
    # a planted tie in the first named slot (entries 0 = 1 = 2 where the bank is that long) and a zero token (the eps path)
    feat[rows[0], 1] = feat[rows[0], 0]
    if cap > 3:
        feat[rows[0], 2] = feat[rows[0], 0]
    feat[rows[-1], 1, N - 1] = 0
    return feat, ts, idle


def _idle_untouched(feat, ts, idle):
    return bool((feat[idle] == SENTINEL_F).all()) and bool((ts[idle] == SENTINEL_T).all())


@pytest.mark.parametrize("fifo", [False, True], ids=["tome", "fifo"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_at_kernels_equal_the_existing_kernels_on_the_gathered_slots(shape, dtype, fifo):
    """one step of the bank — stage, append, consolidation — through the _at kernels and through the existing kernels on the
    gathered copy; counts cover 0, 1, mem_length - 1 and mem_length on every row of every row set"""
    from dexbotic_amd import kernels as K
    S, cap, N, D = shape
    ml = cap - 1
    vals = (0, ml, 1, ml - 1)
    for name, rows in _row_sets(S).items():
        R = len(rows)
        for rot in range(4):
            cnt = [vals[(r + rot) % 4] for r in range(R)]
            what = (name, cnt)
            feat, ts, idle = _bank(S, cap, N, D, dtype, rows, 11 + rot)
            gen = torch.Generator().manual_seed(5 + rot)
            tokens = torch.randn((R, N, D), generator=gen).to(DEV, dtype)
            steps = (torch.rand(R, generator=gen) * 9).to(DEV)
            ids = torch.tensor(K.distinct_slots(rows, S), dtype=torch.int32, device=DEV)
            counts = torch.tensor(cnt, dtype=torch.int32, device=DEV)
            g_feat, g_ts = feat[rows].contiguous(), ts[rows].contiguous()          # the gathered copy
            feat0, ts0 = feat.clone(), ts.clone()
            # stage: reads only
            got = K.bank_stage_fwd_at(feat, ts, ids, counts, tokens, steps)
            want = K.bank_stage_fwd(g_feat, g_ts, counts, tokens, steps)
            for a, b in zip(got, want):
                assert a.shape == b.shape and torch.equal(a, b), what
            assert torch.equal(feat, feat0) and torch.equal(ts, ts0), what
            # append
            K.bank_append_at(feat, ts, ids, counts, tokens, steps)
            K.bank_append(g_feat, g_ts, counts, tokens, steps)
            want_f, want_t = feat0.clone(), ts0.clone()
            want_f[rows], want_t[rows] = g_feat, g_ts
            assert torch.equal(feat, want_f) and torch.equal(ts, want_t), what
            assert _idle_untouched(feat, ts, idle), what
            # consolidation of the rows the append took over mem_length
            sims_at = torch.full((R * (cap - 1),), 9.0, device=DEV)
            sims = torch.full((R * (cap - 1),), 9.0, device=DEV)
            K.bank_consolidate_batched_at(feat, ts, ids, counts, 1, ml, None if fifo else sims_at, fifo=fifo)
            K.bank_consolidate_batched(g_feat, g_ts, counts, 1, ml, None if fifo else sims, fifo=fifo)
            want_f[rows], want_t[rows] = g_feat, g_ts
            assert torch.equal(feat, want_f) and torch.equal(ts, want_t), what
            assert torch.equal(sims_at, sims), what                                  # the scratch is indexed by the row
            assert _idle_untouched(feat, ts, idle), what
            if fifo:                               # the consolidation did fire: a full row's oldest entry is gone
                for r, s in enumerate(rows):
                    if cnt[r] == ml:
                        assert torch.equal(feat[s, 0], feat0[s, 1]) and torch.equal(feat[s, ml - 1], tokens[r]), what


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_an_id_outside_the_bank_makes_its_row_a_no_op(shape, dtype):
    from dexbotic_amd import kernels as K
    S, cap, N, D = shape
    ml = cap - 1
    gen = torch.Generator().manual_seed(3)
    feat = torch.randn((S, cap, N, D), generator=gen).to(DEV, dtype)
    ts = (torch.rand((S, cap), generator=gen) * 50).to(DEV)
    for bad in ([S, -1], [-7], [2 ** 31 - 1, S + 3, -(2 ** 31)]):
        R = len(bad)
        tokens = torch.randn((R, N, D), generator=gen).to(DEV, dtype)
        steps = (torch.rand(R, generator=gen) * 9).to(DEV)
        ids = torch.tensor(bad, dtype=torch.int32, device=DEV)
        counts = torch.full((R,), ml, dtype=torch.int32, device=DEV)
        f2, t2 = feat.clone(), ts.clone()
        mem, ts_eff, kv_len = K.bank_stage_fwd_at(f2, t2, ids, counts, tokens, steps)
        want_mem, want_ts = torch.zeros_like(mem), torch.zeros_like(ts_eff)
        want_mem[:, 0], want_ts[:, 0] = tokens, steps                                  # as a slot without history
        assert torch.equal(mem, want_mem) and torch.equal(ts_eff, want_ts) and kv_len.tolist() == [N] * R, bad
        K.bank_append_at(f2, t2, ids, torch.zeros_like(counts), tokens, steps)
        for fifo in (False, True):
            K.bank_consolidate_batched_at(f2, t2, ids, counts, 1, ml, torch.empty(R * (cap - 1), device=DEV), fifo=fifo)
        assert torch.equal(f2, feat) and torch.equal(t2, ts), bad
    # one bad row between two good ones: the good rows work, the bad one does nothing
    rows, good = [1, S + 2, 0], [1, 0]
    tokens = torch.randn((3, N, D), generator=gen).to(DEV, dtype)
    steps = (torch.rand(3, generator=gen) * 9).to(DEV)
    counts = torch.tensor([1, 1, ml], dtype=torch.int32, device=DEV)
    f2, t2 = feat.clone(), ts.clone()
    K.bank_append_at(f2, t2, torch.tensor(rows, dtype=torch.int32, device=DEV), counts, tokens, steps)
    want_f, want_t = feat.clone(), ts.clone()
    want_f[1, 1], want_t[1, 1] = tokens[0], steps[0]
    want_f[0, ml], want_t[0, ml] = tokens[2], steps[2]
    assert torch.equal(f2, want_f) and torch.equal(t2, want_t)


def test_a_duplicate_slot_in_the_host_list_raises():
    from dexbotic_amd import kernels as K
    for bad in ([3, 0, 3], [1, 1]):
        with pytest.raises(ValueError, match="duplicate"):
            K.distinct_slots(bad, 5)
    with pytest.raises(ValueError):
        K.distinct_slots([0, 5], 5)
