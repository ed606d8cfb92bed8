"""The references of tests/optim_mem_ref.py checked on their own (no GPU): Philox4x32-10 against the published Random123
known-answer vectors, the dropout mask's keep rate, and the float64 AdamW against torch.optim.AdamW run in float64."""
import math

import numpy as np
import pytest
import torch

from tests import optim_mem_ref as R

# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, expected)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(counter, key)
    assert tuple(int(x[0]) for x in got) == want


def test_philox_vectorised_equals_scalar():
    """a batch of counters gives, lane by lane, what each counter gives alone (the three vectors above in one call)"""
    cs = [np.array([k[0][i] for k in KAT], dtype=np.uint32) for i in range(4)]
    for lane, (counter, key, _) in enumerate(KAT):
        got = R.philox4x32_10(cs, key)
        one = R.philox4x32_10(counter, key)
        assert all(int(g[lane]) == int(o[0]) for g, o in zip(got, one))


def test_dropout_counter_layout():
    """element i comes from word i % 4 of counter (i // 4, offset) under key seed, both split into 32-bit halves"""
    seed, offset, n = (0x299f31d0 << 32) | 0xa4093822, (0x03707344 << 32) | 0x13198a2e, 4 * 7 + 3
    u = R.dropout_uniforms(n, seed, offset)
    assert u.dtype == np.float32 and u.shape == (n,)
    for i in (0, 5, 14, 30):
        w = R.philox4x32_10((i // 4, 0, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))[i % 4][0]
        assert u[i] == np.float32(int(w) >> 8) * np.float32(2.0 ** -24)
    assert float(u.max()) < 1.0 and float(u.min()) >= 0.0


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_keep_rate(p):
    n = 65536
    keep = R.dropout_keep(n, p, seed=1234, offset=1)
    se = math.sqrt(p * (1 - p) / n)
    assert abs(keep.mean() - (1 - p)) < 4 * se, (keep.mean(), se)
    assert R.dropout_keep(n, 0.0, seed=1234, offset=1).all()
    assert not np.array_equal(keep, R.dropout_keep(n, p, seed=1234, offset=2))


def test_adamw_ref_matches_torch_float64():
    """five steps of two groups: with hyper-parameters that are exact in fp32 the reference is torch's AdamW in float64"""
    rs = np.random.RandomState(0)
    sizes, grp = [37, 300, 5], [0, 1, 0]
    lrs, wds, b1, b2, eps = [2.0 ** -10, 2.0 ** -11], [2.0 ** -6, 0.0], 0.875, 0.96875, 2.0 ** -27
    n = sum(sizes)
    p = rs.standard_normal(n)
    m, v = np.zeros(n), np.zeros(n)
    starts = np.cumsum([0] + sizes[:-1]).tolist()
    params = [torch.tensor(p[s:s + z]).requires_grad_(True) for s, z in zip(starts, sizes)]
    opt = torch.optim.AdamW([dict(params=[params[0], params[2]], lr=lrs[0], weight_decay=wds[0]),
                             dict(params=[params[1]], lr=lrs[1], weight_decay=wds[1])], betas=(b1, b2), eps=eps)
    chunks = [(s, s, z, g) for s, z, g in zip(starts, sizes, grp)]
    for step in range(1, 6):
        g = 0.1 * rs.standard_normal(n)
        for q, s, z in zip(params, starts, sizes):
            q.grad = torch.tensor(g[s:s + z])
        opt.step()
        p, m, v = R.adamw_ref(p, g, m, v, chunks, lrs, wds, b1, b2, eps, step)
        ref = torch.cat([q.detach() for q in params]).numpy()
        # (7/8)^t and (31/32)^t, t <= 5, fit fp32 too: only float64 rounding separates the two
        np.testing.assert_allclose(p, ref, rtol=0, atol=1e-9)


def test_adamw_ref_packed_and_untouched():
    """packed moments land at mstart, and nothing outside the chunks moves"""
    rs = np.random.RandomState(1)
    p, g = rs.standard_normal(40), rs.standard_normal(40)
    m, v = np.zeros(40), np.zeros(40)
    pm, pv = np.full(12, 7.0), np.full(12, 9.0)
    pm[1:8], pv[1:8] = 0.0, 0.0
    hp = ([1e-3], [0.01], 0.9, 0.999, 1e-8, 3)
    p1, m1, v1 = R.adamw_ref(p, g, m, v, [(10, 10, 7, 0)], *hp, clip=0.5)
    p2, m2, v2 = R.adamw_ref(p, g, pm, pv, [(10, 1, 7, 0)], *hp, clip=0.5)
    assert np.array_equal(p1, p2) and np.array_equal(m1[10:17], m2[1:8]) and np.array_equal(v1[10:17], v2[1:8])
    assert np.array_equal(p1[:10], p[:10]) and np.array_equal(p1[17:], p[17:]) and not np.any(p1[10:17] == p[10:17])
    assert m2[0] == 7.0 and np.all(m2[8:] == 7.0) and v2[0] == 9.0 and np.all(v2[8:] == 9.0)
