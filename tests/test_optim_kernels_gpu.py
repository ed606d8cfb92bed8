"""The optimizer tail on the MI355X: dxa_sumsq / dxa_sumsq_ranges / dxa_sum_f32 on integer-valued data whose sums are exact (one
element read zero times or twice changes the result), dxa_adamw with packed moments, the sparse-table chunk state, a scaled clip
coefficient and twenty consecutive steps against the float64 per-element AdamW of tests/optim_mem_ref.py, dxa_clip_coef_scaled
and dxa_scale_dev.  The Gaussian-data checks of tests/test_kernels_gpu.py stay where they are."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import optim_mem_ref as R
from tests.test_kernels_gpu import assert_close, rnd

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K

DEV = "cuda"
ADAMW_TOL = (1e-5, 2e-6)          # (rtol, atol) of test_adamw_matches_torch
DTYPES = [torch.float32, torch.bfloat16]

# dxa_sumsq launches min(ceil(ceil(n / 4) / 256), 4096) blocks of 256 threads (dxa_grid1d(.., 256, 4096)): once the cap binds the
# grid stride is STRIDE = 4096 * 256 float4 groups, and the 4-way unrolled loop `i + 3 * stride < n4` first runs at n4 > 3 * STRIDE.
# With n4 = 4 * STRIDE + STRIDE / 2 + 77 every thread runs the unrolled loop once (i + 3 * STRIDE < 4 * STRIDE), the threads with
# i < STRIDE / 2 + 77 run the remainder loop once more, and n = 4 * n4 + 3 leaves 3 elements to the scalar tail.
STRIDE = 4096 * 256
N4_BIG = 4 * STRIDE + STRIDE // 2 + 77
N_BIG = 4 * N4_BIG + 3
assert N_BIG == 18_874_679


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def int_data(n, hi, seed, dtype=torch.float32):
    """n values drawn from {0, .., hi - 1} by a seeded generator -> (device tensor of ``dtype``, exact sum of squares)"""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    v = torch.randint(0, hi, (n,), generator=g, dtype=torch.int64)
    return v.to(DEV).to(dtype), int((v * v).sum())


def scratch_out(fill=0.0):
    return torch.empty(4096, device=DEV, dtype=torch.float64), torch.full((1,), fill, device=DEV)


# ------------------------------------------------------------------------------------------------ sums
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 1024 * 4 + 1])
def test_sumsq_exact_small(dtype, n):
    x, exact = int_data(max(n, 1), 3, 200 + n, dtype)
    scratch, out = scratch_out(float("nan"))
    if n == 0:
        # an empty torch tensor has no data pointer: the C entry takes n = 0 with any valid pointer
        L.check(L.lib.dxa_sumsq(x.data_ptr(), 0, K.dt(x), scratch.data_ptr(), out.data_ptr(), 0, K._stream()), "dxa_sumsq")
        exact = 0
    else:
        K.sumsq(x, out, scratch)
    assert out.item() == exact
    out.fill_(7.0)
    if n == 0:
        L.check(L.lib.dxa_sumsq(x.data_ptr(), 0, K.dt(x), scratch.data_ptr(), out.data_ptr(), 1, K._stream()), "dxa_sumsq")
    else:
        K.sumsq(x, out, scratch, accumulate=True)
    assert out.item() == exact + 7


@pytest.fixture(scope="module")
def big_ones():
    """N_BIG values in {0, 1}, about a quarter of them 1 (total ~4.7e6 < 2^24: every fp32 partial, the double fold and the final
    cast are exact) -> (bool device tensor, exact count)"""
    g = torch.Generator(device=DEV)
    g.manual_seed(2024)
    ones = torch.randint(0, 4, (N_BIG,), device=DEV, dtype=torch.uint8, generator=g) == 0
    exact = int(ones.sum())
    assert N_BIG // 5 < exact < 2 ** 24 - 8
    return ones, exact


@pytest.mark.parametrize("dtype", DTYPES)
def test_sumsq_exact_unrolled_loop(big_ones, dtype):
    ones, exact = big_ones
    x = ones.to(dtype)
    scratch, out = scratch_out(float("nan"))
    K.sumsq(x, out, scratch)
    assert out.item() == exact
    out.fill_(5.0)
    K.sumsq(x, out, scratch, accumulate=True)
    assert out.item() == exact + 5


# element index of each probe: the first float4 of the four unrolled streams of thread 0 of block 0 (a different component of the
# float4 each time), the first and the last float4 of the remainder loop, the 3 tail elements
PROBES = {"stream0": 0, "stream1": 4 * STRIDE + 1, "stream2": 4 * 2 * STRIDE + 2, "stream3": 4 * 3 * STRIDE + 3,
          "remainder_first": 4 * 4 * STRIDE, "remainder_last": 4 * (N4_BIG - 1) + 3,
          "tail0": N_BIG - 3, "tail1": N_BIG - 2, "tail2": N_BIG - 1}


@pytest.mark.parametrize("dtype", DTYPES)
def test_sumsq_one_hot_probes(dtype):
    x = torch.zeros(N_BIG, device=DEV, dtype=dtype)
    scratch, out = scratch_out(float("nan"))
    got = {}
    for name, i in PROBES.items():
        assert 0 <= i < N_BIG
        x[i] = 3.0
        K.sumsq(x, out, scratch)
        got[name] = out.item()
        x[i] = 0.0
    assert got == {name: 9.0 for name in PROBES}


@pytest.mark.parametrize("dtype,shift", [(torch.float32, 1), (torch.bfloat16, 1), (torch.bfloat16, 2), (torch.bfloat16, 3),
                                         (torch.float32, 4), (torch.bfloat16, 4)])
@pytest.mark.parametrize("n", [5, 70001])
def test_sumsq_unaligned_view(dtype, shift, n):
    """base[shift:] is not 16-byte (fp32) / 8-byte (bf16) aligned for shift < 4: the scalar branch; shift = 4 is the aligned control"""
    base, _ = int_data(n + shift, 3, 300 + shift, dtype)
    x = base[shift:]
    assert (x.data_ptr() % (4 * x.element_size()) == 0) == (shift == 4)
    exact = int((x.double() ** 2).sum().item())
    scratch, out = scratch_out(float("nan"))
    K.sumsq(x, out, scratch)
    assert out.item() == exact
    out.fill_(11.0)
    K.sumsq(x, out, scratch, accumulate=True)
    assert out.item() == exact + 11


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n", [0, 1, 1023, 1025, 5000])
def test_sum_f32_exact(n, accumulate):
    g = torch.Generator(device="cpu")
    g.manual_seed(400 + n)
    v = torch.randint(-3, 4, (max(n, 1),), generator=g)
    x = v.to(DEV).float()
    out = torch.full((1,), 5.0, device=DEV)
    if n == 0:
        L.check(L.lib.dxa_sum_f32(x.data_ptr(), 0, out.data_ptr(), int(accumulate), K._stream()), "dxa_sum_f32")
        exact = 0
    else:
        K.sum_f32(x, out, accumulate=accumulate)
        exact = int(v.sum())
    assert out.item() == exact + (5 if accumulate else 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sumsq_ranges_exact(dtype):
    base, _ = int_data(50021, 3, 500, dtype)
    host = base.double().cpu().numpy()
    rs = np.random.RandomState(501)
    scratch, out = scratch_out(float("nan"))

    def run(starts, lens, accumulate=False):
        K.sumsq_ranges(base, torch.tensor(starts, dtype=torch.int64, device=DEV), torch.tensor(lens, dtype=torch.int64, device=DEV),
                       out, scratch, accumulate=accumulate)
        return out.item(), int(sum((host[s:s + n] ** 2).sum() for s, n in zip(starts, lens)))

    # a range of length 0 among others, starts at every residue modulo 4, lengths around the 256-thread block, the last element
    starts, lens = [0, 1, 2, 3, 7, 1001, 4098, 50020, 13], [5, 0, 256, 257, 1, 511, 1025, 1, 0]
    got, exact = run(starts, lens)
    assert got == exact and exact > 0
    got, exact = run([17], [0])
    assert got == 0.0 and exact == 0
    # 4096 ranges, the documented maximum: every partial slot of stage 2 is used
    lens = rs.randint(0, 300, 4096)
    lens[::97] = 0
    starts = rs.randint(0, 50021 - 300, 4096)
    assert len({int(s) % 4 for s in starts}) == 4
    got, exact = run(starts.tolist(), lens.tolist())
    assert got == exact and 2 ** 18 < exact < 2 ** 24
    out.fill_(3.0)
    got, exact = run(starts.tolist(), lens.tolist(), accumulate=True)
    assert got == exact + 3


# ------------------------------------------------------------------------------------------------ AdamW
HP = dict(lrs=[1e-3, 5e-4], wds=[0.01, 0.0], beta1=0.9, beta2=0.999, eps=1e-8)


def tables(chunks):
    """chunks [(start, mstart, length, group)] -> device chunk_start, chunk_len, chunk_grp, chunk_mv_start"""
    col = lambda i, dtype: torch.tensor([c[i] for c in chunks], dtype=dtype, device=DEV)
    return col(0, torch.int64), col(2, torch.int32), col(3, torch.int32), col(1, torch.int64)


def run_adamw(p, g, m, v, shadow, chunks, step, clip=None, state=None, packed=True, hp=HP):
    cs, cl, cg, cms = tables(chunks)
    K.adamw(p, g, m, v, shadow, cs, cl, cg, hp["lrs"], hp["wds"], hp["beta1"], hp["beta2"], hp["eps"], step, clip=clip,
            chunk_state=state, chunk_mv_start=cms if packed else None)


def ref_adamw(p, g, m, v, chunks, step, clip=1.0, hp=HP):
    """float64 reference from the device tensors' values -> (p, m, v) float64 device tensors"""
    out = R.adamw_ref(*(t.double().cpu().numpy() for t in (p, g, m, v)), chunks, hp["lrs"], hp["wds"], hp["beta1"], hp["beta2"],
                      hp["eps"], step, clip=clip)
    return tuple(torch.from_numpy(o).to(DEV) for o in out)


def owned_mask(n, chunks, packed):
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    for c in chunks:
        s = c[1] if packed else c[0]
        mask[s:s + c[2]] = True
    return mask


def sentinel_bf16(n):
    return ((torch.arange(n, device=DEV) % 127) + 129).to(torch.bfloat16)        # 129 .. 255: exact in bf16, never a parameter


N_ARENA = 20011
# (start, mstart, length, group).  MIXED: (start, mstart) modulo 4 = (0,0) (0,1) (0,2) (3,0) (1,1) (0,0); lengths: a multiple of 4
# above 2048 (every thread runs the two-groups-in-flight loop), non-multiples, one on the scalar path above 2048, 1.  Gaps in both
# layouts, the arena's head and tail are not owned.
MIXED = [(8, 0, 2500, 0), (3000, 2501, 1030, 1), (5000, 3534, 37, 0), (6003, 3600, 4100, 1), (11001, 7701, 1, 0),
         (12000, 7704, 3003, 0)]
# every start of both layouts a multiple of 4: the packed and the unpacked run take the vector path alike
ALIGNED = [(8, 0, 2500, 0), (3000, 2500, 1030, 1), (5000, 3532, 37, 0), (6004, 3600, 4100, 1), (11000, 7700, 1, 0),
           (12000, 7704, 3003, 0)]
N_PACKED = 10720


def packed_inputs(chunks, gdtype):
    p = rnd(N_ARENA, seed=600)
    g = rnd(N_ARENA, seed=601, scale=0.1).to(gdtype)
    m_full, v_full = rnd(N_ARENA, seed=602, scale=0.05), rnd(N_ARENA, seed=603, scale=0.05).square() + 1e-6
    sent = torch.arange(N_PACKED, device=DEV, dtype=torch.float32)
    m_pk, v_pk = 1000.0 + sent, 5000.0 + sent                                    # distinct sentinels where no chunk maps
    for s, ms, n, _ in chunks:
        m_pk[ms:ms + n], v_pk[ms:ms + n] = m_full[s:s + n], v_full[s:s + n]
    return p, g, m_full, v_full, m_pk, v_pk, sentinel_bf16(N_ARENA)


@pytest.mark.parametrize("gdtype", DTYPES)
@pytest.mark.parametrize("layout", ["mixed", "aligned"])
def test_adamw_packed_moments(layout, gdtype):
    chunks = MIXED if layout == "mixed" else ALIGNED
    assert {(c[0] % 4, c[1] % 4) for c in MIXED} == {(0, 0), (0, 1), (0, 2), (3, 0), (1, 1)}
    assert all(c[0] % 4 == 0 and c[1] % 4 == 0 for c in ALIGNED) and max(c[1] + c[2] for c in chunks) < N_PACKED
    p0, g, m_full0, v_full0, m_pk0, v_pk0, sh0 = packed_inputs(chunks, gdtype)
    own_a, own_p = owned_mask(N_ARENA, chunks, False), owned_mask(N_PACKED, chunks, True)
    assert 0 < int(own_a.sum()) < N_ARENA and 0 < int(own_p.sum()) < N_PACKED and int(own_a.sum()) == int(own_p.sum())
    step = 3
    # packed run
    p, m_pk, v_pk, sh = p0.clone(), m_pk0.clone(), v_pk0.clone(), sh0.clone()
    run_adamw(p, g, m_pk, v_pk, sh, chunks, step, packed=True)
    # unpacked run of the same chunks
    p_u, m_u, v_u, sh_u = p0.clone(), m_full0.clone(), v_full0.clone(), sh0.clone()
    run_adamw(p_u, g, m_u, v_u, sh_u, chunks, step, packed=False)
    # nothing outside the owned chunks moves, in either run
    for name, new, old, own in (("p", p, p0, own_a), ("shadow", sh, sh0, own_a), ("m packed", m_pk, m_pk0, own_p),
                                ("v packed", v_pk, v_pk0, own_p), ("p unpacked", p_u, p0, own_a),
                                ("shadow unpacked", sh_u, sh0, own_a), ("m unpacked", m_u, m_full0, own_a),
                                ("v unpacked", v_u, v_full0, own_a)):
        assert torch.equal(bits(new)[~own], bits(old)[~own]), f"{name}: an element outside the owned chunks changed"
    # both runs against the float64 reference (they may take the vector and the scalar loop for the same chunk)
    rp, rm, rv = ref_adamw(p0, g, m_pk0, v_pk0, chunks, step)
    assert_close(p, rp, *ADAMW_TOL, "p packed")
    assert_close(m_pk[own_p], rm[own_p], *ADAMW_TOL, "m packed")
    assert_close(v_pk[own_p], rv[own_p], *ADAMW_TOL, "v packed")
    assert_close(p_u, rp, *ADAMW_TOL, "p unpacked")
    for s, ms, n, _ in chunks:
        assert_close(m_u[s:s + n], rm[ms:ms + n], *ADAMW_TOL, f"m unpacked chunk at {s}")
        assert_close(v_u[s:s + n], rv[ms:ms + n], *ADAMW_TOL, f"v unpacked chunk at {s}")
    # every owned element was written: its shadow is no longer the sentinel but the new parameter's bf16 rounding
    assert same_bits(sh[own_a], p.to(torch.bfloat16)[own_a]) and same_bits(sh_u[own_a], p_u.to(torch.bfloat16)[own_a])
    if layout == "aligned":
        assert same_bits(p, p_u) and same_bits(sh, sh_u)
        for s, ms, n, _ in chunks:
            assert same_bits(m_pk[ms:ms + n], m_u[s:s + n]) and same_bits(v_pk[ms:ms + n], v_u[s:s + n])


def same_bits_nan(a, b):
    """bit-identical, NaNs equal by position"""
    na, nb = torch.isnan(a.float()), torch.isnan(b.float())
    return torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


# (start, length, group, state, gradient)
SPARSE = [(0, 1000, 1, 1, "zero"), (1000, 515, 1, 1, "negzero"), (1517, 203, 1, 1, "last"), (1720, 1027, 1, 1, "last"),
          (2748, 2000, 1, 1, "nan"), (4748, 600, 0, 1, "zero"), (5348, 3001, 0, 0, "random")]
SPARSE_AFTER = [1, 1, 2, 2, 2, 1, 0]


@pytest.mark.parametrize("gdtype", DTYPES)
def test_adamw_sparse_state(gdtype):
    """chunks in state 1 (m = v = 0): skipped on an all-zero gradient unless the group decays; the skip changes no bit"""
    n = 5348 + 3001
    assert SPARSE[2][0] % 4 == 1 and SPARSE[2][1] % 4 == 3 and SPARSE[3][0] % 4 == 0 and SPARSE[3][1] % 4 == 3
    assert HP["wds"][1] == 0.0 and HP["wds"][0] != 0.0
    chunks = [(s, s, ln, grp) for s, ln, grp, _, _ in SPARSE]
    p0 = rnd(n, seed=610)
    m0, v0 = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    s_last, l_last = SPARSE[-1][0], SPARSE[-1][1]
    m0[s_last:] = rnd(l_last, seed=611, scale=0.05)
    v0[s_last:] = rnd(l_last, seed=612, scale=0.05).square() + 1e-6
    sh0 = p0.to(torch.bfloat16)                               # skipped chunks do not rewrite their shadow

    def grads(seed):
        g = torch.zeros(n, device=DEV)
        for s, ln, _, _, kind in SPARSE:
            if kind == "negzero":
                g[s:s + ln] = -0.0
            elif kind == "last":
                g[s + ln - 1] = 0.25
            elif kind == "nan":
                g[s + 777] = float("nan")                     # in the float4 part of an aligned chunk
            elif kind == "random":
                g[s:s + ln] = rnd(ln, seed=seed, scale=0.1)
        g = g.to(gdtype)
        assert bool(torch.signbit(g[1000:1515].float()).all()) and bool((g[1000:1515] == 0).all())
        return g

    state = torch.tensor([c[3] for c in SPARSE], dtype=torch.uint8, device=DEV)
    a = [p0.clone(), m0.clone(), v0.clone(), sh0.clone()]
    b = [p0.clone(), m0.clone(), v0.clone(), sh0.clone()]
    for step, seed in ((1, 613), (2, 614)):
        g = grads(seed)
        run_adamw(a[0], g, a[1], a[2], a[3], chunks, step, state=state, packed=False)
        run_adamw(b[0], g, b[1], b[2], b[3], chunks, step, state=None, packed=False)
        for name, x, y in zip(("p", "m", "v", "shadow"), a, b):
            assert same_bits_nan(x, y), f"step {step}: {name} differs from the run without chunk states"
        assert state.tolist() == SPARSE_AFTER, f"step {step}"
        assert same_bits_nan(a[3], a[0].to(torch.bfloat16))
    # the runs did something: the decayed chunk and the chunks with a non-zero moved, the skipped ones kept every bit
    for (s, ln, _, _, _), after in zip(SPARSE, SPARSE_AFTER):
        moved = not same_bits(a[0][s:s + ln], p0[s:s + ln])
        assert moved == (after != 1 or (s, ln) == (4748, 600))
    assert int(torch.isnan(a[0]).sum()) == 1 and bool(torch.isnan(a[0][2748 + 777]))


@pytest.mark.parametrize("max_norm", [1.0, 100.0])
@pytest.mark.parametrize("s", [0.5, 0.125])
def test_clip_coef_scaled_and_adamw(s, max_norm):
    """the arena holds g / s (a loss scale); dxa_clip_coef_scaled folds s into the norm and the coefficient"""
    n = 5003
    g_true = rnd(n, seed=620, scale=0.1)
    arena = g_true / s                                        # exact: s is a power of two
    scratch, ss = scratch_out(float("nan"))
    K.sumsq(arena, ss, scratch)
    norm, coef = torch.full((1,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
    K.clip_coef(ss, max_norm, norm, coef, grad_scale=s)
    want_norm = math.sqrt(ss.double().item()) * s
    want_coef = min(max_norm / (want_norm + 1e-6), 1.0) * s
    assert (want_norm > max_norm) == (max_norm == 1.0)        # |g| ~ 7: clipped at 1, not at 100
    assert abs(norm.item() - want_norm) <= 1e-6 * want_norm, (norm.item(), want_norm)
    assert abs(coef.item() - want_coef) <= 1e-6 * want_coef, (coef.item(), want_coef)
    chunks = [(0, 0, 2052, 0), (2052, 2052, 2951, 1)]
    p0 = rnd(n, seed=621)
    m0, v0 = rnd(n, seed=622, scale=0.05), rnd(n, seed=623, scale=0.05).square() + 1e-6
    p, m, v, sh = p0.clone(), m0.clone(), v0.clone(), sentinel_bf16(n)
    run_adamw(p, arena, m, v, sh, chunks, 2, clip=coef, packed=False)
    # float64 reference fed the clipped true gradient, its norm taken in float64
    c64 = min(max_norm / (math.sqrt(g_true.double().square().sum().item()) + 1e-6), 1.0)
    rp, rm, rv = ref_adamw(p0, g_true.double() * c64, m0, v0, chunks, 2)
    assert_close(p, rp, *ADAMW_TOL, "p")
    assert_close(m, rm, *ADAMW_TOL, "m")
    assert_close(v, rv, *ADAMW_TOL, "v")
    assert same_bits(sh, p.to(torch.bfloat16))


def test_adamw_twenty_steps_vs_float64():
    chunks = [(0, 0, 1500, 0), (1500, 1500, 41, 1), (1541, 1541, 1200, 0), (2741, 2741, 260, 1)]
    n = 3001
    p = rnd(n, seed=630)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sh = sentinel_bf16(n)
    rp, rm, rv = (t.double().cpu().numpy() for t in (p, m, v))
    base = rnd(n, seed=631, scale=0.1)
    for step in range(1, 21):
        g = base * (1 + 0.3 * math.sin(step)) + rnd(n, seed=640 + step, scale=0.03)
        run_adamw(p, g, m, v, sh, chunks, step, packed=False)
        rp, rm, rv = R.adamw_ref(rp, g.double().cpu().numpy(), rm, rv, chunks, HP["lrs"], HP["wds"], HP["beta1"], HP["beta2"],
                                 HP["eps"], step)
        for name, got, want in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
            assert_close(got, torch.from_numpy(want).to(DEV), *ADAMW_TOL, f"{name} after step {step}")
        assert same_bits(sh, p.to(torch.bfloat16))
    assert float((p - rnd(n, seed=630)).abs().max()) > 5e-3      # twenty steps of ~lr each moved the parameters


@pytest.mark.parametrize("n", [1, 1000, 70001])
def test_scale_dev(n):
    x0 = rnd(n, seed=650)
    s = torch.tensor([0.37], device=DEV)
    x = x0.clone()
    assert K.scale_dev_(x, s) is x
    assert same_bits(x, x0 * s)


def test_adamw_no_chunks_touches_nothing():
    n = 64
    p, g, m, v, sh = rnd(n, seed=660), rnd(n, seed=661), rnd(n, seed=662), rnd(n, seed=663).square(), sentinel_bf16(n)
    keep = [t.clone() for t in (p, g, m, v, sh)]
    cs, cl, cg, _ = tables([(0, 0, n, 0)])                    # valid tables, zero chunks of them used
    d = L.AdamWDesc()
    d.p, d.g, d.m, d.v, d.shadow = (t.data_ptr() for t in (p, g, m, v, sh))
    d.g_dtype = K.dt(g)
    d.chunk_start, d.chunk_len, d.chunk_grp, d.n_chunks = cs.data_ptr(), cl.data_ptr(), cg.data_ptr(), 0
    d.lr[0], d.wd[0] = 1e-3, 0.01
    d.beta1, d.beta2, d.eps, d.bc1, d.bc2 = 0.9, 0.999, 1e-8, 0.1, 0.001
    L.check(L.lib.dxa_adamw(ctypes.byref(d), K._stream()), "dxa_adamw")
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip((p, g, m, v, sh), keep))
