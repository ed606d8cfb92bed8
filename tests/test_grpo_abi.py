"""dxa_bin_logprob_fwd / dxa_bin_logprob_bwd / dxa_ppo_clip_fwd refuse what they cannot run, with a message and before any launch:
no GPU needed (the pointers below are never dereferenced).  tests/test_abi.py holds the header, the exports and ``_lib.SIGNATURES``
together."""
import pytest

PTR = 4096                            # any non-null, 16-byte aligned address
F32, BF16 = 0, 1


def logprob_fwd(**over):
    from dexbotic_amd import _lib as L
    a = dict(logits=PTR, ld=255, bins=PTR, inv_t=0.625, logp=PTR, entropy=PTR, lse=PTR, rows=6, NB=255, dtype=F32)
    a.update(over)
    rc = L.lib.dxa_bin_logprob_fwd(a["logits"], a["ld"], a["bins"], a["inv_t"], a["logp"], a["entropy"], a["lse"], a["rows"], a["NB"],
                                   a["dtype"], None)
    return rc, L.last_error()


def logprob_bwd(**over):
    from dexbotic_amd import _lib as L
    a = dict(logits=PTR, ld=255, bins=PTR, lse=PTR, coef=PTR, gscale=PTR, inv_t=0.625, dlogits=PTR, rows=6, NB=255, dtype=BF16)
    a.update(over)
    rc = L.lib.dxa_bin_logprob_bwd(a["logits"], a["ld"], a["bins"], a["lse"], a["coef"], a["gscale"], a["inv_t"], a["dlogits"],
                                   a["rows"], a["NB"], a["dtype"], None)
    return rc, L.last_error()


def ppo_clip(**over):
    from dexbotic_amd import _lib as L
    a = dict(logp=PTR, old_logp=PTR, adv=PTR, mask=PTR, mask_u8=0, n=12, clip_low=0.2, clip_high=0.28, inv_denom=0.5, sums=PTR, loss=PTR,
             coef=PTR)
    a.update(over)
    rc = L.lib.dxa_ppo_clip_fwd(a["logp"], a["old_logp"], a["adv"], a["mask"], a["mask_u8"], a["n"], a["clip_low"], a["clip_high"],
                                a["inv_denom"], a["sums"], a["loss"], a["coef"], None)
    return rc, L.last_error()


@pytest.mark.parametrize("name", ["logits", "bins", "logp", "entropy", "lse"])
def test_logprob_fwd_refuses_a_null_pointer(name):
    rc, msg = logprob_fwd(**{name: None})
    assert rc == -1 and "dxa_bin_logprob_fwd" in msg and "null" in msg


@pytest.mark.parametrize("name", ["logits", "bins", "lse", "coef", "dlogits"])
def test_logprob_bwd_refuses_a_null_pointer(name):
    rc, msg = logprob_bwd(**{name: None})
    assert rc == -1 and "dxa_bin_logprob_bwd" in msg and "null" in msg


@pytest.mark.parametrize("name", ["logp", "old_logp", "adv", "mask", "sums", "coef"])
def test_ppo_clip_refuses_a_null_pointer(name):
    rc, msg = ppo_clip(**{name: None})
    assert rc == -1 and "dxa_ppo_clip_fwd" in msg and "null" in msg


@pytest.mark.parametrize("fn", [logprob_fwd, logprob_bwd])
def test_bin_kernels_refuse_bad_sizes_strides_and_dtypes(fn):
    for NB in (0, -1, 65537):
        rc, msg = fn(NB=NB, ld=1 << 20)
        assert rc == -1 and "NB" in msg and "65536" in msg
    rc, msg = fn(ld=254)
    assert rc == -1 and "ld" in msg
    rc, msg = fn(rows=-1)
    assert rc == -1 and "rows" in msg
    rc, msg = fn(dtype=7)
    assert rc == -1 and "dtype" in msg
    for inv_t in (0.0, -1.0, float("inf"), float("nan")):
        rc, msg = fn(inv_t=inv_t)
        assert rc == -1 and "inv_temperature" in msg


def test_ppo_clip_refuses_bad_sizes_and_ranges():
    for n in (0, -5):
        rc, msg = ppo_clip(n=n)
        assert rc == -1 and "n =" in msg
    rc, msg = ppo_clip(mask_u8=2)
    assert rc == -1 and "mask_u8" in msg
    for over in (dict(clip_low=-0.1), dict(clip_low=1.0), dict(clip_high=-0.1), dict(clip_high=float("inf")), dict(clip_low=float("nan"))):
        rc, msg = ppo_clip(**over)
        assert rc == -1 and "clip range" in msg
    for inv in (float("inf"), float("nan")):
        rc, msg = ppo_clip(inv_denom=inv)
        assert rc == -1 and "inv_denom" in msg


def test_optional_operands_and_empty_work_are_accepted():
    """rows = 0 returns before any launch; (a null ``gscale`` / ``loss`` is legal too, which only a launch could show)"""
    assert logprob_fwd(rows=0)[0] == 0
    assert logprob_bwd(rows=0, gscale=None)[0] == 0
