"""The entry points of csrc/oft_diffusion.hip refuse what they cannot run, with a message and before any launch: no GPU needed (the
pointers below are never dereferenced).  tests/test_abi.py holds the header, the exports and ``_lib.SIGNATURES`` together."""
import pytest

PTR = 4096                            # any non-null, 16-byte aligned address
ODD = 4100                            # non-null, not 16-byte aligned
F32, BF16 = 0, 1


def _call(name, order, defaults, over):
    from dexbotic_amd import _lib as L
    assert (L.F32, L.BF16) == (F32, BF16)
    a = dict(defaults)
    a.update(over)
    rc = getattr(L.lib, name)(*[a[k] for k in order], None)
    return rc, L.last_error()


def embed_fwd(**over):
    return _call("dxa_noisy_embed_fwd", ("a", "w1", "b1", "h", "R", "d", "dtype", "w_dtype"),
                 dict(a=PTR, w1=PTR, b1=PTR, h=PTR, R=6, d=96, dtype=F32, w_dtype=F32), over)


def embed_bwd(**over):
    return _call("dxa_noisy_embed_bwd", ("dh", "a", "w1", "b1", "dw1", "db1", "partial", "R", "d", "accumulate", "dtype", "w_dtype"),
                 dict(dh=PTR, a=PTR, w1=PTR, b1=PTR, dw1=PTR, db1=PTR, partial=PTR, R=6, d=96, accumulate=0, dtype=F32, w_dtype=F32), over)


def put_fwd(**over):
    return _call("dxa_diffusion_put_fwd", ("x", "proj", "time", "state", "off", "B", "Sq", "d", "n_rows", "dtype"),
                 dict(x=PTR, proj=PTR, time=PTR, state=PTR, off=PTR, B=2, Sq=20, d=96, n_rows=6, dtype=F32), over)


def put_bwd(**over):
    return _call("dxa_diffusion_put_bwd", ("dx", "off", "dproj", "dstate", "B", "Sq", "d", "n_rows", "skip", "dtype"),
                 dict(dx=PTR, off=PTR, dproj=PTR, dstate=PTR, B=2, Sq=20, d=96, n_rows=6, skip=1, dtype=F32), over)


def step(**over):
    return _call("dxa_ddim_step_embed", ("eps", "x", "c0", "c1", "c2", "c3", "clip", "time_row", "w1", "b1", "suffix", "h", "n", "d",
                                         "dtype", "w_dtype"),
                 dict(eps=PTR, x=PTR, c0=1.0, c1=0.1, c2=1.0, c3=0.0, clip=1.0, time_row=PTR, w1=PTR, b1=PTR, suffix=PTR, h=PTR, n=6,
                      d=96, dtype=F32, w_dtype=F32), over)


NULLS = [(embed_fwd, "dxa_noisy_embed_fwd", ["a", "w1", "b1", "h"]),
         (embed_bwd, "dxa_noisy_embed_bwd", ["dh", "a", "w1", "b1", "dw1", "db1", "partial"]),
         (put_fwd, "dxa_diffusion_put_fwd", ["x", "proj", "time", "off"]),
         (put_bwd, "dxa_diffusion_put_bwd", ["dx", "off", "dproj"]),
         (step, "dxa_ddim_step_embed", ["x", "time_row", "w1", "b1", "suffix", "h"])]


@pytest.mark.parametrize("fn,name,arg", [(f, n, a) for f, n, args in NULLS for a in args])
def test_a_null_pointer_is_refused(fn, name, arg):
    rc, msg = fn(**{arg: None})
    assert rc == -1 and name in msg and "null" in msg


def test_optional_pointers_may_be_null():
    """state / dstate / eps are optional: their absence is not an argument error (B = 0 and R = 0 return before any launch; the step
    kernel has no empty case, so only its argument checks are exercised with the pointer present)"""
    assert put_fwd(state=None, B=0)[0] == 0
    assert put_bwd(dstate=None, B=0)[0] == 0 and put_bwd(dstate=None, skip=0, B=0)[0] == 0
    assert embed_fwd(R=0)[0] == 0
    rc, msg = put_bwd(skip=0)
    assert rc == -1 and "dstate without a state row" in msg


@pytest.mark.parametrize("fn", [embed_fwd, embed_bwd, put_fwd, put_bwd, step])
@pytest.mark.parametrize("d", [0, -8, 4, 100, (1 << 20) + 8])
def test_a_width_that_is_no_multiple_of_8_is_refused(fn, d):
    rc, msg = fn(d=d)
    assert rc == -1 and "multiple of 8" in msg


ALIGNED = [(embed_fwd, ["w1", "b1", "h"]), (embed_bwd, ["dh", "w1", "b1", "dw1", "db1", "partial"]),
           (put_fwd, ["x", "proj", "time", "state"]), (put_bwd, ["dx", "dproj", "dstate"]),
           (step, ["time_row", "w1", "b1", "suffix", "h"])]


@pytest.mark.parametrize("fn,arg", [(f, a) for f, args in ALIGNED for a in args])
def test_a_misaligned_row_operand_is_refused(fn, arg):
    rc, msg = fn(**{arg: ODD})
    assert rc == -1 and "16-byte aligned" in msg


@pytest.mark.parametrize("fn", [embed_fwd, embed_bwd, put_fwd, put_bwd, step])
def test_a_bad_dtype_is_refused(fn):
    rc, msg = fn(dtype=7)
    assert rc != 0 and "dtype" in msg
    if fn in (embed_fwd, embed_bwd, step):
        rc, msg = fn(dtype=F32, w_dtype=BF16)          # fp32 activations never meet bf16 weights
        assert rc != 0 and "dtype" in msg
        assert fn(dtype=BF16, w_dtype=7)[0] != 0


def test_sizes_out_of_range_are_refused():
    assert embed_fwd(R=-1)[0] == -1
    rc, msg = embed_bwd(R=0)
    assert rc == -1 and "R = 0" in msg
    assert embed_bwd(R=(1 << 19) + 1)[0] == -1
    for fn in (put_fwd, put_bwd):
        rc, msg = fn(Sq=7)                             # 1 + 1 + 6 rows do not fit
        assert rc == -1 and "fit into Sq" in msg
        rc, msg = fn(n_rows=0)
        assert rc == -1 and "bad sizes" in msg
        assert fn(B=-1)[0] == -1 and fn(Sq=0)[0] == -1
    rc, msg = put_bwd(skip=2, dstate=None)
    assert rc == -1 and "bad sizes" in msg
    rc, msg = step(n=0)
    assert rc == -1 and "n = 0" in msg
    rc, msg = step(clip=float("nan"))
    assert rc == -1 and "clip" in msg


def test_backward_chunk_count():
    from dexbotic_amd import _lib as L
    f = L.lib.dxa_noisy_embed_bwd_blocks
    assert (f(0), f(1), f(16), f(17), f(896)) == (1, 1, 1, 2, 56)
