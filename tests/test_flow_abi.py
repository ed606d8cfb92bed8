"""dxa_flow_suffix_in / dxa_flow_euler_tail refuse what they cannot run, with a message and before any launch: no GPU needed (the
pointers below are never dereferenced).  tests/test_abi.py holds the header, the exports and ``_lib.SIGNATURES`` together."""
import pytest

PTR = 4096                            # any non-null, 16-byte aligned address
F32 = 0


def suffix_in(**over):
    from dexbotic_amd import _lib as L
    a = dict(x=PTR, ldx=48, progress=PTR, ldp=1, te=PTR, w_in=PTR, b_in=PTR, w_p=PTR, b_p=PTR, out=PTR, B=2, n=6, A=8, da=64, p=1,
             dtype=F32)
    a.update(over)
    rc = L.lib.dxa_flow_suffix_in(a["x"], a["ldx"], a["progress"], a["ldp"], a["te"], a["w_in"], a["b_in"], a["w_p"], a["b_p"],
                                  a["out"], a["B"], a["n"], a["A"], a["da"], a["p"], a["dtype"], None)
    return rc, L.last_error()


def euler_tail(**over):
    from dexbotic_amd import _lib as L
    a = dict(h=PTR, g=PTR, w_out=PTR, b_out=PTR, w_q=PTR, b_q=PTR, x=PTR, ldx=48, prog_min=PTR, ldm=1, B=2, n=6, A=8, da=64, p=1,
             eps=1e-6, dt=-0.1, dtype=F32)
    a.update(over)
    rc = L.lib.dxa_flow_euler_tail(a["h"], a["g"], a["w_out"], a["b_out"], a["w_q"], a["b_q"], a["x"], a["ldx"], a["prog_min"],
                                   a["ldm"], a["B"], a["n"], a["A"], a["da"], a["p"], a["eps"], a["dt"], a["dtype"], None)
    return rc, L.last_error()


@pytest.mark.parametrize("name", ["x", "te", "w_in", "b_in", "out"])
def test_suffix_in_refuses_a_null_pointer(name):
    rc, msg = suffix_in(**{name: None})
    assert rc == -1 and "dxa_flow_suffix_in" in msg and "null" in msg


@pytest.mark.parametrize("name", ["h", "g", "w_out", "b_out", "x"])
def test_euler_tail_refuses_a_null_pointer(name):
    rc, msg = euler_tail(**{name: None})
    assert rc == -1 and "dxa_flow_euler_tail" in msg and "null" in msg


@pytest.mark.parametrize("fn", [suffix_in, euler_tail])
@pytest.mark.parametrize("p", [-1, 2])
def test_p_outside_0_1_is_refused(fn, p):
    rc, msg = fn(p=p)
    assert rc == -1 and "progress rows" in msg


@pytest.mark.parametrize("name", ["progress", "w_p", "b_p"])
def test_suffix_in_with_a_progress_row_needs_its_operands(name):
    rc, msg = suffix_in(**{name: None})
    assert rc == -1 and "p = 1 needs" in msg
    assert suffix_in(ldp=0)[0] == -1


@pytest.mark.parametrize("name", ["prog_min", "w_q", "b_q"])
def test_euler_tail_with_a_progress_row_needs_its_operands(name):
    rc, msg = euler_tail(**{name: None})
    assert rc == -1 and "p = 1 needs" in msg
    assert euler_tail(ldm=0)[0] == -1


@pytest.mark.parametrize("fn", [suffix_in, euler_tail])
@pytest.mark.parametrize("over", [dict(B=0), dict(n=0), dict(A=0), dict(da=0), dict(B=-1), dict(n=-3), dict(A=-8), dict(da=-64)])
def test_non_positive_sizes_are_refused(fn, over):
    rc, msg = fn(**over)
    assert rc == -1 and "non-positive size" in msg


@pytest.mark.parametrize("fn", [suffix_in, euler_tail])
def test_da_above_the_limit_a_short_stride_and_a_bad_dtype_are_refused(fn):
    rc, msg = fn(da=8192 + 8)
    assert rc == -1 and "8192" in msg
    rc, msg = fn(ldx=47)
    assert rc == -1 and "ldx" in msg
    rc, msg = fn(A=1025, ldx=6 * 1025)
    assert rc == -1 and "out of range" in msg
    rc, msg = fn(dtype=7)
    assert rc != 0 and "dtype" in msg
