"""CPU checks of dxa_sample_rows' argument handling: the library refuses what it cannot run before any launch (no GPU
needed: the checks come first), and K.sample_rows raises ValueError for the two parameters it checks itself."""
import ctypes as C

import pytest
import torch

V = 16
ADDR = 4096                     # a non-null "device pointer": the argument checks fail before anything dereferences it


def call(logits=ADDR, ld=V, rows=1, v=V, dtype=None, temperature=1.0, top_k=0, top_p=1.0, u=ADDR, token=ADDR):
    from dexbotic_amd import _lib as L
    rc = L.lib.dxa_sample_rows(logits, ld, rows, v, L.BF16 if dtype is None else dtype, temperature, top_k, top_p, u, token,
                               None, None, None, None)
    return rc, L.last_error()


@pytest.mark.parametrize("null", ["logits", "u", "token"])
def test_null_pointer_is_refused(null):
    rc, msg = call(**{null: None})
    assert rc == -1 and "null pointer" in msg


def test_zero_temperature_is_refused():
    rc, msg = call(temperature=0.0)
    assert rc == -1 and "temperature" in msg
    rc, msg = call(temperature=-1.0)
    assert rc == -1 and "temperature" in msg


@pytest.mark.parametrize("top_p", [0.0, 1.5])
def test_top_p_outside_unit_interval_is_refused(top_p):
    rc, msg = call(top_p=top_p)
    assert rc == -1 and "top_p" in msg


def test_short_row_stride_and_bad_shapes_are_refused():
    rc, msg = call(ld=V - 1)
    assert rc == -1 and "ld" in msg
    rc, msg = call(v=0, ld=0)
    assert rc == -1 and "V" in msg
    rc, msg = call(rows=-1)
    assert rc == -1 and "rows" in msg


def test_bad_dtype_is_refused():
    rc, msg = call(dtype=7)
    assert rc == -1 and "dtype" in msg


def test_no_rows_is_not_an_error():
    rc, _ = call(rows=0)
    assert rc == 0


def test_python_wrapper_checks_temperature_and_top_p():
    from dexbotic_amd import kernels as K
    x, u = torch.zeros(1, V), torch.zeros(1)
    for bad in (0.0, -0.5):
        with pytest.raises(ValueError, match="temperature"):
            K.sample_rows(x, u, temperature=bad)
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="top_p"):
            K.sample_rows(x, u, top_p=bad)


def test_signature_table_matches_the_declaration():
    from dexbotic_amd import _lib as L
    res, args = L.SIGNATURES["dxa_sample_rows"]
    assert res is C.c_int and len(args) == 14
