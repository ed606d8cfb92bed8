"""dxa_decode_desc.qk_norm (the q / k norm of a Qwen3 decoder in the persistent decode step): the field is NULL in a zeroed
descriptor, and a descriptor that carries it is held to the same head_dim set as one that does not.  No GPU needed: the argument
checks come before anything touches the device."""
import ctypes as C


def _desc(D: int):
    from dexbotic_amd import _lib as L
    q = L.DecodeDesc()
    # (never dereferenced: the head_dim check fails first)
    q.layers = q.x_in = q.out = q.final_norm_w = q.cos_row = q.sin_row = q.workspace = q.qk_norm = 4096
    q.n_layers, q.d, q.Hq, q.Hkv, q.D, q.F = 2, 64, 4, 2, D, 128
    q.slot, q.kv_lo, q.max_len, q.eps = 6, 0, 9, 1e-6
    return q


def test_a_descriptor_with_qk_norm_and_head_dim_32_is_refused():
    from dexbotic_amd import _lib as L
    assert L.lib.dxa_decode_step(C.byref(_desc(32)), None) == -1
    assert "head_dim 64, 128 or 256 (got 32)" in L.last_error()


def test_the_python_gate_keeps_head_dim_32_off_the_persistent_step():
    from dexbotic_amd import kernels as K
    assert K.decode_step_supported(64, 4, 2, 32, 128) is False
    assert K.decode_step_supported(128, 4, 2, 64, 256) is True         # the widths of tests/golden/qwen3_d64.npz: Hq D != d


def test_a_zeroed_descriptor_has_no_qk_norm():
    from dexbotic_amd import _lib as L
    q = L.DecodeDesc()
    assert q.qk_norm is None
    assert L.DecodeDesc._fields_[-1][0] == "qk_norm"                   # appended: every earlier field keeps its offset
    assert L.DecodeDesc.qk_norm.offset == C.sizeof(L.DecodeDesc) - C.sizeof(C.c_void_p)
