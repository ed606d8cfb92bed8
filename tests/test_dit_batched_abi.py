"""CPU checks of the batched bf16 DiT sampler's C boundary (csrc/dit_fused.hip, request groups): the three entry points exist in the
library, the header and the ctypes table; the workspace is G single-request workspaces; a group count the launch cannot take is
refused with a message before anything touches a device."""
import re
import subprocess

import pytest

from tests.test_abi import header_symbols

NAMES = ("dxa_dit_sample_bf16_batched_workspace", "dxa_dit_sample_bf16_batched_fwd", "dxa_dit_sample_bf16_per_batched_fwd")
SHAPES = [(34, 768, 3072), (34, 1024, 4096), (10, 128, 512), (17, 192, 768)]


def test_the_three_entry_points_are_declared_exported_and_bound():
    from dexbotic_amd import _lib as L
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dxa_[a-z0-9_]+)", out))
    declared = header_symbols()
    for n in NAMES:
        assert n in exported and n in declared and n in L.SIGNATURES, n
    # the batched launches take the single launches' arguments plus the group count
    assert len(L.SIGNATURES["dxa_dit_sample_bf16_batched_fwd"][1]) == len(L.SIGNATURES["dxa_dit_sample_bf16_fwd"][1]) + 1
    assert len(L.SIGNATURES["dxa_dit_sample_bf16_per_batched_fwd"][1]) == len(L.SIGNATURES["dxa_dit_sample_bf16_per_fwd"][1]) + 1


@pytest.mark.parametrize("M,H,I", SHAPES)
def test_workspace_is_one_single_request_workspace_per_group(M, H, I):
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K
    one = L.lib.dxa_dit_sample_bf16_workspace(M, H, I)
    assert one > 0 and L.lib.dxa_dit_sample_bf16_batched_workspace(1, M, H, I) == one
    sizes = [L.lib.dxa_dit_sample_bf16_batched_workspace(G, M, H, I) for G in range(1, K.DIT_SAMPLE_MAX_GROUPS + 1)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sizes == [G * one for G in range(1, K.DIT_SAMPLE_MAX_GROUPS + 1)]
    assert one % 256 == 0                       # every group's arrays keep the alignment of the first


def test_group_count_outside_the_cap_is_refused_with_a_message():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K
    cap = K.DIT_SAMPLE_MAX_GROUPS
    assert cap == 16
    for G in (0, -1, cap + 1):
        assert L.lib.dxa_dit_sample_bf16_batched_workspace(G, 34, 768, 3072) == 0
        # (no pointer is dereferenced: the group count is checked first)
        nul = [None] * 9
        rc = L.lib.dxa_dit_sample_bf16_batched_fwd(*nul, 10, 7, G, 1, 1, 1.5, None, 12, 2, 17, 768, 12, 3072, 1e-6, None, 0, None)
        assert rc < 0 and "request groups" in L.last_error() and "dxa_dit_sample_bf16_batched_fwd" in L.last_error()
        rc = L.lib.dxa_dit_sample_bf16_per_batched_fwd(*nul, 10, 7, G, 1, 1, 1.5, None, 4096, 64, 12, 2, 17, 768, 12, 3072, 1e-6, None, 0,
                                                       None)
        assert rc < 0 and "request groups" in L.last_error()
    # a group count inside the cap gets as far as the next check
    rc = L.lib.dxa_dit_sample_bf16_batched_fwd(*([None] * 9), 10, 7, cap, 1, 1, 1.5, None, 12, 2, 17, 768, 12, 3072, 1e-6, None, 0, None)
    assert rc < 0 and "null buffer" in L.last_error()
    assert K.dit_sample_bf16_groups_supported(cap, 2, 17, 768, 12, 3072) and not K.dit_sample_bf16_groups_supported(cap + 1, 2, 17, 768, 12, 3072)
    assert not K.dit_sample_bf16_groups_supported(0, 2, 17, 768, 12, 3072)
    assert not K.dit_sample_bf16_groups_supported(2, 2, 25, 768, 12, 3072)            # 50 rows a group
    assert K.dit_sample_bf16_groups_supported(4, 2, 17, 1024, 16, 4096, 256) and not K.dit_sample_bf16_groups_supported(4, 1, 25, 1024, 16, 4096, 256)
