"""CPU checks of the drop-in boundary: the C-ABI library loads, exports every symbol the header
declares, the ctypes table covers all of them, and the product path refuses to run without a GPU
(no CPU fallback, no oracle import)."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dexbotic_amd.h")


def header_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dxa_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from dexbotic_amd import _lib as L
    syms = header_symbols()
    assert len(syms) >= 40
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dxa_[a-z0-9_]+)", out))
    missing = [s for s in syms if s not in exported]
    assert not missing, f"declared in include/dexbotic_amd.h but not exported: {missing}"
    assert sorted(L.SIGNATURES) == syms, (set(L.SIGNATURES) ^ set(syms))
    assert L.lib.dxa_version() >= 100
    assert L.last_error() == ""


def test_struct_layouts_match_header_field_order():
    from dexbotic_amd import _lib as L
    src = open(HEADER).read()
    for cname, cls in (("dxa_gemm_desc", L.GemmDesc), ("dxa_attn_desc", L.AttnDesc), ("dxa_adamw_desc", L.AdamWDesc),
                       ("dxa_decode_desc", L.DecodeDesc), ("dxa_split3_op", L.Split3Op),
                       ("dxa_gemm_step_info", L.GemmStepInfo), ("dxa_gemm_plan_info", L.GemmPlanInfo),
                       ("dxa_attn_plan_info", L.AttnPlanInfo), ("dxa_norm_desc", L.NormDesc),
                       ("dxa_norm_plan_info", L.NormPlanInfo)):
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname, src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                m = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[\d+\])?\s*$", part.strip())
                names.append(m.group(1))
        assert names == [f[0] for f in cls._fields_], cname


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_cpu_fallback():
    from dexbotic_amd import _lib as L
    from dexbotic_amd import kernels as K
    a = torch.zeros(4, 4)
    with pytest.raises(L.DxaError):
        K.mm_nt(a, a)
    # bad arguments are rejected by the library itself with a message
    d = L.GemmDesc()
    d.layout = 7
    assert L.lib.dxa_gemm(d, None) == -1
    assert "layout" in L.last_error()


def test_new_entry_points_reject_bad_arguments_with_a_message():
    """round 6's entry points refuse what they cannot run instead of launching (no GPU needed: the checks come first)"""
    from dexbotic_amd import _lib as L
    q = L.DecodeDesc()
    assert L.lib.dxa_decode_step(q, None) == -1 and "null pointer" in L.last_error()
    assert L.lib.dxa_decode_step_workspace(3584, 28, 4, 128, 18944) == 2 * (3584 + 4608 + 3584 + 18944)      # bf16, 128-element pads
    assert L.lib.dxa_decode_step_workspace(0, 28, 4, 128, 18944) == 0
    d = L.GemmDesc()
    d.layout, d.in_dtype, d.out_dtype, d.M, d.N, d.K = L.NT, L.BF16, L.BF16, 64, 512, 256
    d.nb[0] = d.nb[1] = d.nb[2] = 1
    d.A = d.B = d.C = 4096                                   # (never dereferenced: the fuse check fails first)
    d.lda = d.ldb = 256
    d.ldc = 256
    d.fuse = L.FUSE_SWIGLU
    assert L.lib.dxa_gemm(d, None) == -1 and "DXA_FUSE_SWIGLU" in L.last_error()          # 64 rows: not the MFMA fast path
    d.fuse = 7
    assert L.lib.dxa_gemm(d, None) == -1 and "unknown fuse mode" in L.last_error()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "dexbotic_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), os.path.join(dp, f)
    code = "import sys; import dexbotic_amd; assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_clean_tree_build_command_runs_without_the_library(tmp_path):
    """`python -m dexbotic_amd.build` is the command the missing-library ImportError names, so it must start in a tree that
    has no .so yet; plain `import dexbotic_amd` in the same tree must still fail loudly (no fallback).  hipcc is replaced by a
    stub that writes empty outputs: the compile itself is __graft_entry__.build()'s check, this one is about the import path."""
    import shutil
    scratch = tmp_path / "tree"
    shutil.copytree(os.path.join(ROOT, "dexbotic_amd"), scratch / "dexbotic_amd",
                    ignore=shutil.ignore_patterns("*.so", "_obj", "__pycache__"))
    shutil.copytree(os.path.join(ROOT, "include"), scratch / "include")
    assert not (scratch / "dexbotic_amd" / "libdexbotic_amd.so").exists()
    r = subprocess.run([sys.executable, "-c", "import dexbotic_amd"], cwd=scratch, capture_output=True, text=True)
    assert r.returncode != 0 and "python -m dexbotic_amd.build" in r.stderr
    stub = tmp_path / "hipcc_stub.sh"
    stub.write_text("#!/bin/bash\nwhile [ $# -gt 0 ]; do if [ \"$1\" = \"-o\" ]; then : > \"$2\"; fi; shift; done\n")
    stub.chmod(0o755)
    env = dict(os.environ, HIPCC=str(stub))
    r = subprocess.run([sys.executable, "-m", "dexbotic_amd.build"], cwd=scratch, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert (scratch / "dexbotic_amd" / "libdexbotic_amd.so").exists()
