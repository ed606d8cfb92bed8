"""CPU checks of the 'parallel_stream' memory-bank entry points (csrc/memvla.hip): exported, declared, bound with the same
argument count, and refusing bad arguments with DXA_ERR_BAD_ARG and a message before anything is launched."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dexbotic_amd.h")
NEW = ("dxa_bank_stage_fwd", "dxa_bank_stage_bwd", "dxa_bank_append", "dxa_bank_consolidate_batched")
F32, BF16 = 0, 1


def test_new_symbols_are_exported_declared_and_bound():
    from dexbotic_amd import _lib as L
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dxa_[a-z0-9_]+)", out))
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert name in exported, name
        assert name in L.SIGNATURES, name
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl, f"{name} is not declared in the header"
        args = [a.strip() for a in decl.group(1).split(",")]
        restype, argtypes = L.SIGNATURES[name]
        assert len(args) == len(argtypes), (name, args)
        # pointers are bound as void pointers, 64-bit sizes as int64, the rest as int
        for a, t in zip(args, argtypes):
            kind = "ptr" if ("*" in a or "dxa_stream_t" in a) else ("i64" if "int64_t" in a else "int")
            want = {"ptr": "c_void_p", "i64": "c_long", "int": "c_int"}[kind]
            assert want in t.__name__ or (kind == "i64" and "c_int64" in t.__name__), (name, a, t.__name__)


def test_dtype_constants_match_the_library():
    from dexbotic_amd import _lib as L
    assert (L.F32, L.BF16) == (F32, BF16)


def _calls(lib, fake):
    """name -> callable(feat-like pointer overrides) with otherwise valid arguments: B = 2, cap = 4, N = 3, D = 8, fp32"""
    def stage(p=None, B=2, cap=4, N=3, D=8, dtype=F32):
        a = [fake] * 8
        if p is not None:
            a[p] = None
        return lib.dxa_bank_stage_fwd(*a, B, cap, N, D, dtype, None)

    def stage_bwd(p=None, B=2, cap=4, N=3, D=8, dtype=F32):
        a = [fake] * 3
        if p is not None:
            a[p] = None
        return lib.dxa_bank_stage_bwd(*a, B, cap, N, D, dtype, None)

    def append(p=None, B=2, cap=4, N=3, D=8, dtype=F32):
        a = [fake] * 5
        if p is not None:
            a[p] = None
        return lib.dxa_bank_append(*a, B, cap, N, D, dtype, None)

    def cons(p=None, B=2, cap=4, N=3, D=8, dtype=F32, mem_length=3, fifo=0):
        a = [fake] * 4                                          # feat, ts, counts, sims
        if p is not None:
            a[p] = None
        return lib.dxa_bank_consolidate_batched(a[0], a[1], a[2], 1, mem_length, fifo, a[3], B, cap, N, D, dtype, None)
    return {"dxa_bank_stage_fwd": (stage, 8), "dxa_bank_stage_bwd": (stage_bwd, 3), "dxa_bank_append": (append, 5),
            "dxa_bank_consolidate_batched": (cons, 4)}


@pytest.mark.parametrize("name", NEW)
def test_bad_arguments_are_refused_with_a_message(name):
    from dexbotic_amd import _lib as L
    fn, nptr = _calls(L.lib, 4096)[name]                         # (4096: never dereferenced, the checks come first)
    for p in range(nptr):
        assert fn(p=p) == -1 and name in L.last_error() and "null pointer" in L.last_error(), (name, p, L.last_error())
    for dim in ("B", "N", "D", "cap"):
        for bad in (0, -1):
            assert fn(**{dim: bad}) == -1 and "must be positive" in L.last_error(), (name, dim, bad, L.last_error())
    assert fn(cap=1, **({"mem_length": 0} if name == "dxa_bank_consolidate_batched" else {})) == -1
    assert "cap must be at least 2" in L.last_error()
    for bad in (2, 3, -1, 7):
        assert fn(dtype=bad) == -1 and "fp32 or bf16" in L.last_error(), (name, bad, L.last_error())


@pytest.mark.parametrize("mode", ["stream", "parallel_stream", "group"])
def test_bank_constructs_in_every_dataloader_mode_and_keeps_refusing_the_unbuilt_options(mode):
    """host side only: registering the bank's parameters needs no device"""
    from dexbotic_amd.engine import ParamStore
    from dexbotic_amd.model.memvla.memvla_arch import PerCogMemBank
    bank = PerCogMemBank(ParamStore("cpu"), mode, 4, 32, 64, mem_length=3)
    assert bank.dataloader_type == mode and bank.entries("per", (0, 0)) == [] and bank.entries("cog", (1, 0, 0)) == []
    assert bank.eid_stream == {"per": None, "cog": None} and bank.slot_banks == {"per": {}, "cog": {}}
    with pytest.raises(NotImplementedError):
        PerCogMemBank(ParamStore("cpu"), mode, 4, 32, 64, use_timestep_pe=False)
    with pytest.raises(NotImplementedError):
        PerCogMemBank(ParamStore("cpu"), mode, 4, 32, 64, fusion_type="add")
    with pytest.raises(AssertionError):
        PerCogMemBank(ParamStore("cpu"), "episode", 4, 32, 64)


def test_consolidate_refuses_mem_length_of_cap_or_more():
    from dexbotic_amd import _lib as L
    fn, _ = _calls(L.lib, 4096)["dxa_bank_consolidate_batched"]
    for ml in (4, 5, 100):
        assert fn(cap=4, mem_length=ml) == -1 and "mem_length" in L.last_error(), ml
    assert fn(cap=4, mem_length=0) == -1 and "mem_length" in L.last_error()
    # the scratch may be missing only when nothing reads it
    assert fn(p=3, fifo=0) == -1 and "null pointer" in L.last_error()
