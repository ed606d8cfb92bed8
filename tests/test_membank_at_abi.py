"""CPU checks of the slot-indexed memory-bank entry points (csrc/memvla.hip: dxa_bank_stage_fwd_at, dxa_bank_append_at,
dxa_bank_consolidate_batched_at): exported, declared, bound with the same argument lists, refusing bad arguments with
DXA_ERR_BAD_ARG and a message before anything is launched; the host-side slot-list check."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dexbotic_amd.h")
F32 = 0
# name -> the argument names of the declaration, in order
AT = {
    "dxa_bank_stage_fwd_at": ["feat", "ts", "slot_ids", "counts", "tokens", "timesteps", "mem", "ts_eff", "kv_len", "R", "S", "cap",
                              "N", "D", "dtype", "stream"],
    "dxa_bank_append_at": ["feat", "ts", "slot_ids", "counts", "src", "timesteps", "R", "S", "cap", "N", "D", "dtype", "stream"],
    "dxa_bank_consolidate_batched_at": ["feat", "ts", "slot_ids", "counts", "count_add", "mem_length", "fifo", "sims", "R", "S", "cap",
                                        "N", "D", "dtype", "stream"],
}


def test_at_symbols_are_exported_declared_and_bound_with_the_stated_argument_lists():
    from dexbotic_amd import _lib as L
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dxa_[a-z0-9_]+)", out))
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, want_names in AT.items():
        assert name in exported, name
        assert name in L.SIGNATURES, name
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl, f"{name} is not declared in the header"
        args = [a.strip() for a in decl.group(1).split(",")]
        assert [re.split(r"[\s*]+", a)[-1] for a in args] == want_names, (name, args)
        restype, argtypes = L.SIGNATURES[name]
        assert len(args) == len(argtypes), (name, args)
        for a, t in zip(args, argtypes):
            kind = "ptr" if ("*" in a or "dxa_stream_t" in a) else ("i64" if "int64_t" in a else "int")
            want = {"ptr": "c_void_p", "i64": "c_long", "int": "c_int"}[kind]
            assert want in t.__name__ or (kind == "i64" and "c_int64" in t.__name__), (name, a, t.__name__)
        # the existing entry point of the same step keeps its declaration: the _at one adds slot_ids and S, nothing else
        base = re.search(r"\bint\s+" + name[:-3] + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        base_names = [re.split(r"[\s*]+", a.strip())[-1] for a in base.group(1).split(",")]
        assert [n for n in want_names if n not in ("slot_ids", "S")] == ["R" if n == "B" else n for n in base_names], name


def _calls(lib, fake):
    """name -> (callable with otherwise valid arguments: R = 2, S = 3, cap = 4, N = 3, D = 8, fp32; number of pointers)"""
    def stage(p=None, R=2, S=3, cap=4, N=3, D=8, dtype=F32):
        a = [fake] * 9
        if p is not None:
            a[p] = None
        return lib.dxa_bank_stage_fwd_at(*a, R, S, cap, N, D, dtype, None)

    def append(p=None, R=2, S=3, cap=4, N=3, D=8, dtype=F32):
        a = [fake] * 6
        if p is not None:
            a[p] = None
        return lib.dxa_bank_append_at(*a, R, S, cap, N, D, dtype, None)

    def cons(p=None, R=2, S=3, cap=4, N=3, D=8, dtype=F32, mem_length=3, fifo=0):
        a = [fake] * 5                                          # feat, ts, slot_ids, counts, sims
        if p is not None:
            a[p] = None
        return lib.dxa_bank_consolidate_batched_at(a[0], a[1], a[2], a[3], 1, mem_length, fifo, a[4], R, S, cap, N, D, dtype, None)
    return {"dxa_bank_stage_fwd_at": (stage, 9), "dxa_bank_append_at": (append, 6), "dxa_bank_consolidate_batched_at": (cons, 5)}


@pytest.mark.parametrize("name", sorted(AT))
def test_at_bad_arguments_are_refused_with_a_message(name):
    from dexbotic_amd import _lib as L
    fn, nptr = _calls(L.lib, 4096)[name]                         # (4096: never dereferenced, the checks come first)
    for p in range(nptr):
        assert fn(p=p) == -1 and name in L.last_error() and "null pointer" in L.last_error(), (name, p, L.last_error())
    for dim in ("R", "N", "D", "cap"):
        for bad in (0, -1):
            assert fn(**{dim: bad}) == -1 and "must be positive" in L.last_error(), (name, dim, bad, L.last_error())
    assert fn(cap=1, **({"mem_length": 0} if "consolidate" in name else {})) == -1 and "cap must be at least 2" in L.last_error()
    for bad in (2, 3, -1, 7):
        assert fn(dtype=bad) == -1 and "fp32 or bf16" in L.last_error(), (name, bad, L.last_error())
    # more rows than slots, no slots
    for kw in ({"R": 4, "S": 3}, {"S": 0}, {"S": -2}):
        assert fn(**kw) == -1 and name in L.last_error() and "slots" in L.last_error(), (name, kw, L.last_error())
    if "consolidate" in name:
        for ml in (4, 5, 0):
            assert fn(cap=4, mem_length=ml) == -1 and "mem_length" in L.last_error(), ml
        assert fn(p=4, fifo=0) == -1 and "null pointer" in L.last_error()


def test_the_host_list_check_refuses_duplicates_and_ids_outside_the_bank():
    from dexbotic_amd import kernels as K
    assert K.distinct_slots([3, 0, 4], 5) == [3, 0, 4]
    for bad in ([1, 1], [0, 2, 0], [5], [-1, 2]):
        with pytest.raises(ValueError):
            K.distinct_slots(bad, 5)


def test_episode_slots_of_the_bank_are_host_state_reset_clears():
    """host side only: opening the slots needs no device"""
    from dexbotic_amd.engine import ParamStore
    from dexbotic_amd.model.memvla.memvla_arch import PerCogMemBank
    for mode in ("group", "stream", "parallel_stream"):
        bank = PerCogMemBank(ParamStore("cpu"), mode, 4, 32, 64, mem_length=3)
        assert bank.episode_time == [] and bank.episode_banks == {}
        bank.open_episode_slots(3)
        bank.open_episode_slots(3)
        assert bank.episode_time == [0, 0, 0]
        with pytest.raises(ValueError, match="reset"):
            bank.open_episode_slots(4)
        with pytest.raises(ValueError):
            bank.open_episode_slots(0)
        bank.reset()
        assert bank.episode_time == [] and bank.episode_banks == {}
        bank.open_episode_slots(4)
        assert len(bank.episode_time) == 4
