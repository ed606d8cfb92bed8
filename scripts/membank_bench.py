#!/usr/bin/env python
"""Forward + backward of the MemVLA memory bank (both roles) for 16 frames at the real widths of the MemVLA configuration
(tests/golden/memvla_real_ref.npz: cognition token 1 x 3584, perceptual tokens 256 x 256 from CLIP-L/14@224), mem_length 16,
bf16 compute, weight gradients deferred as the trainer does:
  group            the serial walk of 16 consecutive frames of ONE episode (the bank cleared per batch and filling up)
  parallel_stream  ONE batched pass over 16 slots whose banks are full (16 entries each: every step stages, retrieves over
                   17 x N padded keys, appends and token-merges all 16 banks)
Timing: the modes alternate round by round inside one process; each round is --iters steps between two device synchronises on a
host clock; medians and quartiles over the rounds.
    python scripts/membank_bench.py [--modes group,parallel_stream] [--rounds 15] [--iters 5]
Launch counts: a kernel-trace run of its own, once per mode and twice with different step counts (the difference leaves out
construction and warm-up), then the summary:
    rocprofv3 --kernel-trace --stats -d DIR_A -o kt --output-format csv -- python scripts/membank_bench.py --trace MODE --iters 2
    rocprofv3 --kernel-trace --stats -d DIR_B -o kt --output-format csv -- python scripts/membank_bench.py --trace MODE --iters 6
    python scripts/membank_bench.py --summarise DIR_A DIR_B --iters 2 6"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES, MEM_LENGTH = 16, 16
DIMS = {"cog": (1, 3584), "per": (256, 256)}
ROLES = ("cog", "per")


class Leg:
    def __init__(self, mode):
        import torch
        from dexbotic_amd import hostcpu
        from dexbotic_amd.engine import ParamStore
        from dexbotic_amd.model.memvla.memvla_arch import PerCogMemBank
        self.torch, self.mode = torch, mode
        dev = torch.device("cuda", 0)
        st = self.store = ParamStore(dev, torch.bfloat16)
        self.bank = PerCogMemBank(st, mode, FRAMES, DIMS["per"][1], DIMS["cog"][1], mem_length=MEM_LENGTH, retrieval_layers=2,
                                  use_timestep_pe=True, fusion_type="gate", consolidate_type="tome", retrieval_dropout=0.0)
        st.finalize(train=True)
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        st.master.normal_(0.0, 0.02, generator=g)
        for name in st.slots:
            if name.endswith(".bias"):
                st.w32(name).zero_()
            elif name.endswith("norm.weight"):
                st.w32(name).fill_(1.0)
        st.defer_wgrad = True
        st.set_expected(())
        self.bank.train()
        self.x = {r: torch.randn((FRAMES,) + DIMS[r], device=dev, generator=g).to(torch.bfloat16).requires_grad_() for r in ROLES}
        self.proj = {r: torch.randn((FRAMES,) + DIMS[r], device=dev, generator=g).to(torch.bfloat16) for r in ROLES}
        self.frame = 0
        self.upload = lambda a: hostcpu.upload(torch.tensor(a, dtype=torch.float32), dev)

    def step(self):
        """one training step's worth of bank work: both roles forward, one backward, the deferred weight gradients"""
        torch, st = self.torch, self.store
        st.begin_step()
        if self.mode == "group":
            eids = [(0, 3)] * FRAMES
            ts = self.upload([float(self.frame + i) for i in range(FRAMES)])
            self.frame += FRAMES
        else:
            eids = [(0, i) for i in range(FRAMES)]
            ts = self.upload([float(self.frame)] * FRAMES)
            self.frame += 1
        loss = None
        for r in ROLES:
            out = (self.bank.process_batch_cog if r == "cog" else self.bank.process_batch_per)(self.x[r], eids, ts)
            term = (out * self.proj[r]).float().sum()
            loss = term if loss is None else loss + term
        loss.backward()
        st.flush_wgrads()
        for r in ROLES:
            self.x[r].grad = None

    def warm(self):
        for _ in range(MEM_LENGTH + 3 if self.mode == "parallel_stream" else 3):      # (the slots' banks fill up: 16 entries each)
            self.step()
        self.torch.cuda.synchronize()
        if self.mode == "parallel_stream":
            assert all(len(self.bank.entries(r, (i, 0, i))) == MEM_LENGTH for r in ROLES for i in range(FRAMES))


def timed(modes, rounds, iters):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("membank_bench needs the GPU")
    legs = {m: Leg(m) for m in modes}
    for leg in legs.values():
        leg.warm()
    ms = {m: [] for m in modes}
    for _ in range(rounds):
        for m in modes:                                   # alternated: A B A B ...
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                legs[m].step()
            torch.cuda.synchronize()
            ms[m].append(1e3 * (time.perf_counter() - t0) / iters)
    res = {"metric": "ms per 16 frames through the MemVLA bank, forward + backward, both roles", "frames": FRAMES,
           "mem_length": MEM_LENGTH, "rounds": rounds, "iters": iters}
    for m in modes:
        q1, med, q3 = np.percentile(ms[m], [25, 50, 75])
        res[m] = {"median_ms": round(float(med), 3), "q1_ms": round(float(q1), 3), "q3_ms": round(float(q3), 3)}
    if len(modes) == 2:
        res["speedup_group_over_parallel_stream"] = round(res["group"]["median_ms"] / res["parallel_stream"]["median_ms"], 2)
    print(json.dumps(res), flush=True)


def trace(mode, iters):
    import torch
    leg = Leg(mode)
    leg.warm()
    for _ in range(iters):
        leg.step()
    torch.cuda.synchronize()


def summarise(dirs, iters):
    counts = []
    for d in dirs:
        n = 0
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            n += sum(1 for _ in csv.DictReader(open(path)))
        counts.append(n)
    per_step = (counts[1] - counts[0]) / float(iters[1] - iters[0])
    print(json.dumps({"kernel_launches": counts, "steps": iters, "launches_per_step": per_step}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="group,parallel_stream")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, nargs="+", default=[5])
    ap.add_argument("--trace", default=None, metavar="MODE")
    ap.add_argument("--summarise", default=None, nargs=2, metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.iters)
    elif a.trace:
        trace(a.trace, a.iters[0])
    else:
        timed(a.modes.split(","), a.rounds, a.iters[0])
