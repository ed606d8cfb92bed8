#!/usr/bin/env python
"""R running MemVLA episodes answered from one model: the three ways to answer R frames, and where a request's time goes.

    python scripts/memvla_batch_bench.py                  # every leg, each a child process under its own time limit -> profiles/memvla_batched_episodes.txt
    python scripts/memvla_batch_bench.py --leg requests   # one leg in this process

Legs
  requests  MemVLA at the real shapes (oracle.gen_golden_memvla_real.REAL: Qwen2.5-7B / CLIP-L widths, DiT-L head with perceptual
            attention over P = 256 keys, per_token_size 256, bank depth 4), random weights, bf16 serving, guidance 1.5, 10 DDIM
            steps, graph replay, R in {1, 2, 4, 8, 16}:
              (a) R calls of inference_action, one after the other         (one model: the only way before)
              (b) inference_action_batch on the per-step sampler at batch R  (fused_sampler=False)
              (c) inference_action_batch on ONE launch of R request groups   (BATCHED_GROUPS_PER opened for the measurement)
            The three sides alternate inside one process; device events and the host clock around calls that end in a device-to-host
            copy; median and quartiles over the rounds.  The banks are full (every step consolidates).
  between   the same three sides at every other R up to the launch's 16 groups (3, 5, 6, 7, 9 .. 15).
  stages    at the same shapes, eager launches, device events: the bank pass of a call (both roles, R rows) and the projection of
            the perceptual keys / values (per request — the routed variant; one product per block over all R requests; what there
            was before: one product per block plus the transposing copy), and their share of request (c).
  distance  the bf16 batched-vs-served-alone distance and its cap, as tests/test_memvla_episodes_gpu.py measures them."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RS = (1, 2, 4, 8, 16)
RS_BETWEEN = tuple(r for r in range(2, 17) if r not in RS)       # the routing constant names every R: each one is measured
LEGS = {"requests": 420, "between": 420, "stages": 240, "distance": 240}          # seconds a leg may take
ARGS = {"cfg_scale": 1.5, "num_ddim_steps": 10, "action_norms": {"min": [-1.0] * 7, "max": [1.0] * 7}}


def quartiles(v):
    import numpy as np
    return tuple(float(np.percentile(v, q)) for q in (25, 50, 75))


def fmt(v):
    q1, med, q3 = quartiles(v)
    return f"{med:8.3f} [{q1:7.3f} {q3:7.3f}]"


def verdict(t):
    """(c) wins where its upper quartile is under the lower quartile of every other side"""
    c = quartiles(t["c"])
    return all(c[2] < quartiles(v)[0] for k, v in t.items() if k != "c")


def build_memvla():
    import torch
    from oracle.gen_golden_memvla_real import MEM_LEN, PER, REAL as c
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config
    from dexbotic_amd.model.memvla.memvla_arch import MemVLAConfig, MemVLAForCausalLM
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    llm = Qwen2Config(vocab_size=c.vocab_size, hidden_size=c.hidden_size, intermediate_size=c.intermediate_size,
                      num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                      num_key_value_heads=c.num_key_value_heads, rms_norm_eps=c.rms_norm_eps, rope_theta=c.rope_theta)
    vis = CLIPVisionConfig(hidden_size=c.v_hidden, intermediate_size=c.v_inter, num_hidden_layers=c.v_layers,
                           num_attention_heads=c.v_heads, image_size=c.v_image, patch_size=c.v_patch, layer_norm_eps=c.v_eps)
    mc = MemVLAConfig(llm_config=llm, mm_vision_tower=vis, mm_projector_type="mlp2x_gelu", action_model_type="DiT-L",
                      action_dim=c.action_dim, chunk_size=c.chunk_size, compute_dtype="bfloat16", per_token_size=PER,
                      dataloader_type="group", group_size=6, mem_length=MEM_LEN, retrieval_layers=2, use_timestep_pe=True,
                      fusion_type="gate", consolidate_type="tome", retrieval_dropout=0.0)
    m = MemVLAForCausalLM(mc, device=torch.device("cuda"), train=False)
    m.init_random_(seed=0)
    m.eval()
    return m, c


def request_inputs(c, R, gen):
    import torch
    images = torch.randn(R, 3, c.v_image, c.v_image, generator=gen).clamp_(-2.5, 2.5).cuda()
    ids = torch.randint(10, c.vocab_size - 10, (R, 32), generator=gen)
    ids[:, 1] = -200
    return ids.cuda(), images


def leg_requests(rounds, rs=RS):
    import numpy as np
    import torch
    from dexbotic_amd import kernels as K
    from dexbotic_amd.model.cogact.action_model.dit import DiT
    DiT.BATCHED_GROUPS_PER = range(2, 17)                        # (c) is measured at every R, whatever is routed
    m, c = build_memvla()
    net = m.model.action_head.net
    gen = torch.Generator().manual_seed(3)
    print("MemVLA request at the real shapes (1 decoder layer / 3 ViT layers of the 7B / CLIP-L widths, DiT-L + perceptual attention, P = 256),")
    print("bf16 serving, guidance 1.5, 10 DDIM steps, graph replay, full banks; ms per R frames: median [lower upper quartile]")
    head = (f"{'R':>3} {'(a) R x inference_action':>28} {'(b) batch, per-step sampler':>28} {'(c) batch, one launch':>28}  (c) faster than both")
    tables = {"device events": [], "host clock": []}
    for R in rs:
        ids, images = request_inputs(c, R, gen)
        flags = ["False"] * R
        fused_seen = {}

        def one_by_one():
            return [m.inference_action(ids[b:b + 1], images[b:b + 1], "False", ARGS) for b in range(R)]

        def per_step():
            out = m.inference_action_batch(ids, images, flags, dict(ARGS, fused_sampler=False), num_slots=max(RS))
            fused_seen["b"] = bool(net.used_fused)
            return out

        def grouped():
            out = m.inference_action_batch(ids, images, flags, ARGS, num_slots=max(RS))
            fused_seen["c"] = bool(net.used_fused)
            return out
        sides = {"a": one_by_one, "b": per_step, "c": grouped}
        ev, wall = {k: [] for k in sides}, {k: [] for k in sides}
        for i in range(5 + rounds):                              # 5 warm rounds: eager, capture, replay, and the banks fill up
            for k, fn in sides.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= 5:
                    wall[k].append(1e3 * (time.perf_counter() - t0))
                    ev[k].append(e0.elapsed_time(e1))
        assert not K.dit_blocks_timed_out() and getattr(net, "allow_fused", True)
        assert fused_seen == {"b": False, "c": True}, fused_seen
        for name, t in (("device events", ev), ("host clock", wall)):
            t = {k: np.asarray(v) for k, v in t.items()}
            tables[name].append(f"{R:>3} {fmt(t['a']):>28} {fmt(t['b']):>28} {fmt(t['c']):>28}  {'yes' if verdict(t) else 'no'}")
        print(f"  (R = {R} measured)", flush=True)
    for name, rows in tables.items():
        print(f"\n{name}\n{head}")
        for r in rows:
            print(r)
    if 1 in rs:
        print("\n(R = 1: (c) is the single-request launch, the same work as (a).)", flush=True)


def leg_stages(rounds):
    import numpy as np
    import torch
    from dexbotic_amd import hostcpu
    from dexbotic_amd.model.cogact.action_model.dit import DiT
    DiT.BATCHED_GROUPS_PER = range(2, 17)
    m, c = build_memvla()
    net, bank = m.model.action_head.net, m.model.per_cog_mem_bank
    gen = torch.Generator().manual_seed(4)
    args = dict(ARGS, use_graph=False)
    P_, D_, d = (c.v_image // c.v_patch) ** 2, 256, c.hidden_size

    def timed(fn, warm=3):
        out = []
        for i in range(warm + rounds):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warm:
                out.append(e0.elapsed_time(e1))
        return np.asarray(out)
    print("stages of a batched request, eager launches, device events; ms: median [lower upper quartile]")
    print(f"{'R':>3} {'request (c), eager':>28} {'bank pass (both roles)':>28} {'per-KV, per request (kept)':>28} {'per-KV, one product/block':>28} "
          f"{'per-KV, before (+ copy)':>28}  bank / per-KV share of (c)")
    with torch.no_grad():
        for R in RS:
            ids, images = request_inputs(c, R, gen)
            flags = ["False"] * R
            req = timed(lambda: m.inference_action_batch(ids, images, flags, args, num_slots=max(RS)), warm=6)
            per = (torch.randn(R, P_, D_, generator=gen) * 0.5).to("cuda", torch.bfloat16)
            cog = (torch.randn(R, 1, d, generator=gen) * 0.5).to("cuda", torch.bfloat16)
            slots, first = list(range(R)), [False] * R

            def bank_pass():
                ts = hostcpu.upload(torch.full((R,), 7.0), "cuda")
                bank.step_episode_rows("cog", cog, slots, ts, first)
                bank.step_episode_rows("per", per, slots, ts, first)
            pt = per.float().repeat(2, 1, 1)
            t_bank = timed(bank_pass)
            t_req = timed(lambda: net.precompute_per_kv_groups(pt, R, per_request=True))
            t_all = timed(lambda: net.precompute_per_kv_groups(pt, R, per_request=False))

            def before():
                kv = net.precompute_per_kv(pt, packed=True)
                return kv.view(net.depth, 2, R, *kv.shape[2:]).transpose(1, 2).contiguous()
            t_old = timed(before)
            same = torch.equal(net.precompute_per_kv_groups(pt, R, per_request=True), net.precompute_per_kv_groups(pt, R, per_request=False))
            med = lambda v: quartiles(v)[1]
            print(f"{R:>3} {fmt(req):>28} {fmt(t_bank):>28} {fmt(t_req):>28} {fmt(t_all):>28} {fmt(t_old):>28}  "
                  f"{100 * med(t_bank) / med(req):4.1f} % / {100 * med(t_req) / med(req):4.1f} %   "
                  f"(one product per block has the per-request bits: {'yes' if same else 'NO'})", flush=True)


def leg_distance(_rounds):
    cmd = [sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", os.path.join(ROOT, "tests", "test_memvla_episodes_gpu.py"), "-k",
           "grouped_launch"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print("bf16, R = 3 episodes over 4 frames at the smallest grouped shape (tests/test_memvla_episodes_gpu.py, max-norm relative distance of")
    print("the de-normalised actions); cap = the slot's one-launch episode against its block-by-block episode, both served alone:")
    for line in r.stdout.splitlines():
        if line.lstrip(".").startswith("slot ") or " passed" in line or " failed" in line:
            print("  " + line.lstrip("."))
    sys.stdout.flush()
    sys.exit(r.returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--legs", help="comma-separated legs of the whole run (default: all)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memvla_batched_episodes.txt"))
    a = ap.parse_args()
    if a.leg:
        import torch
        if not torch.cuda.is_available():
            sys.exit("memvla_batch_bench: needs the GPU (no timing without one)")
        {"requests": leg_requests, "between": lambda n: leg_requests(n, RS_BETWEEN), "stages": leg_stages,
         "distance": leg_distance}[a.leg](a.rounds)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rc = 0
    with open(a.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"scripts/memvla_batch_bench.py --rounds {a.rounds}: one MI355X, every leg a process of its own\n")
        for leg in (a.legs.split(",") if a.legs else LEGS):
            cmd = ["timeout", "-k", "10", str(LEGS[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--rounds", str(a.rounds)]
            with subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT) as child:
                for line in child.stdout:
                    say(line.rstrip("\n"))
            say("")
            rc = child.returncode
            if rc != 0:                                          # nothing more is started on the GPU after a leg that failed
                say(f"leg {leg} ended with status {rc}")
                break
    sys.exit(rc)


if __name__ == "__main__":
    main()
