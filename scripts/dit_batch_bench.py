#!/usr/bin/env python
"""Several action requests in one launch of the bf16 DiT sampler: what it costs against what there was before.

    python scripts/dit_batch_bench.py              # every leg, each a child process under its own time limit -> profiles/dit_sampler_batched.txt
    python scripts/dit_batch_bench.py --leg dit-b  # one leg in this process

Legs
  dit-b     DiT-B head (768 / 12 heads / 3072, 12 blocks, 10 DDIM steps, guidance) of a CogACT model, G in {1, 2, 4, 8, 16}:
              (a) G single launches, one after the other          (DiT.ddim_sample_fused on one request: the fast path before)
              (b) the per-step sampler at batch G                  (ddim_sample_loop over forward_with_cfg: what B > 1 took before)
              (c) one launch with G request groups                 (DiT.ddim_sample_fused on G requests)
  dit-l     DiT-L blocks with perceptual attention over P = 256 keys (1024 / 16 / 4096, 24 blocks) at kernel level: (a) and (c).
            (b) needs MemVLA's batched episodes, which do not exist yet: not measured.
  request   CogACT at the benchmark's shapes (Qwen2.5-7B decoder, CLIP ViT-L, two views, 32-token instruction): inference_action_batch
            on B requests against B calls of inference_action, B in {1, 4, 8}; host clock around calls that end in a device-to-host copy.
Device events around each sample, the sides alternated inside one process, median and quartiles over the rounds."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GS = (1, 2, 4, 8, 16)
LEGS = {"dit-b": 240, "dit-l": 300, "request": 600}          # seconds a leg may take


def quartiles(v):
    import numpy as np
    return tuple(float(np.percentile(v, q)) for q in (25, 50, 75))


def fmt(v):
    q1, med, q3 = quartiles(v)
    return f"{med:8.3f} [{q1:7.3f} {q3:7.3f}]"


def alternate(sides, rounds, warm=2):
    """sides: {name: fn}; every round runs each side once, timed with device events; -> {name: [ms]}"""
    import torch
    for _ in range(warm):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def verdict(t):
    """(c) wins where its upper quartile is under the lower quartile of every other side"""
    c = quartiles(t["c"])
    return all(c[2] < quartiles(v)[0] for k, v in t.items() if k != "c")


def build_cogact(llm_layers, vit_layers):
    import torch
    from dexbotic_amd.model.cogact.cogact_arch import CogActConfig, CogACTForCausalLM
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
    cfg = CogActConfig(llm_config=Qwen2Config(num_hidden_layers=llm_layers), mm_vision_tower=CLIPVisionConfig(num_hidden_layers=vit_layers),
                       mm_projector_type="mlp2x_gelu", action_model_type="DiT-B", action_dim=7, chunk_size=16, compute_dtype="bfloat16")
    m = CogACTForCausalLM(cfg, device=torch.device("cuda"), train=False)
    m.init_random_(seed=0)
    m.eval()
    return m, cfg


def leg_dit_b(rounds):
    import torch
    from dexbotic_amd import kernels as K
    m, cfg = build_cogact(1, 1)
    head = m.model.action_head
    head.create_ddim(ddim_step=10)
    net, dif = head.net, head.ddim_diffusion
    g = torch.Generator().manual_seed(1)
    print("DiT-B sampler, 10 DDIM steps, guidance 1.5, bf16 serving; ms per G requests: median [lower upper quartile]")
    print(f"{'G':>3} {'(a) G single launches':>28} {'(b) per-step at batch G':>28} {'(c) one launch, G groups':>28}  (c) faster than both")
    with torch.no_grad():
        unc = m.store.w32("model.action_head.net.z_embedder.uncondition")
        for G in GS:
            noise = torch.randn(G, 16, 7, generator=g).cuda()
            cog = (torch.randn(G, 1, net.token_size, generator=g) * 0.5).cuda()
            z = torch.cat([cog, unc.unsqueeze(0).expand(G, 1, -1)], 0)
            assert net.fused_sampler_ok(2, 17) and K.dit_sample_bf16_groups_supported(G, 2, 17, net.hidden_size, net.num_heads, net.mlp_hidden)
            singles = lambda: [net.ddim_sample_fused(noise[b:b + 1], torch.cat([cog[b:b + 1], unc.unsqueeze(0)], 0), dif, 1.5) for b in range(G)]
            per_step = lambda: dif.ddim_sample_loop(net.forward_with_cfg, (2 * G, 16, 7), torch.cat([noise, noise], 0), clip_denoised=False,
                                                    model_kwargs=dict(z=z, cfg_scale=1.5), eta=0.0, device=noise.device)
            # (G = 1 too goes through the batched entry point here; the module routes a single request to the single-request kernel)
            batched = lambda: net._ddim_sample_groups(noise, z, *net._sampler_tables(dif, noise.device), 1.5, None)
            a, c = torch.cat(singles(), 0), batched()
            assert torch.equal(a, c), "the batched launch does not give the single launches' bits"
            t = alternate({"a": singles, "b": per_step, "c": batched}, rounds)
            assert not K.dit_blocks_timed_out()
            print(f"{G:>3} {fmt(t['a']):>28} {fmt(t['b']):>28} {fmt(t['c']):>28}  {'yes' if verdict(t) else 'no'}", flush=True)


def leg_dit_l(rounds):
    import torch
    from dexbotic_amd import kernels as K
    H, heads, I, depth, steps, P_, T, A = 1024, 16, 4096, 24, 10, 256, 16, 7
    gen = torch.Generator().manual_seed(2)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).cuda()
    ws = []
    for _ in range(depth):
        ws.append([rnd(3 * H, H, scale=H ** -0.5), rnd(3 * H, scale=0.1), rnd(H, H, scale=H ** -0.5), rnd(H, scale=0.1),
                   rnd(I, H, scale=H ** -0.5), rnd(I, scale=0.1), rnd(H, I, scale=I ** -0.5), rnd(H, scale=0.1),
                   rnd(3 * H, H, scale=H ** -0.5), rnd(3 * H, scale=0.1), rnd(H, H, scale=H ** -0.5), rnd(H, scale=0.1),
                   1.0 + rnd(H, scale=0.2), rnd(H, scale=0.2)])
    table = torch.tensor([w.data_ptr() for blk in ws for w in blk], dtype=torch.int64).cuda()
    arena, ptab = K.dit_bf16_pack(table, depth, H, I, per=True)
    te, pos = rnd(steps, H, scale=0.5), rnd(T + 1, H, scale=0.1)
    xw, xb, fw, fb = rnd(H, A, scale=0.3), rnd(H, scale=0.1), rnd(A, H, scale=H ** -0.5), rnd(A, scale=0.1)
    ab = torch.linspace(0.05, 0.95, steps + 1, dtype=torch.float64)
    coef = torch.zeros(steps, 4)
    coef[:, 0] = (1.0 / ab[:-1]).sqrt().float(); coef[:, 1] = (1.0 / ab[:-1] - 1.0).sqrt().float(); coef[:, 2] = ab[1:].float()
    coef = coef.cuda()
    tail = (ptab, depth, T + 1, H, heads, I, 1e-6)
    print(f"DiT-L blocks with perceptual attention (P = {P_}), 10 DDIM steps, guidance 1.5, kernel level; ms per G requests: median [quartiles]")
    print(f"{'G':>3} {'(a) G single launches':>28} {'(b) per-step at batch G':>28} {'(c) one launch, G groups':>28}  (c) faster than (a)")
    for G in GS:
        x0, ze, kv = rnd(G, T, A), rnd(G, 2, H, scale=0.5), rnd(depth, G, 2, P_, 2, H)
        kvs = [kv[:, b].contiguous() for b in range(G)]
        singles = lambda: [K.dit_sample_bf16_fwd(x0[b:b + 1].clone(), ze[b], te, pos, xw, xb, fw, fb, coef, 1, True, 1.5, *tail, per_kv=kvs[b])
                           for b in range(G)]
        batched = lambda: K.dit_sample_bf16_batched_fwd(x0.clone(), ze, te, pos, xw, xb, fw, fb, coef, True, 1.5, *tail, per_kv=kv)
        assert torch.equal(torch.cat(singles(), 0), batched()), "the batched launch does not give the single launches' bits"
        t = alternate({"a": singles, "c": batched}, rounds)
        assert not K.dit_blocks_timed_out()
        print(f"{G:>3} {fmt(t['a']):>28} {'not measured':>28} {fmt(t['c']):>28}  {'yes' if verdict(t) else 'no'}", flush=True)


def leg_request(rounds):
    import numpy as np
    import torch
    m, cfg = build_cogact(28, 24)
    norms = {"min": [-1.0] * 7, "max": [1.0] * 7}
    args = {"cfg_scale": 1.5, "num_ddim_steps": 10, "action_norms": norms}
    gen = torch.Generator().manual_seed(3)
    print("CogACT request (Qwen2.5-7B decoder, CLIP ViT-L, 2 views, 32-token instruction, guidance 1.5, 10 DDIM steps, graph replay);")
    print("ms per B requests, host clock: median [lower upper quartile]")
    print(f"{'B':>3} {'B x inference_action':>28} {'inference_action_batch':>28}  one-launch sampler")
    for B in (1, 4, 8):
        images = torch.randn(B, 2, 3, 224, 224, generator=gen).clamp_(-2.5, 2.5).cuda()
        ids = torch.randint(1000, 30000, (B, 32), generator=gen)
        ids[:, 1] = -200
        ids = ids.cuda()

        def one_by_one():
            return [m.inference_action(ids[b:b + 1], images[b:b + 1], args) for b in range(B)]

        def together():
            return m.inference_action_batch(ids, images, args)
        t = {"seq": [], "batch": []}
        for i in range(3 + rounds):                              # 3 warm rounds: eager, capture, replay
            for k, fn in (("seq", one_by_one), ("batch", together)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= 3:
                    t[k].append(1e3 * (time.perf_counter() - t0))
        fused = bool(m.model.action_head.net.used_fused)
        print(f"{B:>3} {fmt(np.asarray(t['seq'])):>28} {fmt(np.asarray(t['batch'])):>28}  {'yes' if fused else 'no'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--legs", help="comma-separated legs of the whole run (default: all)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dit_sampler_batched.txt"))
    a = ap.parse_args()
    if a.leg:
        import torch
        if not torch.cuda.is_available():
            sys.exit("dit_batch_bench: needs the GPU (no timing without one)")
        {"dit-b": leg_dit_b, "dit-l": leg_dit_l, "request": leg_request}[a.leg](a.rounds)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rc = 0
    with open(a.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"scripts/dit_batch_bench.py --rounds {a.rounds}: one MI355X, every leg a process of its own\n")
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
