#!/usr/bin/env python
"""POST /process_frame of the flow policies against the bare model call, in one process: what the serving route adds to a request.

Random weights at the shapes of scripts/pi0_bench.py (pi0: SigLIP-So400m/14 + Gemma-2B + 300 M action expert), scripts/pi05_bench.py
(pi0.5: the same with the adaptive-RMSNorm expert) and scripts/dm0_bench.py (DM0: CLIP ViT-L/14 + an ASSUMED Qwen3-1.7B geometry), bf16
compute, chunk 50, action_dim 32, 48-token prompt, 10 Euler steps, B = 1.  The tokenizer is the hash stand-in of
tests/flow_serve_tokenizers.py (no vocabulary is needed to time a request); the frames are 256 x 256 PNGs of a colour ramp with noise.

Per policy, written to the file given with --out (profiles/flow_serve.txt), each leg two things ALTERNATED request by request after
three warm-up requests apiece (eager, capture, first replay), --reqs (>= 30) timed requests each, wall clock around the call:
 1. ``FlowInferenceServer.get_response`` — PNG bytes in, list out, 3 of 3 views — against ``inference_action`` on the same request's
    device tensors with the chunk read back (``.cpu()``): the difference is PNG decode, process_images, tokeniser, state transforms
    and the answer's numpy;
 2. 1 of 3 views sent: ``views="pad"`` (two zero pixel tensors, masked) against ``views="present"`` (the one view alone);
 3. the route's stage medians (PNG decode, process_images, prompt and states, inference_action, answer) with the server's optional
    stage timing on, which synchronises the device after every stage.

    python scripts/flow_serve_bench.py [--policies pi0,pi05,dm0] [--reqs 30] [--out profiles/flow_serve.txt]
"""
import argparse
import gc
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHUNK, ADIM, TEXT, WARM = 50, 32, 48, 3
PROMPT = "pick up the red block and place it in the drawer on the left"


def build(policy, dev):
    vis = dict(model_type="siglip_vision_model")                                # SiglipVisionConfig defaults = So400m/14
    if policy == "pi0":
        from dexbotic_amd.model.pi0.pi0_arch import Pi0Config, Pi0ForCausalLM
        cfg = Pi0Config(vision_config=vis, llm_config=dict(model_type="gemma"),
                        action_config=dict(model_type="gemma", hidden_size=1024, intermediate_size=4096),
                        mm_projector_type="linear", action_dim=ADIM, chunk_size=CHUNK, compute_dtype="bfloat16")
        m = Pi0ForCausalLM(cfg, device=dev, train=False)
    elif policy == "pi05":
        from dexbotic_amd.model import Pi05Config, Pi05ForCausalLM
        cfg = Pi05Config(vision_config=vis, llm_config=dict(model_type="adarms_gemma"),
                         action_config=dict(model_type="adarms_gemma", hidden_size=1024, intermediate_size=4096, use_adarms=True),
                         mm_projector_type="linear", action_dim=ADIM, chunk_size=CHUNK, compute_dtype="bfloat16")
        m = Pi05ForCausalLM(cfg, device=dev, train=False)
    else:
        from dexbotic_amd.model import DM0Config, DM0ForCausalLM
        from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
        q3 = dict(model_type="qwen3", vocab_size=151936, num_hidden_layers=28, num_attention_heads=16, num_key_value_heads=8,
                  head_dim=128, rms_norm_eps=1e-6, rope_theta=1e6, max_position_embeddings=40960)
        cfg = DM0Config(llm_config=dict(q3, hidden_size=2048, intermediate_size=6144),
                        action_config=dict(q3, hidden_size=1024, intermediate_size=3072), mm_vision_tower=CLIPVisionConfig(),
                        action_dim=ADIM, chunk_size=CHUNK, bf16=True)
        m = DM0ForCausalLM(cfg, device=dev, train=False)
    m.init_random_(seed=0)
    if policy != "dm0":
        for n in m.store.slots:                                                 # GemmaRMSNorm scales by (1 + w)
            if n.startswith(("model.llm.", "model.action_expert.")) and n.endswith("norm.weight"):
                m.store.w32(n).zero_()
    m.post_load()
    m.eval()
    return m


def png_frames(n, side=256):
    from dexbotic_amd.serve import encode_png
    rs = np.random.RandomState(2)
    ramp = np.linspace(0, 200, side)[None, :, None] + np.linspace(0, 40, side)[:, None, None]
    return [encode_png(np.clip(ramp + rs.randint(0, 16, size=(side, side, 3)) + 10 * i, 0, 255).astype(np.uint8)) for i in range(n)]


def quartiles(ms):
    p = np.percentile(np.asarray(ms), [25, 50, 75, 90])
    return f"p25 {p[0]:7.2f}  p50 {p[1]:7.2f}  p75 {p[2]:7.2f}  p90 {p[3]:7.2f}  min {min(ms):7.2f}  max {max(ms):7.2f}"


def alternate(fns, reqs):
    """{name: fn} called in turn, WARM + reqs rounds; wall-clock ms per call of the last ``reqs`` rounds"""
    t = {k: [] for k in fns}
    for i in range(WARM + reqs):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            dt = 1e3 * (time.perf_counter() - t0)
            if i >= WARM:
                t[k].append(dt)
    return t


def bench(policy, reqs, lines):
    from dexbotic_amd import hostcpu
    from dexbotic_amd.serve import FlowInferenceServer
    from tests.flow_serve_tokenizers import StandInTokenizer
    dev = torch.device("cuda", 0)
    m = build(policy, dev)
    rs = np.random.RandomState(3)
    quant = policy != "pi0"
    a, b = ("min", "max") if quant else ("mean", "std")
    stats = {"state": {a: (-rs.uniform(0.5, 2, ADIM)).tolist(), b: rs.uniform(0.5, 2, ADIM).tolist()},
             "action": {a: (-rs.uniform(0.5, 2, 7)).tolist(), b: rs.uniform(0.5, 2, 7).tolist()}}
    tok = StandInTokenizer(TEXT, pad_token_id=2 if policy == "dm0" else 0)
    srv = {v: FlowInferenceServer(m, tok, json.loads(json.dumps(stats)), policy=policy, views=v) for v in ("pad", "present")}
    blobs = png_frames(3)
    states = json.dumps(rs.uniform(-1, 1, 8).tolist())
    lines.append(f"{policy}: {m.store.total / 1e9:.3f} B parameters, bf16, chunk {CHUNK}, B = 1, host threads {srv['pad'].host_threads}")

    # ---- 1. the route against the bare call on the same request's tensors
    s = srv["pad"]
    s.get_response(PROMPT, [io.BytesIO(x) for x in blobs], states=states)
    from PIL import Image
    pix = m.process_images([Image.open(io.BytesIO(x)).convert("RGB") for x in blobs]).to(dtype=m.dtype)[None]
    ids, am = s.tokenize([PROMPT])
    ids_d, st_d = hostcpu.upload(ids, dev), hostcpu.upload(s.last_state, dev)
    masks = np.ones((1, 3), dtype=bool)
    t = alternate({"get_response": lambda: s.get_response(PROMPT, [io.BytesIO(x) for x in blobs], states=states),
                   "inference_action": lambda: m.inference_action(input_ids=ids_d, attention_mask=am, states=st_d, images=pix,
                                                                  image_masks=masks).cpu()}, reqs)
    lines.append(f" 1. 3 of 3 views, {reqs} alternated requests each, ms:")
    for k, v in t.items():
        lines.append(f"    {k:18s} {quartiles(v)}")
    d = np.median(t["get_response"]) - np.median(t["inference_action"])
    lines.append(f"    get_response - inference_action at the medians: {d:+.2f} ms ({100 * d / np.median(t['inference_action']):+.1f} %)")

    # ---- 2. one of three views sent: the empty views padded against left out
    one = blobs[:1]
    t = alternate({v: (lambda v=v: srv[v].get_response(PROMPT, [io.BytesIO(x) for x in one], states=states)) for v in srv}, reqs)
    lines.append(f" 2. 1 of 3 views, get_response, {reqs} alternated requests each, ms:")
    for k, v in t.items():
        lines.append(f"    views={k:13s} {quartiles(v)}")
    d = np.median(t["present"]) - np.median(t["pad"])
    lines.append(f"    present - pad at the medians: {d:+.2f} ms ({100 * d / np.median(t['pad']):+.1f} %)")

    # ---- 3. where the route's own time goes: the optional stage timing (a device synchronisation per stage, so the stages do not
    #         overlap as they do in a served request and their sum is above leg 1's figure)
    s.stage_ms = {}
    for _ in range(WARM + reqs):
        s.get_response(PROMPT, [io.BytesIO(x) for x in blobs], states=states)
    lines.append(f" 3. 3 of 3 views, stage medians with a device synchronisation after each stage (DXA_SERVE_STAGES=1), {reqs} requests, ms:")
    lines.append("    " + "  ".join(f"{k} {np.median(v[WARM:]):.2f}" for k, v in s.stage_ms.items()))
    lines.append("")
    del srv, s, m, pix
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", default="pi0,pi05,dm0")
    ap.add_argument("--reqs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reqs < 30:
        sys.exit("flow_serve_bench: --reqs below 30 gives no usable quartiles")
    lines = [__doc__.split("\n\n")[0], ""]
    for policy in a.policies.split(","):
        try:
            bench(policy, a.reqs, lines)
        except Exception as e:                                   # noqa: BLE001  (a leg that cannot run is said so in the file)
            lines += [f"{policy}: NOT RUN — {type(e).__name__}: {e}", ""]
            raise
        finally:
            text = "\n".join(lines) + "\n"
            if a.out:
                with open(a.out, "w") as f:
                    f.write(text)
    print(text)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("flow_serve_bench: needs the GPU (no timing is taken on a CPU)")
    main()
