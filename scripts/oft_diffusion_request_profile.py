#!/usr/bin/env python
"""Where an OFT diffusion action request spends its time, at the size of scripts/oft_diffusion_bench.py: per path (cached prefix, full
pass per step) the host time to enqueue one request against the time until the device is done.  Run under
``rocprofv3 --kernel-trace --stats -- python scripts/oft_diffusion_request_profile.py`` (ONLY_CACHED=1 REPS=3) it gives the
per-kernel split of the cached path (profiles/oft_diffusion_kernel_stats.txt)."""
import os, sys, time, statistics
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dexbotic_amd.model import OFTDiffusionConfig, OFTDiffusionForCausalLM
from dexbotic_amd.model.llm.qwen2 import Qwen2Config
from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig
if not torch.cuda.is_available():
    sys.exit("oft_diffusion_request_profile: needs the GPU (no timing is taken on a CPU)")
A, T = 7, 8
dev = torch.device("cuda", 0)
cfg = OFTDiffusionConfig(llm_config=Qwen2Config(), mm_vision_tower=CLIPVisionConfig(), mm_projector_type="mlp2x_gelu",
                         action_model_type="DiT", action_dim=A, chunk_size=T, use_proprio=True, proprio_dim=8, compute_dtype="bfloat16")
m = OFTDiffusionForCausalLM(cfg, device=dev, train=False)
m.init_random_(seed=0)
m.eval()
g = torch.Generator().manual_seed(1)
ids = torch.randint(1000, 30000, (1, 32), generator=g); ids[:, 1] = -200
images = torch.randn(1, 3, 224, 224, generator=g).clamp_(-2.5, 2.5).to(dev)
states = torch.randn(1, 8, generator=g).to(dev)
noise = torch.randn(1, T, A, generator=g).to(dev)
reps = int(os.environ.get("REPS", "5"))
for cached in (True, False):
    enq, tot = [], []
    for i in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.sample_actions(ids, images, states=states, noise=noise, cached=cached)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= 2:
            enq.append(1e3 * (t1 - t0)); tot.append(1e3 * (t2 - t0))
    print(f"cached={cached}: host enqueue median {statistics.median(enq):.1f} ms, until the device is done {statistics.median(tot):.1f} ms")
    if os.environ.get("ONLY_CACHED"):
        break
