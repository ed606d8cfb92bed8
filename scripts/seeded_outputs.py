#!/usr/bin/env python
"""What a tree computes on fixed seeded inputs, for an old-against-new comparison in one job:
    python scripts/seeded_outputs.py OUT.npz [--root TREE] [--only ce]     # TREE: another checkout with its own built library
    python scripts/seeded_outputs.py --diff A.npz B.npz                    # per array: bit-identical or the largest difference
Arrays: dxa_cross_entropy_fwd / bwd at [64, 152064] bf16 and [64, 1000] fp32 (dlogits as a SHA-256), pi0 ``inference_action`` on the
t1 fixture with injected noise (fp32 and bf16, eager launches and graph replay), the greedy ids of the full-size discrete VLA
(scripts/decode_bench.py's model and prompt, 32 new tokens, persistent decode step on and off)."""
import argparse
import hashlib
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--only", choices=["ce"], default=None)
ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
args = ap.parse_args()

if args.diff:
    a, b = np.load(args.diff[0]), np.load(args.diff[1])
    assert sorted(a.files) == sorted(b.files), (a.files, b.files)
    bad = 0
    for k in sorted(a.files):
        same = a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        bad += not same
        note = "bit-identical" if same else f"DIFFERENT, max |diff| {np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max():.3e}"
        print(f"{k:34s} {str(a[k].shape):14s} {note}")
    print("ALL BIT-IDENTICAL" if not bad else f"{bad} arrays differ")
    sys.exit(1 if bad else 0)

ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dexbotic_amd import kernels as K  # noqa: E402

dev = torch.device("cuda", 0)
res = {}
for tag, rows, V, dtype in (("bf16_152064", 64, 152064, torch.bfloat16), ("f32_1000", 64, 1000, torch.float32)):
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn((rows, V), generator=g) * 3.0).to(device=dev, dtype=dtype)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[::7] = -100
    labels = labels.to(dev)
    rl, lse = K.cross_entropy_fwd(logits, labels)
    dl = K.cross_entropy_bwd(logits, labels, lse, torch.tensor([0.37], device=dev), 1.0 / rows)
    res[f"ce_{tag}_row_loss"], res[f"ce_{tag}_lse"] = rl.cpu().numpy(), lse.cpu().numpy()
    res[f"ce_{tag}_dlogits_sha256"] = np.frombuffer(hashlib.sha256(dl.float().cpu().numpy().tobytes()).digest(), dtype=np.uint8)
    del logits, dl

if args.only is None:
    from tests import test_pi0_gpu as TP  # noqa: E402
    for dtype in ("float32", "bfloat16"):
        g, m = TP.build(os.path.join(ROOT, "tests", "golden"), dtype)
        kw = dict(input_ids=TP.T(g["input_ids"]), attention_mask=TP.T(g["attention_mask"]), states=TP.T(g["states"]),
                  images=TP.T(g["images"]), image_masks=TP.T(g["image_masks"]), diffusion_steps=10, noise=TP.T(g["init_noise"]))
        res[f"pi0_{dtype}_eager"] = m.inference_action(use_graph=False, **kw).float().cpu().numpy()
        for _ in range(3):                                    # eager, capture, replay
            a = m.inference_action(use_graph=True, **kw)
        res[f"pi0_{dtype}_graph"] = a.float().cpu().numpy()
        del m
    import bench  # noqa: E402
    from dexbotic_amd.model.dexbotic_arch import DexboticConfig, DexboticForCausalLM  # noqa: E402
    from dexbotic_amd.model.llm.qwen2 import Qwen2Config  # noqa: E402
    from dexbotic_amd.model.modules.mm_vision.clip.clip_encoder import CLIPVisionConfig  # noqa: E402
    cfg = DexboticConfig(llm_config=Qwen2Config(), mm_vision_tower=CLIPVisionConfig(), mm_projector_type="mlp2x_gelu",
                         compute_dtype="bfloat16")
    m = DexboticForCausalLM(cfg, device=dev, train=False)
    m.init_random_(seed=0)
    m.eval()
    b = bench.synthetic_batch(1, 1, 32, dev, seed=3)
    for fused in ("1", "0"):
        os.environ["DXA_DECODE_FUSED"] = fused
        res[f"decode_ids_fused{fused}"] = m.generate(b["input_ids"], images=b["images"], max_new_tokens=32).cpu().numpy()
np.savez(args.out, **res)
print(f"wrote {len(res)} arrays to {args.out}")
