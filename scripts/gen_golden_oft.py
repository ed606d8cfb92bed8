"""Generate tests/golden/oft_t1.npz by running the REFERENCE's OFTForCausalLM on the CPU.

TEST INFRASTRUCTURE, CPU only.  Needs the reference tree next to this repository's build container (oracle/gen_golden.py: REF); the
fixture it writes is committed, so no test reads the reference.

    python scripts/gen_golden_oft.py            # from the repository root

Pinned: a tiny OFT with the ``Linear`` (L1 regression) head — CLIP tower 32 wide, 3 layers, 28 px / patch 14 (4 patches),
mlp2x_gelu projector, Qwen2 of 2 layers (hidden 96, 3 heads, 1 kv head, vocab 264), action_dim 3, chunk_size 2, proprio_dim 5 — on a
batch of 2 samples, 9 text tokens with one image placeholder, sample 1 three tokens shorter (right padding).  Built TWICE:
``use_proprio`` False (keys under ``np/``) and True (``pp/``).  Per build: the inserted attention mask and ``non_padding_lengths`` of
the reference's ``insert_action_embedding``, the predicted actions, the L1 loss, five gradients in full (``grad/``), every gradient
norm (``gradN/``), the parameters whose gradient is None (``no_grad``), the ordered key / shape list of the state dict, a call without
``attention_mask`` on sample 0, and ``inference_action`` of sample 0 with given ``action_norms``.
The weights and the images are NOT stored: tests/muvla_weights.py regenerates them from the seed and the ordered key / shape list
(N(0, 0.05) on the bf16 grid — also for ``action_query``, which the reference initialises to zeros), the archive keeps checksums.

The L1 gradient is a sign: an element with pred ~ target would flip it between implementations.  The targets come from a seeded stream
of their own, and the first stream for which min |pred - target| > 1e-2 in the fp32 run and > 5e-2 in the bf16 run, in both builds, is
taken (``target_seed``); the script asserts both.

bf16: the reference converted to bf16 (``.to(torch.bfloat16)``) runs the same batch on the CPU, images and states in bf16, the
targets in fp32 (the loss is then taken in fp32 on the bf16 predictions, as under the reference's autocast(float32) region); its
``loss`` / ``actions`` are recorded under ``bf16/`` with their distance from the fp32 run (``bf16_gap_loss``: relative;
``bf16_gap_actions``: largest difference over the largest fp32 magnitude).

Shims, none of which edits the reference: the timm stub of oracle/gen_golden.py (imported, not edited), a locally saved tiny CLIP
directory, and a stub ``diffusers`` package whose ``DDIMScheduler`` is never instantiated (only the ``DiT`` head would; the reference
imports the name at module level and the package is not installed).
"""
from __future__ import annotations

import importlib.machinery
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

SEED = 61
VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS = 264, 96, 128, 2, 3, 1
V_HIDDEN, V_INTER, V_LAYERS, V_HEADS, V_IMAGE, V_PATCH = 32, 64, 3, 2, 28, 14
B, L_TXT, ADIM, CHUNK, PDIM = 2, 9, 3, 2, 5
IMG = -200
FP32_MARGIN, BF16_MARGIN = 1e-2, 5e-2
ACTION_NORMS = {"min": [-0.5, -1.0, 0.0], "max": [0.5, 2.0, 4.0]}
FULL_GRADS = ("model.action_head.action_query", "model.action_head.model.layer_norm1.weight", "model.action_head.model.fc1.weight",
              "model.llm.layers.0.self_attn.q_proj.weight", "model.action_head.proprio_projector.fc1.weight")


def install_diffusers_stub():
    if "diffusers" in sys.modules:
        return

    class DDIMScheduler:                                         # never instantiated by the ``Linear`` head
        def __init__(self, *a, **k):
            raise RuntimeError("the diffusers stub has no scheduler: only the Linear head of OFT is generated")

    names = ("diffusers", "diffusers.schedulers", "diffusers.schedulers.scheduling_ddim")
    mods = {n: types.ModuleType(n) for n in names}
    mods[names[2]].DDIMScheduler = DDIMScheduler
    mods[names[1]].scheduling_ddim = mods[names[2]]
    mods[names[0]].schedulers = mods[names[1]]
    for n, m in mods.items():
        m.__spec__ = importlib.machinery.ModuleSpec(n, None)
        sys.modules[n] = m


def rel_err(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def main():
    from oracle.gen_golden import GOLD, REF, install_timm_shim
    from tests.muvla_weights import checksums, make_images, make_weights, pack_shapes
    sys.path.insert(0, REF)
    install_timm_shim()
    install_diffusers_stub()
    from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModel, Qwen2Config
    from dexbotic.model.oft.oft_arch import OFTConfig, OFTForCausalLM

    torch.manual_seed(SEED)
    torch.set_num_threads(8)
    d = os.path.join(tempfile.mkdtemp(), "tiny_clip")
    vcfg = CLIPVisionConfig(hidden_size=V_HIDDEN, intermediate_size=V_INTER, num_hidden_layers=V_LAYERS,
                            num_attention_heads=V_HEADS, image_size=V_IMAGE, patch_size=V_PATCH, layer_norm_eps=1e-5)
    CLIPVisionModel(vcfg).save_pretrained(d)
    CLIPImageProcessor(size={"shortest_edge": V_IMAGE}, crop_size={"height": V_IMAGE, "width": V_IMAGE}).save_pretrained(d)

    def build(use_proprio: bool):
        llm = Qwen2Config(vocab_size=VOCAB, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=LAYERS,
                          num_attention_heads=HEADS, num_key_value_heads=KV_HEADS, max_position_embeddings=4096,
                          rope_theta=1e6, rms_norm_eps=1e-6)
        cfg = OFTConfig(llm_config=llm, mm_vision_tower=d, mm_projector_type="mlp2x_gelu", action_model_type="Linear",
                        action_dim=ADIM, chunk_size=CHUNK, use_proprio=use_proprio, proprio_dim=PDIM)
        m = OFTForCausalLM(cfg)
        for p_ in m.parameters():
            p_.requires_grad = True
        return m

    rs = np.random.RandomState(SEED + 2)
    ids = rs.randint(10, 250, size=(B, L_TXT)).astype(np.int64)
    ids[:, 2] = IMG
    mask = np.ones((B, L_TXT), dtype=bool)
    mask[1, L_TXT - 3:] = False                      # sample 1: three tokens shorter (right padding)
    image_shape = (B, 3, V_IMAGE, V_IMAGE)
    images = make_images(image_shape, SEED)
    states = rs.uniform(-1, 1, size=(B, PDIM)).astype(np.float32)
    t = torch.from_numpy
    bf = torch.bfloat16

    def run_fp32(m, kw, actions):
        m.zero_grad(set_to_none=True)
        out = m(input_ids=t(ids), attention_mask=t(mask), images=t(images), actions=t(actions), **kw)
        return out

    def run_bf16(mb, kw, actions):
        with torch.no_grad():
            return mb(input_ids=t(ids), attention_mask=t(mask), images=t(images).to(bf), actions=t(actions),
                      **{k: v.to(bf) for k, v in kw.items()})

    builds = {}
    for tag, use_proprio in (("np", False), ("pp", True)):
        m = build(use_proprio)
        keys = list(m.state_dict().keys())
        shapes = [tuple(v.shape) for v in m.state_dict().values()]
        w = make_weights(keys, shapes, SEED)
        m.load_state_dict({k: t(v) for k, v in w.items()}, strict=True)
        m.train()
        mb = build(use_proprio)
        mb.load_state_dict({k: t(v) for k, v in w.items()}, strict=True)
        mb = mb.to(bf)
        mb.train()
        builds[tag] = dict(m=m, mb=mb, keys=keys, shapes=shapes, w=w, kw=dict(states=t(states)) if use_proprio else {})

    # the targets: the first seeded stream that keeps every |pred - target| away from zero, in both builds and both precisions
    target_seed = None
    for ts in range(200):
        actions = np.random.RandomState(SEED + 100 + ts).uniform(-1, 1, size=(B, CHUNK, ADIM)).astype(np.float32)
        ok = True
        for bd in builds.values():
            with torch.no_grad():
                p32 = run_fp32(bd["m"], bd["kw"], actions).logits.float().numpy()
            pbf = run_bf16(bd["mb"], bd["kw"], actions).logits.float().numpy()
            ok = ok and np.abs(p32 - actions).min() > FP32_MARGIN and np.abs(pbf - actions).min() > BF16_MARGIN
        if ok:
            target_seed = ts
            break
    assert target_seed is not None, "no target stream keeps pred - target away from zero"

    res = dict(seed=np.int64(SEED), target_seed=np.int64(target_seed), input_ids=ids, attention_mask=mask, actions=actions,
               states=states, image_shape=np.array(image_shape, dtype=np.int64),
               image_checksum=checksums(["images"], {"images": images}),
               action_norm_min=np.array(ACTION_NORMS["min"], dtype=np.float64), action_norm_max=np.array(ACTION_NORMS["max"], dtype=np.float64),
               cfg=np.array([VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS, V_HIDDEN, V_INTER, V_LAYERS, V_HEADS, V_IMAGE, V_PATCH,
                             ADIM, CHUNK, PDIM], dtype=np.int64))
    notes = []
    for tag, bd in builds.items():
        m, mb, kw, keys, shapes, w = bd["m"], bd["mb"], bd["kw"], bd["keys"], bd["shapes"], bd["w"]
        P = tag + "/"
        # the reference's own insertion on this batch: the mask and the lengths the plan must reproduce
        with torch.no_grad():
            (_, _, new_mask, _, embeds, _, _) = m.model._prepare_inputs_labels_for_multimodal(t(ids), None, t(mask), None, None, None,
                                                                                            t(images))
            Q = CHUNK * ADIM + (1 if tag == "pp" else 0)
            _, ins_mask, lengths = OFTForCausalLM.insert_action_embedding(embeds, new_mask, torch.zeros(B, Q, HIDDEN))
        out = run_fp32(m, kw, actions)
        out.loss.backward()
        pred = out.logits.detach().float().numpy()
        assert np.abs(pred - actions).min() > FP32_MARGIN
        sd = dict(m.named_parameters())
        res.update({P + "w_keys": np.array(keys), P + "w_shapes": pack_shapes(shapes), P + "w_checksums": checksums(keys, w),
                    P + "inserted_mask": ins_mask.numpy().astype(bool), P + "non_padding_lengths": lengths.numpy().astype(np.int64),
                    P + "pred": pred.astype(np.float32), P + "loss": np.float32(out.loss.item())})
        gsq, no_grad = 0.0, []
        for n, p_ in sd.items():
            if p_.grad is None:
                no_grad.append(n)
                continue
            gn = p_.grad.double().norm().item()
            gsq += gn * gn
            res[P + "gradN/" + n] = np.float64(gn)
        res[P + "grad_norm"] = np.float64(gsq ** 0.5)
        res[P + "no_grad"] = np.array(sorted(no_grad))
        for n in FULL_GRADS:
            if n in sd:
                res[P + "grad/" + n] = sd[n].grad.numpy().astype(np.float32)
        # no attention mask, sample 0 alone
        m.eval()
        kw0 = {k: v[:1] for k, v in kw.items()}
        with torch.no_grad():
            nm = m(input_ids=t(ids[:1]), images=t(images[:1]), **kw0)
        res[P + "nomask_pred"] = nm.logits.float().numpy().astype(np.float32)
        got = m.inference_action(t(ids[:1]), t(images[:1]), dict(action_norms=ACTION_NORMS, **kw0))
        res[P + "infer_actions"] = np.array(got, dtype=np.float64)
        # the reference's own bf16 arithmetic on the same batch
        ob = run_bf16(mb, kw, actions)
        pbf = ob.logits.float().numpy()
        assert np.abs(pbf - actions).min() > BF16_MARGIN
        res[P + "bf16/loss"] = np.float32(ob.loss.float().item())
        res[P + "bf16/pred"] = pbf.astype(np.float32)
        res[P + "bf16_gap_loss"] = np.float64(abs(float(res[P + "bf16/loss"]) - float(res[P + "loss"])) / abs(float(res[P + "loss"])))
        res[P + "bf16_gap_actions"] = np.float64(rel_err(pbf, pred))
        notes.append(f"{tag}: loss {res[P + 'loss']:.5f} |g| {res[P + 'grad_norm']:.4f} no_grad {len(no_grad)} min|d| "
                     f"{np.abs(pred - actions).min():.3f}/{np.abs(pbf - actions).min():.3f} bf16 loss {res[P + 'bf16/loss']:.5f} gaps "
                     f"{res[P + 'bf16_gap_loss']:.3e}/{res[P + 'bf16_gap_actions']:.3e}")
    path = os.path.join(GOLD, "oft_t1.npz")
    np.savez_compressed(path, **res)
    print(f"[gen_golden_oft] target stream {target_seed}; " + "; ".join(notes) + f"; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
