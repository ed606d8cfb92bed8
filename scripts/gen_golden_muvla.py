"""Generate tests/golden/muvla_t1.npz by running the REFERENCE's MUVLAForCausalLM on the CPU.

TEST INFRASTRUCTURE, CPU only.  Needs the reference tree next to this repository's build container (oracle/gen_golden.py:
REF); the fixture it writes is committed, so no test reads the reference.

    python scripts/gen_golden_muvla.py            # from the repository root

Pinned: a tiny MuVLA (two CLIP towers 1024 wide — the fuser and the Q-former are fixed at that width — of 2 layers on a 24 x 24
patch grid, so 576 patches as the reference's history reshape assumes; Qwen2 of 2 layers) on a batch of 2 samples x 5 images (map,
current observation, three history frames), one placeholder per sample, sample 1 right-padded by 3 and with fewer supervised tokens
than sample 0, reward = [0.3, -1.2].  Recorded: spliced labels / mask, the projected fused features (every 16th row), the logits of
the supervised rows, the loss with labels and reward, with labels only, with reward only (0.2 x the expectile loss) and of the same
batch cut to two images per sample (no history), all gradient norms and a few gradients, the parameters without a gradient, 6
greedy ids for sample 0 from a full-prefix recompute loop (generate() itself does not run under this transformers), and the
reference's own loss with the model cast to bf16.
The 36.9 M weights and the images are NOT stored: tests/muvla_weights.py regenerates them from the seed and the ordered key / shape
list, and the archive keeps per-tensor checksums.
Shims: the timm stub of oracle/gen_golden.py (imported, not edited), locally saved tiny CLIP / Qwen2 directories, and an empty
``deepspeed.utils`` module around the import of muvla_arch only (it imports a helper it never calls), removed right after:
``save_pretrained`` would otherwise trip over ``deepspeed.__spec__`` through accelerate.
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

SEED = 31
VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS = 264, 96, 128, 2, 3, 1
V_HIDDEN, V_INTER, V_LAYERS, V_HEADS, V_IMAGE, V_PATCH = 1024, 64, 2, 16, 48, 2
B, VIEWS, N_NEW = 2, 5, 6
REWARD = [0.3, -1.2]
IMG = -200
FEAT_STRIDE = 16


def import_muvla_arch():
    stubs = {}
    for n in ("deepspeed", "deepspeed.utils"):
        m = types.ModuleType(n)
        m.__spec__ = importlib.machinery.ModuleSpec(n, None)
        stubs[n] = m
    stubs["deepspeed"].utils = stubs["deepspeed.utils"]
    stubs["deepspeed.utils"].safe_get_full_fp32_param = None
    sys.modules.update(stubs)
    try:
        from dexbotic.model.muvla import muvla_arch
    finally:
        for n in stubs:
            sys.modules.pop(n, None)
    return muvla_arch


def main():
    from oracle.gen_golden import GOLD, REF, install_timm_shim
    from tests.muvla_weights import checksums, make_images, make_weights, pack_shapes
    sys.path.insert(0, REF)
    install_timm_shim()
    from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModel, Qwen2Config
    arch = import_muvla_arch()

    torch.manual_seed(SEED)
    tmp = tempfile.mkdtemp()
    d_clip, d_llm = os.path.join(tmp, "tiny_clip"), os.path.join(tmp, "tiny_qwen2")
    vcfg = CLIPVisionConfig(hidden_size=V_HIDDEN, intermediate_size=V_INTER, num_hidden_layers=V_LAYERS,
                            num_attention_heads=V_HEADS, image_size=V_IMAGE, patch_size=V_PATCH)
    CLIPVisionModel(vcfg).save_pretrained(d_clip)
    CLIPImageProcessor(size={"shortest_edge": V_IMAGE}, crop_size={"height": V_IMAGE, "width": V_IMAGE}).save_pretrained(d_clip)
    Qwen2Config(vocab_size=VOCAB, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=LAYERS,
                num_attention_heads=HEADS, num_key_value_heads=KV_HEADS, max_position_embeddings=4096,
                rope_theta=1e6, rms_norm_eps=1e-6, tie_word_embeddings=False).save_pretrained(d_llm)
    cfg = arch.MUVLAConfig(llm_config=d_llm, mm_vision_tower=d_clip, obs_vision_tower=d_clip, mm_projector_type="mlp2x_gelu")
    m = arch.MUVLAForCausalLM(cfg)
    assert m.model.obs_vision_tower is not m.model.mm_vision_tower

    keys = list(m.state_dict().keys())
    shapes = [tuple(v.shape) for v in m.state_dict().values()]
    w = make_weights(keys, shapes, SEED)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    for p_ in m.parameters():
        p_.requires_grad = True
    n_par = sum(int(np.prod(s)) for s in shapes)

    rs = np.random.RandomState(SEED + 2)
    L = 14
    ids = rs.randint(10, 190, size=(B, L)).astype(np.int64)
    mask = np.ones((B, L), dtype=bool)
    ids[:, 2] = IMG                           # one placeholder per sample
    mask[1, L - 3:] = False                   # sample 1: right-padded by 3
    labels = ids.copy()
    labels[0, :7] = -100                      # sample 0: 7 supervised tokens
    labels[1, :8] = -100                      # sample 1: 3 (positions 8..10)
    labels[~mask] = -100
    image_shape = (B, VIEWS, 3, V_IMAGE, V_IMAGE)
    images = make_images(image_shape, SEED)
    reward = np.array(REWARD, dtype=np.float32)
    t = torch.from_numpy
    kw = dict(input_ids=t(ids), attention_mask=t(mask), images=t(images))

    m.train()
    with torch.no_grad():
        (_, _, new_mask, _, _, new_labels, _) = m.model._prepare_inputs_labels_for_multimodal(
            t(ids), None, t(mask), None, t(labels), None, t(images))
        feats = m.model.fuse_obs_with_history_and_project(t(images[:, 0]), t(images[:, 1:]))
    out = m(labels=t(labels), reward=t(reward), **kw)
    out.loss.backward()
    sd = dict(m.named_parameters())
    sl = new_labels.numpy().astype(np.int64)
    rows = np.argwhere(sl[:, 1:] != -100)                             # (b, t): position t is scored against label t + 1
    lg = out.logits.detach().numpy().astype(np.float32)
    res = dict(seed=np.int64(SEED), w_keys=np.array(keys), w_shapes=pack_shapes(shapes), w_checksums=checksums(keys, w),
               image_shape=np.array(image_shape, dtype=np.int64), image_checksum=checksums(["images"], {"images": images}),
               input_ids=ids, attention_mask=mask, labels=labels, reward=reward,
               spliced_labels=sl, spliced_mask=new_mask.numpy().astype(bool),
               feat_stride=np.int64(FEAT_STRIDE), feats=feats[:, ::FEAT_STRIDE].numpy().astype(np.float32),
               logit_rows=rows.astype(np.int64), logits=lg[rows[:, 0], rows[:, 1]], logits_shape=np.array(lg.shape, dtype=np.int64),
               loss=np.float32(out.loss.item()),
               cfg=np.array([VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS, V_HIDDEN, V_INTER, V_LAYERS, V_HEADS, V_IMAGE,
                             V_PATCH], dtype=np.int64))
    gsq, no_grad = 0.0, []
    for n, p_ in sd.items():
        if p_.grad is None:
            no_grad.append(n)
            continue
        gsq += float(p_.grad.double().pow(2).sum())
        res["gradN/" + n] = np.float64(p_.grad.double().norm().item())
    res["grad_norm"] = np.float64(gsq ** 0.5)
    res["no_grad"] = np.array(sorted(no_grad))
    # a few gradients, the large ones by their leading rows only (the test compares as many rows as are stored)
    keep = {"lm_head.weight": None, "reward_head.weight": None, "model.mm_projector.2.bias": None, "model.fuser.ln.weight": None,
            "model.fuser.ln.bias": None, "model.fuser.cross_attn.in_proj_bias": None, "model.fuser.cross_attn.in_proj_weight": 8,
            "model.history_qformer.norm.weight": None, "model.history_qformer.query_embeddings": 8,
            "model.history_qformer.attn.in_proj_weight": 8, "model.history_qformer.input_proj.bias": None,
            "model.llm.layers.0.self_attn.q_proj.weight": None}
    for n, p_ in sd.items():
        if n.endswith("encoder.layers.0.mlp.fc1.bias"):               # one tensor of each tower
            keep[n] = None
    for n, r in keep.items():
        g_ = sd[n].grad.numpy().astype(np.float32)
        res["grad/" + n] = g_ if r is None else g_[:r]
    with torch.no_grad():
        res["loss_labels"] = np.float32(m(labels=t(labels), **kw).loss.item())
        res["loss_reward"] = np.float32(m(reward=t(reward), **kw).loss.item())
        res["loss_no_history"] = np.float32(m(input_ids=t(ids), attention_mask=t(mask), images=t(images[:, :2]),
                                              labels=t(labels), reward=t(reward)).loss.item())
    # greedy continuation of sample 0's prompt by full-prefix recompute
    m.eval()
    cur = t(ids[:1]).clone()
    img1 = t(images[:1])
    new, rows_l = [], []
    with torch.no_grad():
        for _ in range(N_NEW):
            row = m(input_ids=cur, images=img1).logits[0, -1].float()
            nxt = int(torch.argmax(row))
            new.append(nxt)
            rows_l.append(row.numpy().astype(np.float32))
            cur = torch.cat([cur, torch.tensor([[nxt]], dtype=cur.dtype)], dim=1)
    res["decode_prompt"] = ids[:1]
    res["decode_new_ids"] = np.array(new, dtype=np.int64)
    top2 = np.sort(np.stack(rows_l), axis=1)[:, -2:]
    res["decode_margin"] = (top2[:, 1] - top2[:, 0]).astype(np.float32)
    # the reference's own bf16 arithmetic on the same batch
    m.train()
    m.bfloat16()
    with torch.no_grad():
        res["loss_bf16"] = np.float32(m(input_ids=t(ids), attention_mask=t(mask), images=t(images).bfloat16(), labels=t(labels),
                                        reward=t(reward)).loss.float().item())
    path = os.path.join(GOLD, "muvla_t1.npz")
    np.savez_compressed(path, **res)
    print(f"[gen_golden_muvla] params {n_par} loss {res['loss']:.5f} labels-only {res['loss_labels']:.5f} reward-only "
          f"{res['loss_reward']:.5f} no-history {res['loss_no_history']:.5f} bf16 {res['loss_bf16']:.5f} |g| {res['grad_norm']:.4f} "
          f"new ids {new} min margin {res['decode_margin'].min():.4g} no_grad {len(no_grad)} spliced {sl.shape} "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
