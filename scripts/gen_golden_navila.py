"""Generate tests/golden/navila_t1.npz by running the REFERENCE's NaVILAForCausalLM on the CPU.

TEST INFRASTRUCTURE, CPU only.  Needs the reference tree next to this repository's build container (oracle/gen_golden.py:
REF); the fixture it writes is committed, so no test reads the reference.

    python scripts/gen_golden_navila.py            # from the repository root

Pinned: a tiny NaVILA (SigLIP of 3 layers on a 3x3 patch grid -> hidden_states[-2] -> mlp_downsample -> Qwen2 of 2 layers) on a
batch of 2 samples x 3 frames — sample 0 with three placeholders (4 feature rows each), sample 1 with ONE (all 12 rows), unequal
text lengths (right padding) — its spliced labels / mask, logits, the training-mode (soft-target) loss, the eval-mode
(standard) loss, selected gradients and all gradient norms, the parameters without a gradient, and 6 greedy token ids for sample
0's prompt from a full-prefix recompute loop (as for lm_t1: generate() itself does not run under this transformers).
Weights, images and nothing else are rounded to bf16-representable fp32 values: the archive deflates to half the size and the
bf16 model starts from exactly the same weights.
Shims: the timm stub of oracle/gen_golden.py (imported, not edited) and a locally saved tiny SigLIP directory.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

SEED = 23
VOCAB, HIDDEN, INTER, LAYERS, HEADS, KV_HEADS = 264, 96, 128, 2, 3, 1
V_HIDDEN, V_INTER, V_LAYERS, V_HEADS, V_IMAGE, V_PATCH = 32, 64, 3, 2, 42, 14
B, FRAMES, N_NEW = 2, 3, 6
TIME_IDS = list(range(200, 208))
IMG = -200


def bf16_grid(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def main():
    from oracle.gen_golden import GOLD, REF, install_timm_shim
    sys.path.insert(0, REF)
    install_timm_shim()
    from transformers import Qwen2Config, SiglipImageProcessor, SiglipVisionConfig, SiglipVisionModel
    from dexbotic.model.navila.navila_arch import NaVILAConfig, NaVILAForCausalLM

    torch.manual_seed(SEED)
    d = os.path.join(tempfile.mkdtemp(), "tiny_siglip")
    vcfg = SiglipVisionConfig(hidden_size=V_HIDDEN, intermediate_size=V_INTER, num_hidden_layers=V_LAYERS,
                              num_attention_heads=V_HEADS, image_size=V_IMAGE, patch_size=V_PATCH, layer_norm_eps=1e-6)
    SiglipVisionModel(vcfg).save_pretrained(d)
    SiglipImageProcessor(size={"height": V_IMAGE, "width": V_IMAGE}).save_pretrained(d)
    llm = Qwen2Config(vocab_size=VOCAB, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=LAYERS,
                      num_attention_heads=HEADS, num_key_value_heads=KV_HEADS, max_position_embeddings=4096,
                      rope_theta=1e6, rms_norm_eps=1e-6, tie_word_embeddings=False)
    cfg = NaVILAConfig(llm_config=llm.to_dict(), mm_vision_tower=d, mm_projector_type="mlp_downsample",
                       time_token_ids=TIME_IDS, soft_ce_std=1.0, tie_word_embeddings=False)
    m = NaVILAForCausalLM(cfg)
    assert m.model.mm_vision_tower.select_layer == -2

    # deterministic weights on the bf16 grid: N(0, 0.05) matrices, norm weights around 1, small biases
    rs = np.random.RandomState(SEED)
    w = {}
    for k, v in m.state_dict().items():
        shape = tuple(v.shape)
        leaf = k.rsplit(".", 1)[-1]
        if leaf == "weight" and len(shape) == 1:
            a = 1.0 + 0.1 * rs.standard_normal(shape)
        elif leaf == "bias":
            a = 0.05 * rs.standard_normal(shape)
        else:
            a = 0.05 * rs.standard_normal(shape)
        w[k] = bf16_grid(a)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    for p_ in m.parameters():
        p_.requires_grad = True

    # sample 0: three placeholders (4 rows each) and 9 more tokens; sample 1: ONE placeholder (12 rows), 3 tokens shorter
    L = 14
    ids = rs.randint(10, 190, size=(B, L)).astype(np.int64)
    mask = np.ones((B, L), dtype=bool)
    ids[0, [1, 3, 5]] = IMG
    ids[1, 2] = IMG
    mask[1, L - 3:] = False
    labels = ids.copy()
    labels[:, :7] = -100                      # the prompt part (placeholders included) is not supervised
    labels[~mask] = -100
    # time tokens in the supervised part: both ends of the id range and one inside, next to ordinary tokens
    for b, (pos, tok) in enumerate([((8, 10, 12), (TIME_IDS[0], TIME_IDS[3], TIME_IDS[-1])),
                                    ((7, 9), (TIME_IDS[-1], TIME_IDS[1]))]):
        for p_, t_ in zip(pos, tok):
            ids[b, p_] = labels[b, p_] = t_
    for b in range(B):
        sup = labels[b][labels[b] != -100]
        assert np.isin(sup, TIME_IDS).sum() >= 2 and (~np.isin(sup, TIME_IDS)).sum() >= 2
        assert (np.isin(sup, [TIME_IDS[0], TIME_IDS[-1]])).any()
    images = bf16_grid(np.clip(rs.standard_normal((B, FRAMES, 3, V_IMAGE, V_IMAGE)), -2.5, 2.5))
    t = torch.from_numpy

    m.train()
    (_, _, new_mask, _, _, new_labels, _) = m.model._prepare_inputs_labels_for_multimodal(
        t(ids), None, t(mask), None, t(labels), None, t(images))
    out = m(input_ids=t(ids), attention_mask=t(mask), labels=t(labels), images=t(images))
    out.loss.backward()
    sd = dict(m.named_parameters())
    res = {"w/" + k: v for k, v in w.items()}
    res.update(seed=np.int64(SEED), input_ids=ids, attention_mask=mask, labels=labels, images=images,
               time_token_ids=np.array(TIME_IDS, dtype=np.int64), soft_ce_std=np.float32(1.0),
               spliced_labels=new_labels.numpy().astype(np.int64), spliced_mask=new_mask.numpy().astype(bool),
               logits=out.logits.detach().numpy().astype(np.float32), loss=np.float32(out.loss.item()),
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
    keep = ["lm_head.weight", "model.mm_projector.1.weight", "model.mm_projector.2.weight", "model.mm_projector.4.weight",
            "model.llm.layers.0.self_attn.q_proj.weight", "model.mm_vision_tower.vision_tower.encoder.layers.1.mlp.fc1.weight"]
    for n in keep:
        res["grad/" + n] = sd[n].grad.numpy().astype(np.float32)
    # eval mode: the standard causal-LM loss on the same batch
    m.eval()
    with torch.no_grad():
        ev = m(input_ids=t(ids), attention_mask=t(mask), labels=t(labels), images=t(images))
    res["eval_loss"] = np.float32(ev.loss.item())
    # greedy continuation of sample 0's prompt (three placeholders, three frames) by full-prefix recompute
    cur = t(ids[:1]).clone()
    img1 = t(images[:1])
    new, rows_l = [], []
    with torch.no_grad():
        for _ in range(N_NEW):
            lg = m(input_ids=cur, images=img1).logits[0, -1].float()
            nxt = int(torch.argmax(lg))
            new.append(nxt)
            rows_l.append(lg.numpy().astype(np.float32))
            cur = torch.cat([cur, torch.tensor([[nxt]], dtype=cur.dtype)], dim=1)
    res["decode_prompt"] = ids[:1]
    res["decode_new_ids"] = np.array(new, dtype=np.int64)
    top2 = np.sort(np.stack(rows_l), axis=1)[:, -2:]
    res["decode_margin"] = (top2[:, 1] - top2[:, 0]).astype(np.float32)
    path = os.path.join(GOLD, "navila_t1.npz")
    np.savez_compressed(path, **res)
    print(f"[gen_golden_navila] loss {res['loss']:.5f} eval {res['eval_loss']:.5f} |g| {res['grad_norm']:.4f} new ids {new} "
          f"min margin {res['decode_margin'].min():.4g} no_grad {len(no_grad)} spliced {res['spliced_labels'].shape} "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
